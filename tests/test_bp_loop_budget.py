"""The instruction budget of the LDPC kernel's BP loop, from the compiler's own assembly (tools/isa_census.py; no GPU).

The kernel is bound by VALU issue, so an instruction in the loop of the fast stream is time.  After the moves and the select that
computed nothing the reference computes were removed (csrc/decode.hip: the zeroing of states nobody reads, the select in front
of the guard, the copies that built broadcast operands of the row products, the copies of fast_atanh's -735.0f), an iteration of
the fast path of ft8_decode_kernel<false, 3> holds no register move and no select at all; a compiler or a source change that
brings one back, or lengthens the iteration, fails here."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VALU_PER_ITERATION_PARENT = 221          # 76 single-rate + 127 packed + 18 v_rcp_f32, among them 6 v_mov_b32, 2 v_mov_b64, 1 v_cndmask_b32
VALU_PER_ITERATION = 212                 # 67 + 127 + 18
MOVES_AND_SELECTS = ("v_mov_b32", "v_mov_b64", "v_pk_mov_b32", "v_cndmask_b32", "v_accvgpr")
DOCUMENTED_EXCEPTIONS = {}               # opcode -> count; none


@pytest.fixture(scope="module")
def census(tmp_path_factory):
    out = tmp_path_factory.mktemp("census") / "census.json"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_census.py"), "--kernel", "ft8_decode_kernelILb0ELi3", "--json", str(out)],
                   check=True, stdout=subprocess.DEVNULL, timeout=600)
    with open(out) as f:
        return json.load(f)


def test_fast_stream_has_no_moves_or_selects(census):
    assert census["kernel"] == "ft8_decode_kernelILb0ELi3"
    ops = census["per_iteration_valu_opcodes"]
    assert ops.get("v_rcp_f32_e32", 0) == 18 and sum(v for k, v in ops.items() if k.startswith("v_pk_")) > 100, ops     # it IS the fast stream of the BP loop
    found = {k: v for k, v in ops.items() if k.startswith(MOVES_AND_SELECTS)}
    assert found == DOCUMENTED_EXCEPTIONS, found


def test_valu_instructions_per_iteration(census):
    it = census["per_iteration_fast_path"]
    n = it["valu"] + it["valu_pk"] + it["trans"]
    print(f"VALU instructions per iteration of the fast path: {n} ({it['valu']} single-rate, {it['valu_pk']} packed, {it['trans']} transcendental); "
          f"parent {VALU_PER_ITERATION_PARENT}; {census['valu_issue_slots_per_iteration']} issue slots")
    assert n <= VALU_PER_ITERATION
    assert n < VALU_PER_ITERATION_PARENT
    # the division chains and the packing are what they were: the cut came out of the single-rate instructions alone
    assert it["trans"] == 18 and it["valu_pk"] <= 127
