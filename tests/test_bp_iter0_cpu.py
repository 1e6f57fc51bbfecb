"""Iteration 0 of the LDPC kernel in front of the BP loop (csrc/decode.hip), without a GPU.

1. The compiler's own assembly (tools/isa_census.py): the loop is no longer than it was, and the fast form of iteration 0
   holds exactly three v_rcp_f32 -- fast_tanh on one pair and one single value -- against the nine tanh divisions of an
   iteration of the loop.
2. A restatement in numpy float32 (every operation one IEEE single-precision operation, as the kernel is compiled): with all
   messages zero the nine values an iteration of the loop would hand to fast_tanh are three distinct ones, and the
   three-value form stores the same bits to toc as the nine-value form -- in the half domain, where x = (cwh + 0) + 0 and an
   LLR of +0 (cwh = -0) comes out as +0, and in the reference's own domain, where x = ((cw + -0) + -0) * -0.5 = cwh keeps
   the sign of a zero.  Random and edge LLR vectors, zeros of both signs, infinities and NaN included."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the loop before iteration 0 left it: tests/test_bp_loop_budget.py, profiles/r03_isa_census.json
LOOP_VALU, LOOP_PACKED, LOOP_RCP, LOOP_SLOTS = 212, 127, 18, 340.7


@pytest.fixture(scope="module")
def census(tmp_path_factory):
    out = tmp_path_factory.mktemp("census0") / "census.json"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_census.py"), "--kernel", "ft8_decode_kernelILb0ELi3", "--json", str(out)],
                   check=True, stdout=subprocess.DEVNULL, timeout=600)
    with open(out) as f:
        return json.load(f)


def test_the_loop_is_no_longer_than_it_was(census):
    it = census["per_iteration_fast_path"]
    n = it["valu"] + it["valu_pk"] + it["trans"]
    print(f"loop: {n} VALU ({it['valu']} + {it['valu_pk']} packed + {it['trans']} rcp), {census['valu_issue_slots_per_iteration']} issue slots")
    assert n <= LOOP_VALU and it["valu_pk"] <= LOOP_PACKED and it["trans"] == LOOP_RCP
    assert census["valu_issue_slots_per_iteration"] <= LOOP_SLOTS
    ops = census["per_iteration_valu_opcodes"]
    assert not {k: v for k, v in ops.items() if k.startswith(("v_mov", "v_pk_mov", "v_cndmask", "v_accvgpr"))}


def test_iteration_0_divides_three_times_on_the_fast_form(census):
    p = census["iteration0_fast_tanh"]
    print(f"iteration 0, fast form: blocks {p['fast_division_blocks']} + {p['polynomial_blocks']}: {p['valu']} + {p['valu_pk']} packed + "
          f"{p['trans']} rcp = {p['valu_issue_slots']} issue slots; {p['valu_opcodes']}")
    assert p["trans"] == 3 and p["valu_opcodes"].get("v_rcp_f32_e32", 0) == 3          # one pair and one single
    assert p["valu_opcodes"].get("v_cmpx_gt_f32_e64", 0) == 3 and p["valu_opcodes"].get("v_bfi_b32", 0) == 3   # ... and their clamps
    # an iteration of the loop spends 4 tanh_pair + 1 tanh_one, about 159 slots; one pair and one single are about 54
    assert p["valu_issue_slots"] <= 60


# ---- the restatement -----------------------------------------------------------------------------------------------------------

F = np.float32


def fast_tanh(x):
    """ft8_lib ldpc.c fast_tanh on float32 arrays, operation by operation"""
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        x2 = x * x
        a = x * (F(945.0) + x2 * (F(105.0) + x2))
        b = F(945.0) + x2 * (F(420.0) + x2 * F(15.0))
        q = a / b
    return np.where(x < F(-4.97), F(-1.0), np.where(x > F(4.97), F(1.0), q)).astype(F)


def nine_value_form(cw, fast):
    """what an iteration of the loop hands to fast_tanh when every state is +0: [n][3 variables][3 edges]"""
    cw = np.asarray(cw, F)
    z, mz = F(0.0), F(-0.0)
    with np.errstate(all="ignore"):
        if fast:                                                   # half domain: A = B = c2 = +0
            cwh = cw * F(-0.5)
            u = cwh + z
            x1, x2 = u + z, u + z                                  # X = u + A
            x0 = (cwh + z) + z                                     # Y / z
            hard = ((x2 + z) < z)
        else:                                                      # tov = -2 * 0 = -0
            u = cw + mz
            x0 = ((cw + mz) + mz) * F(-0.5)
            x1, x2 = (u + mz) * F(-0.5), (u + mz) * F(-0.5)
            hard = ((u + mz) + mz) > z
    return np.stack([fast_tanh(x0), fast_tanh(x1), fast_tanh(x2)], axis=-1), hard


def three_value_form(cw, fast):
    cw = np.asarray(cw, F)
    with np.errstate(all="ignore"):
        cwh = cw * F(-0.5)
        x = cwh + F(0.0) if fast else cwh
        hard = (x < F(0.0)) if fast else (cw > F(0.0))
    t = fast_tanh(x)
    return np.stack([t, t, t], axis=-1), hard


def _vectors():
    rng = np.random.default_rng(20)
    ints = rng.integers(-255, 256, (64, 174)).astype(F)
    ints[:, ::5] = 0                                               # exactly-zero LLRs: +0 from the integer difference
    f = np.sqrt(F(24.0) / rng.uniform(1.0, 255.0 ** 2, (64, 1)).astype(F)).astype(F)
    edge = np.array([0.0, -0.0, 1e-45, -1e-45, 1.17549435e-38, -1.17549435e-38, 9.94, -9.94, 9.9400005, -9.9400005, 9.939999, -9.939999,
                     1.0, -1.0, 255.0, -255.0, 3.4e38, -3.4e38, np.inf, -np.inf, np.nan, 0.0192, -0.0192], F)
    bits = rng.integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32).view(F)      # any bit pattern
    return [(ints * f).astype(F).reshape(-1), edge, bits]


@pytest.mark.parametrize("fast", [True, False])
def test_three_values_give_the_bits_of_nine(fast):
    for cw in _vectors():
        nine, hard9 = nine_value_form(cw, fast)
        three, hard3 = three_value_form(cw, fast)
        assert nine.view(np.uint32).tolist() == three.view(np.uint32).tolist()
        assert hard9.tolist() == hard3.tolist()
    # an LLR of +0: cwh = -0; the half domain stores fast_tanh(+0) = +0, the reference's domain fast_tanh(-0) = -0
    t, _ = three_value_form(np.array([0.0], F), fast)
    assert t.view(np.uint32)[0, 0] == (0 if fast else 0x80000000)
    assert nine_value_form(np.array([0.0], F), fast)[0].view(np.uint32)[0, 0] == (0 if fast else 0x80000000)
