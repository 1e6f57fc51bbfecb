"""The call-hint kernels from the compiler's own code object metadata (tools/kernel_resources.py on csrc/hint.hip; no GPU
needed): ft8_hint_kernel uses no scratch memory and no more LDS than ft8_ap_kernel, whose loop body it shares; the update kernel
holds one table in LDS; the pre-kernel that encodes the tables uses neither; one instance of the tag kernel.  The wave count found is printed (DESIGN.md "Call hints" records it)."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hint_kernel_uses_no_scratch_and_no_more_lds_than_ap():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as K
    seen = {}
    for src in ("hint.hip", "ap.hip"):
        text = K.assemble(os.path.join(K.CSRC, src))
        ks = K.kernels_of(text)
        seen[src] = dict(zip(K.demangle([k["symbol"] for k in ks]), ks))
        if src == "hint.hip":
            assert not re.findall(r"^\s*scratch_(load|store)", text, re.M) and K.cmpx_dpp_hazards(text) == []
    hint, ap = seen["hint.hip"]["ft8_hint_kernel"], seen["ap.hip"]["ft8_ap_kernel"]
    print("ft8_hint_kernel", hint, "waves per SIMD", K.waves_per_simd(hint), "; ft8_ap_kernel waves per SIMD", K.waves_per_simd(ap))
    assert hint["scratch_bytes_per_lane"] == 0 and hint["max_workgroup"] == 256
    assert 0 < hint["lds_bytes"] <= ap["lds_bytes"] == 13824
    update = seen["hint.hip"]["ft8_hint_update_kernel"]
    assert update["scratch_bytes_per_lane"] == 0 and update["lds_bytes"] == 8192
    enc = seen["hint.hip"]["ft8_hint_encode_kernel"]
    assert enc["scratch_bytes_per_lane"] == 0 and enc["lds_bytes"] == 0
    tags = [n for n in seen["hint.hip"] if n.startswith("ft8_tag_kernel<")]
    assert len(tags) == 1 and seen["hint.hip"][tags[0]]["scratch_bytes_per_lane"] == 0 and seen["hint.hip"][tags[0]]["lds_bytes"] == 0
    assert sorted(seen["hint.hip"]) == sorted(["ft8_hint_kernel", "ft8_hint_encode_kernel", "ft8_hint_update_kernel"] + tags)
