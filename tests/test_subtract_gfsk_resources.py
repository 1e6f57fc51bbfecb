"""The GFSK kernels of subtract.hip from the compiler's own code object metadata (tools/kernel_resources.py on that source; no GPU
needed): both are there beside the CPFSK kernels, neither uses scratch memory, the estimate kernel's LDS is at or below 81 920
bytes so that two workgroups still fit a CU's 160 KiB, and the CPFSK kernels' LDS is what it was."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GFSK_KERNELS = ("ft8_subtract_estimate_gfsk_kernel", "ft8_subtract_apply_gfsk_kernel")


def test_gfsk_kernels_use_no_scratch_and_fit_two_workgroups_per_cu():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as K
    text = K.assemble(os.path.join(K.CSRC, "subtract.hip"))
    ks = K.kernels_of(text)
    by_name = dict(zip(K.demangle([k["symbol"] for k in ks]), ks))
    for name in GFSK_KERNELS:
        assert name in by_name, sorted(by_name)
        assert by_name[name]["scratch_bytes_per_lane"] == 0 and by_name[name]["lds_bytes"] <= 81920, by_name[name]
        assert by_name[name]["max_workgroup"] == 256
    assert not re.findall(r"^\s*scratch_(load|store)", text, re.M) and K.cmpx_dpp_hazards(text) == []
    est, app = (by_name[n] for n in GFSK_KERNELS)
    # w4 as two planes, Q at k + (k >> 5), four waves' planes, rings, sums and tones; w4 as float2, the headers, Q and the ramp
    assert est["lds_bytes"] == 72448 + 4 * 1585 and app["lds_bytes"] == 37168 + 4 * 1540 + 4 * 64
    assert K.waves_per_simd(est) >= 2
    assert by_name["ft8_subtract_estimate_kernel"]["lds_bytes"] == 72448 and by_name["ft8_subtract_apply_kernel"]["lds_bytes"] == 37168
