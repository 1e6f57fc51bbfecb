"""The kernels of AP on the demodulated soft bits keep the resources of the kernels they stand beside (CPU box: hipcc
cross-compiles gfx950 without a GPU; tools/kernel_resources.py reads the kernels' metadata).  ft8_demod_soft_kernel is
ft8_demod_kernel's body with the soft bits written out: the same 36 608 bytes of LDS, no scratch, at least its 3 waves per SIMD.
ft8_ap_soft_kernel is ap.hip's hypothesis loop inside a loop over three rows: at most ft8_ap_kernel's 13 824 bytes, no scratch, at
least its 4 waves.  The tag kernel's new instances use neither scratch nor LDS."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernels_of(src):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as K
    ks = K.kernels_of(K.assemble(os.path.join(K.CSRC, src)))
    return K, dict(zip(K.demangle([k["symbol"] for k in ks]), ks))


def test_the_emitting_demod_kernel_keeps_the_demod_kernel_s_lds_and_waves():
    K, seen = kernels_of("demod.hip")
    for name in ("ft8_demod_kernel", "ft8_demod_soft_kernel"):
        assert name in seen, (name, sorted(seen))                      # both plain, non-template kernels
        k = seen[name]
        print(name, k, "waves", K.waves_per_simd(k))
        assert k["scratch_bytes_per_lane"] == 0 and k["lds_bytes"] == 36608 and K.waves_per_simd(k) >= 3
    assert len([n for n in seen if n.startswith("ft8_tag_kernel<")]) == 1


def test_the_ap_soft_kernel_keeps_the_ap_kernel_s_lds_and_waves():
    K, seen = kernels_of("apsoft.hip")
    _K, ap = kernels_of("ap.hip")
    k, ref = seen["ft8_ap_soft_kernel"], ap["ft8_ap_kernel"]
    print(k, "waves", K.waves_per_simd(k), "beside", ref, "waves", K.waves_per_simd(ref))
    assert ref["lds_bytes"] == 13824 and K.waves_per_simd(ref) >= 4
    assert k["scratch_bytes_per_lane"] == 0 and k["lds_bytes"] <= 13824 and K.waves_per_simd(k) >= 4
    tags = [(n, t) for n, t in seen.items() if n.startswith("ft8_tag_kernel<")]
    assert len(tags) == 2 and all("ft8gpu_apsoft_info" in n for n, _t in tags), sorted(seen)
    for n, t in tags:
        print(n, t)
        assert t["scratch_bytes_per_lane"] == 0 and t["lds_bytes"] == 0 and K.waves_per_simd(t) == 8
