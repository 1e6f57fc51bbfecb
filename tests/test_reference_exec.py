"""The reference's own code, executed: every parity claim of this repository has the form "equals the oracle, bit for bit",
and the oracle (oracle/ft8_oracle.c) is our restatement of the reference.  These tests run the reference's rtlsdr_ft8d.c
itself (oracle/_ref/ref_oracle and ref_gpu, built by `make -C oracle ref`: oracle/ref_harness.c compiles it unmodified
with stand-ins for librtlsdr, libcurl and FFTW) beside the oracle and the library's host code, so that a mistake shared
by the oracle and a kernel (a FIR coefficient, the window, the quantiser, the record fill) shows as a difference.

What the reference executes here: rtlsdr_callback (the RX chain), ft8_subsystem (window, |X|^2 -> dB quantiser, the
candidate loop, hash-table dedup, the strtok / snprintf CQ fill), readRawIQfile, readC2file, writeRawIQfile, printSpots,
decoderSelfTest and main's -t / -r modes.  What it cannot execute: ft8_lib (its submodule is empty; ref_oracle takes those
names from the oracle, ref_gpu from libft8gpu.so) and FFTW (oracle/ref_fftw_shim.c runs the oracle's transform and
counts the calls).

CPU tests need a checkout of the reference (oracle_lib.reference_dir) or what build() left in oracle/_ref.  The GPU tests
read oracle/_ref only.  Every child process runs under its own timeout and is never retried."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import oracle_lib
import synth_util as S
from test_rx import make_capture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_OUT = os.path.join(ROOT, "oracle", "_ref")
NS = oracle_lib.NSAMPLES
REC = oracle_lib.RESULT_DTYPE
FFTS_PER_FRAME = 184                       # 92 blocks x 2 time offsets (rtlsdr_ft8d.c:1398-1411)
MAX_NSIG = 12                              # far below the 50 unique messages that would fill the reference's hash table


def _binary(name):
    """oracle/_ref/<name>.  A missing binary skips the test only when nothing tried to build it: `make -C oracle ref`
    writes <name>.log whenever it attempts the link (ref_gpu: whenever libft8gpu.so exists), so a missing binary
    beside its log, or beside a checkout of the reference (ref_oracle), is a build failure and fails the test."""
    path = os.path.join(REF_OUT, name)
    if os.path.exists(path):
        return path
    log = os.path.join(REF_OUT, name + ".log")
    if os.path.exists(log):
        with open(log) as f:
            pytest.fail(f"oracle/_ref/{name} was not built; oracle/_ref/{name}.log:\n{f.read()[-4000:]}", pytrace=False)
    if name == "ref_oracle" and oracle_lib.reference_dir() is not None:
        pytest.fail(f"a checkout of the reference is at {oracle_lib.reference_dir()}, but oracle/_ref/{name} and its log "
                    "are missing: `make -C oracle ref` did not run to the harness step", pytrace=False)
    why = "no checkout of the reference" if name == "ref_oracle" else "no checkout of the reference, or no libft8gpu.so"
    pytest.skip(f"oracle/_ref/{name} was not built ({why} when build() ran)")


@pytest.fixture(scope="module")
def ref_oracle():
    oracle_lib.build()
    oracle_lib.build_ref()
    return _binary("ref_oracle")


def run(binary, args, stdin=b"", cwd=None, timeout=120):
    """one child process under its own timeout; a non-zero exit fails the test with the child's stderr"""
    p = subprocess.run([binary, *map(str, args)], input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       cwd=cwd, timeout=timeout)
    assert p.returncode == 0, f"{os.path.basename(binary)} {' '.join(map(str, args))}: exit {p.returncode}\n{p.stderr.decode(errors='replace')}"
    return p.stdout


def _report(capsys, request, text):
    """a line in pytest's output, also under -q and for a passing test (how many frames / records a test compared)"""
    with capsys.disabled():
        print(f"\n{request.node.name}: {text}", flush=True)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# RX: rtlsdr_callback (rtlsdr_ft8d.c:76-202) from reset, fed in chunks as librtlsdr would
# ---------------------------------------------------------------------------------------------------------------------
RX_CASES = [("signal", 751 * 3000 + 8 * 37), ("random", 751 * 2000), ("extremes", 751 * 1500 + 744), ("zeros", 751 * 100),
            ("signal", 8 * 50), ("random", 751 * 48000 + 8 * 1000),          # the last one: iqIndex stops at 48000
            ("random", 752), ("extremes", 751 * 17 + 1), ("random", 751 * 16)]   # 1, 17 and 16 blocks
RX_CHUNKS = (512, 65536, 8 * 37)           # 65536 = DEFAULT_BUF_LENGTH (rtlsdr_ft8d.h:40); 296 = an odd multiple of 8


def ref_rx(binary, raw, chunk):
    out = run(binary, ["rx", chunk], np.ascontiguousarray(raw, np.uint8).tobytes())
    assert len(out) == 8 * NS + 4
    i = np.frombuffer(out, np.float32, NS, 0)
    q = np.frombuffer(out, np.float32, NS, 4 * NS)
    return i, q, struct.unpack_from("<I", out, 8 * NS)[0]


def _rx_raw(kind, npairs, seed=10):
    npairs -= npairs % 8
    return make_capture(seed, npairs, kind), npairs


@pytest.mark.parametrize("kind,npairs", RX_CASES)
def test_reference_rx_callback_equals_the_oracle(ref_oracle, kind, npairs):
    raw, npairs = _rx_raw(kind, npairs)
    i, q, n = oracle_lib.rx_capture(raw)
    assert n == min(NS, npairs // 751)
    for chunk in RX_CHUNKS:
        ri, rq, rn = ref_rx(ref_oracle, raw, chunk)
        assert rn == n, (chunk, rn, n)
        assert np.array_equal(_bits(ri), _bits(i)), f"{kind}/{npairs}: I differs at chunk {chunk}"
        assert np.array_equal(_bits(rq), _bits(q)), f"{kind}/{npairs}: Q differs at chunk {chunk}"


# ---------------------------------------------------------------------------------------------------------------------
# ft8_subsystem: the reference's waterfall (seen at the ft8_lib boundary) and its records
# ---------------------------------------------------------------------------------------------------------------------
def _encode_fn():
    return S.oracle_encode_fn(oracle_lib)


def finite_frames():
    """(name, iq [2][48000]) for the waterfall / record comparisons: CQ traffic, mixed traffic, the self-test frame,
    noise only, all zeros, full-scale samples"""
    from rtlsdr_ft8d_amd import workload
    enc = _encode_fn()
    out = []
    for seed, nsig, snr in ((101, 8, (-16.0, 0.0)), (102, MAX_NSIG, (-12.0, 4.0)), (103, 3, (-22.0, -10.0))):
        out.append((f"cq{seed}", S.make_frame(seed, nsig, enc, snr_range=snr)[0]))
    texts, tones = workload.mixed_message_pool(256, seed=5)
    for seed, nsig, snr in ((201, 10, (-14.0, 2.0)), (202, MAX_NSIG - 1, (-10.0, 6.0)), (203, 6, (-18.0, 0.0))):
        out.append((f"mixed{seed}", S.make_mixed_frame(seed, nsig, snr, texts, tones)[0]))
    out.append(("selftest", np.stack(oracle_lib.selftest_signal())))
    rng = np.random.default_rng(301)
    noise = rng.normal(0, 1, (2, NS)).astype(np.float32)
    out.append(("noise", (noise * (np.float32(0.5) / np.abs(noise).max())).astype(np.float32)))
    out.append(("zeros", np.zeros((2, NS), np.float32)))
    out.append(("fullscale", np.where(rng.random((2, NS)) < 0.5, -1.0, 1.0).astype(np.float32)))
    return out


def nonfinite_frames():
    """frames holding +-inf, NaN and finite values whose |X|^2 overflows float32 (1e30^2): the reference's x86 build
    quantises a non-finite dB value to 0 (cvttss2si -> INT_MIN -> clamp)"""
    enc = _encode_fn()
    base = S.make_frame(401, 6, enc, snr_range=(-10.0, 4.0))[0]
    out = []
    f = base.copy()
    f[0, 5000] = np.inf
    f[1, 20000] = -np.inf
    out.append(("inf", f))
    f = base.copy()
    f[0, 12345] = np.nan
    f[1, 30000:30004] = np.nan
    out.append(("nan", f))
    f = base.copy()
    f[0, 40000] = 1e30
    f[1, 7000] = -3e38
    out.append(("overflow", f))
    f = base.copy()
    f[0, 100] = np.inf
    f[1, 200] = np.nan
    f[0, 44000] = 2e20
    out.append(("mixed_nonfinite", f))
    return out


def ref_subsystem(binary, iq, fill, waterfall_file=None, timeout=300):
    """ft8_subsystem of the reference over B frames in ONE process: (records [B][50], n [B], ffts [B], waterfalls or None)"""
    iq = np.ascontiguousarray(iq, np.float32)
    B = iq.shape[0]
    args = ["subsystem", B, fill] + ([waterfall_file] if waterfall_file else [])
    out = run(binary, args, iq.tobytes(), timeout=timeout)
    step = 4 + 50 * REC.itemsize + 4
    assert len(out) == B * step
    n = np.array([struct.unpack_from("<i", out, f * step)[0] for f in range(B)], np.int32)
    dec = np.stack([np.frombuffer(out, REC, 50, f * step + 4) for f in range(B)])
    ffts = np.array([struct.unpack_from("<I", out, f * step + 4 + 50 * REC.itemsize)[0] for f in range(B)])
    wf = None
    if waterfall_file:
        wf = np.fromfile(waterfall_file, np.uint8)
        assert wf.size == B * oracle_lib.MAG_ARRAY
        wf = wf.reshape(B, oracle_lib.MAG_ARRAY)
    return dec, n, ffts, wf


def _pattern(B, fill):
    return np.frombuffer(bytes([fill]) * (B * 50 * REC.itemsize), REC).reshape(B, 50).copy()


def _check_subsystem(names, iq, dec, n, ffts, fill):
    odec, on = oracle_lib.subsystem_batch(iq, nthreads=8, decodes=_pattern(len(names), fill))
    for k, name in enumerate(names):
        assert ffts[k] == FFTS_PER_FRAME, (name, ffts[k])
        assert n[k] == on[k], (name, n[k], on[k])
        assert dec[k].tobytes() == odec[k].tobytes(), f"{name}: records differ (fill {fill:#04x})"
    return int(n.sum())


def test_reference_waterfall_and_records_equal_the_oracle(ref_oracle, tmp_path, request, capsys):
    frames = finite_frames()
    names = [f[0] for f in frames]
    iq = np.stack([f[1] for f in frames])
    compared = 0
    for fill in (0xA5, 0x00):
        wf_file = str(tmp_path / f"wf{fill}.bin")
        dec, n, ffts, wf = ref_subsystem(ref_oracle, iq, fill, wf_file)
        if fill == 0xA5:
            owf = oracle_lib.waterfall_batch(iq, nthreads=8)
            for k, name in enumerate(names):
                diff = np.flatnonzero(wf[k] != owf[k])
                assert diff.size == 0, f"{name}: {diff.size} waterfall bytes differ, first at {diff[:5]}"
        compared += _check_subsystem(names, iq, dec, n, ffts, fill)
    assert n[names.index("selftest")] == 1 and dec[names.index("selftest"), 0]["call"] == b"K1JT"
    assert compared > 20            # the frames decode: a record comparison of empty lists would prove little
    _report(capsys, request, f"{len(frames)} frames, waterfalls of {len(frames) * oracle_lib.MAG_ARRAY} bytes, "
                     f"{compared} records x 2 fills compared")


def test_reference_nonfinite_frames_follow_the_x86_quantiser(ref_oracle, tmp_path):
    """the oracle's x86 quantiser form claims to be what the reference's x86 build does; the fenced default (the product's
    definition, +inf dB -> 255) differs from it exactly where |X|^2 is +inf, and nowhere else"""
    frames = nonfinite_frames()
    names = [f[0] for f in frames]
    iq = np.stack([f[1] for f in frames])
    wf_file = str(tmp_path / "wf.bin")
    dec, n, ffts, wf = ref_subsystem(ref_oracle, iq, 0xA5, wf_file)
    fenced = oracle_lib.waterfall_batch(iq)
    L = oracle_lib.lib()
    L.ft8o_set_quantiser_x86(1)
    try:
        x86 = oracle_lib.waterfall_batch(iq)
        for k, name in enumerate(names):
            diff = np.flatnonzero(wf[k] != x86[k])
            assert diff.size == 0, f"{name}: {diff.size} waterfall bytes differ from the x86 quantiser, first at {diff[:5]}"
        _check_subsystem(names, iq, dec, n, ffts, 0xA5)
    finally:
        L.ft8o_set_quantiser_x86(0)
    saw_fence = False
    for k, name in enumerate(names):
        d = np.flatnonzero(wf[k] != fenced[k])
        # the documented difference: only bins the fence sets to 255 where the reference's x86 conversion gives 0
        assert np.all(fenced[k][d] == 255) and np.all(wf[k][d] == 0), name
        saw_fence |= d.size > 0
    assert saw_fence


# ---------------------------------------------------------------------------------------------------------------------
# readRawIQfile / readC2file / writeRawIQfile (rtlsdr_ft8d.c:744-856) against the library's and the oracle's
# ---------------------------------------------------------------------------------------------------------------------
def _reader_payloads():
    rng = np.random.default_rng(501)

    def recs(n, scale=1.0):
        return (rng.normal(0, scale, 2 * n)).astype(np.float32)

    special = recs(NS)
    special[0:6] = [np.nan, -0.0, 1e-45, -1e-40, 0.0, 1.5e-38]
    special[1000:1003] = [-np.nan, 5e-44, -0.0]
    infs = recs(2000)
    infs[77] = np.inf
    infs[500] = -np.inf
    tiny = (recs(3000) * np.float32(1e-42)).astype(np.float32)       # subnormal peak: the 1e-24f floor of the peak search
    return {
        "full": recs(NS).tobytes(),
        "short": recs(1000).tobytes(),
        "long": recs(NS + 2000).tobytes(),
        "odd_floats": recs(1000).tobytes() + np.float32(3.25).tobytes(),
        "ragged_bytes": recs(1000).tobytes() + b"\x01\x02\x03",
        "zeros": np.zeros(2 * NS, np.float32).tobytes(),
        "special": special.tobytes(),
        "inf": infs.tobytes(),
        "subnormal": tiny.tobytes(),
        "empty": b"",
    }


def _c2_header(dial_hz):
    return b"FT8TESTNAME\0\0\0" + struct.pack("<i", 2) + struct.pack("<d", dial_hz)


def _fill_buffers(fill):
    a = np.frombuffer(bytes([fill]) * (4 * NS), np.float32).copy()
    return a, a.copy()


def _library():
    import rtlsdr_ft8d_amd as ft8
    return ft8.load_library()


@pytest.mark.parametrize("fmt", ["iq", "c2"])
def test_reference_readers_equal_the_library_and_the_oracle(ref_oracle, tmp_path, fmt):
    lib, L = _library(), oracle_lib.lib()
    dials = (14074000.0, 7074000.75, 0.0, 1296174000.0)
    for k, (name, payload) in enumerate(_reader_payloads().items()):
        path = tmp_path / f"{name}.{fmt}"
        dial = dials[k % len(dials)]
        path.write_bytes((_c2_header(dial) if fmt == "c2" else b"") + payload)
        for fill in (0xA5, 0x00):
            out = run(ref_oracle, [f"read-{fmt}", path, fill])
            assert len(out) == 8 + 8 * NS
            rc, rdial = struct.unpack_from("<iI", out)
            ri, rq = np.frombuffer(out, np.uint32, NS, 8), np.frombuffer(out, np.uint32, NS, 8 + 4 * NS)
            assert rc == min(NS, len(payload) // 8), (name, rc)
            assert rdial == (int(dial) if fmt == "c2" else 0), (name, rdial)
            for who in ("library", "oracle"):
                i, q = _fill_buffers(fill)
                d = C.c_double(-1.0)
                if who == "library":
                    got = (lib.ft8gpu_read_c2(i.ctypes.data, q.ctypes.data, str(path).encode(), C.byref(d)) if fmt == "c2"
                           else lib.ft8gpu_read_raw_iq(i.ctypes.data, q.ctypes.data, str(path).encode()))
                else:
                    fp = C.POINTER(C.c_float)
                    got = (L.ft8o_read_c2(i.ctypes.data_as(fp), q.ctypes.data_as(fp), str(path).encode(), C.byref(d)) if fmt == "c2"
                           else L.ft8o_read_raw_iq(i.ctypes.data_as(fp), q.ctypes.data_as(fp), str(path).encode()))
                assert got == rc, (name, who, got, rc)
                if fmt == "c2":
                    assert int(d.value) == rdial, (name, who, d.value, rdial)
                # the samples AND the untouched tail of the pattern-filled buffers
                assert np.array_equal(_bits(i), ri), f"{name}.{fmt}: I differs ({who}, fill {fill:#04x})"
                assert np.array_equal(_bits(q), rq), f"{name}.{fmt}: Q differs ({who}, fill {fill:#04x})"


def test_reference_writer_equals_the_library_and_the_oracle(ref_oracle, tmp_path):
    lib, L = _library(), oracle_lib.lib()
    rng = np.random.default_rng(601)
    i = rng.normal(0, 0.2, NS).astype(np.float32)
    q = rng.normal(0, 0.2, NS).astype(np.float32)
    i[:5] = [np.nan, np.inf, -0.0, 1e-45, -np.inf]
    q[:5] = [-0.0, np.nan, 0.0, -1e-44, 3e38]
    for frame in ((i, q), (np.zeros(NS, np.float32), np.zeros(NS, np.float32)), oracle_lib.selftest_signal()):
        fi, fq = (np.ascontiguousarray(x, np.float32) for x in frame)
        rc = struct.unpack("<i", run(ref_oracle, ["write-iq", tmp_path / "ref.iq"], fi.tobytes() + fq.tobytes()))[0]
        fp = C.POINTER(C.c_float)
        assert rc == NS
        assert lib.ft8gpu_write_raw_iq(fi.ctypes.data, fq.ctypes.data, str(tmp_path / "lib.iq").encode()) == NS
        assert L.ft8o_write_raw_iq(fi.ctypes.data_as(fp), fq.ctypes.data_as(fp), str(tmp_path / "oracle.iq").encode()) == NS
        ref = (tmp_path / "ref.iq").read_bytes()
        assert len(ref) == 8 * NS
        assert (tmp_path / "lib.iq").read_bytes() == ref
        assert (tmp_path / "oracle.iq").read_bytes() == ref


# ---------------------------------------------------------------------------------------------------------------------
# printSpots (rtlsdr_ft8d.c:643-663)
# ---------------------------------------------------------------------------------------------------------------------
def _spot_records():
    rng = np.random.default_rng(701)
    d = np.zeros(50, REC)
    for k in range(50):
        d[k]["call"] = ("K%dABC" % k).encode()
        d[k]["loc"] = b"FN%02d" % (k % 100)
        d[k]["freq"] = int(rng.integers(0, 3000))
        d[k]["snr"] = int(rng.integers(10, 60))
    d[0]["call"], d[0]["loc"], d[0]["freq"], d[0]["snr"] = b"PJ4/K1ABCDEF", b"", -1250, 123        # 12 characters, empty loc
    d[1]["call"], d[1]["loc"], d[1]["snr"] = b"(null)", b"(null)", 999                               # snprintf("%s", NULL)
    d[2]["freq"], d[2]["snr"] = 2147483000, -7                                                       # freq + dial wraps
    d[3]["freq"], d[3]["snr"] = -2147483000, 100
    d[4]["call"], d[4]["loc"] = b"", b"JO22"
    return d


@pytest.mark.parametrize("n", [0, 1, 2, 5, 50])
@pytest.mark.parametrize("dial", [0, 14074000, 1296174000])
def test_reference_print_spots_equals_the_library_and_the_oracle(ref_oracle, n, dial):
    import rtlsdr_ft8d_amd as ft8
    d = _spot_records()
    when = (2026, 3, 9, 7, 45)
    ref = run(ref_oracle, ["print-spots", n, dial, *when], d.tobytes()).decode()
    assert ref == ft8.format_spots(d, n, dial, *when)
    assert ref == oracle_lib.format_spots(d, n, dial, *when)
    assert ref.count("\n") == (1 if n == 0 else n + 1)


# ---------------------------------------------------------------------------------------------------------------------
# main(): -t and -r (they return before the first rtlsdr call, rtlsdr_ft8d.c:1181-1195)
# ---------------------------------------------------------------------------------------------------------------------
DAEMON = ["daemon", "-f", "14074000", "-c", "K1ABC", "-l", "FN20"]


def _selftest_iq(tmp_path):
    i, q = oracle_lib.selftest_signal()
    path = str(tmp_path / "oracle_selftest.iq")
    fp = C.POINTER(C.c_float)
    assert oracle_lib.lib().ft8o_write_raw_iq(i.ctypes.data_as(fp), q.ctypes.data_as(fp), path.encode()) == NS
    with open(path, "rb") as f:
        return f.read()


def daemon_selftest(binary, tmp_path):
    wd = tmp_path / os.path.basename(binary)
    wd.mkdir()
    out = run(binary, DAEMON + ["-t"], cwd=wd).decode()
    assert out.endswith("Self-test SUCCESS!\n"), out
    assert (wd / "selftest.iq").read_bytes() == _selftest_iq(tmp_path)
    return out


def replay_files(tmp_path):
    """(path, expected stdout) for an .iq and a .c2 replay; frames with n > 0, so no wall-clock date is printed"""
    import rtlsdr_ft8d_amd as ft8
    enc = _encode_fn()
    cases = []
    for fmt, seed in (("iq", 801), ("c2", 802)):
        iq = S.make_frame(seed, 7, enc, snr_range=(-12.0, 4.0))[0]
        raw = np.empty(2 * NS, np.float32)
        raw[0::2], raw[1::2] = iq[0], -iq[1]
        path = tmp_path / f"replay.{fmt}"
        path.write_bytes((_c2_header(7074000.0) if fmt == "c2" else b"") + raw.tobytes())
        i, q = np.zeros(NS, np.float32), np.zeros(NS, np.float32)
        fp = C.POINTER(C.c_float)
        L = oracle_lib.lib()
        d = C.c_double()
        n_samples = (L.ft8o_read_c2(i.ctypes.data_as(fp), q.ctypes.data_as(fp), str(path).encode(), C.byref(d)) if fmt == "c2"
                     else L.ft8o_read_raw_iq(i.ctypes.data_as(fp), q.ctypes.data_as(fp), str(path).encode()))
        dec, n = oracle_lib.subsystem(i, q)
        assert n > 0
        # the dial frequency printed is -f's: main copies it to dec_options.freq before the file is read (:1177)
        table = oracle_lib.format_spots(dec, n, 14074000, 0, 0, 0, 0, 0)
        assert table == ft8.format_spots(dec, n, 14074000, 0, 0, 0, 0, 0)
        cases.append((path, f"Reading IQ file: {path}\nNumber of samples: {n_samples}\n" + table))
    return cases


def test_reference_daemon_selftest_and_replay(ref_oracle, tmp_path):
    out = daemon_selftest(ref_oracle, tmp_path)
    assert "K1JT   FN20" in out
    for path, expected in replay_files(tmp_path):
        assert run(ref_oracle, DAEMON + ["-r", path], cwd=tmp_path).decode() == expected


# ---------------------------------------------------------------------------------------------------------------------
# the binaries themselves
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_binaries_leave_no_device_or_network_name_to_the_dynamic_linker(ref_oracle):
    bins = [ref_oracle] + [p for p in [os.path.join(REF_OUT, "ref_gpu")] if os.path.exists(p)]
    for b in bins:
        undefined = [ln.split()[-1].split("@")[0] for ln in subprocess.check_output(["nm", "-u", b], timeout=60).decode().splitlines()
                     if ln.strip()]
        bad = [s for s in undefined if s.startswith(("curl_", "rtlsdr_")) or s in ("socket", "connect", "sendto", "send", "getaddrinfo")]
        assert not bad, (b, bad)
        assert "fftwf_execute" not in undefined                  # the shim, not a system FFTW
    for log in ("ref_oracle.log",) + (("ref_gpu.log",) if len(bins) > 1 else ()):
        with open(os.path.join(REF_OUT, log)) as f:
            assert f.read().rstrip().endswith("rc=0"), log


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the reference's unmodified ft8_subsystem over libft8gpu.so's ft8_find_sync / ft8_decode (the level-2 drop-in)
# ---------------------------------------------------------------------------------------------------------------------
def _gpu_frames():
    """72 frames of CQ and mixed traffic, including the same frame twice in a row and frames that differ from their
    predecessor in a few samples only (the reference's mag_power is a stack buffer: same address, almost the same bytes)"""
    from rtlsdr_ft8d_amd import workload
    enc = _encode_fn()
    texts, tones = workload.mixed_message_pool(256, seed=9)
    frames, names = [], []
    for k in range(24):
        frames.append(S.make_frame(900 + k, 4 + k % 9, enc, snr_range=(-16.0, 2.0))[0]); names.append(f"cq{900 + k}")
        frames.append(S.make_mixed_frame(950 + k, 3 + k % 9, (-14.0, 4.0), texts, tones)[0]); names.append(f"mixed{950 + k}")
        if k % 2 == 0:
            frames.append(frames[-1].copy()); names.append(names[-1] + "-again")
        else:
            f = frames[-1].copy()
            rng = np.random.default_rng(k)
            pos = rng.integers(0, NS, 6)
            f[0, pos] *= np.float32(-0.25)
            f[1, pos[:3]] = np.float32(0.0)
            frames.append(f); names.append(names[-1] + "-nudged")
    return names, np.stack(frames).astype(np.float32)


@pytest.mark.gpu
def test_gpu_reference_subsystem_over_the_drop_in_in_one_process(gpu_decoder, request, capsys):
    ref_gpu = _binary("ref_gpu")
    names, iq = _gpu_frames()
    B = len(names)
    assert B >= 64
    fill = 0xA5
    dec, n, ffts, _ = ref_subsystem(ref_gpu, iq, fill, timeout=600)
    assert np.all(ffts == FFTS_PER_FRAME), ffts          # the reference's own waterfall code ran for every frame
    odec, on = oracle_lib.subsystem_batch(iq, nthreads=16, decodes=_pattern(B, fill))
    gdec, gn = gpu_decoder.decode_batch(iq, decodes=_pattern(B, fill))
    for k, name in enumerate(names):
        assert n[k] == on[k] == gn[k], (name, n[k], on[k], gn[k])
        assert dec[k].tobytes() == odec[k].tobytes(), f"{name}: reference over libft8gpu.so != oracle"
        assert dec[k].tobytes() == gdec[k].tobytes(), f"{name}: reference over libft8gpu.so != ft8gpu_decode_batch"
    # the nudged frames guard against a stale candidate list only if some of them must decode differently from the
    # frame before them (same stack address, almost the same bytes, other records)
    nudged = [k for k, s in enumerate(names) if s.endswith("-nudged")]
    assert all(not np.array_equal(iq[k], iq[k - 1]) for k in nudged)
    changed = [names[k] for k in nudged if on[k] != on[k - 1] or odec[k].tobytes() != odec[k - 1].tobytes()]
    assert changed, "no nudged frame has records that differ from its predecessor's"
    assert int(n.sum()) > 100
    _report(capsys, request, f"{B} frames, {int(n.sum())} records (n_results summed) compared with the oracle and decode_batch; "
                             f"{len(changed)} of {len(nudged)} nudged frames decode differently from their predecessor")


@pytest.mark.gpu
def test_gpu_reference_daemon_modes_match_ref_oracle(tmp_path):
    ref_gpu, ref_oracle = _binary("ref_gpu"), _binary("ref_oracle")
    assert daemon_selftest(ref_gpu, tmp_path) == daemon_selftest(ref_oracle, tmp_path)
    for path, expected in replay_files(tmp_path):
        assert run(ref_gpu, DAEMON + ["-r", path], cwd=tmp_path, timeout=300).decode() == expected
        assert run(ref_oracle, DAEMON + ["-r", path], cwd=tmp_path).decode() == expected


@pytest.mark.gpu
@pytest.mark.parametrize("kind,npairs,chunk", [("signal", 751 * 3000 + 8 * 37, 65536), ("random", 751 * 48000 + 8 * 1000, 65536),
                                               ("extremes", 751 * 17 + 1, 512)])
def test_gpu_rx_decimate_equals_the_reference_callback(gpu_decoder, kind, npairs, chunk):
    ref_oracle = _binary("ref_oracle")
    raw, npairs = _rx_raw(kind, npairs, seed=20)
    ri, rq, rn = ref_rx(ref_oracle, raw, chunk)
    assert rn == min(NS, npairs // 751)
    iq = gpu_decoder.rx_decimate(raw[None, :], normalise=False)
    assert np.array_equal(_bits(iq[0, 0]), _bits(ri)), f"{kind}: I differs"
    assert np.array_equal(_bits(iq[0, 1]), _bits(rq)), f"{kind}: Q differs"
