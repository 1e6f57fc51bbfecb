"""Boundary check: the UNMODIFIED reference source compiles against
this repository's drop-in headers.

`rtlsdr_ft8d.c:38-44` includes seven `./ft8_lib/ft8/*.h` headers of a git submodule that is empty in the snapshot;
`include/ft8_lib/ft8/` provides them (declaring `ft8_find_sync`, `ft8_decode`, `pack77`, `ft8_encode`, `waterfall_t`,
`candidate_t`, `message_t`, `decode_status_t`, the constants), so with `-I include` the reference's own
`ft8_subsystem()` (`:1387-1524`, call sites `:1439-1494`) builds around GPU `ft8_find_sync` / `ft8_decode`.  The
reference is not part of this repository: `make -C oracle ref` compiles it where it lies into oracle/_ref/ (the syntax
check, the header tree gcc reports and the object file checked here; nothing is copied).  The same recipe also links it,
with stand-ins for librtlsdr, libcurl and FFTW, into the programs tests/test_reference_exec.py runs.  These tests run that recipe
against the headers of this tree whenever a checkout of the reference is at hand (oracle_lib.reference_dir) and
otherwise read what build() left there; `rtl-sdr.h`, `fftw3.h` and `curl/curl.h` are absent from the image and are
replaced by declaration-only stand-ins (tests/stub_sys/README.md).  Skipped only where neither is there."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_OUT = os.path.join(ROOT, "oracle", "_ref")


@pytest.fixture(scope="module", autouse=True)
def ref_out():
    import oracle_lib
    oracle_lib.build_ref()
    if not os.path.exists(os.path.join(REF_OUT, "syntax.log")):
        pytest.skip("no checkout of the reference at hand, and oracle/_ref was not built by build() either")


def _log(name):
    """(gcc's stderr, gcc's exit status) of one `make -C oracle ref` step"""
    with open(os.path.join(REF_OUT, name)) as f:
        text = f.read()
    m = re.search(r"^rc=(\d+)\s*\Z", text, re.M)
    assert m, f"oracle/_ref/{name} has no exit status line"
    return text[:m.start()], int(m.group(1))


def test_unmodified_reference_compiles_against_the_drop_in_headers():
    stderr, rc = _log("syntax.log")
    assert rc == 0, stderr
    assert "error" not in stderr
    # no name of the hot path may be used without a declaration, and no struct may be passed as another type
    assert not re.search(r"implicit declaration|incompatible pointer|has no member|unknown type|undeclared", stderr), stderr


def test_the_ft8_lib_names_resolve_to_our_headers_not_to_anything_else():
    """the seven ft8_lib includes of the reference must come from include/ft8_lib/ft8/ (gcc -H lists every header;
    the recipe runs gcc from the repository root, so ours are named by their repository-relative path)"""
    stderr, rc = _log("headers.log")
    assert rc == 0, stderr
    ours = os.path.join("include", "ft8_lib", "ft8")
    seen = {os.path.basename(m.group(1)) for m in re.finditer(r"^\.+ (\S+)$", stderr, re.M)
            if os.path.normpath(os.path.dirname(m.group(1))) == ours}
    assert seen >= {"constants.h", "pack.h", "unpack.h", "ldpc.h", "crc.h", "decode.h", "encode.h"}, seen


def test_every_hot_path_symbol_the_reference_calls_is_exported():
    """what the compiled reference needs at link time from the ft8_lib side is in libft8gpu.so"""
    lib = os.path.join(ROOT, "rtlsdr_ft8d_amd", "libft8gpu.so")
    obj = os.path.join(REF_OUT, "rtlsdr_ft8d.o")
    stderr, rc = _log("object.log")
    assert rc == 0 and os.path.exists(obj), stderr
    sym = subprocess.check_output(["nm", "-D", "--defined-only", lib]).decode()
    exported = {ln.split()[-1] for ln in sym.splitlines() if ln.strip()}
    needs = {ln.split()[-1] for ln in subprocess.check_output(["nm", "--undefined-only", obj]).decode().splitlines() if ln.strip()}
    defines = {ln.split()[-1] for ln in subprocess.check_output(["nm", "--defined-only", obj]).decode().splitlines() if ln.strip()}
    for name in ("ft8_find_sync", "ft8_decode", "pack77", "ft8_encode"):
        assert name in needs, name                # the reference really calls it (rtlsdr_ft8d.c:1450, :1476, :927, :934)
        assert name in exported, name
    for name in ("ft8_subsystem", "initFFTW", "freeFFTW"):            # the subsystem-level drop-in (rtlsdr_ft8d.h:155-156, :164)
        assert name in defines, name
        assert name in exported, name
