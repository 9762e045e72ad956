"""cc_evpack_pack / cc_evpack_check / cc_evpack_unpack (copycat_amd/csrc/evpack.cpp) under AddressSanitizer +
UndefinedBehaviorSanitizer, host only.

An event blob crosses a process boundary (the engine's host hands it to a JVM, a file or a socket), so a consumer treats
it as untrusted input, and cc_evpack_check is the one gate in front of the decoder.  tests/fuzz/evpack_fuzz.cpp (a
stand-alone program) packs random event columns and checks the round trip, then feeds the validator and the decoder
100,000 mutated blobs (byte flips, boundary values, truncations, spliced directory entries, payload tables whose entry
count or pos bytes changed), each from an exact-size heap copy with exact-size output columns: any overread, overwrite,
leak or undefined behaviour aborts the run; every input must come back CC_OK or CC_ERR_INVALID."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_evpack_asan_ubsan_fuzz(tmp_path):
    exe = tmp_path / "evpack_fuzz"
    cmd = [HIPCC, "-std=c++17", "-g", "-O1", "-pthread", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
           "-fno-sanitize-recover=all", f"{ROOT}/copycat_amd/csrc/evpack.cpp", f"{HERE}/fuzz/evpack_fuzz.cpp", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), "100000", "1"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert "checked 100000 mutated blobs" in r.stdout
    shutil.rmtree(tmp_path, ignore_errors=True)
