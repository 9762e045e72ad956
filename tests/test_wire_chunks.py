"""The chunk planner of cc_apply_wire_host_packed (copycat_amd/csrc/wire.cpp wire_plan_chunks), host only, under
AddressSanitizer + UndefinedBehaviorSanitizer.

tests/fuzz/wire_chunk_fuzz.cpp is a stand-alone program (its own main, nothing preloaded) linked with wire.cpp.  Over
seeded random offset arrays (decreasing, past-the-end, garbage and huge-entry ones included) the plan must cut whole
blocks, cover [0, n) once and in order, keep every chunk's copied span under the cap unless the chunk is a single
block, and its end-offset check must agree with a full scan about whether the chunk's copy stays inside the buffer."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_chunk_planner_properties_asan_ubsan(tmp_path):
    exe = tmp_path / "wire_chunk_fuzz"
    cmd = [HIPCC, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
           "-fno-sanitize-recover=all", f"-I{ROOT}/copycat_amd/csrc", f"-I{ROOT}/include",
           f"{ROOT}/copycat_amd/csrc/wire.cpp", f"{HERE}/fuzz/wire_chunk_fuzz.cpp", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), "3000"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    m = re.search(r"cases=(\d+) bad_cases=(\d+) chunks=(\d+) capped=(\d+) single_over=(\d+) not_ok=(\d+)", r.stdout)
    assert m, r.stdout
    cases, bad, chunks, capped, single_over, not_ok = map(int, m.groups())
    # the cases exercise every answer: clean and violated arrays, chunks shortened by the cap, single blocks over it,
    # chunks that fail the end-offset check
    assert cases == 3000 and 500 < bad < 2500 and chunks > 2 * cases, r.stdout
    assert capped > 500 and single_over > 20 and not_ok > 100, r.stdout
    shutil.rmtree(tmp_path, ignore_errors=True)
