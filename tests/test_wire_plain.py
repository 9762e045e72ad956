"""The parser the GPU wire decoder runs (copycat_amd/csrc/wire_plain.h wire_plain_parse) against the host decoder
(wire.cpp decode_one), host only, under AddressSanitizer + UndefinedBehaviorSanitizer.

tests/fuzz/wire_plain_fuzz.cpp is a stand-alone program (its own main, nothing preloaded) built from wire.cpp and the
shared header.  Over the committed fixture, every truncation of every fixture entry and 200,000 seeded mutations under
random codec parameters, the shared parser must either escape or return exactly decode_one's columns with CC_OK, and
never read outside an exact-size heap copy of the entry.  Every fixture row that carries no String and is no manager
entry must come back plain, so a parser that escapes everything fails."""
import json
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
TAG_HANDLE = 4


def fixture_plain_rows(rows):
    """fixture rows the GPU decodes: resource operations (kind 0) with no HANDLE tag on a, b or the key"""
    return [i for i, r in enumerate(rows)
            if r["kind"] == 0 and (r["flags"] & 7) != TAG_HANDLE and ((r["flags"] >> 3) & 7) != TAG_HANDLE
            and (r["flags"] >> 6) != 3]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_plain_parser_matches_decode_one_asan_ubsan(tmp_path):
    exe = tmp_path / "wire_plain_fuzz"
    cmd = [HIPCC, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
           "-fno-sanitize-recover=all", f"-I{ROOT}/copycat_amd/csrc", f"-I{ROOT}/include",
           f"{ROOT}/copycat_amd/csrc/wire.cpp", f"{HERE}/fuzz/wire_plain_fuzz.cpp", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(os.path.join(HERE, "golden", "wire_fixture.json")) as f:
        meta = json.load(f)
    (tmp_path / "offs.txt").write_text(" ".join(map(str, meta["offsets"])))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), os.path.join(HERE, "golden", "wire_fixture.bin"), str(tmp_path / "offs.txt"),
                        "200000"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    m = re.search(r"fixture_plain=(\d+) plain=(\d+) escaped=(\d+) .* mutated_plain=(\d+)", r.stdout)
    assert m, r.stdout
    want = len(fixture_plain_rows(meta["rows"]))
    assert want > 20 and int(m.group(1)) == want, (r.stdout, want)
    # the mutations exercise both answers: many plain rows under random codecs, many escapes
    assert int(m.group(4)) > 10000 and int(m.group(3)) > 10000, r.stdout
    shutil.rmtree(tmp_path, ignore_errors=True)
