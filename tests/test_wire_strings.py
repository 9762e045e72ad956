"""The parser the GPU wire decoder runs with a String dictionary (copycat_amd/csrc/wire_plain.h wire_parse over a
DictView) against the host decoder (wire.cpp decode_one), host only, under AddressSanitizer + UndefinedBehaviorSanitizer.

tests/fuzz/wire_str_fuzz.cpp is a stand-alone program (its own main, nothing preloaded) built from wire.cpp, which holds
the host mirror of the dictionary, and the shared header.  It runs the shared parser over the mirror's image: the
fixture with its Strings interned, every truncation of it, 200,000 seeded mutations under random codecs and a generator
that writes Strings from a pool (interned, not interned, too long, null; prefixes of each other, bytes >= 0x80, NULs).
Conservative on every input, complete where the generator knows the dictionary holds every String, at least a quarter
of the unmutated generated entries of that kind, and a dictionary grown from 0 to 5,000 Strings resolves each one.
The second build cuts the dictionary hash to 4 bits (-DCC_WIRE_DICT_WEAK_HASH): every property holds unchanged, which
is the byte compare's doing."""
import json
import os
import re
import struct
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("define", [None, "CC_WIRE_DICT_WEAK_HASH"], ids=["hash64", "hash4"])
def test_dictionary_parser_matches_decode_one_asan_ubsan(tmp_path, define):
    exe = tmp_path / "wire_str_fuzz"
    cmd = [HIPCC, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
           "-fno-sanitize-recover=all", f"-I{ROOT}/copycat_amd/csrc", f"-I{ROOT}/include"] + \
          ([f"-D{define}"] if define else []) + \
          [f"{ROOT}/copycat_amd/csrc/wire.cpp", f"{HERE}/fuzz/wire_str_fuzz.cpp", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(os.path.join(HERE, "golden", "wire_fixture.json")) as f:
        meta = json.load(f)
    (tmp_path / "offs.txt").write_text(" ".join(map(str, meta["offsets"])))
    with open(tmp_path / "strs.bin", "wb") as f:
        for s in meta["strings"]:
            b = s.encode()
            f.write(struct.pack("<I", len(b)) + b)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), os.path.join(HERE, "golden", "wire_fixture.bin"), str(tmp_path / "offs.txt"),
                        str(tmp_path / "strs.bin"), "200000"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    out = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", r.stdout)}
    assert "growth=ok" in r.stdout, r.stdout
    # complete on the fixture: every resource operation resolves, the String-carrying ones among them
    handle = lambda fl: (fl & 7) == 4 or ((fl >> 3) & 7) == 4 or (fl >> 6) == 3  # noqa: E731
    ops = [row for row in meta["rows"] if row["kind"] == 0]
    with_str = sum(1 for row in ops if handle(row["flags"]))
    assert with_str > 5 and len(ops) > 40
    assert out["fixture_resolved"] == len(ops) and out["fixture_with_string"] == with_str, r.stdout
    # the generator's share (the program fails by itself when it falls short), and both answers under mutation
    assert 4 * out["sure_with_string"] >= out["unmutated_generated"] > 20000, r.stdout
    assert out["mutated_resolved"] > 1000 and out["escaped"] > 10000 and out["dict_long"] > 0, r.stdout
