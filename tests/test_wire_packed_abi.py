"""cc_apply_wire_host_packed / cc_wire_packed_timeline on CPU: the header, the exported symbols and abi.py agree.

No compute call is made (no GPU needed): the library is loaded, its symbol table read, and the calls that return
before they touch a device (argument checks) are made."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from copycat_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "copycat_apply.h")
CTYPE = {"const uint8_t*": C.c_void_p, "const uint64_t*": C.c_void_p, "const void*": C.c_void_p, "uint64_t": C.c_uint64}


def test_abi_version_is_unchanged():
    assert abi.CC_ABI_VERSION == 6


def test_wire_segment_layout_matches_header():
    hdr = open(HEADER).read()
    body = hdr[hdr.index("typedef struct cc_wire_segment {"):hdr.index("} cc_wire_segment;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"((?:const\s+)?\w+\*?)\s+(\w+);", body)
    assert [f[1] for f in fields] == ["buf", "buf_len", "offsets", "n", "aux_blob", "aux_bytes"]
    assert [name for name, _ in abi.cc_wire_segment._fields_] == [f[1] for f in fields]
    for (ctype, name), (_, py) in zip(fields, abi.cc_wire_segment._fields_):
        assert CTYPE[re.sub(r"\s+", " ", ctype)] is py, name
    assert C.sizeof(abi.cc_wire_segment) == 48
    assert [getattr(abi.cc_wire_segment, n).offset for n, _ in abi.cc_wire_segment._fields_] == [0, 8, 16, 24, 32, 40]


def test_symbols_exported_and_bound():
    from copycat_amd import build
    import copycat_amd.engine as eng

    so = build.build_engine()
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (cc_[a-z_0-9]+)$", syms, re.M))
    assert {"cc_apply_wire_host_packed", "cc_wire_packed_timeline"} <= exported
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    L = eng.lib()
    for name in ("cc_apply_wire_host_packed", "cc_wire_packed_timeline"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        fn = getattr(L, name)
        assert fn.restype is C.c_int and fn.argtypes is not None and len(fn.argtypes) == len(params), name
        for p, t in zip(params, fn.argtypes):  # a pointer is a pointer, a uint64_t a uint64_t
            assert (t is C.c_uint64) == (re.match(r"uint64_t\s+\w+$", p) is not None), (name, p, t)
            assert (t is C.c_void_p) == ("*" in p), (name, p, t)


def test_null_arguments_are_refused_before_any_device_call():
    import copycat_amd.engine as eng

    L = eng.lib()
    done, size = C.c_uint64(7), C.c_uint64()
    ctl = abi.cc_wire_control()
    res = np.zeros(256, np.uint8)
    rc = L.cc_apply_wire_host_packed(None, None, None, None, res.ctypes.data, res.nbytes, C.byref(size), None, 0, 0, None,
                                     None, None, C.byref(done), C.byref(ctl), None)
    assert rc == abi.CC_ERR_INVALID and done.value == 0
    n = C.c_uint64()
    assert L.cc_wire_packed_timeline(None, 0, C.byref(n), None) == abi.CC_ERR_INVALID
