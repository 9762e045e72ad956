"""The ABI 6 boundary on CPU: cc_apply_batch_prefix (the prefix apply on device-resident columns) is declared in the
header, exported by the built library and bound with explicit argtypes, and the ABI version is 6 on both sides.

No compute call is made here: the library is loaded and its symbol table read."""
import ctypes as C
import re
import subprocess

from copycat_amd import abi
from tests.test_abi import HEADER, header_defines, header_functions

NAME = "cc_apply_batch_prefix"


def test_header_declares_the_device_prefix_apply():
    assert NAME in header_functions()
    txt = re.sub(r"\s+", " ", open(HEADER).read())
    m = re.search(r"int " + NAME + r"\(([^)]*)\)", txt)
    assert m, "no prototype"
    args = [a.strip() for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["e", "d_cols", "n", "d_out", "d_events", "stream", "h_applied"]
    assert args[2].startswith("uint64_t") and args[5].startswith("void*") and args[6].startswith("uint64_t*")


def test_library_exports_the_device_prefix_apply():
    from copycat_amd import build

    so = build.build_engine()
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T " + NAME + r"$", syms, re.M), f"{NAME} is not exported"


def test_engine_binds_the_device_prefix_apply():
    import copycat_amd.engine as eng

    f = getattr(eng.lib(), NAME)
    P, u64 = C.c_void_p, C.c_uint64
    assert f.restype is C.c_int
    assert f.argtypes is not None and list(f.argtypes) == [P, P, u64, P, P, P, P]
    assert callable(getattr(eng.Engine, "apply_prefix", None))


def test_abi_version_is_6_on_both_sides():
    assert abi.CC_ABI_VERSION == 6
    assert header_defines()["CC_ABI_VERSION"] == abi.CC_ABI_VERSION
