"""cc_snapshot_info and cc_snapshot_restore_grow on CPU: the library exports them, copycat_amd/abi.py declares them, and
cc_snapshot_info -- a host call that reads a snapshot's header and makes no HIP call -- refuses what is no snapshot."""
import ctypes as C

import numpy as np
import pytest

from copycat_amd import abi
from copycat_amd.engine import Engine, EngineError, lib


def test_symbols_exported_and_declared():
    L = lib()
    for name in ("cc_snapshot_info", "cc_snapshot_restore_grow"):
        assert name in abi.SNAPSHOT_GROW_PROTOTYPES
        res, args = abi.SNAPSHOT_GROW_PROTOTYPES[name]
        f = getattr(L, name)  # (AttributeError: the library does not export it)
        assert f.restype is res and list(f.argtypes) == list(args)
    # the struct is the header's: u32 u32 u64 u32 u32 u64
    assert C.sizeof(abi.cc_snapshot_info_t) == 32
    assert [n for n, _ in abi.cc_snapshot_info_t._fields_] == ["max_resources", "max_instances", "map_capacity", "coord_cap",
                                                              "flags", "applied"]


def _info(buf, size, out=True):
    info = abi.cc_snapshot_info_t()
    p = buf.ctypes.data_as(C.c_void_p) if buf is not None else None
    rc = lib().cc_snapshot_info(p, size, C.byref(info) if out else None)
    return rc, lib().cc_last_error()


@pytest.mark.parametrize("case", ["null buffer", "null out", "10 bytes", "wrong magic"])
def test_snapshot_info_refuses(case):
    junk = np.arange(64, dtype=np.uint8)
    rc, msg = {"null buffer": lambda: _info(None, 64), "null out": lambda: _info(junk, 64, out=False),
               "10 bytes": lambda: _info(junk, 10), "wrong magic": lambda: _info(junk, 64)}[case]()
    assert rc == abi.CC_ERR_INVALID
    assert msg


def test_python_wrapper_raises_invalid():
    with pytest.raises(EngineError) as ei:
        Engine.snapshot_info(bytes(64))
    assert ei.value.rc == abi.CC_ERR_INVALID
