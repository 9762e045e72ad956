"""cc_split_device_bound / cc_split_batch_device / cc_merge_results_device (copycat_amd/csrc/split_gpu.hip) on CPU.

The workspace bound is host arithmetic, and both device calls check their arguments before the first HIP call: every
case here is refused with CC_ERR_INVALID on a machine without a GPU.  Pointer values are plain integers and are never
dereferenced (each call fails its check first)."""
import ctypes as C

import numpy as np
import pytest

from copycat_amd import abi
from copycat_amd.engine import lib

T = abi.CC_SPLIT_TILE_ROWS
A = 0x10000  # a 16-byte aligned "device address"


def _bound(n, world):
    out = C.c_uint64(0)
    rc = lib().cc_split_device_bound(n, world, C.byref(out))
    return rc, out.value


def test_bound_header_and_monotone():
    rc, b0 = _bound(0, 1)
    assert rc == abi.CC_OK and b0 > 0
    sizes = [0, 1, 63, T - 1, T, T + 1, 3 * T + 17, 100_003, 100_000_000, 1 << 33]
    worlds = [1, 2, 3, 8, 13, 64, 256]
    grid = np.zeros((len(sizes), len(worlds)), np.uint64)
    for i, n in enumerate(sizes):
        for j, w in enumerate(worlds):
            rc, grid[i, j] = _bound(n, w)
            assert rc == abi.CC_OK
    assert np.all(grid[1:] >= grid[:-1]) and np.all(grid[:, 1:] >= grid[:, :-1])
    assert grid[-1, -1] > grid[0, 0]
    # the owner byte per row and the per-tile counters fit: at least n + 12 bytes per (tile, rank)
    for i, n in enumerate(sizes):
        for j, w in enumerate(worlds):
            assert int(grid[i, j]) >= n + 12 * ((n + T - 1) // T) * w


@pytest.mark.parametrize("world", [0, 257])
def test_bound_refuses_world(world):
    assert _bound(1000, world)[0] == abi.CC_ERR_INVALID
    assert lib().cc_split_device_bound(1000, 8, None) == abi.CC_ERR_INVALID


def _split_args(n=1000, world=4):
    """a full set of acceptable arguments (fake addresses), as a dict the cases below change one item of"""
    cols = abi.cc_batch(**{name: A * (k + 1) for k, (name, _) in enumerate(abi.BATCH_COLUMNS)})
    outs = (abi.cc_batch_out * 256)()
    for r in range(256):
        for k, (name, _) in enumerate(abi.BATCH_COLUMNS):
            setattr(outs[r], name, A * 64 + 8 * (r * 16 + k))
    return {"cols": cols, "n": n, "tab": C.c_void_p(A * 32), "n_inst": 100, "world": world, "outs": outs,
            "cap": np.full(256, n, np.uint64), "counts": np.zeros(256, np.uint64), "work": C.c_void_p(A * 48),
            "work_bytes": _bound(n, min(max(world, 1), 256))[1]}


def _split(a):
    cap = a["cap"].ctypes.data_as(C.c_void_p) if a["cap"] is not None else None
    counts = a["counts"].ctypes.data_as(C.c_void_p) if a["counts"] is not None else None
    cols = C.byref(a["cols"]) if a["cols"] is not None else None
    return lib().cc_split_batch_device(cols, a["n"], a["tab"], a["n_inst"], a["world"], a["outs"], cap, counts, None,
                                       a["work"], a["work_bytes"], None)


SPLIT_CASES = {
    "world 0": lambda a: a.update(world=0),
    "world 257": lambda a: a.update(world=257),
    "null d_in": lambda a: a.update(cols=None),
    "null inst": lambda a: setattr(a["cols"], "inst", None),
    "null counts": lambda a: a.update(counts=None),
    "outs without out_cap": lambda a: a.update(cap=None),
    "misaligned inst": lambda a: setattr(a["cols"], "inst", A * 3 + 4),
    "misaligned key": lambda a: setattr(a["cols"], "key", A * 6 + 8),
    "misaligned op": lambda a: setattr(a["cols"], "op", A * 4 + 1),
    "work_bytes one short": lambda a: a.update(work_bytes=a["work_bytes"] - 1),
    "null workspace": lambda a: a.update(work=None),
    "null table": lambda a: a.update(tab=None),
}


@pytest.mark.parametrize("case", sorted(SPLIT_CASES))
def test_split_device_refuses_before_any_hip_call(case):
    a = _split_args()
    SPLIT_CASES[case](a)
    assert _split(a) == abi.CC_ERR_INVALID, case
    assert lib().cc_last_error()  # worded


def _merge_args(n=1000, world=4):
    parts = (abi.cc_results * 256)()
    for r in range(256):
        parts[r].status, parts[r].value = A * 64 + r, A * 80 + 8 * r
    return {"inst": C.c_void_p(A), "n": n, "tab": C.c_void_p(A * 32), "n_inst": 100, "world": world, "parts": parts,
            "out": abi.cc_results(A * 96, A * 97), "work": C.c_void_p(A * 48),
            "work_bytes": _bound(n, min(max(world, 1), 256))[1]}


def _merge(a):
    out = C.byref(a["out"]) if a["out"] is not None else None
    return lib().cc_merge_results_device(a["inst"], a["n"], a["tab"], a["n_inst"], a["world"], a["parts"], out,
                                         a["work"], a["work_bytes"], None)


MERGE_CASES = {
    "world 0": lambda a: a.update(world=0),
    "world 257": lambda a: a.update(world=257),
    "null inst": lambda a: a.update(inst=None),
    "null parts": lambda a: a.update(parts=None),
    "null out": lambda a: a.update(out=None),
    "null out status": lambda a: setattr(a["out"], "status", None),
    "misaligned inst": lambda a: a.update(inst=C.c_void_p(A + 4)),
    "work_bytes one short": lambda a: a.update(work_bytes=a["work_bytes"] - 1),
    "null workspace": lambda a: a.update(work=None),
    "null table": lambda a: a.update(tab=None),
}


@pytest.mark.parametrize("case", sorted(MERGE_CASES))
def test_merge_device_refuses_before_any_hip_call(case):
    a = _merge_args()
    MERGE_CASES[case](a)
    assert _merge(a) == abi.CC_ERR_INVALID, case
    assert lib().cc_last_error()


def test_empty_batch_needs_no_device():
    """n = 0 is complete without a HIP call: zero counts, CC_OK (the host call's answer)"""
    a = _split_args(n=0)
    a["counts"][:] = 7
    setattr(a["cols"], "inst", None)
    assert _split(a) == abi.CC_OK and not a["counts"][:4].any()
    m = _merge_args(n=0)
    m.update(inst=None)
    assert _merge(m) == abi.CC_OK


def test_timing_aid_is_off_and_reads_zeros_without_a_call():
    ms = (C.c_float * 3)(1.0, 1.0, 1.0)
    assert lib().cc_split_device_timing(0, ms) == abi.CC_OK and list(ms) == [0.0, 0.0, 0.0]
    assert lib().cc_split_device_timing(0, None) == abi.CC_OK


def test_python_wrappers_validate_the_owner_table():
    from copycat_amd import shard

    with pytest.raises(ValueError):
        shard._rank_table(np.full(10, 9, np.int32), 4)
    assert abi.CC_SPLIT_TILE_ROWS == T and T % 1024 == 0
