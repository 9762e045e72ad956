"""cc_merge_events (copycat_amd/csrc/evmerge.cpp) and the argument checks of cc_merge_events_device on CPU.

The host call is compared byte for byte with the independent numpy reference of tests/evmerge_cases.py over the whole
case grid; every precondition and capacity case is refused with its code, with the sentinel-filled outputs untouched.
The device call's workspace bound is host arithmetic and its argument checks run before the first HIP call: those
cases use fake addresses that are never dereferenced (as tests/test_split_device_abi.py)."""
import ctypes as C

import numpy as np
import pytest

from copycat_amd import abi, shard
from copycat_amd.engine import lib
from tests import evmerge_cases as ec

T = ec.T


def _check_case(case, threads):
    rc, total, out, ocnt = ec.host_merge(lib(), case.parts, case.rows, case.row_counts, case.n, threads)
    assert rc == abi.CC_OK, lib().cc_last_error()
    assert total == case.total == ocnt
    assert ec.equal_columns(out, case.ref, total)
    assert ec.untouched(out, total)


@pytest.mark.parametrize("world", ec.WORLDS)
@pytest.mark.parametrize("events", ec.EVENTS)
def test_host_merge_equals_reference(events, world):
    for n in ec.SIZES:
        for owner in ec.OWNERS:
            case = ec.build(n, world, owner, events, seed=n + world)
            for threads in (1, 16):
                _check_case(case, threads)


def test_pos_is_non_decreasing_and_runs_keep_their_order():
    case = ec.build(3 * T + 17, 8, "random", "mixed", seed=3)
    rc, total, out, _ = ec.host_merge(lib(), case.parts, case.rows, case.row_counts, case.n, 16)
    assert rc == abi.CC_OK and total > 3 * T
    assert np.all(np.diff(out["pos"][:total].astype(np.int64)) >= 0)


def test_python_wrapper():
    case = ec.build(T + 1, 3, "random", "mixed", seed=4)
    got = shard.merge_events(case.parts, case.rows, case.n, threads=2)
    assert got["count"] == case.total and ec.equal_columns(got, case.ref, case.total)


# ---- refusals ----------------------------------------------------------------------------------------------------------
def _base():
    return ec.build(T + 65, 3, "random", "mixed", seed=11)


def _refused(case, want, parts=None, rows=None, row_counts=None, n=None, total=None, **kw):
    for threads in (1, 16):
        rc, tot, out, ocnt = ec.host_merge(lib(), parts or case.parts, rows or case.rows,
                                           case.row_counts if row_counts is None else row_counts,
                                           case.n if n is None else n, threads, **kw)
        assert rc == want, (rc, lib().cc_last_error())
        assert ec.untouched(out) and ocnt == 0x7777
        if total is not None:
            assert tot == total
    return lib().cc_last_error().decode()


def _with(case, r, name, j, value):
    parts = [dict(p) for p in case.parts]
    parts[r][name] = parts[r][name].copy()
    parts[r][name][j] = value
    return parts


def test_refuses_pos_decreasing_at_one_event():
    case = _base()
    j = len(case.parts[1]["pos"]) // 2
    assert case.parts[1]["pos"][j] > 0
    msg = _refused(case, abi.CC_ERR_INVALID, parts=_with(case, 1, "pos", j, case.parts[1]["pos"][j - 1] - 1))
    assert "rank 1" in msg and f"event {j}" in msg


def test_refuses_pos_equal_to_row_count():
    case = _base()
    last = len(case.parts[2]["pos"]) - 1
    msg = _refused(case, abi.CC_ERR_INVALID, parts=_with(case, 2, "pos", last, int(case.row_counts[2])))
    assert "rank 2" in msg and f"event {last}" in msg


def test_refuses_session_close_stream():
    """a cc_sessions_close / cc_advance_time_events stream: pos = 0xFFFFFFFF is no row of the share"""
    case = _base()
    parts = [dict(p) for p in case.parts]
    parts[0]["pos"] = np.full_like(parts[0]["pos"], 0xFFFFFFFF)
    assert "rank 0, event 0" in _refused(case, abi.CC_ERR_INVALID, parts=parts)


def test_refuses_rows_value_equal_to_n():
    case = _base()
    rows = [x.copy() for x in case.rows]
    p = int(case.parts[1]["pos"][-1])
    rows[1][p] = case.n
    assert "rank 1" in _refused(case, abi.CC_ERR_INVALID, rows=rows)


def test_refuses_a_log_row_claimed_twice():
    case = _base()
    rows = [x.copy() for x in case.rows]
    a, b = int(case.parts[0]["pos"][0]), int(case.parts[0]["pos"][-1])
    assert a != b
    rows[0][a] = rows[0][b]  # (not increasing, and two runs on one log row)
    _refused(case, abi.CC_ERR_INVALID, rows=rows)


def test_refuses_part_count_above_capacity_with_total():
    case = _base()
    caps = [len(p["pos"]) for p in case.parts]
    counts = list(caps)
    counts[1] += 5  # that rank's apply had overflowed
    _refused(case, abi.CC_ERR_CAPACITY, capacities=caps, counts=counts, total=case.total + 5)


def test_refuses_output_one_event_short_with_total():
    case = _base()
    _refused(case, abi.CC_ERR_CAPACITY, out_capacity=case.total - 1, total=case.total)


@pytest.mark.parametrize("world", [0, 257])
def test_refuses_world(world):
    case = ec.build(64, 1, "round_robin", "one_per_row")
    pr, rowp, keep = ec.host_structs(case.parts, case.rows)
    out = ec.sentinel_columns(64)
    o = abi.cc_events(*[out[c].ctypes.data for c in ec.COLS], 64, None)
    tot = C.c_uint64()
    rcs = np.zeros(257, np.uint64)
    assert lib().cc_merge_events(pr, rowp, rcs.ctypes.data, 64, world, 1, C.byref(o), C.byref(tot)) == abi.CC_ERR_INVALID
    assert ec.untouched(out)
    assert lib().cc_merge_events(pr, rowp, rcs.ctypes.data, 1 << 32, 1, 1, C.byref(o), C.byref(tot)) == abi.CC_ERR_INVALID
    assert lib().cc_merge_events(None, rowp, rcs.ctypes.data, 64, 1, 1, C.byref(o), C.byref(tot)) == abi.CC_ERR_INVALID


def test_empty_log_and_rank_without_rows():
    rc, total, out, ocnt = ec.host_merge(lib(), [{c: np.zeros(0, ec.DT[c]) for c in ec.COLS}], [np.zeros(0, np.uint64)],
                                         [0], 0)
    assert rc == abi.CC_OK and total == 0 and ocnt == 0 and ec.untouched(out)
    case = ec.build(65, 8, "one_rank", "mixed", seed=2)  # ranks 0..6: no rows, NULL columns, NULL row ids
    assert all(len(case.rows[r]) == 0 for r in range(7))
    _check_case(case, 16)


# ---- the device call's bound and argument checks (no GPU) ----------------------------------------------------------------
A = 0x10000  # an aligned "device address"


def _bound(n, world):
    out = C.c_uint64(0)
    return lib().cc_merge_events_device_bound(n, world, C.byref(out)), out.value


def test_bound_is_monotone():
    sizes = [0, 1, 63, T - 1, T, T + 1, 3 * T + 17, 100_003, 100_000_000, (1 << 32) - 1]
    worlds = [1, 2, 3, 8, 13, 64, 256]
    grid = np.zeros((len(sizes), len(worlds)), np.uint64)
    for i, n in enumerate(sizes):
        for j, w in enumerate(worlds):
            rc, grid[i, j] = _bound(n, w)
            assert rc == abi.CC_OK
            assert int(grid[i, j]) >= 12 * n + 16 * ((n + T - 1) // T)  # a record and an end per row; two words per tile
    assert np.all(grid[1:] >= grid[:-1]) and np.all(grid[:, 1:] >= grid[:, :-1]) and grid[-1, -1] > grid[0, 0]
    assert _bound(10, 0)[0] == _bound(10, 257)[0] == _bound(1 << 32, 1)[0] == abi.CC_ERR_INVALID
    assert lib().cc_merge_events_device_bound(10, 1, None) == abi.CC_ERR_INVALID


def _dev_args(n=1000, world=4):
    parts = (abi.cc_events * 256)()
    rows = (C.c_void_p * 256)()
    for r in range(256):
        parts[r] = abi.cc_events(*[A * (8 * r + k + 1) for k in range(6)], 100, A * (8 * r + 7))
        rows[r] = A * (8 * r + 8)
    out = abi.cc_events(*[A * 4096 + A * k for k in range(6)], 1000, A * 5000)
    return {"parts": parts, "rows": rows, "row_counts": np.full(256, n // max(world, 1), np.uint64), "n": n, "world": world,
            "out": out, "total": C.c_uint64(0x7777), "work": C.c_void_p(A * 6000),
            "work_bytes": _bound(n, min(max(world, 1), 256))[1]}


def _dev(a):
    out = C.byref(a["out"]) if a["out"] is not None else None
    tot = C.byref(a["total"]) if a["total"] is not None else None
    rcs = a["row_counts"].ctypes.data_as(C.c_void_p) if a["row_counts"] is not None else None
    return lib().cc_merge_events_device(a["parts"], a["rows"], rcs, a["n"], a["world"], out, tot, a["work"],
                                        a["work_bytes"], None)


DEV_CASES = {
    "world 0": lambda a: a.update(world=0),
    "world 257": lambda a: a.update(world=257),
    "n 2^32": lambda a: a.update(n=1 << 32),
    "null parts": lambda a: a.update(parts=None),
    "null rows": lambda a: a.update(rows=None),
    "null row_counts": lambda a: a.update(row_counts=None),
    "null out": lambda a: a.update(out=None),
    "null total": lambda a: a.update(total=None),
    "null out column": lambda a: setattr(a["out"], "tag", None),
    "null workspace": lambda a: a.update(work=None),
    "misaligned workspace": lambda a: a.update(work=C.c_void_p(A * 6000 + 8)),
    "work_bytes one short": lambda a: a.update(work_bytes=a["work_bytes"] - 1),
    "misaligned part pos": lambda a: setattr(a["parts"][1], "pos", A + 2),
    "misaligned part payload": lambda a: setattr(a["parts"][3], "payload", A + 4),
    "misaligned part count": lambda a: setattr(a["parts"][0], "count", A + 4),
    "misaligned out target": lambda a: setattr(a["out"], "target", A + 1),
    "misaligned rows": lambda a: a["rows"].__setitem__(2, A + 4),
    "row count above n": lambda a: a["row_counts"].__setitem__(0, a["n"] + 1),
}


@pytest.mark.parametrize("case", sorted(DEV_CASES))
def test_device_call_refuses_before_any_hip_call(case):
    a = _dev_args()
    DEV_CASES[case](a)
    assert _dev(a) == abi.CC_ERR_INVALID, case
    assert lib().cc_last_error()


def test_device_call_with_nothing_to_do_needs_no_device():
    a = _dev_args(n=0)
    assert _dev(a) == abi.CC_OK and a["total"].value == 0
    a = _dev_args()
    for r in range(256):
        a["parts"][r] = abi.cc_events()  # all-NULL empty parts
        a["rows"][r] = None
    assert _dev(a) == abi.CC_OK and a["total"].value == 0


def test_timing_aid_is_off_and_reads_zeros_without_a_call():
    ms = (C.c_float * 4)(1.0, 1.0, 1.0, 1.0)
    assert lib().cc_merge_events_device_timing(0, ms) == abi.CC_OK and list(ms) == [0.0] * 4


def test_constants():
    assert abi.CC_EVMERGE_TILE_ROWS == T and T % abi.CC_EVMERGE_WINDOW_EVENTS == 0
