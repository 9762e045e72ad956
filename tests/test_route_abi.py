"""cc_route_events (copycat_amd/csrc/route.cpp) and the argument checks of cc_route_events_device on CPU.

The host call is compared byte for byte with the independent numpy reference of tests/route_cases.py over the whole
case grid, with 1 and 16 threads; every refusal returns its code, names the offending event, and leaves the
sentinel-filled outputs untouched.  The device call's workspace bound is host arithmetic and its argument checks run
before the first HIP call: those cases use fake addresses that are never dereferenced (as tests/test_split_device_abi.py)."""
import ctypes as C

import numpy as np
import pytest

from copycat_amd import abi, route
from copycat_amd.engine import lib
from tests import route_cases as rc_

T, D = rc_.T, rc_.D


@pytest.mark.parametrize("pattern", rc_.DISTRIBUTIONS)
def test_host_route_equals_reference(pattern):
    for case in rc_.grid(pattern):
        for threads in (1, 16):
            rc, active, out = rc_.host_route(lib(), case, threads)
            assert rc == abi.CC_OK, lib().cc_last_error()
            assert active == case.n_active, (case.n, case.n_sessions)
            assert out.equals(case), (case.n, case.n_sessions, threads)


def test_many_threads_on_a_long_stream():
    """enough events that 16 workers each own a slice (a worker takes at least 16 Ki events)"""
    case = rc_.build(16 * 16384 + 1234, D * D + 1, "zipf", seed=5)
    rc, active, out = rc_.host_route(lib(), case, 16)
    assert rc == abi.CC_OK and active == case.n_active and out.equals(case)


def test_runs_are_contiguous_and_keep_input_order():
    case = rc_.build(3 * T + 17, D + 1, "uniform", seed=3)
    rc, active, out = rc_.host_route(lib(), case, 16)
    assert rc == abi.CC_OK
    key = case.session_of_inst[out.cols["target"][:case.n]]
    assert np.all(np.diff(key.astype(np.int64)) >= 0)
    for k in range(active):
        lo, hi = int(out.start[k]), int(out.start[k + 1])
        assert lo < hi and np.all(key[lo:hi] == out.session[k])
        mine = np.nonzero(case.session_of_inst[case.ev["target"]] == out.session[k])[0]
        assert np.array_equal(out.cols["payload"][lo:hi], case.ev["payload"][mine])


def test_without_instance_ids():
    case = rc_.build(T + 65, D + 1, "uniform", seed=4)
    rc, active, out = rc_.host_route(lib(), case, 2, with_ids=False)
    assert rc == abi.CC_OK and active == case.n_active and out.equals(case, with_ids=False)


def test_python_wrapper():
    case = rc_.build(T + 1, D * D, "zipf", seed=4)
    got, inst, (session, start) = route.route_events(case.ev, case.session_of_inst, case.n_sessions, case.id_of_inst, threads=2)
    assert got["count"] == case.n and all(np.array_equal(got[c], case.ref[c]) for c in rc_.COLS)
    assert np.array_equal(inst, case.ref_inst)
    assert np.array_equal(session, case.ref_session) and np.array_equal(start, case.ref_start)
    got, inst, (session, start) = route.route_events(case.ev, case.session_of_inst, case.n_sessions)
    assert inst is None and np.array_equal(got["payload"], case.ref["payload"])
    empty = {c: np.zeros(0, rc_.DT[c]) for c in rc_.COLS}
    got, inst, (session, start) = route.route_events(empty, case.session_of_inst, case.n_sessions)
    assert got["count"] == 0 and len(session) == 0 and start.tolist() == [0]


# ---- refusals ----------------------------------------------------------------------------------------------------------
def _base():
    return rc_.build(T + 65, D + 1, "uniform", seed=11)


def _refused(case, want, active=rc_.COUNT_SENTINEL, **kw):
    for threads in (1, 16):
        rc, act, out = rc_.host_route(lib(), case, threads, **kw)
        assert rc == want, (rc, lib().cc_last_error())
        assert out.untouched() and act == active
    return lib().cc_last_error().decode()


def _with_target(case, events, value):
    ev = dict(case.ev)
    ev["target"] = ev["target"].copy()
    ev["target"][list(events)] = value
    return ev


def test_refuses_target_equal_to_n_inst_and_names_the_lowest_event():
    case = _base()
    msg = _refused(case, abi.CC_ERR_INVALID, ev=_with_target(case, (case.n - 1, 77, 3000), case.n_inst))
    assert "event 77:" in msg and "target" in msg
    assert "event 0:" in _refused(case, abi.CC_ERR_INVALID, ev=_with_target(case, (0,), 0xFFFFFFFF))
    assert f"event {case.n - 1}:" in _refused(case, abi.CC_ERR_INVALID, ev=_with_target(case, (case.n - 1,), case.n_inst))


def test_refuses_table_entry_equal_to_n_sessions():
    case = _base()
    tab = case.session_of_inst.copy()
    slot = int(case.ev["target"][500])
    tab[slot] = case.n_sessions
    first = int(np.nonzero(case.ev["target"] == slot)[0][0])
    msg = _refused(case, abi.CC_ERR_INVALID, session_of_inst=tab)
    assert f"event {first}:" in msg and "session_of_inst" in msg
    # an entry no event names is not looked at
    unused = np.setdiff1d(np.arange(case.n_inst), case.ev["target"])
    tab = case.session_of_inst.copy()
    tab[unused] = 0xFFFFFFFF
    rc, active, out = rc_.host_route(lib(), case, 16, session_of_inst=tab)
    assert rc == abi.CC_OK and out.equals(case)


def test_the_lowest_event_wins_between_the_two_kinds():
    case = _base()
    tab = case.session_of_inst.copy()
    slot = int(case.ev["target"][40])
    tab[slot] = case.n_sessions + 5
    first = int(np.nonzero(case.ev["target"] == slot)[0][0])
    ev = _with_target(case, (first + 1,), case.n_inst + 1)
    assert f"event {first}:" in _refused(case, abi.CC_ERR_INVALID, ev=ev, session_of_inst=tab)


def test_refuses_no_sessions_and_too_many_events():
    case = _base()
    _refused(case, abi.CC_ERR_INVALID, n_sessions=0)
    i_s = abi.cc_events(*[rc_._p(case.ev[c]) for c in rc_.COLS], 0, None)
    out = rc_.Outputs(8, 8)
    o_s = abi.cc_events(*[rc_._p(out.cols[c]) for c in rc_.COLS], 1 << 33, rc_._p(out.count))
    d_s = abi.cc_route_dir(rc_._p(out.session), rc_._p(out.start), 8, rc_._p(out.dir_count))
    act = C.c_uint64(rc_.COUNT_SENTINEL)
    args = (rc_._p(case.session_of_inst), rc_._p(case.id_of_inst), case.n_inst, case.n_sessions, 1, C.byref(o_s),
            rc_._p(out.inst), C.byref(d_s), C.byref(act))
    assert lib().cc_route_events(C.byref(i_s), 1 << 32, *args) == abi.CC_ERR_INVALID
    assert out.untouched() and act.value == rc_.COUNT_SENTINEL


def test_capacity_of_out_and_of_the_directory():
    case = _base()
    assert "output" in _refused(case, abi.CC_ERR_CAPACITY, out_capacity=case.n - 1)
    assert case.n_active > 2
    assert "directory" in _refused(case, abi.CC_ERR_CAPACITY, active=case.n_active, dir_capacity=case.n_active - 1)
    _refused(case, abi.CC_ERR_CAPACITY, active=case.n_active, dir_capacity=0)
    rc, active, out = rc_.host_route(lib(), case, 16, dir_capacity=case.n_active, out_capacity=case.n)
    assert rc == abi.CC_OK and out.equals(case)  # exactly enough of both


def _structs(case, out):
    i_s = abi.cc_events(*[rc_._p(case.ev[c]) for c in rc_.COLS], case.n, None)
    o_s = abi.cc_events(*[rc_._p(out.cols[c]) for c in rc_.COLS], out.capacity, rc_._p(out.count))
    d_s = abi.cc_route_dir(rc_._p(out.session), rc_._p(out.start), out.dir_capacity, rc_._p(out.dir_count))
    return i_s, o_s, d_s


HOST_CASES = {
    "null in": lambda a: a.update(i=None),
    "null out": lambda a: a.update(o=None),
    "null dir": lambda a: a.update(d=None),
    "null n_active": lambda a: a.update(act=None),
    "null table": lambda a: a.update(tab=None),
    "null input column": lambda a: setattr(a["i"], "tag", None),
    "null output column": lambda a: setattr(a["o"], "payload", None),
    "null dir session": lambda a: setattr(a["d"], "session", None),
    "null dir start": lambda a: setattr(a["d"], "start", None),
    "null dir count": lambda a: setattr(a["d"], "count", None),
    "ids without out_instance": lambda a: a.update(inst=None),
    "out_instance without ids": lambda a: a.update(ids=None),
    "misaligned in pos": lambda a: setattr(a["i"], "pos", a["i"].pos + 2),
    "misaligned in target": lambda a: setattr(a["i"], "target", a["i"].target + 1),
    "misaligned in payload": lambda a: setattr(a["i"], "payload", a["i"].payload + 4),
    "misaligned out pos": lambda a: setattr(a["o"], "pos", a["o"].pos + 2),
    "misaligned out payload": lambda a: setattr(a["o"], "payload", a["o"].payload + 4),
    "misaligned out count": lambda a: setattr(a["o"], "count", a["o"].count + 4),
    "misaligned table": lambda a: a.update(tab=C.c_void_p(a["tab"].value + 2)),
    "misaligned ids": lambda a: a.update(ids=C.c_void_p(a["ids"].value + 4)),
    "misaligned out_instance": lambda a: a.update(inst=C.c_void_p(a["inst"].value + 4)),
    "misaligned dir session": lambda a: setattr(a["d"], "session", a["d"].session + 2),
    "misaligned dir start": lambda a: setattr(a["d"], "start", a["d"].start + 1),
    "misaligned dir count": lambda a: setattr(a["d"], "count", a["d"].count + 4),
}


@pytest.mark.parametrize("what", sorted(HOST_CASES))
def test_host_call_refuses_bad_arguments(what):
    case = rc_.build(300, D + 1, "uniform", seed=2)
    out = rc_.Outputs(case.n, case.n)
    i_s, o_s, d_s = _structs(case, out)
    a = {"i": i_s, "o": o_s, "d": d_s, "act": C.c_uint64(rc_.COUNT_SENTINEL), "tab": rc_._p(case.session_of_inst),
         "ids": rc_._p(case.id_of_inst), "inst": rc_._p(out.inst)}
    HOST_CASES[what](a)
    ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
    rc = lib().cc_route_events(ref(a["i"]), case.n, a["tab"], a["ids"], case.n_inst, case.n_sessions, 1, ref(a["o"]),
                               a["inst"], ref(a["d"]), ref(a["act"]))
    assert rc == abi.CC_ERR_INVALID, what
    assert lib().cc_last_error() and out.untouched()


def test_empty_stream_stores_nothing_but_n_active():
    case = rc_.build(0, 7, "uniform")
    rc, active, out = rc_.host_route(lib(), case, 16)
    assert rc == abi.CC_OK and active == 0 and out.untouched()
    rc, active, out = rc_.host_route(lib(), case, 1, n_sessions=0)  # no sessions and no events: nothing to refuse
    assert rc == abi.CC_OK and active == 0 and out.untouched()


# ---- the device call's bound and argument checks (no GPU) ----------------------------------------------------------------
A = 0x10000  # an aligned "device address"


def _bound(n, sessions=1000):
    out = C.c_uint64(0)
    return lib().cc_route_events_device_bound(n, sessions, C.byref(out)), out.value


def test_bound_arithmetic():
    sizes = [0, 1, 63, T - 1, T, T + 1, 3 * T + 17, 100_003, 25_000_000, (1 << 32) - 1]
    got = []
    for n in sizes:
        rc, b = _bound(n)
        assert rc == abi.CC_OK
        tiles = (n + T - 1) // T
        assert b >= 16 * n + 4 * D * tiles  # two (key, permutation) buffers, a counter per digit value and tile
        assert b <= 16 * n + 4 * D * tiles + tiles + 4096  # ... and no more than the scan's chunk sums and the padding
        assert b % 16 == 0
        got.append(b)
    assert got == sorted(got) and got[-1] > got[0]
    # no array is sized by the session count
    assert len({_bound(100_003, s)[1] for s in (1, 2, D, D * D + 1, D ** 3 + 1, (1 << 32) - 1)}) == 1
    assert _bound(1 << 32)[0] == abi.CC_ERR_INVALID and _bound(10, 0)[0] == abi.CC_ERR_INVALID
    assert _bound(0, 0)[0] == abi.CC_OK
    assert lib().cc_route_events_device_bound(10, 1, None) == abi.CC_ERR_INVALID


def _dev_args(n=1000, sessions=300):
    return {"i": abi.cc_events(*[A * (k + 1) for k in range(6)], n, A * 7),
            "o": abi.cc_events(*[A * (k + 11) for k in range(6)], n, A * 17),
            "d": abi.cc_route_dir(A * 21, A * 22, n, A * 23), "n": n, "tab": C.c_void_p(A * 31), "ids": C.c_void_p(A * 32),
            "inst": C.c_void_p(A * 33), "n_inst": 64, "sessions": sessions, "act": C.c_uint64(rc_.COUNT_SENTINEL),
            "work": C.c_void_p(A * 6000), "work_bytes": _bound(n)[1]}


def _dev(a):
    ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
    return lib().cc_route_events_device(ref(a["i"]), a["n"], a["tab"], a["ids"], a["n_inst"], a["sessions"], ref(a["o"]),
                                        a["inst"], ref(a["d"]), ref(a["act"]), a["work"], a["work_bytes"], None)


DEV_CASES = dict(HOST_CASES)
DEV_CASES.update({
    "n 2^32": lambda a: a.update(n=1 << 32),
    "no sessions": lambda a: a.update(sessions=0),
    "null workspace": lambda a: a.update(work=None),
    "misaligned workspace": lambda a: a.update(work=C.c_void_p(A * 6000 + 8)),
    "work_bytes one short": lambda a: a.update(work_bytes=a["work_bytes"] - 1),
})


@pytest.mark.parametrize("what", sorted(DEV_CASES))
def test_device_call_refuses_before_any_hip_call(what):
    a = _dev_args()
    DEV_CASES[what](a)
    assert _dev(a) == abi.CC_ERR_INVALID, what
    assert lib().cc_last_error()
    assert a["act"] is None or a["act"].value == rc_.COUNT_SENTINEL


def test_device_call_answers_the_output_capacity_before_any_hip_call():
    a = _dev_args()
    a["o"].capacity = a["n"] - 1
    assert _dev(a) == abi.CC_ERR_CAPACITY and a["act"].value == rc_.COUNT_SENTINEL


def test_device_call_with_nothing_to_do_needs_no_device():
    a = _dev_args(n=0)
    assert _dev(a) == abi.CC_OK and a["act"].value == 0


def test_timing_aid_is_off_and_reads_zeros_without_a_call():
    ms = (C.c_float * abi.CC_ROUTE_TIMING_SLOTS)(*([1.0] * abi.CC_ROUTE_TIMING_SLOTS))
    assert lib().cc_route_events_device_timing(0, ms) == abi.CC_OK and list(ms) == [0.0] * abi.CC_ROUTE_TIMING_SLOTS


def test_constants_match_the_header():
    import os
    import re

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "copycat_apply.h")).read()
    for name in ("CC_ROUTE_DIGIT_BITS", "CC_ROUTE_TILE_EVENTS", "CC_ROUTE_TIMING_SLOTS"):
        assert int(re.search(rf"#define {name} (\d+)", hdr).group(1)) == getattr(abi, name)
    assert lib().cc_abi_version() == 6
