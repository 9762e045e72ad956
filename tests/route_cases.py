"""Shared case builder of the route tests (cc_route_events / cc_route_events_device; numpy only).

A case is an event stream seen from the route: `n` events, each owned by a client session (an ordinal below
n_sessions), and the two host tables that say so: every session that owns events has two instance slots (so that two
targets share a session), a few more slots belong to the highest ordinal, and the slots are shuffled.  Pos, code, src,
tag and payload differ from event to event (pos 0xFFFFFFFF and CC_EVSRC_RESULT rows included), so a misplaced row shows
in every column.

The reference is independent of both implementations: a stable numpy argsort by session_of_inst[target], and np.unique
on the sorted keys for the directory."""
import ctypes as C

import numpy as np

from copycat_amd import abi

T = abi.CC_ROUTE_TILE_EVENTS
D = 1 << abi.CC_ROUTE_DIGIT_BITS
COLS = tuple(name for name, _ in abi.EVENT_COLUMNS)
DT = {"pos": np.uint32, "target": np.uint32, "code": np.uint8, "src": np.uint8, "tag": np.uint8, "payload": np.uint64}
SENTINEL = {"pos": 0xDEADBEEF, "target": 0xFEEDFACE, "code": 0xA5, "src": 0x5A, "tag": 0xC3, "payload": 0xDEADBEEFCAFEF00D}
INST_SENTINEL = 0xABADCAFE0BADF00D
DIR_SENTINEL = 0xD1D1D1D1
COUNT_SENTINEL = 0x7777

SIZES = (0, 1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 17)
SESSIONS = (1, 2, D - 1, D, D + 1, D * D - 1, D * D, D * D + 1, D ** 3 + 1)  # the last one: a fourth round
DISTRIBUTIONS = ("one_session", "own_session", "reversed", "alternating", "uniform", "zipf")


def owners(n, n_sessions, pattern, rng):
    """the session ordinal of every event"""
    top = n_sessions - 1
    spread = np.arange(n, dtype=np.int64) * max(1, n_sessions // max(n, 1)) % n_sessions  # distinct while n <= n_sessions
    if pattern == "one_session":
        return np.full(n, top, np.int64)
    if pattern == "own_session":
        return rng.permutation(spread)
    if pattern == "reversed":  # session order exactly reversed against input order
        return np.sort(spread)[::-1].copy()
    if pattern == "alternating":  # the lowest and the highest ordinal, across every wave and tile boundary
        return np.where(np.arange(n) % 2 == 0, 0, top).astype(np.int64)
    if pattern == "uniform":
        s = rng.integers(0, n_sessions, n)
        s[:1] = top
        return s
    if pattern == "zipf":
        return (rng.zipf(1.3, n).astype(np.uint64) * np.uint64(2654435761) % np.uint64(n_sessions)).astype(np.int64)
    raise ValueError(pattern)


class Case:
    """ev: the input columns; session_of_inst, id_of_inst; ref / ref_inst / ref_session / ref_start: the answer"""

    def __init__(self, n, n_sessions, owner, seed=0):
        rng = np.random.default_rng(seed + 1000)
        self.n, self.n_sessions = int(n), int(n_sessions)
        owner = np.asarray(owner, np.int64)
        uniq, idx = np.unique(owner, return_inverse=True)
        extra = 5
        self.n_inst = 2 * len(uniq) + extra
        slots = rng.permutation(self.n_inst)
        self.session_of_inst = np.empty(self.n_inst, np.uint32)
        self.session_of_inst[slots[0:2 * len(uniq):2]] = uniq
        self.session_of_inst[slots[1:2 * len(uniq):2]] = uniq
        self.session_of_inst[slots[2 * len(uniq):]] = n_sessions - 1
        self.id_of_inst = (np.uint64(1) << np.uint64(40)) + np.arange(self.n_inst, dtype=np.uint64) * np.uint64(7)
        pos = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        pos[rng.random(n) < 0.1] = 0xFFFFFFFF  # close / timer rows
        self.ev = {"pos": pos,
                   "target": slots[2 * idx.reshape(-1) + rng.integers(0, 2, n)].astype(np.uint32),
                   "code": rng.integers(1, 14, n).astype(np.uint8),
                   "src": rng.integers(0, 4, n).astype(np.uint8),  # CC_EVSRC_RESULT included
                   "tag": rng.integers(0, 8, n).astype(np.uint8),
                   "payload": rng.integers(0, 1 << 64, n, dtype=np.uint64)}
        self.ref, self.ref_inst, self.ref_session, self.ref_start = reference(self.ev, self.session_of_inst, self.id_of_inst)
        self.n_active = len(self.ref_session)


def reference(ev, session_of_inst, id_of_inst):
    key = session_of_inst[ev["target"].astype(np.int64)]
    order = np.argsort(key, kind="stable")
    ref = {name: ev[name][order] for name in COLS}
    session, start = np.unique(key[order], return_index=True)
    return (ref, id_of_inst[ref["target"].astype(np.int64)], session.astype(np.uint32),
            np.append(start, len(key)).astype(np.uint32))


def build(n, n_sessions, pattern, seed=0):
    rng = np.random.default_rng(seed)
    return Case(n, n_sessions, owners(n, n_sessions, pattern, rng), seed)


def grid(pattern):
    for n in SIZES:
        for s in SESSIONS:
            yield build(n, s, pattern, seed=n + s)


class Outputs:
    """sentinel-filled outputs with guard rows behind every capacity"""

    GUARD = 3

    def __init__(self, capacity, dir_capacity):
        self.capacity, self.dir_capacity = capacity, dir_capacity
        self.cols = {name: np.full(capacity + self.GUARD, SENTINEL[name], DT[name]) for name in COLS}
        self.inst = np.full(capacity + self.GUARD, INST_SENTINEL, np.uint64)
        self.session = np.full(dir_capacity + self.GUARD, DIR_SENTINEL, np.uint32)
        self.start = np.full(dir_capacity + 1 + self.GUARD, DIR_SENTINEL, np.uint32)
        self.count = np.array([COUNT_SENTINEL], np.uint64)      # *out->count
        self.dir_count = np.array([COUNT_SENTINEL], np.uint64)  # *dir->count

    def untouched(self, rows=0, active=None):
        """rows past `rows` and directory entries past `active` (+ 1 for start) keep their sentinel; active None: all"""
        ok = all(np.all(self.cols[name][rows:] == DT[name](SENTINEL[name])) for name in COLS)
        ok &= bool(np.all(self.inst[rows:] == np.uint64(INST_SENTINEL)))
        if active is None:
            ok &= bool(np.all(self.session == DIR_SENTINEL) and np.all(self.start == DIR_SENTINEL))
            ok &= int(self.count[0]) == COUNT_SENTINEL and int(self.dir_count[0]) == COUNT_SENTINEL
        else:
            ok &= bool(np.all(self.session[active:] == DIR_SENTINEL) and np.all(self.start[active + 1:] == DIR_SENTINEL))
        return bool(ok)

    def equals(self, case, with_ids=True):
        """the whole answer of `case`, and nothing beyond it (an empty stream stores nothing at all)"""
        n, k = case.n, case.n_active
        if n == 0:
            return self.untouched()
        ok = all(np.array_equal(self.cols[name][:n], case.ref[name]) for name in COLS)
        if with_ids:
            ok &= np.array_equal(self.inst[:n], case.ref_inst)
        else:
            ok &= bool(np.all(self.inst == np.uint64(INST_SENTINEL)))
        ok &= np.array_equal(self.session[:k], case.ref_session) and np.array_equal(self.start[:k + 1], case.ref_start)
        ok &= int(self.count[0]) == n and int(self.dir_count[0]) == k
        return bool(ok) and self.untouched(n, k)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and len(a) else None


def host_route(lib, case, threads=1, out_capacity=None, dir_capacity=None, with_ids=True, ev=None, session_of_inst=None,
               n_inst=None, n_sessions=None):
    """cc_route_events into sentinel-filled outputs -> (rc, n_active, Outputs); n_active starts as COUNT_SENTINEL"""
    ev = ev or case.ev
    tab = case.session_of_inst if session_of_inst is None else session_of_inst
    cap = case.n if out_capacity is None else out_capacity
    dcap = min(case.n, case.n_sessions) if dir_capacity is None else dir_capacity
    o = Outputs(cap, dcap)
    i_s = abi.cc_events(*[_p(ev[name]) for name in COLS], case.n, None)
    o_s = abi.cc_events(*[_p(o.cols[name]) for name in COLS], cap, _p(o.count))
    d_s = abi.cc_route_dir(_p(o.session), _p(o.start), dcap, _p(o.dir_count))
    active = C.c_uint64(COUNT_SENTINEL)
    rc = lib.cc_route_events(C.byref(i_s), case.n, _p(tab), _p(case.id_of_inst) if with_ids else None,
                             len(tab) if n_inst is None else n_inst, case.n_sessions if n_sessions is None else n_sessions,
                             threads, C.byref(o_s), _p(o.inst) if with_ids else None, C.byref(d_s), C.byref(active))
    return rc, active.value, o
