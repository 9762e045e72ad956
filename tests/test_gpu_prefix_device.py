"""GPU: cc_apply_batch_prefix (ABI 6), the prefix apply on device-resident columns.

The contract of cc_apply_batch_host_prefix restated for HBM: the call stops before the first row a full coordination
collection, map table region or event stream cannot hold, with the state, the device result rows and the device event
stream exactly those after the rows before it, and the result rows from there on byte for byte what the caller had
there.  The rows that can overflow a coordination collection are found by the scan kernels of
copycat_amd/csrc/prefix_scan.hip; the boundary cases below aim the stop row at every position where their ranking
(lane, wave, tile, chunk) changes hands.  Expected values come from the oracle (oracle/oracle.cpp) or from a twin
engine driven through the host entry point (apply_host_prefix) or the plain one (apply_events).  Integer equality only.
Every stop here is a handled capacity code."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from copycat_amd import abi
from copycat_amd.batch import Batch
from tests.test_gpu_coord import L, _canon, _check_state, _oracle_events
from tests.test_gpu_map import _assert_maps, _engines
from tests.test_gpu_prefix import _map_rows, _table_region

pytestmark = pytest.mark.gpu

_EVK = ("pos", "src", "target", "code", "tag", "payload")
_SV = 0xA5A5A5A5A5A5A5A5  # the value prefill (status: 0xFF, engine.RESULT_SENTINEL)
LOCK, UNLOCK = abi.CC_OP_LOCK_LOCK, abi.CC_OP_LOCK_UNLOCK


def _scan_block():
    """Rows of one ranked tile of the scan kernels (kPxBlock, engine_internal.h)."""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "copycat_amd", "csrc",
                       "engine_internal.h")
    return int(re.search(r"constexpr uint32_t kPxBlock = (\d+);", open(src).read()).group(1))


def _dev_prefix(E, b, capacity=None):
    """One apply_prefix call on an uploaded batch with sentinel-prefilled device results and a DeviceEvents:
    (applied, status, value, events as DeviceEvents.host())."""
    from copycat_amd.engine import RESULT_SENTINEL, DeviceBatch, DeviceEvents

    n = len(b)
    db = DeviceBatch.upload(b)
    status = torch.full((n,), RESULT_SENTINEL, dtype=torch.uint8, device="cuda")
    value = torch.full((n,), _SV - (1 << 64), dtype=torch.int64, device="cuda")
    evs = DeviceEvents(capacity if capacity is not None else max(4 * n, 1024))
    evs.count.fill_(-7)  # (the call writes the count itself)
    applied = E.apply_prefix(db, status, value, evs)
    s, v, ev = status.cpu().numpy(), value.cpu().numpy().view(np.uint64), evs.host()
    assert 0 <= applied <= n
    assert np.all(s[applied:] == RESULT_SENTINEL) and np.all(v[applied:] == _SV)  # rows not applied: byte for byte
    assert not np.any(s[:applied] == RESULT_SENTINEL)                           # every applied row has a result
    assert ev["count"] == len(ev["pos"])                                        # all the events are present
    assert len(ev["pos"]) == 0 or int(ev["pos"].max()) < applied
    assert np.all(np.diff(ev["pos"].astype(np.int64)) >= 0)                     # ordered by log row
    return applied, s, v, ev


def _rows(rows, index0=1, t0=0):
    """(inst, op, aux) rows as a Batch; the clock advances by one per row."""
    n = len(rows)
    b = Batch(n)
    b.index[:] = np.arange(index0, index0 + n, dtype=np.uint64)
    b.time[:] = np.arange(t0, t0 + n, dtype=np.uint64)
    b.inst[:] = [x[0] for x in rows]
    b.op[:] = [x[1] for x in rows]
    b.aux[:] = np.array([x[2] for x in rows], np.int64).view(np.uint64)
    return b


def _lock_engine(R, K, coord_cap=0):
    from copycat_amd.engine import Engine

    E = Engine(R, R * K + 8, 1 << 14, flags=abi.CC_CFG_TIMERS_DEFERRED, max_events=1 << 16, coord_cap=coord_cap)
    for r in range(R):
        E.resource_create(r, L)
        for k in range(K):
            E.instance_open(r * K + k, r, 1000 + r * K + k, 7 + r * K + k)
    return E


def _same_events(a, b):
    return _canon(*(a[k] for k in _EVK)) == _canon(*(b[k] for k in _EVK))


# ---- 1. a full map table region ----------------------------------------------------------------------------------------
def test_device_prefix_map_region_full_fails_one_commit():
    """One map in two 2,048-entry table regions (map_capacity 1,024).  Distinct keys are put, 2,048 + 20 into each
    region (shaped with the table's hash, gets between them), so up to 40 puts meet a full region.  The host calls the
    prefix apply again after each row it reports (failing that commit); every applied row, the map's entries and the
    applied index equal the oracle applying the same rows, and the device rows from `applied` on keep the sentinel."""
    E, O = _engines(1, 4, 16384, 1024)
    rng = np.random.default_rng(43)
    per = {0: [], 1: []}
    k = 3
    while min(len(per[0]), len(per[1])) < 2068:
        r = _table_region(0, 0, k)
        if len(per[r]) < 2068:
            per[r].append(k)
        k += 7919
    k1 = np.array(per[0] + per[1], np.uint64)[rng.permutation(4136)]
    keys, ops = [], []
    for i, key in enumerate(k1):
        keys.append(key)
        ops.append(abi.CC_OP_MAP_PUT)
        if i % 5 == 0:
            keys.append(k1[int(rng.integers(0, i + 1))])
            ops.append(abi.CC_OP_MAP_GET)
    b = _map_rows(keys, ops)
    n = len(b)
    pos, failed, calls = 0, [], 0
    gs, gv = np.zeros(n, np.uint8), np.zeros(n, np.uint64)
    while pos < n:
        calls += 1
        assert calls < 100
        rest = b.slice(pos, n)
        applied, s, v, ev = _dev_prefix(E, rest)
        assert ev["count"] == 0
        gs[pos:pos + applied], gv[pos:pos + applied] = s[:applied], v[:applied]
        if applied == len(rest):
            break
        failed.append(pos + applied)
        pos += applied + 1
    assert failed, "no region filled"
    assert len(failed) <= 40  # at most the 20 keys too many per region
    cuts = [0] + failed + [n]
    for a, z in zip(cuts[:-1], cuts[1:]):
        lo = a + 1 if a in failed else a
        if z > lo:
            s2, v2 = O.apply(b.slice(lo, z))
            assert np.array_equal(gs[lo:z], s2) and np.array_equal(gv[lo:z], v2), (lo, z)
    _assert_maps(E, O, [0])


# ---- 2. a full event stream --------------------------------------------------------------------------------------------
def test_device_prefix_event_stream_full_resumes():
    """Lock traffic on 64 locks whose events outnumber a DeviceEvents of 300: each call stops before the first row whose
    events do not fit, the stream holding exactly the events of the rows before it; the host drains it and calls again
    from that row.  Results, the concatenated events and the lock state equal the oracle's over the whole batch."""
    from copycat_amd.engine import Engine
    from copycat_amd.workload import coord_random_stream
    from oracle.oracle_py import Oracle

    R, K = 64, 4
    max_inst = R * K + 8
    E = Engine(R, max_inst, 1 << 16, flags=abi.CC_CFG_TIMERS_DEFERRED, max_events=1 << 16)
    O = Oracle(R, max_inst, abi.CC_CFG_TIMERS_DEFERRED)
    for r in range(R):
        E.resource_create(r, L)
        O.resource_create(r, L)
        for k in range(K):
            E.instance_open(r * K + k, r, 1000 + r * K + k, 7 + k)
            O.instance_open(r * K + k, r, 1000 + r * K + k, 7 + k)
    b = coord_random_stream(6000, np.full(R, L, np.uint8), K, max_inst, seed=77, p_delete=0.0)
    n = len(b)
    gs, gv = np.zeros(n, np.uint8), np.zeros(n, np.uint64)
    evs = {k: [] for k in _EVK}
    pos, calls = 0, 0
    while pos < n:
        calls += 1
        assert calls < 200
        applied, s, v, ev = _dev_prefix(E, b.slice(pos, n), capacity=300)
        assert applied > 0
        gs[pos:pos + applied], gv[pos:pos + applied] = s[:applied], v[:applied]
        assert ev["count"] <= 300  # (every pos < applied: _dev_prefix)
        for k in evs:
            evs[k].append(ev[k].astype(np.int64) + pos if k == "pos" else ev[k])
        pos += applied
    assert calls > 3  # the stream filled several times
    s2, v2 = O.apply(b)
    assert np.array_equal(gs, s2) and np.array_equal(gv, v2)
    oe, _, _ = _oracle_events(O)
    assert _canon(*(np.concatenate(evs[k]) for k in _EVK)) == _canon(*(oe[k] for k in _EVK))
    _check_state(E, O, [L] * R)


# ---- 3. a full coordination collection ---------------------------------------------------------------------------------
def _resume(apply, b):
    """The host's resume loop: a reported commit fails and is skipped.  (applied per call, results, events)."""
    n = len(b)
    gs, gv = np.full(n, 0xFF, np.uint8), np.zeros(n, np.uint64)
    evs = {k: [] for k in _EVK}
    pos, log = 0, []
    while pos < n:
        assert len(log) < 50
        rest = b.slice(pos, n)
        applied, s, v, ev = apply(rest)
        log.append(applied)
        gs[pos:pos + applied], gv[pos:pos + applied] = s[:applied], v[:applied]
        for k in evs:
            evs[k].append(ev[k].astype(np.int64) + pos if k == "pos" else ev[k])
        pos += applied + 1
    return log, gs, gv, {k: np.concatenate(evs[k]) for k in _EVK}


def _same_lock_state(E, T, R):
    for r in range(R):
        assert E.lock_state(r) == T.lock_state(r), r
    assert E.applied_index() == T.applied_index()


def test_device_prefix_stops_before_a_full_lock_queue_like_the_host_path():
    """One lock at coord_cap 64 with more waiters than it holds: the call stops exactly before the first waiter that
    does not fit.  The host fails that commit and resumes; the rows applied per call, every result, the events and the
    lock's state equal a twin engine driven through apply_host_prefix with the same rows."""
    K = 100
    rows = [(k, LOCK, -1) for k in range(65)]          # the holder and 64 waiters: the queue is full
    rows += [(65, LOCK, -1), (66, LOCK, -1)]             # two waiters too many (rows 65 and 66)
    rows += [(0, UNLOCK, 0), (67, LOCK, -1)]             # the holder leaves: one more fits ...
    rows += [(68, LOCK, -1), (69, LOCK, 0)]              # ... the next does not; a tryLock() never queues
    rows += [(k, UNLOCK, 0) for k in range(1, 30)] + [(70 + k, LOCK, 50) for k in range(20)]
    b = _rows(rows)
    E, T = _lock_engine(1, K), _lock_engine(1, K)
    got = _resume(lambda rest: _dev_prefix(E, rest), b)
    want = _resume(lambda rest: T.apply_host_prefix(rest), b)
    assert got[0] == want[0], (got[0], want[0])
    assert got[0][:3] == [65, 0, 2]  # stopped before rows 65, 66 and 69
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert _same_events(got[3], want[3])
    _same_lock_state(E, T, 1)


def test_device_prefix_queue_held_at_capacity_under_churn():
    """A lock queue that stays at coord_cap while the holder leaves and a new client queues, 40 times, among other
    locks' traffic: every add meets the bound, fits after all, and the call goes on from that row (parts that start at
    any row, not only at the alignment the plain call asks for).  Nothing overflows: every row applies, and results,
    events and lock state equal the twin's through apply_host_prefix and the oracle's."""
    from oracle.oracle_py import Oracle

    R, K, churn = 3, 120, 40
    rng = np.random.default_rng(19)
    rows = [(k, LOCK, -1) for k in range(65)]
    for j in range(churn):
        rows.append((j, UNLOCK, 0))
        rows.append((65 + j, LOCK, -1))
        for _ in range(int(rng.integers(0, 4))):
            r = int(rng.integers(1, R))
            rows.append((r * K + int(rng.integers(0, 8)), LOCK if rng.random() < 0.5 else UNLOCK,
                         int(rng.choice([-1, 0, 50]))))
    b = _rows(rows)
    E, T = _lock_engine(R, K), _lock_engine(R, K)
    O = Oracle(R, R * K + 8, abi.CC_CFG_TIMERS_DEFERRED)
    for r in range(R):
        O.resource_create(r, L)
        for k in range(K):
            O.instance_open(r * K + k, r, 1000 + r * K + k, 7 + r * K + k)
    applied, s, v, ev = _dev_prefix(E, b)
    applied2, s2, v2, ev2 = T.apply_host_prefix(b)
    assert applied == applied2 == len(b)
    assert np.array_equal(s, s2) and np.array_equal(v, v2) and _same_events(ev, ev2)
    s3, v3 = O.apply(b)
    assert np.array_equal(s, s3) and np.array_equal(v, v3)
    oe, _, _ = _oracle_events(O)
    assert _same_events(ev, oe)
    _check_state(E, O, [L] * R)


# ---- 4. scan boundaries --------------------------------------------------------------------------------------------------
_B = _scan_block()
_K4 = 200  # instances per lock


def _boundary_batch(n, stop, slot=0, room=4, mixed=False):
    """n rows on lock `slot` whose queue has `room` entries left: min(room, stop) adding rows spread over [0, stop), the
    next adding row at `stop` (the first that does not fit) and a few more behind it; every other row is one that must
    not count: a tryLock() (timeout 0), an unlock by a client that neither holds nor waits, or (mixed) a row on an
    instance slot past max_instances."""
    base = slot * _K4
    fill = [(base + 190, LOCK, 0), (base + 191, UNLOCK, 0)]
    if mixed:
        fill.append((2 * _K4 + 8 + 5, LOCK, -1))  # >= max_instances
    rows = [fill[i % len(fill)] for i in range(n)]
    before = min(room, stop)
    at = sorted({(stop - 1) - (j * max(stop - 1, 0)) // max(before - 1, 1) for j in range(before)}) if before else []
    assert len(at) == before and all(0 <= r < stop for r in at)
    adders = at + [stop] + [r for r in (stop + 1, stop + 2, n - 1) if stop < r < n]
    for j, r in enumerate(sorted(set(adders))):
        rows[r] = (base + 100 + j, LOCK, -1)
    return rows, before


def _prefilled_pair(waiters):
    """Two engines with two locks, lock r holding a holder and waiters[r] waiters (applied through the plain path)."""
    E, T = _lock_engine(2, _K4), _lock_engine(2, _K4)
    rows = []
    for r, w in enumerate(waiters):
        rows += [(r * _K4 + k, LOCK, -1) for k in range(w + 1)]
    pre = _rows(rows)
    for X in (E, T):
        X.apply_host_events(pre)
    return E, T, len(pre)


def _check_against_twin(E, T, b, want_applied):
    applied, s, v, ev = _dev_prefix(E, b)
    applied2, s2, v2, ev2 = T.apply_host_prefix(b)
    assert applied == applied2, (applied, applied2)
    assert applied == want_applied, (applied, want_applied)  # the row the case aimed at
    assert np.array_equal(s[:applied], s2[:applied]) and np.array_equal(v[:applied], v2[:applied])
    assert _same_events(ev, ev2)
    _same_lock_state(E, T, 2)


@pytest.mark.parametrize("n,stop", [
    (300, 0), (300, 63), (300, 64), (2 * _B + 44, _B - 1), (2 * _B + 44, _B), (300, 299), (3 * _B + 1, 2 * _B + 77),
], ids=["row0", "row63", "row64", "block-1", "block", "last", "third_block"])
def test_device_prefix_scan_stop_row_positions(n, stop):
    """The true stop row on each position where the scan's ranking changes hands: the first lane, the last lane of a
    wave, the first of the next, the last row of a tile, the first of the next, the last row of the batch, and a row in
    the third chunk of three chunks plus one row."""
    room = min(4, stop)
    E, T, n0 = _prefilled_pair([64 - room, 3])
    rows, before = _boundary_batch(n, stop, room=room)
    assert before == room
    _check_against_twin(E, T, _rows(rows, index0=n0 + 1, t0=n0), stop)


def test_device_prefix_scan_higher_slot_stops_first():
    """Two locks overflow in one batch, and the one in the higher slot does first."""
    E, T, n0 = _prefilled_pair([62, 62])
    n = 2 * _B + 30
    lo, _ = _boundary_batch(n, _B + 150, slot=0, room=2)
    hi, _ = _boundary_batch(n, 100, slot=1, room=2)
    rows = [h if h[0] >= _K4 and h[2] == -1 else l for l, h in zip(lo, hi)]  # lock 1's adding rows over lock 0's rows
    assert rows[100][0] >= _K4 and rows[_B + 150][0] < _K4
    _check_against_twin(E, T, _rows(rows, index0=n0 + 1, t0=n0), 100)


def test_device_prefix_scan_skips_rows_that_do_not_count():
    """Adding rows among tryLock() rows, unlocks and rows on an instance slot past max_instances: only the adding rows
    are ranked."""
    E, T, n0 = _prefilled_pair([60, 3])
    rows, _ = _boundary_batch(_B + 90, _B + 11, room=4, mixed=True)
    assert sum(r[0] >= 2 * _K4 + 8 for r in rows) > 50
    _check_against_twin(E, T, _rows(rows, index0=n0 + 1, t0=n0), _B + 11)


def test_device_prefix_scan_nothing_overflows():
    """No resource's bound passes coord_cap (the scan's list is empty): every row applies."""
    E, T, n0 = _prefilled_pair([10, 3])
    rows, _ = _boundary_batch(3 * _B + 1, 2 * _B + 77, room=4)
    _check_against_twin(E, T, _rows(rows, index0=n0 + 1, t0=n0), len(rows))


# ---- 5. no stop: the plain call ------------------------------------------------------------------------------------------
def test_device_prefix_without_a_stop_equals_the_plain_call():
    """A mixed coordination + map batch that fits, with an event stream: results, events, state and the path counters
    of apply_prefix equal those of apply_events on a twin engine."""
    from copycat_amd.engine import RESULT_SENTINEL, DeviceBatch, DeviceEvents, Engine
    from copycat_amd.workload import coord_random_stream

    locks, K, maps, n, nm = 32, 4, 2, 6000, 2000
    R = locks + maps
    max_inst = R * K + 8
    rng = np.random.default_rng(23)
    lk = coord_random_stream(n - nm, np.full(locks, L, np.uint8), K, max_inst, seed=23, p_delete=0.0)
    mrows = np.sort(rng.choice(n, nm, replace=False))
    at = np.ones(n, bool)
    at[mrows] = False
    cols = {}
    for name, _ in abi.BATCH_COLUMNS:
        src = getattr(lk, name)
        col = np.zeros(n, src.dtype)
        col[at] = src
        cols[name] = col
    cols["index"] = np.arange(1, n + 1, dtype=np.uint64)
    cols["time"] = np.maximum.accumulate(cols["time"])
    cols["op"][mrows] = rng.choice(np.array([abi.CC_OP_MAP_PUT, abi.CC_OP_MAP_GET, abi.CC_OP_MAP_REMOVE], np.uint8), nm)
    cols["inst"][mrows] = (locks + rng.integers(0, maps, nm)) * K + rng.integers(0, K, nm)
    cols["key"][mrows] = rng.integers(0, 300, nm).astype(np.uint64)
    cols["a"][mrows] = rng.integers(0, 9, nm).astype(np.uint64)
    cols["flags"][mrows] = abi.cc_flags(abi.CC_TAG_LONG, 0, 0)
    cols["aux"][mrows] = 0
    b = Batch.from_columns(**cols)
    out = []
    for prefix in (True, False):
        E = Engine(R, max_inst, n, flags=abi.CC_CFG_TIMERS_DEFERRED, max_events=1 << 16, map_capacity=4096)
        for r in range(R):
            E.resource_create(r, L if r < locks else abi.CC_RES_MAP)
            for k in range(K):
                E.instance_open(r * K + k, r, 1000 + r * K + k, 7 + k)
        db = DeviceBatch.upload(b)
        status = torch.full((n,), RESULT_SENTINEL, dtype=torch.uint8, device="cuda")
        value = torch.full((n,), -1, dtype=torch.int64, device="cuda")
        evs = DeviceEvents(4 * n)
        if prefix:
            assert E.apply_prefix(db, status, value, evs) == n
        else:
            E.apply_events(db, status, value, evs)
            E.sync()
        ev = evs.host()
        state = ([E.lock_state(r) for r in range(locks)],
                 [tuple(a.tolist() for a in E.map_entries(r)) for r in range(locks, R)], E.applied_index())
        out.append((status.cpu().numpy(), value.cpu().numpy(), ev, state, E.counters()[0:4]))
    p, q = out
    assert not np.any(q[0] == RESULT_SENTINEL)
    assert np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1])
    assert p[2]["count"] == q[2]["count"] > 0 and np.array_equal(p[2]["pos"], q[2]["pos"])
    assert _same_events(p[2], q[2])
    assert p[3] == q[3]
    assert p[4] == q[4]


# ---- 6. arguments --------------------------------------------------------------------------------------------------------
def test_device_prefix_arguments():
    """n == 0: CC_OK, applied 0 and an event count of 0.  A null h_applied: CC_ERR_INVALID before anything runs (state,
    result rows and the event count untouched)."""
    from copycat_amd.engine import RESULT_SENTINEL, DeviceBatch, DeviceEvents

    E = _lock_engine(1, 8)
    E.apply_host_events(_rows([(0, LOCK, -1), (1, LOCK, -1)]))
    before = (E.lock_state(0), E.applied_index())
    applied, s, v, ev = _dev_prefix(E, Batch(0), capacity=16)
    assert applied == 0 and ev["count"] == 0 and len(s) == 0
    assert (E.lock_state(0), E.applied_index()) == before
    b = _rows([(2, LOCK, -1), (3, LOCK, -1)], index0=3, t0=2)
    db = DeviceBatch.upload(b)
    status = torch.full((2,), RESULT_SENTINEL, dtype=torch.uint8, device="cuda")
    value = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    evs = DeviceEvents(16)
    evs.count.fill_(-7)
    cols, res, evc = db.struct(), abi.cc_results(status.data_ptr(), value.data_ptr()), evs.struct()
    rc = E.L.cc_apply_batch_prefix(E.h, C.byref(cols), 2, C.byref(res), C.byref(evc), None, None)
    assert rc == abi.CC_ERR_INVALID
    assert (E.lock_state(0), E.applied_index()) == before
    assert np.all(status.cpu().numpy() == RESULT_SENTINEL) and int(evs.count.item()) == -7
    assert E.apply_prefix(db, status, value, evs) == 2  # the same arguments with h_applied apply
    assert len(E.lock_state(0)[3]) == 3
