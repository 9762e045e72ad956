"""GPU: cc_apply_batch_host_prefix (ABI 5) on the fixed capacities beyond coordination collections.

A full map table region or a full event stream fails one commit, not the batch: the call stops before the row that
does not fit, with the engine state, results and events exactly those after the rows before it (a device checkpoint
and a bisection over the part, copycat_amd/csrc/host_path.hip), and the host resumes from there.  In the reference an
exception fails one commit only (ResourceManager.operateResource, manager/src/main/java/io/atomix/manager/
ResourceManager.java:56-72).  Bar: bit-exact against the oracle (oracle/oracle.cpp) on the rows that were applied.

The scenarios after the first two tests drive engines whose batches move every state component a rolled-back attempt
can touch (the leak log, schedule timers, TTL mode, small-map window, big HashMap models, compacted keys, whole-map
rows, retained value commits, snapshots) through stopped prefix applies and compare every reader with the oracle and
with replicas that applied only the applied rows through the plain entry points.  All comparisons are integer
equality."""
import functools

import numpy as np
import pytest

from copycat_amd import abi
from copycat_amd.batch import Batch
from tests.test_gpu_coord import L, _canon, _check_state, _oracle_events
from tests.test_gpu_map import _assert_maps, _engines

pytestmark = pytest.mark.gpu


def _map_rows(keys, ops, index0=1):
    n = len(keys)
    return Batch.from_columns(index=np.arange(index0, index0 + n, dtype=np.uint64), inst=np.zeros(n, np.uint32),
                              op=np.asarray(ops, np.uint8),
                              flags=np.full(n, abi.cc_flags(abi.CC_TAG_LONG, 0, 0), np.uint8),
                              key=np.asarray(keys, np.uint64), a=np.asarray(keys, np.uint64) * np.uint64(3) + np.uint64(1))


def test_prefix_apply_map_region_full_fails_one_commit():
    """One map in two 2,048-entry table regions (map_capacity 1,024): 4,300 distinct keys are put (gets between), so
    puts into a full region cannot be held; then half the keys are removed (the next launches compact the regions)
    and more keys are put.  The host calls the prefix apply again after each row it reports (failing that commit), and
    every applied row, the map's entries and the applied index equal the oracle applying the same rows."""
    from oracle.oracle_py import Oracle  # noqa: F401  (the _engines oracle)

    E, O = _engines(1, 4, 16384, 1024)
    rng = np.random.default_rng(41)
    k1 = rng.permutation(4300).astype(np.uint64) * np.uint64(7919) + np.uint64(3)
    keys, ops = [], []
    for i, k in enumerate(k1):
        keys.append(k)
        ops.append(abi.CC_OP_MAP_PUT)
        if i % 5 == 0:
            keys.append(k1[int(rng.integers(0, i + 1))])
            ops.append(abi.CC_OP_MAP_GET)
    for k in k1[:2150]:
        keys.append(k)
        ops.append(abi.CC_OP_MAP_REMOVE)
    k2 = np.arange(600, dtype=np.uint64) * np.uint64(104729) + np.uint64(1 << 40)
    for k in k2:
        keys.append(k)
        ops.append(abi.CC_OP_MAP_PUT)
    b = _map_rows(keys, ops)
    n = len(b)
    pos, failed, calls = 0, [], 0
    gs = np.zeros(n, np.uint8)
    gv = np.zeros(n, np.uint64)
    while pos < n:
        calls += 1
        assert calls < 400
        rest = b.slice(pos, n)
        applied, s, v, _ = E.apply_host_prefix(rest)
        gs[pos:pos + applied] = s[:applied]
        gv[pos:pos + applied] = v[:applied]
        assert np.all(s[applied:] == 0xFF)  # rows not applied keep the caller's prefill
        if applied == len(rest):
            break
        failed.append(pos + applied)
        pos += applied + 1
    assert failed, "no region filled"
    keep = np.ones(n, bool)
    keep[failed] = False
    cuts = [0] + [f for f in failed] + [n]
    for a, z in zip(cuts[:-1], cuts[1:]):
        lo = a + 1 if a in failed else a
        if z > lo:
            s2, v2 = O.apply(b.slice(lo, z))
            assert np.array_equal(gs[lo:z], s2) and np.array_equal(gv[lo:z], v2), (lo, z)
    _assert_maps(E, O, [0])


def test_prefix_apply_event_stream_full_resumes():
    """Lock traffic on 64 locks whose events (LockState.lock / unlock publish to the waiter, LockState.java:41-85)
    outnumber a host event stream of 300: each prefix call stops before the first row whose events do not fit, with
    that stream holding exactly the events of the rows before it; the host drains it and calls again from that row.
    Every result and every event (row, target, code, payload) equals the oracle applying the whole batch."""
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
    gs = np.zeros(n, np.uint8)
    gv = np.zeros(n, np.uint64)
    evs = {k: [] for k in ("pos", "src", "target", "code", "tag", "payload")}
    pos, calls = 0, 0
    while pos < n:
        calls += 1
        assert calls < 200
        rest = b.slice(pos, n)
        applied, s, v, ev = E.apply_host_prefix(rest, capacity=300)
        assert applied > 0 or len(rest) == 0
        gs[pos:pos + applied] = s[:applied]
        gv[pos:pos + applied] = v[:applied]
        assert len(ev["pos"]) <= 300 and (len(ev["pos"]) == 0 or ev["pos"].max() < applied)
        for k in evs:
            evs[k].append(ev[k] + (pos if k == "pos" else 0))
        pos += applied
    assert calls > 3  # the stream filled several times
    s2, v2 = O.apply(b)
    assert np.array_equal(gs, s2) and np.array_equal(gv, v2)
    oe, _, _ = _oracle_events(O)
    got = _canon(*(np.concatenate(evs[k]) for k in ("pos", "src", "target", "code", "tag", "payload")))
    assert got == _canon(oe["pos"], oe["src"], oe["target"], oe["code"], oe["tag"], oe["payload"])
    _check_state(E, O, [L] * R)


# ---- a differential harness for stopped prefix applies -----------------------------------------------------------
# _Prefix drives one engine through apply_host_prefix until the batch is exhausted; _Mirror makes the oracle (and
# replica engines, through the plain host entry points) apply exactly the rows each call applied, call for call;
# _compare reads every reader on every side.  cc_read_retained, cc_retained_bitmap and the snapshot
# drain the device leak log, which hides a log the checkpoint restored wrongly: every scenario says through `drain`
# when those readers may run.
_EVK = ("pos", "src", "target", "code", "tag", "payload")
_EVT = {"pos": np.int64, "src": np.uint8, "target": np.uint32, "code": np.uint8, "tag": np.uint8, "payload": np.uint64}
M_, S_, MM_ = abi.CC_RES_MAP, abi.CC_RES_SET, abi.CC_RES_MULTIMAP
E_, G, V = abi.CC_RES_ELECTION, abi.CC_RES_GROUP, abi.CC_RES_VALUE
_KEYED = (M_, S_, MM_)


def _cat(parts, dtype):
    return np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype)


class _Prefix:
    """One engine driven through apply_host_prefix over rows [pos, len(b)) of a batch.  stop = "region": a stop is a
    full map table region, the reported commit fails and is skipped; stop = "events": a stop is a full event stream,
    the host drains it and resumes at the same row.  Any other error raises EngineError out of the test.
    gs / gv: the results of the applied rows (0xFF / 0 elsewhere); ev: the events, rows as batch positions; failed: the
    failed rows; calls: (first row, rows handed in, rows applied) per call."""

    def __init__(self, E, b, stop, capacity=None, pos=0, max_calls=100):
        assert stop in ("region", "events")
        self.E, self.b, self.n, self.stop, self.capacity = E, b, len(b), stop, capacity
        self.pos, self.max_calls = pos, max_calls
        self.gs = np.full(self.n, 0xFF, np.uint8)
        self.gv = np.zeros(self.n, np.uint64)
        self.ev = {k: [] for k in _EVK}
        self.failed, self.calls = [], []

    def done(self):
        return self.pos >= self.n

    def step(self):
        """One call: (first row, end of the applied rows, stopped)."""
        assert not self.done()
        assert len(self.calls) < self.max_calls, f"{len(self.calls)} calls: the stream was shaped for far fewer stops"
        lo = self.pos
        rest = self.b.slice(lo, self.n)
        m = len(rest)
        applied, s, v, ev = self.E.apply_host_prefix(rest, capacity=self.capacity)
        assert 0 <= applied <= m
        assert np.all(s[applied:] == 0xFF) and not v[applied:].any()  # rows not applied keep the caller's prefill
        assert not np.any(s[:applied] == 0xFF)                       # every applied row has a result
        ne = len(ev["pos"])
        assert self.capacity is None or ne <= self.capacity
        assert ne == 0 or int(ev["pos"].max()) < applied             # no event of a row that was not applied
        assert np.all(np.diff(ev["pos"].astype(np.int64)) >= 0)      # the stream is ordered by log row
        self.gs[lo:lo + applied] = s[:applied]
        self.gv[lo:lo + applied] = v[:applied]
        for k in _EVK:
            self.ev[k].append(ev[k].astype(np.int64) + lo if k == "pos" else ev[k].copy())
        self.calls.append((lo, m, applied))
        stopped = applied < m
        if not stopped:
            self.pos = self.n
        elif self.stop == "region":
            self.failed.append(lo + applied)
            self.pos = lo + applied + 1
        else:
            assert applied > 0, f"row {lo}: one commit's events do not fit an empty event stream"
            self.pos = lo + applied
        return lo, lo + applied, stopped

    def stops(self):
        return sum(a < m for _, m, a in self.calls)

    def bisected(self):
        return sum(0 < a < m for _, m, a in self.calls)

    def events(self):
        return {k: _cat(self.ev[k], _EVT[k]) for k in _EVK}


class _Mirror:
    """The oracle, and replica engines through the plain host entry points (apply_host, or apply_host_events when
    `events`), applying the rows [lo, hi) a _Prefix call applied."""

    def __init__(self, O, b, replicas=(), events=False):
        self.O, self.b, self.n, self.with_events = O, b, len(b), events
        self.os = np.full(self.n, 0xFF, np.uint8)
        self.ov = np.zeros(self.n, np.uint64)
        self.oe = {k: [] for k in _EVK}
        self.apos, self.amem = [], []
        self.rep = [{"E": R, "s": self.os.copy(), "v": self.ov.copy(), "ev": {k: [] for k in _EVK}} for R in replicas]

    def apply(self, lo, hi):
        if hi <= lo:
            return
        seg = self.b.slice(lo, hi)
        self.os[lo:hi], self.ov[lo:hi] = self.O.apply(seg)
        oe, apos, amem = _oracle_events(self.O)
        for k in _EVK:
            self.oe[k].append(oe[k].astype(np.int64) + lo if k == "pos" else oe[k])
        self.apos.append(apos.astype(np.int64) + lo)
        self.amem.append(amem)
        for rp in self.rep:
            if self.with_events:
                s, v, ev = rp["E"].apply_host_events(seg, capacity=max(8 * len(seg), 4096))
                for k in _EVK:
                    rp["ev"][k].append(ev[k].astype(np.int64) + lo if k == "pos" else ev[k])
            else:
                s, v = rp["E"].apply_host(seg)
            rp["s"][lo:hi], rp["v"][lo:hi] = s, v


def _drive(P, M, until_stop=False, after_call=None):
    """Calls until the batch is exhausted (or until the first stop), the mirror following each call."""
    while not P.done():
        lo, hi, stopped = P.step()
        M.apply(lo, hi)
        if after_call is not None:
            after_call(stopped)
        if stopped and until_stop:
            return True
    return False


def _assert_same_rows(gs, gv, ws, wv, who):
    bad = np.nonzero((gs != ws) | (gv != wv))[0]
    assert len(bad) == 0, (f"{len(bad)} rows differ from {who}; first {bad[:5]}: prefix {gs[bad[:5]]},{gv[bad[:5]]} "
                           f"{who} {ws[bad[:5]]},{wv[bad[:5]]}")


def _assert_same_events(got, want, who):
    g, w = _canon(*(got[k] for k in _EVK)), _canon(*(want[k] for k in _EVK))
    assert len(g) == len(w), f"{len(g)} events vs {who} {len(w)}"
    assert g == w, (who, next(((i, x, y) for i, (x, y) in enumerate(zip(g, w)) if x != y), None))


def _compare_results(P, M):
    """Status and value of every applied row, the prefill on every other row, and the events as canonical tuples
    (each commit publishes at most one event per target, so this fixes per-target order); join's member rows in
    stream order against the oracle's aux stream.  The replicas the same, member rows included."""
    _assert_same_rows(P.gs, P.gv, M.os, M.ov, "oracle")  # (both sides hold 0xFF / 0 on the rows not applied)
    got = P.events()
    member = got["code"] == abi.CC_EV_MEMBER
    _assert_same_events({k: got[k][~member] for k in _EVK}, {k: _cat(M.oe[k], _EVT[k]) for k in _EVK}, "oracle")
    gm = list(zip(got["pos"][member].tolist(), got["payload"][member].tolist()))
    assert gm == list(zip(_cat(M.apos, np.int64).tolist(), _cat(M.amem, np.uint64).tolist()))
    for i, rp in enumerate(M.rep):
        _assert_same_rows(P.gs, P.gv, rp["s"], rp["v"], f"replica {i}")
        rev = {k: _cat(rp["ev"][k], _EVT[k]) for k in _EVK}
        _assert_same_events(got, rev, f"replica {i}")
        rmem = rev["code"] == abi.CC_EV_MEMBER
        assert gm == list(zip(rev["pos"][rmem].tolist(), rev["payload"][rmem].tolist()))


def _state(X, types, drain, nidx, vret=False, oracle=False):
    """Every reader of an engine or of the oracle as plain Python values: the applied index, per-slot state
    (map_entries of map / set / multimap slots; lock, election, group and value state as _check_state reads them), the
    retained value commits, and -- when `drain` allows -- retained(slot) of every slot and the retained bitmap over log
    indices [1, nidx] with its count (the oracle's: the union of its per-slot sets)."""
    from tests.test_gpu_retained import _bitmap_indices

    st = {("applied_index",): X.applied_index()}
    for r, t in enumerate(types):
        t = int(t)
        if t in _KEYED:
            ent = X.map_entries(r)
            st["entries", r] = None if ent is None else tuple(a.tolist() for a in ent)
        elif t == L:
            h, hi, hc, q = X.lock_state(r)
            st["lock", r] = (h, hi if h >= 0 else 0, hc, q)
        elif t == E_:
            st["election", r] = X.election_state(r)
        elif t == G:
            st["group", r] = X.group_members(r)
        elif t == V:
            st["value", r] = tuple(int(x[0]) for x in X.value_state(r, 1))
    if vret:
        st["value_retained",] = X.value_retained().tolist()
    if drain:
        union = set()
        for r in range(len(types)):
            got = X.retained(r)
            st["retained", r] = got
            union.update(got or ())
        if oracle:
            st["retained_bitmap",] = (len(union), sorted(union))
        else:
            bm, cnt = X.retained_bitmap(1, nidx)
            st["retained_bitmap",] = (cnt, _bitmap_indices(bm, 1, nidx))
    return st


def _assert_same_state(a, b, who_a, who_b):
    assert a.keys() == b.keys()
    for key in a:
        x, y = a[key], b[key]
        if x == y:
            continue
        detail = ""
        if key[0] in ("retained", "retained_bitmap"):
            lx, ly = (x or (), y or ()) if key[0] == "retained" else (x[1], y[1])
            detail = (f": {len(lx)} vs {len(ly)} indices, only {who_a} {sorted(set(lx) - set(ly))[:8]}, "
                      f"only {who_b} {sorted(set(ly) - set(lx))[:8]}")
            if key[0] == "retained_bitmap":
                detail += f", counts {x[0]} vs {y[0]}"
        elif key[0] == "entries":
            detail = f": {len(x[0]) if x else None} vs {len(y[0]) if y else None} entries"
        else:
            detail = f": {x} vs {y}"
        raise AssertionError(f"{who_a} and {who_b} differ in {key}{detail}")


def _compare(P, M, X, types, drain, nidx, vret=False, who="prefix engine"):
    """Engine X (the one P drives, or one restored from its snapshot) against the oracle after exactly the applied
    rows, then against every replica."""
    _compare_results(P, M)
    want = _state(M.O, types, drain, nidx, vret, oracle=True)
    got = _state(X, types, drain, nidx, vret)
    _assert_same_state(got, want, who, "oracle")
    for i, rp in enumerate(M.rep):
        _assert_same_state(got, _state(rp["E"], types, drain, nidx, vret), who, f"replica {i}")


def _snapshot_bytes_equal(P, M):
    """The replica byte check: True / False = the prefix engine's snapshot equals / differs from replica 0's, None =
    not asserted because the control failed (two replicas that applied the same rows through the plain entry point do
    not snapshot to the same bytes, so the engine is not byte-deterministic here).  Snapshots drain the leak log."""
    a, b = M.rep[0]["E"].snapshot(), M.rep[1]["E"].snapshot()
    if a != b:
        return None
    return P.E.snapshot() == a


def _tail_rows(P, rows):
    """How many of `rows` (sorted batch positions) lie in the rolled-back tail of the first failing attempt: that
    attempt is the whole rest of the batch (the engines here never cut a part at a coordination bound), so its tail
    is every row from the stop to the end."""
    lo, m, a = next(c for c in P.calls if c[2] < c[1])
    rows = np.asarray(rows)
    return int(((rows >= lo + a) & (rows < lo + m)).sum())


# ---- keyed streams shaped against the table's regions ----------------------------------------------------------------
_M64 = (1 << 64) - 1
_REGION = 2048  # entries of one table region (common.h kMapRegion); map_capacity 1,024 makes two of them


def _table_region(slot, ktag, key, map_bits=1):
    """The table region of a key (common.h map_hash: its top map_bits bits).  Used only to shape streams (how many
    distinct keys each region is offered); what stops and what applies is the engine's and the oracle's business, and
    every scenario asserts from the call log that the stops it was shaped for happened."""
    h = (key ^ (slot << 32) ^ (ktag << 61) ^ 0x9E3779B97F4A7C15) & _M64
    h ^= h >> 30
    h = (h * 0xBF58476D1CE4E5B9) & _M64
    h ^= h >> 27
    h = (h * 0x94D049BB133111EB) & _M64
    h ^= h >> 31
    return h >> (64 - map_bits)


_PUT = {M_: abi.CC_OP_MAP_PUT, S_: abi.CC_OP_SET_ADD, MM_: abi.CC_OP_MMAP_PUT}
_GET = {M_: abi.CC_OP_MAP_GET, S_: abi.CC_OP_SET_CONTAINS, MM_: abi.CC_OP_MMAP_GET}
_REMOVE = {M_: abi.CC_OP_MAP_REMOVE, S_: abi.CC_OP_SET_REMOVE, MM_: abi.CC_OP_MMAP_REMOVE}
_SIZE = {M_: abi.CC_OP_MAP_SIZE, S_: abi.CC_OP_SET_SIZE, MM_: abi.CC_OP_MMAP_SIZE}
_ISEMPTY = {M_: abi.CC_OP_MAP_ISEMPTY, S_: abi.CC_OP_SET_ISEMPTY, MM_: abi.CC_OP_MMAP_ISEMPTY}
_CLEAR = {M_: abi.CC_OP_MAP_CLEAR, S_: abi.CC_OP_SET_CLEAR, MM_: abi.CC_OP_MMAP_CLEAR}


class _Keyed:
    """Rows over keyed resources (resource slot r = instance slot r, Long keys) with a light model of the shared table
    beside them: a region binds every distinct key put into it until a launch that finds it more than 3/4 bound drops
    the keys that are absent by then (apply_map.hip), and a put of an unbound key into a fully bound region does not
    fit.  The model predicts the rows that will not fit (`misfit`), each of which ends a call, so a stream can offer
    a region exactly a few keys too many.  A call is one launch unless barrier rows (containsValue on a map that stores
    nulls, a multimap's isEmpty / clear, Delete) cut it into several; `eager` is for streams with such rows: the model
    then compacts as early as any launch could, so it predicts no stop the engine does not make (the engine may make a
    few more: keys removed since its last launch).  Time advances by one every `step` rows."""

    def __init__(self, types, seed, index0=1, t0=1000, step=4, eager=False):
        self.types = [int(t) for t in types]
        self.eager = eager
        self.rng = np.random.default_rng(seed)
        self.index0, self.t0, self.step = index0, t0, step
        self.rows = []    # (inst, op, flags, key, a, aux)
        self.bound = [set(), set()]
        self.dead = [set(), set()]  # bound keys that are absent (removed, cleared)
        self.live = {r: set() for r in range(len(types))}
        self.used = set()
        self.misfit = []  # predicted rows that do not fit

    def __len__(self):
        return len(self.rows)

    def _row(self, slot, op, key=0, tag=abi.CC_TAG_LONG, a=0, aux=0):
        self.rows.append((slot, op, abi.cc_flags(tag, 0, 0), key, a if tag else 0, aux))
        return len(self.rows) - 1

    def _launch(self, regions=(0, 1)):
        """A launch loads its regions: one more than 3/4 bound drops the bound keys that are absent."""
        for r in regions:
            if len(self.bound[r]) > _REGION * 3 // 4:
                self.bound[r] -= self.dead[r]
                self.dead[r] = set()

    def fresh(self, slot, region):
        """A key of `slot` nothing has used yet that falls into `region`."""
        while True:
            k = int(self.rng.integers(1 << 20, 1 << 40))
            if (slot, k) not in self.used and _table_region(slot, 0, k) == region:
                self.used.add((slot, k))
                return k

    def room(self, region):
        return _REGION - len(self.bound[region])

    def put(self, slot, key, a=1, tag=abi.CC_TAG_LONG, ttl=0):
        self.used.add((slot, key))
        row = self._row(slot, _PUT[self.types[slot]], key, tag, a, ttl)
        r = _table_region(slot, 0, key)
        if (slot, key) not in self.bound[r]:
            if self.eager:
                self._launch((r,))
            if len(self.bound[r]) >= _REGION:
                self.misfit.append(row)
                self._launch()  # (the row ends its call; the next call's launch compacts)
                return row
            self.bound[r].add((slot, key))
        self.dead[r].discard((slot, key))
        self.live[slot].add(key)
        return row

    def overfill(self, slots, region):
        """Fresh keys of `slots` into `region` until it is fully bound, then one more: a put that does not fit."""
        while True:
            full = self.room(region) == 0
            s = slots[len(self) % len(slots)]
            row = self.put(s, self.fresh(s, region), a=len(self) % 5)
            if full:
                return row

    def _absent(self, slot, key):
        r = _table_region(slot, 0, key)
        if (slot, key) in self.bound[r]:
            self.dead[r].add((slot, key))

    def remove(self, slot, key):
        self.live[slot].discard(key)
        self._absent(slot, key)
        return self._row(slot, _REMOVE[self.types[slot]], key, abi.CC_TAG_NULL)

    def get(self, slot, key):
        return self._row(slot, _GET[self.types[slot]], key, abi.CC_TAG_NULL)

    def size(self, slot):
        return self._row(slot, _SIZE[self.types[slot]], 0, abi.CC_TAG_NULL)

    def is_empty(self, slot):
        return self._row(slot, _ISEMPTY[self.types[slot]], 0, abi.CC_TAG_NULL)

    def contains_value(self, slot, a):
        assert self.types[slot] == M_
        return self._row(slot, abi.CC_OP_MAP_CONTAINSVALUE, 0, abi.CC_TAG_LONG, a)

    def clear(self, slot, delete=False):
        for k in self.live[slot]:
            self._absent(slot, k)
        self.live[slot] = set()
        return self._row(slot, abi.CC_OP_DELETE if delete else _CLEAR[self.types[slot]], 0, abi.CC_TAG_NULL)

    def some_live(self, slot, count):
        keys = sorted(self.live[slot])
        return [keys[i] for i in self.rng.permutation(len(keys))[:count]]

    def batch(self, lo=0):
        rows = self.rows[lo:]
        inst, op, flags, key, a, aux = (np.array(c) for c in zip(*rows))
        n = len(rows)
        at = np.arange(lo, lo + n, dtype=np.uint64)
        return Batch.from_columns(index=at + np.uint64(self.index0), time=at // np.uint64(self.step) + np.uint64(self.t0),
                                  inst=inst.astype(np.uint32), op=op.astype(np.uint8), flags=flags.astype(np.uint8),
                                  key=key.astype(np.uint64), a=a.astype(np.uint64),
                                  aux=aux.astype(np.int64).view(np.uint64))


def _keyed_engine(types):
    from copycat_amd.engine import Engine

    R = len(types)
    return Engine(R, R + 8, 1 << 14, map_capacity=1024, flags=abi.CC_CFG_TIMERS_DEFERRED)


def _keyed_pair(types):
    """An engine and an oracle holding resource r (instance slot r) of types[r]: one table of two regions."""
    from oracle.oracle_py import Oracle

    R = len(types)
    E = _keyed_engine(types)
    O = Oracle(R, R + 8, abi.CC_CFG_TIMERS_DEFERRED)
    for s, t in enumerate(types):
        for X in (E, O):
            X.resource_create(s, int(t))
            X.instance_open(s, s, 1000 + s, 7)
    return E, O


def _plain(engines, O, b, events=False):
    """One batch through the plain entry point on every engine and on the oracle: results (and events) agree.  Reads
    nothing that drains the leak log."""
    s2, v2 = O.apply(b)
    oe, _, _ = _oracle_events(O)
    for X in engines:
        if events:
            s, v, ev = X.apply_host_events(b, capacity=max(8 * len(b), 4096))
            member = ev["code"] == abi.CC_EV_MEMBER
            _assert_same_events({k: ev[k][~member] for k in _EVK}, oe, "oracle")
        else:
            s, v = X.apply_host(b)
        _assert_same_rows(s, v, s2, v2, "oracle")


def _report(name, **counts):
    print(f"[prefix scenario {name}] " + ", ".join(f"{k}={v}" for k, v in counts.items()))


# ---- A. the multimap leak log across a region stop -----------------------------------------------------------------
_A_TYPES = (MM_, M_, MM_, M_)


@functools.lru_cache(maxsize=None)
def _scenario_a():
    """(batch 1, batch 2, index of the last row).  Batch 1: 320 multimap Puts on six keys of each multimap (every Put
    commit stays in the log, A18: 320 leak-log records).  Batch 2: more of those Puts, then distinct map and multimap
    keys until region 0 has been offered four keys too many (Puts on the old keys between and after them), removes of
    400 keys, new keys (the first into each full region does not fit: the next launch compacts it), and a last few keys
    too many."""
    K = _Keyed(_A_TYPES, seed=4101)
    old = {s: [K.fresh(s, i % 2) for i in range(6)] for s in (0, 2)}
    for i in range(320):
        s = (0, 2)[i % 2]
        K.put(s, old[s][(i // 2) % 6], a=i)
    n1 = len(K)

    def leak():
        s = (0, 2)[len(K) % 2]
        K.put(s, old[s][int(K.rng.integers(6))], a=len(K))

    for _ in range(40):
        leak()
    filled = {s: [] for s in range(4)}
    i = 0
    while K.room(0) > 0 or K.room(1) > 30:
        s = i % 4
        r = 0 if K.room(0) > 0 and (i % 2 == 0 or K.room(1) <= 30) else 1
        k = K.fresh(s, r)
        K.put(s, k, a=i % 5)
        filled[s].append(k)
        if i % 9 == 0:
            leak()
        if i % 11 == 0:
            K.get(s, filled[s][int(K.rng.integers(len(filled[s])))])
        i += 1
    for j in range(4):  # four keys too many for region 0, leaking rows between them
        K.put(j % 4, K.fresh(j % 4, 0), a=j)
        for _ in range(5):
            leak()
    for s in range(4):
        for k in K.some_live(s, 100):
            if k not in old.get(s, ()):
                K.remove(s, k)
    for j in range(200):  # new keys: the first into each region meets it fully bound, the rest fit after compaction
        K.put(j % 4, K.fresh(j % 4, (j // 4) % 2), a=j % 5)
        if j % 7 == 0:
            leak()
    for r in (0, 1):
        while K.room(r) > 0:
            s = len(K) % 4
            K.put(s, K.fresh(s, r), a=3)
        for j in range(2):
            s = (1, 2)[j]
            K.put(s, K.fresh(s, r), a=4)
            leak()
    for _ in range(30):
        leak()
    return K, n1


def _a_batches():
    K, n1 = _scenario_a()
    b = K.batch()
    return K, b.slice(0, n1), b.slice(n1, len(b)), len(b)


@pytest.mark.parametrize("variant", ["read_at_first_stop", "read_at_end", "snapshot_at_first_stop"])
def test_prefix_multimap_leak_log_across_region_stop(variant):
    """Two multimaps and two maps in one table.  The previous batch's 320 multimap Put commits are still in the device
    leak log (nothing that drains it is read) when a prefix apply bisects on a full region: its checkpoint has to bring
    back a log whose records the failing attempt drained and overwrote.  read_at_first_stop compares every reader,
    the retained sets and the bitmap included, right after the first stop; read_at_end reads nothing that drains until
    the batch is exhausted, so errors of several rollbacks add up; snapshot_at_first_stop takes the snapshot (the
    third consumer of the log) right after the first stop, restores it into a fresh engine and drives both to the end.
    Two replicas apply the applied rows through apply_host, call for call: every reader agrees with them after each
    stop, and the snapshot bytes too where the two replicas' own snapshots agree.  On this engine they do not (the
    control fails: two replicas fed the same batches through apply_host snapshot to different bytes; one launch's
    multimap Puts append to the leak log, and its keys claim table slots, in whatever order the workgroups run), so the
    byte comparison is not asserted here and the reader-level comparisons -- entries, retained sets, bitmap and count,
    applied index, every result row -- stand in for it."""
    types = _A_TYPES
    K, b1, b2, nidx = _a_batches()
    E, O = _keyed_pair(types)
    reps = [_keyed_pair(types)[0] for _ in range(2)]
    _plain([E] + reps, O, b1)
    assert all(len(O.retained(s)) > 0 for s in (0, 2))  # the oracle retains Put commits of batch 1
    P, M = _Prefix(E, b2, "region"), _Mirror(O, b2, reps)
    mm_put = np.nonzero(b2.op == abi.CC_OP_MMAP_PUT)[0]
    early = variant == "read_at_first_stop"

    def after(stopped):
        if stopped:
            _compare(P, M, E, types, drain=early, nidx=nidx)

    assert _drive(P, M, until_stop=True, after_call=after), "no region filled"
    first = P.calls[-1]
    assert 0 < first[2] < first[1], first       # a bisected stop: some rows applied, some not
    tail = _tail_rows(P, mm_put)
    assert tail > 0                             # leaking rows were rolled back
    F = P2 = M2 = None
    if variant == "snapshot_at_first_stop":
        F = _keyed_engine(types)
        F.restore(E.snapshot())
        _, O2 = _keyed_pair(types)  # a second oracle brought to the same point, to follow F's own calls
        O2.apply(b1)
        for lo, _, a in P.calls:
            if a:
                O2.apply(b2.slice(lo, lo + a))
        _oracle_events(O2)
        P2, M2 = _Prefix(F, b2, "region", pos=P.pos), _Mirror(O2, b2)
        _drive(P2, M2)
    _drive(P, M, after_call=after)
    _compare(P, M, E, types, drain=True, nidx=nidx)
    same_bytes = _snapshot_bytes_equal(P, M)
    assert same_bytes is not False, "the snapshot differs from the replicas' although theirs agree"
    if F is not None:
        _compare(P2, M2, F, types, drain=True, nidx=nidx, who="restored engine")
    _report(f"A/{variant}", rows=len(b2), stops=P.stops(), bisected=P.bisected(), predicted=len(K.misfit),
            leaking_rows_rolled_back=tail, snapshot_bytes=same_bytes)
    assert 3 <= P.stops() <= 40 and P.bisected() >= 1
    assert len(P.failed) == P.stops()


# ---- coordination engines (resource r owns instance slots r*K + k, as tests/test_gpu_coord._setup lays them out) ----
def _coord_engine(types, K, flags, coord_cap=0, create=True):
    from copycat_amd.engine import Engine

    R = len(types)
    E = Engine(R, R * K + 8, 1 << 14, flags=flags, max_events=1 << 16, coord_cap=coord_cap)
    if create:
        _coord_open(E, types, K)
    return E


def _coord_oracle(types, K, flags):
    from oracle.oracle_py import Oracle

    O = Oracle(len(types), len(types) * K + 8, flags & abi.CC_CFG_TIMERS_DEFERRED)
    _coord_open(O, types, K)
    return O


def _coord_open(X, types, K):
    for r, t in enumerate(types):
        X.resource_create(r, int(t))
        for k in range(K):
            X.instance_open(r * K + k, r, 1000 + r * K + k, 7 + k)


def _adds_per_resource(b, types, K):
    """Rows that can add an entry to a coordination collection, per resource (host_path.hip adds_entry): the prefix
    apply cuts a part where a resource's entries plus these could pass coord_cap, and the scenarios below want every
    first attempt to be the whole rest of the batch."""
    R = len(types)
    res = np.minimum(b.inst // K, R - 1)
    ty = np.asarray(types)[res]
    add = (((ty == L) & (b.op == abi.CC_OP_LOCK_LOCK) & (b.aux != 0)) | ((ty == E_) & (b.op == abi.CC_OP_ELECT_LISTEN)) |
           ((ty == G) & (b.op == abi.CC_OP_GROUP_JOIN)) | ((ty == V) & (b.op == abi.CC_OP_VALUE_LISTEN))) & (b.inst < R * K)
    return np.bincount(res[add], minlength=R)


def _ev4(ev):
    return sorted(zip(ev["target"].tolist(), ev["code"].tolist(), ev["tag"].tolist(), ev["payload"].tolist()))


# ---- B. value re-listen leaks across an event-stream stop --------------------------------------------------------------
_B_FLAGS = abi.CC_CFG_TIMERS_DEFERRED | abi.CC_CFG_VALUE_EVENTS | abi.CC_CFG_VALUE_RETAINED
_B_R, _B_K = 64, 3


@functools.lru_cache(maxsize=None)
def _scenario_b():
    """Batch 1: every instance listens twice (AtomicValueState.listen replaces the session's commit without clean()ing
    it: one leak-log record per instance).  Batch 2: 3,000 rows of set (publishes to the value's three listeners), CAS
    on small values (about one in four succeeds and publishes) and further re-listens (each leaks)."""
    ni = _B_R * _B_K
    b1 = Batch.from_columns(index=np.arange(1, 2 * ni + 1, dtype=np.uint64), time=np.ones(2 * ni, np.uint64),
                            inst=np.tile(np.arange(ni, dtype=np.uint32), 2),
                            op=np.full(2 * ni, abi.CC_OP_VALUE_LISTEN, np.uint8))
    rng = np.random.default_rng(4201)
    n = 3000
    op = rng.choice(np.array([abi.CC_OP_VALUE_SET, abi.CC_OP_VALUE_CAS, abi.CC_OP_VALUE_LISTEN], np.uint8), n,
                    p=[0.45, 0.25, 0.30])
    lng = abi.CC_TAG_LONG
    flags = np.where(op == abi.CC_OP_VALUE_SET, abi.cc_flags(lng),
                     np.where(op == abi.CC_OP_VALUE_CAS, abi.cc_flags(lng, lng), 0))
    a = np.where(op == abi.CC_OP_VALUE_LISTEN, 0, rng.integers(0, 4, n))
    bb = np.where(op == abi.CC_OP_VALUE_CAS, rng.integers(0, 4, n), 0)
    b2 = Batch.from_columns(index=np.arange(2 * ni + 1, 2 * ni + 1 + n, dtype=np.uint64),
                            time=np.uint64(2) + np.arange(n, dtype=np.uint64) // np.uint64(8),
                            inst=rng.integers(0, ni, n).astype(np.uint32), op=op, flags=flags.astype(np.uint8),
                            a=a.astype(np.uint64), b=bb.astype(np.uint64))
    return b1, b2, 2 * ni + n


@pytest.mark.parametrize("variant", ["read_at_first_stop", "read_at_end"])
def test_prefix_value_relisten_leaks_across_event_stop(variant):
    """64 AtomicValues with three listening instances each, value events and retained commits on.  The previous batch's
    192 re-listen leaks are still in the device leak log when a prefix apply bisects on an event stream of 300: the
    rolled-back attempts drain and overwrite that log, and every attempt leaks again.  The two read variants of scenario
    A; value_retained() (which drains nothing) is compared at every stop.  Two replicas apply the applied rows through
    apply_host_events, call for call, and agree in every reader and event, and in the snapshot's bytes where the
    replicas' own snapshots agree."""
    types = [V] * _B_R
    b1, b2, nidx = _scenario_b()
    E, O = _coord_engine(types, _B_K, _B_FLAGS), _coord_oracle(types, _B_K, _B_FLAGS)
    reps = [_coord_engine(types, _B_K, _B_FLAGS) for _ in range(2)]
    _plain([E] + reps, O, b1, events=True)
    assert all(len(O.retained(r)) == 2 * _B_K for r in range(_B_R))  # per instance: its listener's commit and a leak
    assert int(_adds_per_resource(b2, types, _B_K).max()) + _B_K < abi.CC_VALUE_LISTENERS  # parts are never cut
    P, M = _Prefix(E, b2, "events", capacity=300), _Mirror(O, b2, reps, events=True)
    early = variant == "read_at_first_stop"

    def after(stopped):
        if stopped:
            _compare(P, M, E, types, drain=early, nidx=nidx, vret=True)

    assert _drive(P, M, until_stop=True, after_call=after), "the event stream never filled"
    first = P.calls[-1]
    assert 0 < first[2] < first[1], first
    tail = _tail_rows(P, np.nonzero(b2.op == abi.CC_OP_VALUE_LISTEN)[0])
    assert tail > 0  # re-listens (leaking rows) were rolled back
    _drive(P, M, after_call=after)
    _compare(P, M, E, types, drain=True, nidx=nidx, vret=True)
    assert np.count_nonzero(O.value_retained()) > _B_R // 2
    same_bytes = _snapshot_bytes_equal(P, M)
    assert same_bytes is not False, "the snapshot differs from the replicas' although theirs agree"
    _report(f"B/{variant}", rows=len(b2), stops=P.stops(), bisected=P.bisected(), leaking_rows_rolled_back=tail,
            events=len(P.events()["pos"]), snapshot_bytes=same_bytes)
    assert 3 <= P.stops() <= 40 and P.bisected() >= 1 and not P.failed


# ---- C. the coordination mix with schedule timers across event-stream stops --------------------------------------------
_C_K, _C_CAP = 3, 256


@functools.lru_cache(maxsize=None)
def _scenario_c():
    """The stream of tests/test_gpu_retained.test_retained_coordination_parity at its small shape, 4,000 rows long (16
    locks, elections, groups and values with 3 instances each, 40 MembershipGroup.schedule rows with delays of 1..399
    ms, the clock advancing 1 ms every 8 rows, 500 ms in all: timers come due at boundaries inside the batch)."""
    from copycat_amd.workload import coord_random_stream
    from tests.test_gpu_retained import _with_schedules

    n, R, K, seed = 4_000, 16, _C_K, 31
    types = np.array([L, E_, G, V] * ((R + 3) // 4), np.uint8)[:R]
    rng = np.random.default_rng(seed)
    b = _with_schedules(coord_random_stream(n, types, K, R * K + 8, seed=seed), types, K, R * K + 8, rng, 40)
    return types, b


@pytest.mark.parametrize("variant", ["read_at_end", "snapshot_at_first_stop"])
def test_prefix_coordination_schedule_timers_across_event_stops(variant):
    """Locks, elections, groups (with schedule timers) and values with listeners through prefix applies with an event
    stream of 300: rolled-back attempts arm schedule timers, fire others at the boundaries they cross and leak
    re-listens, none of which may survive.  (coord_cap 256, so no part is ever cut at a collection bound and every
    first attempt is the whole rest of the batch.)  After the batch two clients close and the clock passes the last
    deadline on every side: the close and timer events and the retained sets agree again.  snapshot_at_first_stop:
    the snapshot taken right after the first stop is restored into a fresh engine that finishes the batch on its own.
    Two replicas follow through apply_host_events, call for call."""
    from tests.test_gpu_coord import FLAGS

    types, b = _scenario_c()
    K, flags, nidx, R = _C_K, FLAGS | abi.CC_CFG_VALUE_RETAINED, len(b), len(types)
    assert int(_adds_per_resource(b, types, K).max()) + K < _C_CAP
    E, O = _coord_engine(types, K, flags, _C_CAP), _coord_oracle(types, K, flags)
    reps = [_coord_engine(types, K, flags, _C_CAP) for _ in range(2)]
    P, M = _Prefix(E, b, "events", capacity=300), _Mirror(O, b, reps, events=True)
    pending = []

    def after(stopped):
        if stopped:
            pending.append(int(O.pending_timers()))
            _compare(P, M, E, types, drain=False, nidx=nidx, vret=True)

    assert _drive(P, M, until_stop=True, after_call=after), "the event stream never filled"
    first = P.calls[-1]
    assert 0 < first[2] < first[1], first
    sched_tail = _tail_rows(P, np.nonzero(b.op == abi.CC_OP_GROUP_SCHEDULE)[0])
    relisten_tail = _tail_rows(P, np.nonzero(b.op == abi.CC_OP_VALUE_LISTEN)[0])
    assert sched_tail > 0  # schedule rows were rolled back
    engines = [(E, P, M, "prefix engine")]
    if variant == "snapshot_at_first_stop":
        F = _coord_engine(types, K, flags, _C_CAP, create=False)
        F.restore(E.snapshot())
        O2 = _coord_oracle(types, K, flags)
        for lo, _, a in P.calls:
            O2.apply(b.slice(lo, lo + a))
        _oracle_events(O2)
        P2, M2 = _Prefix(F, b, "events", capacity=300, pos=P.pos), _Mirror(O2, b)
        _drive(P2, M2)
        engines.append((F, P2, M2, "restored engine"))
    _drive(P, M, after_call=after)
    assert max(pending) > 0  # a schedule timer was pending at a stop
    fired = int((_cat(M.oe["src"], np.uint8) == abi.CC_EVSRC_TIMER).sum())
    assert fired > 0         # and timers fired at boundaries inside the batch
    for X, Px, Mx, who in engines:
        _compare(Px, Mx, X, types, drain=True, nidx=nidx, vret=True, who=who)
    same_bytes = _snapshot_bytes_equal(P, M)
    _report(f"C/{variant}", rows=len(b), stops=P.stops(), bisected=P.bisected(), schedule_rows_rolled_back=sched_tail,
            relistens_rolled_back=relisten_tail, timers_pending_at_stops=pending, timer_events_in_batch=fired,
            events=len(P.events()["pos"]), snapshot_bytes=same_bytes)
    assert same_bytes is not False, "the snapshot differs from the replicas' although theirs agree"
    # two clients close (group members dropped without clean(), listeners cleaned), then every pending timer fires
    now = int(b.time[-1]) + 1000
    for X, Px, Mx, who in engines:
        every = [X] + [rp["E"] for rp in Mx.rep]
        for client in (7, 8):
            Mx.O.session_close(client)
            want = _ev4(Mx.O.take_events())
            for Y in every:
                assert _ev4(Y.sessions_close([client], capacity=1 << 16)[1]) == want, (who, client)
        want_state = _state(Mx.O, types, True, nidx, True, oracle=True)
        for Y in every:
            _assert_same_state(_state(Y, types, True, nidx, True), want_state, who, "oracle")
        Mx.O.advance_time(now)
        want = _ev4(Mx.O.take_events())
        for Y in every:
            ev = Y.advance_time_events(now, capacity=4096)
            assert _ev4(ev) == want and (ev["src"] == abi.CC_EVSRC_TIMER).all(), who
        want_state = _state(Mx.O, types, True, nidx, True, oracle=True)
        for Y in every:
            _assert_same_state(_state(Y, types, True, nidx, True), want_state, who, "oracle")
    assert 3 <= P.stops() <= 40 and P.bisected() >= 1 and not P.failed


def _wide_answers(b, P, ops):
    """Per whole-map op: how many of its rows were applied with an OK status."""
    ok = abi.status_code(P.gs) == abi.CC_ST_OK
    return {int(o): int(((b.op == o) & (P.gs != 0xFF) & ok).sum()) for o in ops}


# ---- D. entering TTL mode on either side of a stop ---------------------------------------------------------------------
_D_TYPES = (M_, M_, M_, M_)


@functools.lru_cache(maxsize=None)
def _scenario_d(ttl_first):
    """Four maps on an engine that has seen no ttl > 0 row: puts until region 0 has been offered a key too many, Puts
    with ttls of 100..249 ms on 300 live keys (the clock advances 1 ms every 4 rows: they expire inside the batch, but
    not before the next stop), another key too many, a clear of the small map 3, removes, new keys (some with short
    ttls), keys too many for both regions, and Puts whose timers are still pending when the batch ends; size, isEmpty
    and containsValue rows throughout (values are never null, so containsValue does not depend on HashMap order).
    ttl_first = "before_first_stop" also puts 40 ttl rows early in the fill, before any row that does not fit.  (The
    table model knows nothing of expiry: after the first timers fire, more keys fit than it predicts.)"""
    K = _Keyed(_D_TYPES, seed=4301)
    keys = {s: [] for s in range(3)}

    def wide():
        s = len(K) % 3
        (K.size, K.is_empty, lambda x: K.contains_value(x, len(K) % 5))[(len(K) // 3) % 3](s)

    def ttl_puts(count, lo, hi):
        for j in range(count):
            s = j % 3
            K.put(s, keys[s][int(K.rng.integers(len(keys[s])))], a=j % 5, ttl=int(K.rng.integers(lo, hi)))

    for j in range(60):  # map 3 stays small: it is cleared between two stops
        K.put(3, K.fresh(3, j % 2), a=j % 5)
    i = 0
    while K.room(0) > 0 or K.room(1) > 30:
        s = i % 3
        k = K.fresh(s, 0 if K.room(0) > 0 and (i % 2 == 0 or K.room(1) <= 30) else 1)
        K.put(s, k, a=i % 5)
        keys[s].append(k)
        if i % 97 == 0:
            wide()
        if i == 200 and ttl_first == "before_first_stop":
            ttl_puts(40, 100, 250)
        i += 1
    K.overfill((0, 1, 2), 0)       # the first key too many
    for j in range(3):
        wide()
        K.get(j, keys[j][j])
    ttl_puts(300, 100, 250)        # (none of these timers fires within the next 400 rows)
    K.overfill((0, 1, 2), 0)       # TTL mode is live at this stop
    for j in range(9):
        wide()
    K.clear(3)
    K.size(3)
    for s in (0, 1, 2):
        for k in K.some_live(s, 50):
            K.remove(s, k)
        wide()
    for j in range(100):           # the first new key of a fully bound region does not fit; the next launch compacts it
        K.put(j % 3, K.fresh(j % 3, (j // 3) % 2), a=j % 5, ttl=int(K.rng.integers(5, 100)) if j % 4 == 0 else 0)
        if j % 29 == 0:
            wide()
    K.overfill((0, 1, 2), 1)
    K.overfill((0, 1, 2), 0)
    ttl_puts(30, 5_000, 6_000)     # timers still pending when the batch ends
    for j in range(12):
        wide()
    return K, K.batch()


@pytest.mark.parametrize("ttl_first", ["after_first_stop", "before_first_stop"])
def test_prefix_ttl_mode_entry_around_a_region_stop(ttl_first):
    """The engine enters TTL mode for good at a batch's first ttl > 0 map row (the event buffers grow with it).
    after_first_stop: that row lies behind the first row that does not fit, so the full attempt enters TTL mode, the
    rollback has to leave it, and a later call enters it for real.  before_first_stop: the batch is in TTL mode before
    anything is rolled back.  Every reader (draining is fine here) agrees with the oracle after every call, and again
    after the clock has passed every deadline on both sides."""
    types = _D_TYPES
    K, b = _scenario_d(ttl_first)
    nidx = len(b)
    E, O = _keyed_pair(types)
    P, M = _Prefix(E, b, "region"), _Mirror(O, b)
    _drive(P, M, after_call=lambda stopped: _compare(P, M, E, types, drain=True, nidx=nidx))
    ttl_rows = np.nonzero(b.aux.view(np.int64) > 0)[0]
    first_failed = P.failed[0] if P.failed else len(b)
    entered_in_rollback = bool(ttl_rows[0] > first_failed)  # (the first attempt of call 1 is the whole batch)
    applied_ttl = int((P.gs[ttl_rows] != 0xFF).sum())
    wide = _wide_answers(b, P, (abi.CC_OP_MAP_SIZE, abi.CC_OP_MAP_ISEMPTY, abi.CC_OP_MAP_CONTAINSVALUE, abi.CC_OP_MAP_CLEAR))
    live = sum(len(O.map_entries(s)[0]) for s in range(4))
    now = int(b.time[-1]) + 10_000
    E.advance_time(now)
    O.advance_time(now)
    O.take_events()
    expired = live - sum(len(O.map_entries(s)[0]) for s in range(4))
    _report(f"D/{ttl_first}", rows=len(b), stops=P.stops(), bisected=P.bisected(), failed=P.failed, predicted=K.misfit,
            ttl_mode_entered_in_rolled_back_attempt=entered_in_rollback, ttl_rows_applied=applied_ttl,
            expired_by_final_advance=expired, wide_rows_answered=wide)
    _assert_same_state(_state(E, types, True, nidx), _state(O, types, True, nidx, oracle=True), "prefix engine", "oracle")
    assert 3 <= P.stops() <= 40 and P.bisected() >= 1 and P.calls[0][0] == 0 and P.calls[0][2] < P.calls[0][1]
    assert entered_in_rollback == (ttl_first == "after_first_stop")
    assert applied_ttl > 200
    assert all(v > 0 for v in wide.values()), wide
    assert expired > 0  # timers were still pending at the end of the batch


# ---- E. the keyed mix with whole-map rows ------------------------------------------------------------------------------
_E_TYPES = (M_, M_, S_, MM_, M_, S_, MM_)


def _feed_tree_row(K, slot, row):
    op, k, t, v = row
    if op == abi.CC_OP_MAP_PUT:
        K.put(slot, int(k), a=int(v), tag=int(t))
    elif op == abi.CC_OP_MAP_REMOVE:
        K.remove(slot, int(k))
    elif op == abi.CC_OP_MAP_CONTAINSVALUE:
        K.contains_value(slot, int(v))
    else:
        raise AssertionError(op)


@functools.lru_cache(maxsize=None)
def _scenario_e():
    """(builder, rows of the previous plain batch).  Map 0 is tests/test_gpu_map_tree's map (30 keys in one bin, a tree
    bin at capacity 64, then 300 more keys: a big HashMap model past 64 buckets; stored nulls and containsValue rows
    decided by its order), filled and churned in the previous batch, which also asks maps 1 and 4 their size and
    containsValue (their kMfSize / kMfCv flags are set at the checkpoint).  The prefix batch goes on churning map 0 while
    maps, sets and multimaps 1..6 take distinct keys until region 0 has been offered three too many, hot keys, removes,
    a clear, a Delete, new keys and a few too many again, with size / isEmpty / containsValue rows throughout."""
    from tests.test_gpu_map_tree import _tree_rows

    K = _Keyed(_E_TYPES, seed=4401, eager=True)
    tree = _tree_rows(np.random.default_rng(4402), 30, 300, 1_400)
    for row in tree[:800]:
        _feed_tree_row(K, 0, row)
    keys = {s: [] for s in range(1, 7)}
    for j in range(120):
        s = 1 + j % 6
        k = K.fresh(s, j % 2)
        K.put(s, k, a=j % 5)
        keys[s].append(k)
    for s in (1, 4):
        K.size(s)
        K.contains_value(s, 3)
        K.contains_value(s, 77)
    n1 = len(K)
    churn = list(tree[800:])

    def wide():
        s = 1 + len(K) % 6
        if K.types[s] == M_ and (len(K) // 6) % 2:
            K.contains_value(s, len(K) % 6)
        else:
            (K.size, K.is_empty)[(len(K) // 6) % 2](s)

    def extras(i):
        if i % 10 == 0 and churn:
            _feed_tree_row(K, 0, churn.pop(0))
        if i % 83 == 0:
            wide()

    i = 0
    while K.room(0) > 0 or K.room(1) > 30:
        s = 1 + i % 6
        k = K.fresh(s, 0 if K.room(0) > 0 and (i % 2 == 0 or K.room(1) <= 30) else 1)
        K.put(s, k, a=i % 5)
        keys[s].append(k)
        extras(i)
        i += 1
    every = (1, 2, 3, 4, 5, 6)
    K.overfill(every, 0)  # the first key too many (the next launch compacts away the keys map 0's churn removed)
    hot = {1: keys[1][0], 2: keys[2][0]}
    for j in range(120):  # hot keys: one key of map 1 and one element of set 2 put / read / removed over and over
        s = (1, 2)[j % 2]
        (K.put, K.get, K.remove, K.put)[(j // 2) % 4](s, hot[s])
    K.overfill(every, 0)  # compacted keys are live at this stop
    for s in every:
        for k in K.some_live(s, 40):
            K.remove(s, k)
        wide()
    for j in range(60):
        if churn:
            _feed_tree_row(K, 0, churn.pop(0))
    K.clear(5)            # a set of some 600 elements
    K.size(5)
    for j in range(120):  # the first new key of a fully bound region does not fit; the next launch compacts it
        s = 1 + j % 6
        K.put(s, K.fresh(s, (j // 6) % 2), a=j % 5)
        extras(j)
    K.overfill(every, 1)
    K.overfill(every, 0)
    K.clear(6, delete=True)
    K.clear(4)
    for j in range(30):
        s = 1 + j % 6
        K.put(s, K.fresh(s, j % 2), a=j % 5)
    for j in range(12):
        wide()
    while churn:
        _feed_tree_row(K, 0, churn.pop(0))
    return K, n1


def _removed_before_stops(b, P):
    """Per stop of a call after the first: the keys a remove row of an earlier call took out that are still absent when
    the call starts.  Its first launch finds the regions more than 3/4 bound (a stop left them full) and compacts them:
    those keys move into the compacted-key set, which is then live at the stop."""
    absent, out = set(), []
    removes, puts = set(_REMOVE.values()), set(_PUT.values())
    for lo, m, a in P.calls:
        if a < m and lo > 0:
            out.append(len(absent))
        for i in range(lo, lo + a):
            op, key = int(b.op[i]), (int(b.inst[i]), int(b.key[i]))
            if op in removes:
                absent.add(key)
            elif op in puts:
                absent.discard(key)
    return out


def test_prefix_keyed_mix_with_whole_map_rows():
    """Maps, sets and multimaps in one table, one map followed by a big HashMap model: region stops with size,
    containsValue, clear and Delete rows, hot keys and compaction around them.  Every reader (the retained sets and
    the bitmap included: draining is fine here, scenario A covers the undrained log) agrees with the oracle after
    every call."""
    types = _E_TYPES
    K, n1 = _scenario_e()
    b = K.batch()
    b1, b2, nidx = b.slice(0, n1), b.slice(n1, len(b)), len(b)
    E, O = _keyed_pair(types)
    _plain([E], O, b1)
    assert E.counters()[4] == 1  # map 0 is followed by a big model before the prefix batch
    for s in (1, 4):
        assert {abi.CC_OP_MAP_SIZE, abi.CC_OP_MAP_CONTAINSVALUE} <= set(b1.op[b1.inst == s].tolist())
    P, M = _Prefix(E, b2, "region"), _Mirror(O, b2)
    big = []

    def after(stopped):
        if stopped:
            big.append(E.counters()[4])
        _compare(P, M, E, types, drain=True, nidx=nidx)

    _drive(P, M, after_call=after)
    compacted = _removed_before_stops(b2, P)
    wide = _wide_answers(b2, P, (abi.CC_OP_MAP_SIZE, abi.CC_OP_MAP_CONTAINSVALUE, abi.CC_OP_MAP_CLEAR, abi.CC_OP_SET_SIZE,
                                 abi.CC_OP_SET_CLEAR, abi.CC_OP_MMAP_SIZE, abi.CC_OP_DELETE))
    _report("E", rows=len(b2), stops=P.stops(), bisected=P.bisected(), failed=P.failed,
            predicted=[r - n1 for r in K.misfit], big_models_at_stops=big, compacted_keys_at_stops=compacted,
            wide_rows_answered=wide)
    assert 3 <= P.stops() <= 40 and P.bisected() >= 1
    assert min(big) >= 1                      # a big model was live at every stop
    assert compacted and max(compacted) > 0   # compacted keys were live at a stop
    assert all(v > 0 for v in wide.values()), wide
