"""GPU: cc_snapshot_restore_grow -- a snapshot restored into an engine created with a larger coord_cap and / or
map_capacity (copycat_amd/csrc/grow.hip migrates the map table, the compacted-key set and the coordination blocks).

The way out of a prefix stop on a fixed capacity: snapshot at the stop, a grown engine, resume at the stopped row, and
no commit fails that the reference would have applied.  Every result, event and reader is compared, by integer
equality, with the oracle that never had a limit (oracle.oracle_py.Oracle; topics and buses, which the oracle does not
model, with the Python restatements the topic and bus suites use)."""
import struct

import numpy as np
import pytest

from copycat_amd import abi
from copycat_amd.batch import Batch
from tests.test_gpu_coord import E_, FLAGS, G, L, V, _check_batch, _check_state, _setup
from tests.test_gpu_map import _assert_maps, _assert_rows, _engines
from tests.test_gpu_prefix import _assert_same_state, _map_rows, _state

pytestmark = pytest.mark.gpu

Q, T, B = abi.CC_RES_QUEUE, abi.CC_RES_TOPIC, abi.CC_RES_BUS
M_, S_, MM_ = abi.CC_RES_MAP, abi.CC_RES_SET, abi.CC_RES_MULTIMAP


def _invalid(fn):
    from copycat_amd.engine import EngineError

    with pytest.raises(EngineError) as ei:
        fn()
    assert ei.value.rc == abi.CC_ERR_INVALID


# ---- 1. a full map region, then grown -------------------------------------------------------------------------------
def test_map_region_full_then_grown_no_commit_fails():
    """The key stream of test_prefix_apply_map_region_full_fails_one_commit on two table regions (map_capacity 1,024):
    at the first stop the engine is grown to eight regions (a grow by two bits, from a region that is full) and the
    host resumes at the stopped row.  About 4,900 distinct keys over 8 regions of 2,048 leave a factor 3 of room per
    region: no later stop, no failed commit, and the whole batch equals the oracle applying the whole batch."""
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
    for k in np.arange(600, dtype=np.uint64) * np.uint64(104729) + np.uint64(1 << 40):
        keys.append(k)
        ops.append(abi.CC_OP_MAP_PUT)
    b = _map_rows(keys, ops)
    n = len(b)
    gs, gv = np.zeros(n, np.uint8), np.zeros(n, np.uint64)
    pos, stops = 0, []
    while pos < n:
        rest = b.slice(pos, n)
        applied, s, v, _ = E.apply_host_prefix(rest)
        gs[pos:pos + applied] = s[:applied]
        gv[pos:pos + applied] = v[:applied]
        pos += applied
        if applied == len(rest):
            break
        stops.append(pos)
        assert len(stops) == 1, f"stopped again after the growth, at rows {stops}"
        info = E.snapshot_info(E.snapshot())
        assert info["map_capacity"] == 2048 and info["applied"] == pos  # (two regions: 4,096 entries)
        E = E.grown(map_capacity=8192)  # resume at the stopped row, not after it
    assert len(stops) == 1, "no region filled"
    _assert_rows(gs, gv, *O.apply(b))
    _assert_maps(E, O, [0])


# ---- 2. mixed tables --------------------------------------------------------------------------------------------------
def _halves(E, O, b, types, grow, nidx, fresh):
    """First half, grow, second half: results, every reader (map_entries of the keyed slots, value_state, the applied
    index, retained(slot) of every slot and the retained bitmap) before the growth, right after it and at the end.  A
    snapshot of the grown engine restores through plain restore into `fresh()` and continues bit-exact."""
    cut = len(b) // 2
    _assert_rows(*E.apply_host(b.slice(0, cut)), *O.apply(b.slice(0, cut)))
    want = _state(O, types, True, nidx, oracle=True)
    _assert_same_state(_state(E, types, True, nidx), want, "engine", "oracle")
    E2 = grow(E)
    _assert_same_state(_state(E2, types, True, nidx), want, "grown engine", "oracle")
    E3 = fresh()
    E3.restore(E2.snapshot())
    rest = b.slice(cut, len(b))
    s2, v2 = O.apply(rest)
    want = _state(O, types, True, nidx, oracle=True)
    for X, who in ((E2, "grown engine"), (E3, "engine restored from the grown engine's snapshot")):
        _assert_rows(*X.apply_host(rest), s2, v2)
        _assert_same_state(_state(X, types, True, nidx), want, who, "oracle")


def test_mixed_table_migrates_whole():
    """test_snapshot_restore_values_and_maps's batch (TTL mode, tombstones from removes, whole-map rows, String-handle
    keys with registered hashes, hot keys) with one Set and one MultiMap (Delete rows among theirs: DEAD entries), half
    of it on map_capacity 16,384; then 65,536 (two bits; the compacted-key set doubles too) and the second half."""
    from copycat_amd.engine import Engine
    from copycat_amd.workload import map_random_stream, value_random_stream
    from oracle.oracle_py import Oracle
    from tests.handles import register_key_strings
    from tests.test_gpu_map import _no_null_values, _with_barriers, _with_ttl
    from tests.test_gpu_multimap import _stream

    Vn, Mn = 256, 32
    slots, max_inst = Vn + Mn + 2, Vn + Mn + 2 + 8
    types = [V] * Vn + [M_] * Mn + [S_, MM_]
    bv = value_random_stream(60_000, Vn, max_inst, seed=101, hot=4, p_hot=0.2)
    bm = map_random_stream(60_000, Mn, max_inst, keys=64, first_inst=Vn, seed=102)
    _no_null_values(bm)
    _with_ttl(bm, 103)
    _with_barriers(bm, 0.002, 104, ops=np.array([abi.CC_OP_MAP_SIZE, abi.CC_OP_MAP_CONTAINSVALUE], np.uint8))
    bs = _stream(6_000, np.array([S_, MM_], np.uint8), 48, 105)
    bs.inst[:] = bs.inst + np.uint32(Vn + Mn)  # (its unknown instance, 5, becomes slot + 3: not opened either)
    parts = (bv, bm, bs)
    order = np.random.default_rng(7).permutation(sum(len(p) for p in parts))
    cols = {name: np.concatenate([getattr(p, name) for p in parts])[order] for name, _ in abi.BATCH_COLUMNS}
    cols["index"] = np.arange(1, len(order) + 1, dtype=np.uint64)
    cols["time"] = np.sort(cols["time"])
    b = Batch.from_columns(**cols)
    flags = abi.CC_CFG_TIMERS_DEFERRED | abi.CC_CFG_VALUE_RETAINED  # (retained(slot) of a value slot needs it)

    E = Engine(slots, max_inst, len(b), map_capacity=16384, flags=flags)
    O = Oracle(slots, max_inst, abi.CC_CFG_TIMERS_DEFERRED)
    for r, t in enumerate(types):
        E.resource_create(r, int(t))
        O.resource_create(r, int(t))
    E.instance_open_range(0, slots, 0, 1000, 7)
    for r in range(slots):
        O.instance_open(r, r, 1000 + r, 7)
    register_key_strings(E, O)  # (the grown engine gets them from the snapshot)
    _halves(E, O, b, types, lambda X: X.grown(map_capacity=65536), len(b),
            lambda: Engine(slots, max_inst, len(b), map_capacity=65536, flags=flags))
    assert Engine.snapshot_info(E.snapshot())["flags"] & abi.CC_SNAP_TTL  # (the batch did put the maps into TTL mode)


def test_small_map_models_survive_the_growth():
    """test_snapshot_after_overlapped_small_map_replay's set-up: small-map models, in-stream containsValue, size and
    clear rows, barrier containsValue on maps holding nulls, hot keys.  The growth moves every entry of the table, and
    the order-dependent answers after it still equal the oracle's."""
    from copycat_amd.engine import Engine
    from copycat_amd.workload import map_random_stream
    from oracle.oracle_py import Oracle
    from tests.handles import register_key_strings
    from tests.test_gpu_map import _cv_rows, _with_barriers

    M, n = 12, 160_000
    b = map_random_stream(n, M, M + 8, keys=20, seed=111, hot=2, p_hot=0.4)
    _cv_rows(b, 0.004, 111, clear_rate=0.0005)
    _with_barriers(b, 0.0015, 112, ops=np.array([abi.CC_OP_MAP_CONTAINSVALUE, abi.CC_OP_MAP_SIZE], np.uint8), p=[0.7, 0.3])
    E = Engine(M, M + 8, n, map_capacity=16384, sub_batch=16384)
    E.resource_create_range(0, M, M_)
    E.instance_open_range(0, M, 0, 1000, 7)
    O = Oracle(M, M + 8)
    for r in range(M):
        O.resource_create(r, M_)
        O.instance_open(r, r, 1000 + r, 7)
    register_key_strings(E, O)
    _halves(E, O, b, [M_] * M, lambda X: X.grown(map_capacity=65536), n,
            lambda: Engine(M, M + 8, n, map_capacity=65536, sub_batch=16384))


def test_one_more_region_bit():
    """The smallest growth of a table: one bit (map_capacity 1,024 -> 2,048, two regions -> four), 16 maps with
    removes and hot keys across it."""
    from copycat_amd.engine import Engine
    from copycat_amd.workload import map_random_stream

    M, n = 16, 20_000
    b = map_random_stream(n, M, M + 8, keys=64, seed=121, hot=2, p_hot=0.3)
    E, O = _engines(M, M + 8, n, 1024)
    _halves(E, O, b, [M_] * M, lambda X: X.grown(map_capacity=2048), n, lambda: Engine(M, M + 8, n, map_capacity=2048))


# ---- 3. coordination blocks -------------------------------------------------------------------------------------------
def _rows(spec, index0):
    """[(instance slot, op[, aux[, tag, a]])] as a Batch; index and clock advance by one per row"""
    n = len(spec)
    b = Batch(n)
    b.index[:] = np.arange(index0, index0 + n, dtype=np.uint64)
    b.time[:] = np.arange(index0, index0 + n, dtype=np.uint64)
    b.inst[:] = [x[0] for x in spec]
    b.op[:] = [x[1] for x in spec]
    b.aux[:] = np.array([x[2] if len(x) > 2 else 0 for x in spec], np.int64).view(np.uint64)
    b.flags[:] = [abi.cc_flags(x[3] if len(x) > 3 else 0) for x in spec]
    b.a[:] = np.array([x[4] if len(x) > 4 else 0 for x in spec], np.uint64)
    return b


def test_coordination_blocks_widen_wrapped_rings_included():
    """coord_cap 64 -> 256 (a factor 4) with one Lock, Election, Group, Queue, Topic, MessageBus and a Value with
    listeners.  The lock's waiter ring and the queue's ring have wrapped (64 entries, then 30 taken from the front,
    then 30 more: head 30, 64 live), the group is full, the bus has 40 members at the front of its block and 6
    registrations over 2 topics at its back.  Every reader equals the reference right after the growth; then every
    collection goes past 64 entries, with the results, the whole event stream and the readers the reference's."""
    from tests.test_gpu_bus import World

    LOCK, UNLOCK = abi.CC_OP_LOCK_LOCK, abi.CC_OP_LOCK_UNLOCK
    ADD, POLL = abi.CC_OP_QUEUE_ADD, abi.CC_OP_QUEUE_POLL
    LONG, HANDLE = abi.CC_TAG_LONG, abi.CC_TAG_HANDLE
    types, K = [L, E_, G, Q, T, B, V], 100
    w = World(types, K, flags=FLAGS, coord_cap=64)
    lk, el, gr, qu, tp, bu, va = (r * K for r in range(7))  # each resource's first instance slot
    spec = [(lk, LOCK, -1)] + [(lk + i, LOCK, -1) for i in range(1, 65)]            # a holder and 64 waiters
    spec += [(lk + i, UNLOCK) for i in range(30)]                                    # 30 waiters leave the front
    spec += [(lk + i, LOCK, -1) for i in range(65, 95)]                              # 30 more wrap the ring
    spec += [(qu, ADD, 0, LONG, i) for i in range(64)] + [(qu, POLL)] * 30 + [(qu, ADD, 0, LONG, 100 + i) for i in range(30)]
    spec += [(gr + i, abi.CC_OP_GROUP_JOIN) for i in range(64)]
    spec += [(el + i, abi.CC_OP_ELECT_LISTEN) for i in range(50)]
    spec += [(tp + i, abi.CC_OP_TOPIC_LISTEN) for i in range(50)]
    spec += [(bu + i, abi.CC_OP_BUS_JOIN, 0, HANDLE, 500 + i % 7) for i in range(40)]
    spec += [(bu + i, abi.CC_OP_BUS_REGISTER, 0, HANDLE, t) for i, t in ((0, 1), (1, 1), (2, 1), (0, 2), (1, 2), (3, 2))]
    spec += [(va + i, abi.CC_OP_VALUE_LISTEN) for i in range(50)] + [(va, abi.CC_OP_VALUE_SET, 0, LONG, 5)]
    b1 = _rows(spec, 1)
    w.apply(b1)

    def readers(E):
        w.check_state(E)              # topic listeners, bus members and registrations, their retained commits
        _check_state(E, w.O, types)   # lock, election, group, value state and the applied index
        for r in (0, 1, 2, 3):
            assert E.retained(r) == w.O.retained(r), r

    readers(w.E)
    assert len(w.E.lock_state(0)[3]) == 64 and len(w.E.group_members(2)) == 64
    assert len(w.E.read_bus_members(5)) == 40 and len(w.E.read_bus_registrations(5)) == 6
    old = w.E
    w.E = old.grown(coord_cap=256)
    old.close()
    readers(w.E)  # before any further row
    spec = [(lk + i, LOCK, -1) for i in list(range(95, 100)) + list(range(30))]      # 99 waiters
    spec += [(lk + i, UNLOCK) for i in range(30, 65)]                                # the holders in turn, across the old wrap
    spec += [(qu, ADD, 0, LONG, 200 + i) for i in range(40)] + [(qu, POLL)] * 110  # 104 elements, then drained in order
    spec += [(gr + i, abi.CC_OP_GROUP_JOIN) for i in range(64, 84)]
    spec += [(el + i, abi.CC_OP_ELECT_LISTEN) for i in range(50, 80)]
    spec += [(tp + i, abi.CC_OP_TOPIC_LISTEN) for i in range(50, 80)] + [(tp, abi.CC_OP_TOPIC_PUBLISH, 0, LONG, 77)]
    spec += [(bu + i, abi.CC_OP_BUS_JOIN, 0, HANDLE, 500 + i % 7) for i in range(40, 70)]
    spec += [(bu + 4, abi.CC_OP_BUS_REGISTER, 0, HANDLE, 3), (bu + 5, abi.CC_OP_BUS_REGISTER, 0, HANDLE, 1), (bu + 1, abi.CC_OP_BUS_LEAVE)]
    spec += [(va + i, abi.CC_OP_VALUE_LISTEN) for i in range(50, 80)] + [(va + 1, abi.CC_OP_VALUE_SET, 0, LONG, 9)]
    w.apply(_rows(spec, len(b1) + 1))
    readers(w.E)
    assert len(w.E.lock_state(0)[3]) == 64 and len(w.E.group_members(2)) == 84
    assert len(w.E.topic_listeners(4)) == 80 and len(w.E.read_bus_members(5)) == 69


# ---- 4. a prefix stop on a full block, then grown ---------------------------------------------------------------------
def test_prefix_stop_on_full_lock_queue_then_grown():
    """70 lock rows (no timeout) to one held lock on coord_cap 64: the prefix apply stops at the row that would be the
    65th waiter; a grown engine (coord_cap 128, a factor 2) resumes at that row.  All 70 results, and the `lock` events
    of the unlocks that follow, equal the oracle's."""
    from copycat_amd.engine import Engine

    types = np.array([L], np.uint8)
    E, O, max_inst = _setup(types, 72, FLAGS, coord_cap=64)
    _check_batch(E, O, _rows([(0, abi.CC_OP_LOCK_LOCK, -1)], 1))
    b = _rows([(i, abi.CC_OP_LOCK_LOCK, -1) for i in range(1, 71)], 2)
    applied, s, v, ev = E.apply_host_prefix(b)
    assert applied == 64 and len(ev["pos"]) == 0
    info = Engine.snapshot_info(E.snapshot())
    assert info["coord_cap"] == 64 and info["flags"] & abi.CC_SNAP_COORD and info["applied"] == 65
    E2 = E.grown(coord_cap=128)
    rest = b.slice(64, 70)
    applied2, s3, v3, ev3 = E2.apply_host_prefix(rest)
    assert applied2 == len(rest) and len(ev3["pos"]) == 0
    s2, v2 = O.apply(b)
    assert len(O.take_events()["pos"]) == 0
    assert np.array_equal(np.concatenate([s[:64], s3]), s2) and np.array_equal(np.concatenate([v[:64], v3]), v2)
    _check_state(E2, O, types)
    assert len(E2.lock_state(0)[3]) == 70
    _check_batch(E2, O, _rows([(i, abi.CC_OP_LOCK_UNLOCK) for i in range(71)], 72))
    _assert_same_state(_state(E2, types, True, 200), _state(O, types, True, 200, oracle=True), "grown engine", "oracle")


# ---- 5. round trips (the grown engine's snapshot through plain restore: _halves) --------------------------------------
def test_grow_into_the_same_configuration_is_plain_restore():
    from copycat_amd.engine import Engine
    from copycat_amd.workload import coord_random_stream, map_random_stream

    def engine():
        return Engine(16, 64, 1 << 16, map_capacity=1024, flags=FLAGS, coord_cap=128, max_events=1 << 20)

    E = engine()
    types = np.array([L, E_, G, V] * 2, np.uint8)
    for r, t in enumerate(types):
        E.resource_create(r, int(t))
        for k in range(5):
            E.instance_open(r * 5 + k, r, 1000 + r * 5 + k, 7 + k)
    E.resource_create_range(8, 4, M_)
    E.instance_open_range(40, 4, 8, 2000, 7)
    from tests.handles import register_key_strings

    register_key_strings(E)  # (map_random_stream's String keys)
    E.apply_host_events(coord_random_stream(4_000, types, 5, 48, seed=9))
    E.apply_host(map_random_stream(4_000, 4, 64, keys=64, first_inst=40, seed=10, index0=4_001))
    snap = E.snapshot()
    F = engine()
    F.restore(snap, grow=True)
    assert F.snapshot() == snap


# ---- 6. refusals, 7. snapshot_info ------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_as_it_was():
    """A smaller coord_cap, a smaller map_capacity, another max_resources, a snapshot with maps into an engine without,
    a truncated buffer and test_snapshot_corrupt_counts_rejected_before_any_state_changes's corrupt trailing counts:
    CC_ERR_INVALID each, and the target reads as before.  Plain restore still refuses a smaller-capacity snapshot."""
    from copycat_amd.engine import Engine
    from copycat_amd.workload import value_random_stream

    R = 64
    b = value_random_stream(3000, R, R + 8, seed=5)

    def engine(rows, res=R, **cfg):
        X = Engine(res, R + 8, len(b), **cfg)
        X.resource_create_range(0, R, abi.CC_RES_VALUE)
        X.instance_open_range(0, R, 0, 1000, 7)
        X.apply_host(b.slice(0, rows))
        return X

    def reads(X):
        return [x.tolist() for x in X.value_state(0, R)] + [X.applied_index()]

    S = engine(3000, map_capacity=4096, coord_cap=128)
    snap = S.snapshot()
    assert Engine.snapshot_info(snap) == {"max_resources": R, "max_instances": R + 8, "map_capacity": 4096, "coord_cap": 128,
                                          "flags": 0, "applied": S.applied_index()}
    for cfg in (dict(map_capacity=4096, coord_cap=64), dict(map_capacity=1024, coord_cap=128),
                dict(res=128, map_capacity=4096, coord_cap=128), dict(coord_cap=128)):
        F = engine(1000, **cfg)
        before = reads(F)
        _invalid(lambda: F.restore(snap, grow=True))
        assert reads(F) == before, cfg
    F = engine(1000, map_capacity=8192, coord_cap=256)
    before = reads(F)
    for cut in (len(snap) - 1, len(snap) // 2, 200, 10):
        _invalid(lambda: F.restore(snap[:cut], grow=True))
        assert reads(F) == before, cut
    for off in (32, 16, 8):  # the trailer's ng, ns, nl (no timers, sessions or leaks: the last 32 bytes)
        bad = bytearray(snap)
        struct.pack_into("<Q", bad, len(bad) - off, (1 << 64) - 3)
        _invalid(lambda: F.restore(bytes(bad), grow=True))
        assert reads(F) == before, off
    _invalid(lambda: F.restore(snap))  # plain restore stays strict
    assert reads(F) == before
    F.restore(snap, grow=True)  # the intact snapshot does restore
    assert reads(F) == reads(S)


def test_snapshot_without_maps_grows_into_an_empty_table():
    """A snapshot of an engine without maps restores into an engine with maps as an empty table: the entries the target
    held before do not come back when the slot becomes a map again."""
    from copycat_amd.engine import Engine
    from copycat_amd.workload import value_random_stream
    from oracle.oracle_py import Oracle

    R = 64
    b = value_random_stream(2000, R, R + 8, seed=6)

    def engine(**cfg):
        X = Engine(R + 1, R + 8, 4096, **cfg)
        X.resource_create_range(0, R, abi.CC_RES_VALUE)
        X.instance_open_range(0, R, 0, 1000, 7)
        return X

    def puts(keys, index0):
        rows = _map_rows(keys, [abi.CC_OP_MAP_PUT] * len(keys), index0)
        rows.inst[:] = R
        return rows

    S = engine()
    S.apply_host(b)
    W = engine(map_capacity=1024)
    W.resource_create(R, M_)
    W.instance_open(R, R, 1000 + R, 7)
    W.apply_host(puts(np.arange(100, 400), 1))
    assert len(W.map_entries(R)[0]) == 300
    W.restore(S.snapshot(), grow=True)
    for x, y in zip(W.value_state(0, R), S.value_state(0, R)):
        assert np.array_equal(x, y)
    W.resource_create(R, M_)  # (the snapshot's slot R is free)
    W.instance_open(R, R, 1000 + R, 7)
    assert len(W.map_entries(R)[0]) == 0
    O = Oracle(R + 1, R + 8)
    O.resource_create(R, M_)
    O.instance_open(R, R, 1000 + R, 7)
    rows = puts(np.arange(350, 360), 2001)
    _assert_rows(*W.apply_host(rows), *O.apply(rows))
    for x, y in zip(W.map_entries(R), O.map_entries(R)):
        assert np.array_equal(x, y)
