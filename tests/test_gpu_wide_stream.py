"""GPU parity: whole-collection rows of sets, multimaps and Delete applied in the stream (map_wide.hip, map_clear.hip).

Outside TTL mode a Set's size / isEmpty / clear, a MultiMap's isEmpty / clear / removeValue and Delete on a Map, Set or
MultiMap are ordinary rows of the stream: size queries answered from the size tracking, clear-class rows applied as
clear epochs.  No such row is a batch barrier, so the engine's barrier counter (cc_engine_counters' first value) does
not move.  In TTL mode the size / isEmpty rows join the event replay; clear-class rows stay barriers there.

Bar, every case: bit-exact per-row status and value, every slot's entries (cc_read_map_entries), every slot's retained
commits (cc_read_retained) and the applied index against oracle.oracle_py.Oracle; and the barrier counter moves by
exactly the rows the case names (none, unless it says otherwise).  All comparisons are integer equality."""
import functools

import numpy as np
import pytest

from copycat_amd import abi
from copycat_amd.batch import Batch
from tests.test_gpu_map import _assert_rows, _cv_rows, _no_null_values, _with_ttl
from tests.test_gpu_set import _AS_SET

pytestmark = pytest.mark.gpu

M_, S_, MM_ = abi.CC_RES_MAP, abi.CC_RES_SET, abi.CC_RES_MULTIMAP
DEFERRED = abi.CC_CFG_TIMERS_DEFERRED

# MapState key ops as the MultiMapState rows they turn into (the engine maps them back: common.h mmap_as_map_op)
_AS_MMAP = {abi.CC_OP_MAP_PUT: abi.CC_OP_MMAP_PUT, abi.CC_OP_MAP_PUTIFABSENT: abi.CC_OP_MMAP_PUT,
            abi.CC_OP_MAP_REPLACE: abi.CC_OP_MMAP_PUT, abi.CC_OP_MAP_REPLACEIFPRESENT: abi.CC_OP_MMAP_SIZE,
            abi.CC_OP_MAP_GET: abi.CC_OP_MMAP_GET, abi.CC_OP_MAP_GETORDEFAULT: abi.CC_OP_MMAP_GET,
            abi.CC_OP_MAP_CONTAINSKEY: abi.CC_OP_MMAP_CONTAINSKEY, abi.CC_OP_MAP_REMOVE: abi.CC_OP_MMAP_REMOVE,
            abi.CC_OP_MAP_REMOVEIFPRESENT: abi.CC_OP_MMAP_REMOVE}
# whole-collection rows per type: size queries, and rows that empty the collection (sm_delete / clear in the oracle)
_QUERY = {M_: [abi.CC_OP_MAP_SIZE, abi.CC_OP_MAP_ISEMPTY], S_: [abi.CC_OP_SET_SIZE, abi.CC_OP_SET_ISEMPTY],
          MM_: [abi.CC_OP_MMAP_ISEMPTY]}
_CLEAR = {M_: [abi.CC_OP_MAP_CLEAR, abi.CC_OP_DELETE], S_: [abi.CC_OP_SET_CLEAR, abi.CC_OP_DELETE],
          MM_: [abi.CC_OP_MMAP_CLEAR, abi.CC_OP_MMAP_REMOVEVALUE, abi.CC_OP_DELETE]}


# ---- engines, streams, checks ----------------------------------------------------------------------------------------
def _engine(types, max_batch, map_capacity=65536, sub_batch=0, flags=DEFERRED, create=True):
    """An engine holding resource r (instance slot r, instance id 1000 + r) of types[r]."""
    from copycat_amd.engine import Engine
    from tests.handles import register_key_strings

    R = len(types)
    E = Engine(R, R + 8, max_batch, map_capacity=map_capacity, sub_batch=sub_batch, flags=flags)
    if create:
        for r, t in enumerate(types):
            E.resource_create(r, int(t))
        E.instance_open_range(0, R, 0, 1000, 7)
        register_key_strings(E)
    return E


def _oracle(types, flags=DEFERRED):
    from oracle.oracle_py import Oracle
    from tests.handles import register_key_strings

    R = len(types)
    O = Oracle(R, R + 8, flags & DEFERRED)
    for r, t in enumerate(types):
        O.resource_create(r, int(t))
        O.instance_open(r, r, 1000 + r, 7)
    register_key_strings(None, O)
    return O


def _row_types(b, types):
    """The resource type each row addresses (0: an instance slot nothing is open on)."""
    types = np.asarray(types, np.uint8)
    R = len(types)
    return np.where(b.inst < R, types[np.minimum(b.inst, R - 1)], 0).astype(np.uint8)


def _stream(n, types, seed, keys=64, hot=0, p_hot=0.0, ttl=False):
    """A random key-op stream over the resources (tests' map_random_stream: every key op, all key and value tags, hot
    keys on the first `hot` slots, wrong-type ops, unknown instance slots), each row's op turned into its resource
    type's.  Maps store no null value (a containsValue-free stream needs none; case 5 adds them on purpose)."""
    from copycat_amd.workload import map_random_stream

    R = len(types)
    b = map_random_stream(n, R, R + 8, keys=keys, seed=seed, hot=hot, p_hot=p_hot)
    ty = _row_types(b, types)
    op = b.op.copy()
    for t, table in ((S_, _AS_SET), (MM_, _AS_MMAP)):
        for m, s in table.items():
            b.op[(ty == t) & (op == m)] = s
    f = b.flags
    maps = ty == M_
    f[maps & ((f & 7) == abi.CC_TAG_NULL)] |= np.uint8(abi.CC_TAG_LONG)
    f[maps & (((f >> 3) & 7) == abi.CC_TAG_NULL)] |= np.uint8(abi.CC_TAG_LONG << 3)
    if ttl:
        _with_ttl(b, seed + 1)
    return b


def _wide(b, types, rate, seed, table):
    """Turn a share of the rows that address a live resource into whole-collection rows of that resource's own type
    (`table`: _QUERY, _CLEAR, or both merged).  Rows that are whole-collection rows already are left alone."""
    rng = np.random.default_rng(seed)
    ty = _row_types(b, types)
    taken = _is(b, types, _QUERY) | _is(b, types, _CLEAR)
    rows = (rng.random(len(b)) < rate) & (ty != 0) & ~taken
    for t, ops in table.items():
        at = np.nonzero(rows & (ty == t))[0]
        b.op[at] = rng.choice(np.array(ops, np.uint8), len(at))
    b.aux[rows] = 0
    return np.nonzero(rows)[0]


def _both(*tables):
    return {t: sum((tb.get(t, []) for tb in tables), []) for t in (M_, S_, MM_)}


def _is(b, types, table):
    """Rows whose op is one of `table`'s for the type of the live resource they address."""
    ty = _row_types(b, types)
    m = np.zeros(len(b), bool)
    for t, ops in table.items():
        m |= (ty == t) & np.isin(b.op, np.array(ops, np.uint8))
    return m


def _state(X, types, oracle=False):
    """Every slot's entries and retained commits, and the applied index, as plain Python values."""
    st = {"applied_index": X.applied_index()}
    for r in range(len(types)):
        st["entries", r] = tuple(a.tolist() for a in X.map_entries(r))
        st["retained", r] = list(X.retained(r, cap=1 << 20) if oracle else X.retained(r))
    return st


def _assert_state(got, want):
    assert got.keys() == want.keys()
    for k in got:
        if got[k] != want[k]:
            n = (len(got[k][0]), len(want[k][0])) if k[0] == "entries" else (len(got[k]), len(want[k])) \
                if k[0] == "retained" else (got[k], want[k])
            raise AssertionError(f"{k} differs from the oracle: {n[0]} vs {n[1]}")


def _apply(E, parts, want_rows):
    """The parts through the host entry point: every row as the reference has it; returns how far the barrier counter
    moved."""
    moved = 0
    for p, (s2, v2) in zip(parts, want_rows):
        c0 = E.counters()[0]
        s, v = E.apply_host(p)
        _assert_rows(s, v, s2, v2)
        moved += E.counters()[0] - c0
    return moved


def _reference(types, parts, flags=DEFERRED):
    """The oracle's rows per part and its state after the last one."""
    O = _oracle(types, flags)
    rows = [O.apply(p) for p in parts]
    return rows, _state(O, types, oracle=True)


def _parity(E, types, parts, barriers=0, flags=DEFERRED, ref=None):
    rows, want = ref if ref is not None else _reference(types, parts, flags)
    moved = _apply(E, parts, rows)
    _assert_state(_state(E, types), want)
    assert moved == barriers, f"{moved} barrier rows, {barriers} expected"
    return rows


def _rows(rows, index0=1):
    """A batch of (instance slot, op, key) rows: Long keys, value a = 3 * key + 1 (Long)."""
    inst, op, key = (np.array(c) for c in zip(*rows))
    n = len(rows)
    return Batch.from_columns(index=np.arange(index0, index0 + n, dtype=np.uint64), inst=inst.astype(np.uint32),
                              op=op.astype(np.uint8), flags=np.full(n, abi.cc_flags(abi.CC_TAG_LONG, 0, 0), np.uint8),
                              key=key.astype(np.uint64), a=key.astype(np.uint64) * np.uint64(3) + np.uint64(1))


# ---- 1. scripted, one batch ------------------------------------------------------------------------------------------
_ADD = {M_: abi.CC_OP_MAP_PUT, S_: abi.CC_OP_SET_ADD, MM_: abi.CC_OP_MMAP_PUT}


@pytest.mark.parametrize("kind", [S_, MM_], ids=["set", "multimap"])
def test_scripted_clear_delete_then_reuse_keys(kind):
    """One batch on slot 0 (a set, then a multimap): 40 keys, size (set), clear, isEmpty, 10 of the same keys again,
    isEmpty, Delete, isEmpty, 3 keys, removeValue (multimap), isEmpty.  A second set (slot 1) and a map (slot 2) of the
    same engine, filled first, keep their entries.  No row is a barrier."""
    types = [kind, S_, M_]
    empty_q = _QUERY[kind][-1]
    rows = [(1, abi.CC_OP_SET_ADD, k) for k in range(40)] + [(2, abi.CC_OP_MAP_PUT, k) for k in range(40)]
    rows += [(0, _ADD[kind], k) for k in range(40)]
    if kind == S_:
        rows.append((0, abi.CC_OP_SET_SIZE, 0))
    rows += [(0, _CLEAR[kind][0], 0), (0, empty_q, 0)]
    rows += [(0, _ADD[kind], k) for k in range(10)] + [(0, empty_q, 0)]
    rows += [(0, abi.CC_OP_DELETE, 0), (0, empty_q, 0)]
    rows += [(0, _ADD[kind], k) for k in (3, 50, 51)]
    if kind == MM_:
        rows += [(0, empty_q, 0), (0, abi.CC_OP_MMAP_REMOVEVALUE, 0)]
    rows += [(0, empty_q, 0), (1, abi.CC_OP_SET_SIZE, 0), (2, abi.CC_OP_MAP_SIZE, 0)]
    b = _rows(rows)
    E = _engine(types, 1024, map_capacity=1024)
    want = _parity(E, types, [b])
    s, v = want[0]
    BOOL, INT = abi.cc_status(abi.CC_ST_OK, abi.CC_TAG_BOOL), abi.cc_status(abi.CC_ST_OK, abi.CC_TAG_INT)
    q = np.nonzero((b.inst == 0) & (b.op == empty_q))[0]
    assert (s[q] == BOOL).all() and set(v[q].tolist()) == {0, 1}  # (the reference answers both ways)
    assert s[-1] == INT and v[-1] == 40 and s[-2] == INT and v[-2] == 40  # the neighbours kept their 40 entries
    assert len(E.map_entries(1)[0]) == 40 and len(E.map_entries(2)[0]) == 40


def test_scripted_map_delete_then_reuse_keys():
    """Map put 40, Delete, size, put 10, size in one batch: the Delete is a clear epoch of the stream."""
    types = [M_, M_]
    rows = [(1, abi.CC_OP_MAP_PUT, k) for k in range(40)] + [(0, abi.CC_OP_MAP_PUT, k) for k in range(40)]
    rows += [(0, abi.CC_OP_DELETE, 0), (0, abi.CC_OP_MAP_SIZE, 0)]
    rows += [(0, abi.CC_OP_MAP_PUT, k) for k in range(10)] + [(0, abi.CC_OP_MAP_SIZE, 0), (1, abi.CC_OP_MAP_SIZE, 0)]
    b = _rows(rows)
    E = _engine(types, 1024, map_capacity=1024)
    (s, v), = _parity(E, types, [b])
    sz = np.nonzero(b.op == abi.CC_OP_MAP_SIZE)[0]
    assert v[sz].tolist() == [0, 10, 40]


# ---- 2 / 7. random mix over maps, sets and multimaps; the same stream across a snapshot ------------------------------
_MIX_TYPES = [S_] * 16 + [M_] * 16 + [MM_] * 8  # (hot keys land on the first slots: two sets)
_MIX_CUT = 60_001


@functools.lru_cache(maxsize=None)
def _mix():
    """120,000 rows over 16 sets, 16 maps storing no null and 8 multimaps, hot keys on two sets, 1 % of the rows turned
    into whole-collection rows of their own type (size, isEmpty, clear, removeValue, Delete); two batches cut at an odd
    row; the reference's rows and final state, computed once."""
    n = 120_000
    b = _stream(n, _MIX_TYPES, 2201, keys=64, hot=2, p_hot=0.2)
    rows = _wide(b, _MIX_TYPES, 0.01, 2202, _both(_QUERY, _CLEAR))
    parts = [b.slice(0, _MIX_CUT), b.slice(_MIX_CUT, n)]
    return b, rows, parts, _reference(_MIX_TYPES, parts)


def test_random_mix_several_subbatches_hot_keys():
    b, rows, parts, ref = _mix()
    ty = _row_types(b, _MIX_TYPES)
    for t in (M_, S_, MM_):  # every listed op occurs on its type
        for o in _both(_QUERY, _CLEAR)[t]:
            assert ((ty[rows] == t) & (b.op[rows] == o)).any(), (t, o)
    E = _engine(_MIX_TYPES, len(b), sub_batch=16384)
    _parity(E, _MIX_TYPES, parts, ref=ref)
    assert E.counters()[2] >= 8  # several sub-batches


def test_snapshot_between_batches_of_the_mix():
    """The first batch, cc_snapshot_save, a fresh engine restored from it, the second batch there."""
    b, _, parts, (rows, want) = _mix()
    E = _engine(_MIX_TYPES, len(b), sub_batch=16384)
    assert _apply(E, parts[:1], rows[:1]) == 0
    snap = E.snapshot()
    del E
    E2 = _engine(_MIX_TYPES, len(b), sub_batch=16384, create=False)  # empty registry: everything from the snapshot
    E2.restore(snap)
    assert _apply(E2, parts[1:], rows[1:]) == 0
    _assert_state(_state(E2, _MIX_TYPES), want)


# ---- 3. more than 127 clear epochs of one slot in a sub-batch --------------------------------------------------------
def test_more_than_127_epochs_of_one_slot_in_a_subbatch():
    """4 sets and 2 multimaps, 60,000 rows in one default sub-batch, 5 % of them clear / Delete / removeValue (~500 per
    slot: the host cuts the sub-batch so that none sees more than 127 epochs of a slot), 1 % size / isEmpty."""
    types = [S_] * 4 + [MM_] * 2
    n = 60_000
    b = _stream(n, types, 2301, keys=16)
    _wide(b, types, 0.05, 2302, _CLEAR)
    _wide(b, types, 0.01, 2303, _QUERY)
    clears = _is(b, types, _CLEAR)
    assert np.bincount(b.inst[clears], minlength=6)[:6].min() > 127
    E = _engine(types, n)
    c0 = E.counters()
    _parity(E, types, [b])
    assert E.counters()[2] - c0[2] > 1  # the host did cut


# ---- 4. more rows than one barrier listing holds ---------------------------------------------------------------------
def test_more_whole_set_rows_than_one_barrier_listing():
    """70,000 size / isEmpty / clear / Delete rows on 2 sets in one batch of 150,000 (a barrier listing holds 65,536):
    none is a barrier, so the batch is neither halved nor refused."""
    types = [S_, S_]
    n = 150_000
    b = _stream(n, types, 2401, keys=16)
    rng = np.random.default_rng(2402)
    rows = np.sort(rng.choice(n, 70_000, replace=False))
    rows = rows[b.inst[rows] < 2]
    q = rng.random(len(rows)) < 0.98
    b.op[rows] = np.where(q, rng.choice(np.array(_QUERY[S_], np.uint8), len(rows)),
                          rng.choice(np.array(_CLEAR[S_], np.uint8), len(rows)))
    b.aux[rows] = 0
    assert len(rows) > 65_536
    E = _engine(types, n, map_capacity=4096)
    _parity(E, types, [b])


# ---- 5. Map Delete and containsValue ---------------------------------------------------------------------------------
def test_map_delete_keeps_contains_value_in_the_stream():
    """Maps that never store a null, 2 % containsValue rows, 0.1 % Deletes: a Delete is an epoch like clear, so every
    containsValue row -- those after a Delete of their map too -- is answered in the stream."""
    from copycat_amd.workload import map_random_stream

    maps, n = 16, 100_000
    types = [M_] * maps
    b = map_random_stream(n, maps, maps + 8, keys=64, seed=2501, hot=2, p_hot=0.3)
    _no_null_values(b)
    cv = _cv_rows(b, 0.02, 2502)
    rng = np.random.default_rng(2503)
    d = np.nonzero(rng.random(n) < 0.001)[0]
    d = d[(b.op[d] != abi.CC_OP_MAP_CONTAINSVALUE) & (b.inst[d] < maps)]
    b.op[d] = abi.CC_OP_DELETE
    live_cv = cv[b.inst[cv] < maps]
    after = [r for r in live_cv if ((d < r) & (b.inst[d] == b.inst[r])).any()]
    assert len(d) > 50 and len(after) > 100  # containsValue rows that follow a Delete of their map
    E = _engine(types, n, sub_batch=8192)
    c0 = E.counters()
    (s, v), = _parity(E, types, [b])
    assert E.counters()[1] - c0[1] == len(live_cv)
    ok = s[live_cv] == abi.cc_status(abi.CC_ST_OK, abi.CC_TAG_BOOL)
    assert ok.all() and (v[live_cv] == 1).any() and (v[live_cv] == 0).any()


def test_map_delete_after_a_stored_null_then_contains_value():
    """A map that holds a null value, then a Delete, then containsValue rows (same batch, and a second batch): parity
    only -- the map may hold a null at the batch start, so its containsValue rows of that batch may stay barriers."""
    types = [M_, M_]
    NUL = abi.cc_flags(abi.CC_TAG_NULL, 0, 0)
    rows = [(0, abi.CC_OP_MAP_PUT, 1), (0, abi.CC_OP_MAP_PUT, 2), (1, abi.CC_OP_MAP_PUT, 2),
            (0, abi.CC_OP_MAP_CONTAINSVALUE, 2), (0, abi.CC_OP_DELETE, 0), (0, abi.CC_OP_MAP_CONTAINSVALUE, 2),
            (0, abi.CC_OP_MAP_PUT, 2), (0, abi.CC_OP_MAP_CONTAINSVALUE, 2), (0, abi.CC_OP_MAP_CONTAINSVALUE, 5),
            (1, abi.CC_OP_MAP_CONTAINSVALUE, 2), (0, abi.CC_OP_MAP_SIZE, 0)]
    b = _rows(rows)
    b.flags[0] = NUL  # map 0's first put stores a null
    b2 = _rows([(0, abi.CC_OP_MAP_CONTAINSVALUE, 2), (0, abi.CC_OP_MAP_CONTAINSVALUE, 7), (0, abi.CC_OP_DELETE, 0),
                (0, abi.CC_OP_MAP_CONTAINSVALUE, 2)], index0=len(b) + 1)
    E = _engine(types, 64, map_capacity=1024)
    rows_ref, want = _reference(types, [b, b2])
    _apply(E, [b, b2], rows_ref)  # (the barrier count is free to move)
    _assert_state(_state(E, types), want)


# ---- 6. TTL mode -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [DEFERRED, 0], ids=["manager", "module"])
def test_ttl_mode_size_rows_in_stream_clears_stay_barriers(flags):
    """Sets whose adds arm TTL timers (and multimaps, whose Puts arm none), 0.5 % size / isEmpty rows, 0.1 % clear /
    Delete / removeValue rows: the size rows join the event replay, the clear-class rows are barriers, one each."""
    types = [S_] * 12 + [MM_] * 4
    n = 80_000
    b = _stream(n, types, 2601, keys=64, ttl=True)
    _wide(b, types, 0.005, 2602, _QUERY)
    _wide(b, types, 0.001, 2603, _CLEAR)
    assert (b.aux[(b.op == abi.CC_OP_SET_ADD) & (b.inst < 12)].view(np.int64) > 0).any()
    barriers = int(_is(b, types, _CLEAR).sum())
    assert barriers > 20 and _is(b, types, _QUERY).sum() > 200
    E = _engine(types, n, sub_batch=32768, flags=flags)
    _parity(E, types, [b.slice(0, 50_001), b.slice(50_001, n)], barriers=barriers, flags=flags)


# ---- 8. prefix apply -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _prefix_scenario():
    """Two sets in one table of two 2,048-entry regions: distinct elements with size / isEmpty rows between them, a
    clear of set 0 and a Delete of set 1 on the way (their elements stay bound until a launch compacts the region),
    until region 0 has been offered one element too many; then more elements, a clear, and region 1 overfilled."""
    from tests.test_gpu_prefix import _Keyed

    K = _Keyed([S_, S_], seed=2801)

    def fill(region, keep_room, slots=(0, 1)):
        i = 0
        while K.room(region) > keep_room:
            s = slots[i % len(slots)]
            K.put(s, K.fresh(s, region))
            if i % 13 == 0:
                K.size(s)
            if i % 29 == 0:
                K.is_empty(1 - s)
            i += 1

    fill(0, 900)
    fill(1, 1200)
    K.clear(0)
    K.size(0), K.is_empty(0), K.size(1)
    fill(0, 300)
    K.clear(1, delete=True)
    K.is_empty(1), K.size(0)
    fill(0, 0)
    K.put(0, K.fresh(0, 0))  # the element region 0 cannot hold
    K.size(0), K.size(1)
    for j in range(60):      # the next call's launch compacts region 0: these fit
        K.put(j % 2, K.fresh(j % 2, j % 2))
    K.clear(0)
    K.is_empty(0)
    fill(1, 0)
    K.put(1, K.fresh(1, 1))  # and one too many for region 1
    for j in range(40):
        K.put(j % 2, K.fresh(j % 2, j % 2))
        if j % 9 == 0:
            K.size(j % 2)
    return K


class _DevicePrefix:
    """cc_apply_batch_prefix behind apply_host_prefix's signature (device-resident columns, sentinel-prefilled device
    results), so tests.test_gpu_prefix._Prefix can drive either form."""

    def __init__(self, E):
        self.E = E

    def __getattr__(self, name):
        return getattr(self.E, name)

    def apply_host_prefix(self, b, capacity=None):
        import torch

        from copycat_amd.engine import RESULT_SENTINEL, DeviceBatch

        n = len(b)
        db = DeviceBatch.upload(b)
        status = torch.full((n,), RESULT_SENTINEL, dtype=torch.uint8, device="cuda")
        value = torch.zeros((n,), dtype=torch.int64, device="cuda")
        applied = self.E.apply_prefix(db, status, value)
        ev = {"pos": np.zeros(0, np.uint32), "target": np.zeros(0, np.uint32), "code": np.zeros(0, np.uint8),
              "src": np.zeros(0, np.uint8), "tag": np.zeros(0, np.uint8), "payload": np.zeros(0, np.uint64)}
        return applied, status.cpu().numpy(), value.cpu().numpy().view(np.uint64), ev


@pytest.mark.parametrize("form", ["host", "device"])
def test_prefix_apply_stops_row_exact_with_in_stream_rows(form):
    """A set stream with in-stream clears and size rows whose adds overflow a table region, through
    cc_apply_batch_host_prefix and cc_apply_batch_prefix.  Each stop is the first row that does not fit: the rows
    before it apply through the plain entry point on a replica (same calls, same launches), and a twin of that replica
    (restored from its snapshot before the call) refuses the same rows plus the stop row with CC_ERR_CAPACITY; the first
    stop is no later than the row at which the table model has offered a region more elements than it has entries.
    Rows, entries and retained commits after each stop equal the oracle's and the replica's after exactly the applied
    rows; the calls resume to the oracle's final state."""
    from copycat_amd.engine import EngineError
    from tests.test_gpu_prefix import _compare, _keyed_engine, _keyed_pair, _Mirror, _Prefix, _table_region

    types = [S_, S_]
    K = _prefix_scenario()
    b = K.batch()
    E, O = _keyed_pair(types)
    rep = _keyed_pair(types)[0]
    X = E if form == "host" else _DevicePrefix(E)
    P, M = _Prefix(X, b, "region"), _Mirror(O, b, [rep])
    c0 = E.counters()[0]
    while not P.done():
        snap = rep.snapshot()  # the replica before the call
        lo, hi, stopped = P.step()
        M.apply(lo, hi)
        if stopped:
            assert b.op[hi] == abi.CC_OP_SET_ADD  # only an element that needs an entry can fail to fit
            _compare(P, M, E, types, drain=True, nidx=len(b))
            if P.stops() <= 2:
                twin = _keyed_engine(types)
                twin.restore(snap)
                with pytest.raises(EngineError) as ei:
                    twin.apply_host(b.slice(lo, hi + 1))
                assert ei.value.rc == abi.CC_ERR_CAPACITY
    _compare(P, M, E, types, drain=True, nidx=len(b))
    assert P.stops() >= 2 and P.bisected() >= 1 and len(P.failed) == P.stops()
    # The table model bounds the first stop from above: by its misfit row region 0 has been offered one distinct element
    # more than its 2,048 entries, all in one launch.  (The engine may stop a few elements earlier -- it also binds
    # placeholder entries for hot-key candidates, here key 0 of the whole-set rows -- and what it can hold is its own
    # business: the twin above pins each stop from below.)
    f0 = P.failed[0]
    assert f0 <= K.misfit[0] and _table_region(int(b.inst[f0]), 0, int(b.key[f0])) == 0
    assert E.counters()[0] == c0  # no barrier row in any attempt
    in_stream = _is(b, types, _both(_QUERY, _CLEAR))
    assert in_stream[:P.failed[0]].sum() > 50 and _is(b, types, _CLEAR)[:P.failed[0]].sum() == 2
