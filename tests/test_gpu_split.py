"""GPU: cc_split_batch_device / cc_merge_results_device (copycat_amd/csrc/split_gpu.hip), the device forms of the
global-log split and merge (DESIGN.md §6 "The split on the device").

Every output is compared exactly with shard.split_batch / shard.merge_by_owner on the same host batch (the host pair is
itself pinned to a numpy restatement by tests/test_split.py).  T is CC_SPLIT_TILE_ROWS, the rows one workgroup takes;
a wave ranks T / 4 consecutive rows of a tile in 64-row steps."""
import ctypes as C
import functools

import numpy as np
import pytest

from copycat_amd import abi, shard
from copycat_amd.batch import Batch

pytestmark = pytest.mark.gpu

T = abi.CC_SPLIT_TILE_ROWS
SIZES = [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17, 100_003]
WORLDS = [1, 2, 3, 8, 13, 64, 256]
N_INST = 5000
SENT = 0xA5


@functools.lru_cache(maxsize=None)
def _batch(n, n_inst=N_INST, unknown=0.01):
    """tests/test_split.py::_batch: random full-range columns, 1 % unknown instances (one per size, never changed)"""
    rng = np.random.default_rng(n * 31 + 7)
    b = Batch(n)
    for name in Batch.__slots__:
        a = getattr(b, name)
        a[:] = rng.integers(0, np.iinfo(a.dtype).max, n, dtype=a.dtype, endpoint=True)
    b.inst[:] = rng.integers(0, n_inst, n, dtype=np.uint32)
    if unknown:
        m = rng.random(n) < unknown
        b.inst[m] = n_inst + rng.integers(0, 1000, int(m.sum()), dtype=np.uint32)
    b.index[:] = np.arange(n, dtype=np.uint64) + 1
    return b


@functools.lru_cache(maxsize=None)
def _table(world, n_inst=N_INST):
    return np.random.default_rng(world).integers(0, world, n_inst).astype(np.uint8)


def _host(t):
    import torch

    return t.view({8: torch.int64, 4: torch.int32, 1: torch.uint8}[t.element_size()]).cpu().numpy().view(
        {8: np.uint64, 4: np.uint32, 1: np.uint8}[t.element_size()])


def _upload(b, columns=None):
    from copycat_amd.engine import DeviceBatch

    return DeviceBatch.upload(b, columns=columns)


def _dev(a):
    import torch

    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint8): np.uint8}[a.dtype]
    back = {np.dtype(np.uint64): torch.uint64, np.dtype(np.uint32): torch.uint32, np.dtype(np.uint8): torch.uint8}[a.dtype]
    return torch.from_numpy(a.view(signed)).cuda().view(back)


def _check_split(b, tab, world, stream=None, names=Batch.__slots__):
    """device split (with and without rows) and merge of `b` == the host calls -> the device parts"""
    want = shard.split_batch(b, tab, world, rows=True)
    db = _upload(b, columns=names if names is not Batch.__slots__ else None)
    own = _dev(tab)
    counts = shard.split_counts_device(db, own, world, stream=stream)
    assert counts.tolist() == [len(sub) for _, sub in want]
    for rows in (True, False):
        got = shard.split_batch_device(db, own, world, rows=rows, stream=stream)
        assert len(got) == world
        for r, ((hrows, hsub), (drows, dsub)) in enumerate(zip(want, got)):
            assert dsub.n == len(hsub), f"rank {r} count"
            assert sorted(dsub.cols) == sorted(names)
            if rows:
                assert np.array_equal(_host(drows), hrows), f"rank {r} rows"
            else:
                assert drows is None
            for name in names:
                assert np.array_equal(_host(dsub.cols[name]), getattr(hsub, name)), f"rank {r} column {name}"
    return db, own, want, got


def _check_merge(b, tab, world, db, own, want, stream=None):
    """per-rank results as tests/test_split.py builds them (status: a byte of a; value: index), merged on the device"""
    res = [((sub.a & 0xFF).astype(np.uint8), sub.index.copy()) for _, sub in want]
    hs, hv = shard.merge_by_owner(b.inst, tab, world, res)
    ds, dv = shard.merge_by_owner_device(db.cols["inst"], own, world, [(_dev(s), _dev(v)) for s, v in res], stream=stream)
    ds, dv = _host(ds), _host(dv)
    assert np.array_equal(ds, hs) and np.array_equal(dv, hv)
    assert np.array_equal(dv, b.index) and np.array_equal(ds, (b.a & 0xFF).astype(np.uint8))


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("n", SIZES)
def test_split_and_merge_match_the_host_calls(n, world):
    b, tab = _batch(n), _table(world)
    db, own, want, _ = _check_split(b, tab, world)
    _check_merge(b, tab, world, db, own, want)


def _with_owners(owners, world):
    """a batch whose row i is owned by owners[i]: inst = the row's owner, the table the identity"""
    n = len(owners)
    src = _batch(n, unknown=0.0)
    b = Batch(n)
    for name in Batch.__slots__:
        getattr(b, name)[:] = getattr(src, name)
    b.inst[:] = np.asarray(owners, np.uint32)
    return b, np.arange(world, dtype=np.uint8)


PATTERNS = {
    # every row on one rank (the other ranks have no rows: split_batch_device passes NULL columns for them)
    "one rank": lambda: _with_owners(np.full(2 * T + 100, 5), 8),
    "an empty rank": lambda: _with_owners(np.random.default_rng(3).choice([0, 1, 3], 3 * T + 17), 4),
    "alternating": lambda: _with_owners(np.arange(3 * T + 17) % 2, 2),
    # 64 distinct ranks in every 64-row step: the match loop runs its 64 rounds; the step's ranks rotate so that all
    # 256 ranks occur
    "64 ranks per step": lambda: _with_owners([(i % 64) * 4 + (i // 64) % 4 for i in range(2 * T + 333)], 256),
    # a run of one rank across a wave boundary (T / 4) and a tile boundary (T), among rows of other ranks
    "a run across wave and tile": lambda: _with_owners(
        np.where((np.arange(2 * T + 50) > T // 4 - 40) & (np.arange(2 * T + 50) < T + 90), 2,
                 np.arange(2 * T + 50) % 3), 3),
}


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_rank_patterns(pattern):
    b, tab = PATTERNS[pattern]()
    world = len(tab)
    db, own, want, got = _check_split(b, tab, world)
    _check_merge(b, tab, world, db, own, want)
    if pattern == "one rank":
        assert [p.n for _, p in got] == [0] * 5 + [len(b)] + [0] * 2
    if pattern == "an empty rank":
        assert got[2][1].n == 0 and all(got[r][1].n for r in (0, 1, 3))


def test_stream():
    """the same case on a non-default torch stream"""
    import torch

    b, tab = _batch(3 * T + 17), _table(8)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    db, own, want, _ = _check_split(b, tab, 8, stream=st)
    _check_merge(b, tab, 8, db, own, want, stream=st)


def test_timing_aid_reports_the_three_kernels():
    """cc_split_device_timing: per-kernel times of the thread's last call while enabled; outputs unchanged"""
    from copycat_amd.engine import lib

    b, tab = _batch(3 * T + 17), _table(8)
    ms = (C.c_float * 3)()
    assert lib().cc_split_device_timing(1, None) == abi.CC_OK
    try:
        db, own, want, _ = _check_split(b, tab, 8)
        assert lib().cc_split_device_timing(1, ms) == abi.CC_OK
        assert all(0.0 < x < 1000.0 for x in ms), list(ms)  # count, scan, scatter
        shard.split_counts_device(db, own, 8)
        assert lib().cc_split_device_timing(1, ms) == abi.CC_OK
        assert ms[0] > 0.0 and ms[1] > 0.0 and ms[2] == 0.0  # a counts-only call launches no scatter
        _check_merge(b, tab, 8, db, own, want)
        assert lib().cc_split_device_timing(0, ms) == abi.CC_OK
        assert all(0.0 < x < 1000.0 for x in ms), list(ms)  # count, scan, gather
    finally:
        lib().cc_split_device_timing(0, None)


# ---- the C call itself: missing columns, sentinels, errors -------------------------------------------------------------
class _Raw:
    """Outputs of `cap` rows per rank for every column, prefilled with a sentinel, and the C call on them."""

    def __init__(self, b, tab, world, names, caps, n_inst=None):
        import torch

        self.b, self.world, self.names = b, world, names
        self.db = _upload(b, columns=names)
        self.own = _dev(tab)
        self.n_inst = len(tab) if n_inst is None else n_inst
        self.caps = np.asarray(caps, np.uint64)
        self.outs = []
        for r in range(world):
            width = {name: getattr(b, name).dtype.itemsize for name in Batch.__slots__}
            width["rows"] = 8
            self.outs.append({name: torch.full((int(self.caps[r]) * w,), SENT, dtype=torch.uint8, device="cuda")
                              .view({8: torch.uint64, 4: torch.uint32, 1: torch.uint8}[w]) for name, w in width.items()})
        need = C.c_uint64()
        from copycat_amd.engine import lib

        assert lib().cc_split_device_bound(len(b), world, C.byref(need)) == 0
        self.work = torch.empty(need.value, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def call(self, counts_only=False, rows=False, null=()):
        """-> (rc, counts); null: (rank, column) outputs passed as NULL"""
        import torch

        from copycat_amd.engine import _np, lib

        outs = (abi.cc_batch_out * self.world)()
        rowp = (C.c_void_p * self.world)()
        for r in range(self.world):
            for name in Batch.__slots__:
                setattr(outs[r], name, None if (r, name) in null else self.outs[r][name].data_ptr() or None)
            rowp[r] = self.outs[r]["rows"].data_ptr() or None
        counts = np.full(self.world, 12345, np.uint64)
        cols = self.db.struct()
        tab = C.c_void_p(self.own.data_ptr()) if self.n_inst else None
        rc = lib().cc_split_batch_device(C.byref(cols), len(self.b), tab, self.n_inst,
                                         self.world, None if counts_only else outs, _np(self.caps), _np(counts),
                                         rowp if rows else None, C.c_void_p(self.work.data_ptr()), self.work.numel(), None)
        torch.cuda.synchronize()
        return rc, counts

    def untouched(self, names=None):
        names = list(Batch.__slots__) + ["rows"] if names is None else names
        return all(bool((_host(self.outs[r][name]).view(np.uint8) == SENT).all())
                   for r in range(self.world) for name in names)


def _ref_owner(b, tab):
    inst = b.inst.astype(np.int64)
    return np.where(inst < len(tab), tab[np.minimum(inst, len(tab) - 1)], 0)


def test_missing_columns_keep_their_sentinel():
    """only inst, op, key present (tests/test_split.py::test_split_missing_columns_and_errors): the outputs of the
    absent columns, and `rows` when not asked for, are left alone"""
    n, world = 20_000, 4
    b = _batch(n, n_inst=100, unknown=0.0)
    tab = (np.arange(100) % world).astype(np.uint8)
    own = _ref_owner(b, tab)
    want = [int((own == r).sum()) for r in range(world)]
    present, absent = ("inst", "op", "key"), ["index", "time", "flags", "a", "b", "aux", "rows"]
    raw = _Raw(b, tab, world, present, want)
    rc, counts = raw.call(counts_only=True)
    assert rc == abi.CC_OK and counts.tolist() == want and raw.untouched()
    rc, counts = raw.call()
    assert rc == abi.CC_OK and counts.tolist() == want
    for r in range(world):
        for name in present:
            assert np.array_equal(_host(raw.outs[r][name]), getattr(b, name)[own == r]), (r, name)
    assert raw.untouched(absent)
    rc, _ = raw.call(rows=True)
    assert rc == abi.CC_OK
    for r in range(world):
        assert np.array_equal(_host(raw.outs[r]["rows"]), np.nonzero(own == r)[0].astype(np.uint64))
    assert raw.untouched(absent[:-1])


def test_errors_leave_the_outputs_untouched():
    n, world = 3 * T + 17, 4
    b = _batch(n, n_inst=100, unknown=0.0)
    tab = (np.arange(100) % world).astype(np.uint8)
    own = _ref_owner(b, tab)
    want = [int((own == r).sum()) for r in range(world)]
    # out_cap one short on one rank: CC_ERR_CAPACITY, the right counts, nothing written
    caps = np.array(want, np.uint64)
    caps[2] -= 1
    raw = _Raw(b, tab, world, Batch.__slots__, caps)
    rc, counts = raw.call(rows=True)
    assert rc == abi.CC_ERR_CAPACITY and counts.tolist() == want and raw.untouched()
    # an owner byte equal to world: CC_ERR_INVALID, nothing written (with and without outputs)
    bad = tab.copy()
    bad[int(b.inst[n - 3])] = world
    raw = _Raw(b, bad, world, Batch.__slots__, [n] * world)
    assert raw.call(rows=True)[0] == abi.CC_ERR_INVALID and raw.untouched()
    assert raw.call(counts_only=True)[0] == abi.CC_ERR_INVALID
    # a NULL output column with a nonzero count: CC_ERR_INVALID, nothing written
    raw = _Raw(b, tab, world, Batch.__slots__, want)
    assert raw.call(null={(1, "op")})[0] == abi.CC_ERR_INVALID and raw.untouched()
    # n_inst == 0 with a NULL table: everything goes to rank 0
    raw = _Raw(b, tab, world, ("inst", "a"), [n, 0, 0, 0], n_inst=0)
    rc, counts = raw.call()
    assert rc == abi.CC_OK and counts.tolist() == [n, 0, 0, 0]
    assert np.array_equal(_host(raw.outs[0]["a"]), b.a) and np.array_equal(_host(raw.outs[0]["inst"]), b.inst)
    # the merge refuses a bad owner byte and a NULL part of a rank that has rows
    import torch

    from copycat_amd.engine import EngineError

    db = _upload(b, columns=("inst",))
    parts = [(torch.zeros(c, dtype=torch.uint8, device="cuda"), torch.zeros(c, dtype=torch.uint64, device="cuda"))
             for c in want]
    with pytest.raises(EngineError):
        shard.merge_by_owner_device(db.cols["inst"], _dev(bad), world, parts)
    parts[3] = (parts[3][0][:0], parts[3][1][:0])
    with pytest.raises(EngineError):
        shard.merge_by_owner_device(db.cols["inst"], _dev(tab), world, parts)


# ---- the loop with the engine: the device-resident twin of tests/test_gpu_shard.py ------------------------------------
def _ranks(world, slots, max_inst, types, map_capacity=0):
    from copycat_amd.engine import Engine

    engines = []
    for rank in range(world):
        E = Engine(slots, max_inst, 1 << 20, map_capacity=map_capacity, flags=abi.CC_CFG_TIMERS_DEFERRED)
        for g in range(slots):
            if shard.owner_of(g, world) == rank:  # each rank hosts the slots it owns (the others stay unused)
                E.resource_create(g, int(types[g]))
                E.instance_open(g, g, 1000 + g, 7)
        engines.append(E)
    return engines


def _oracle(slots, max_inst, types):
    from oracle.oracle_py import Oracle

    O = Oracle(slots, max_inst, abi.CC_CFG_TIMERS_DEFERRED)
    for g in range(slots):
        O.resource_create(g, int(types[g]))
        O.instance_open(g, g, 1000 + g, 7)
    return O


def _apply_parts(engines, parts):
    """each rank's Engine.apply on its device share -> [(status, value)] device tensors"""
    import torch

    from copycat_amd.engine import RESULT_SENTINEL

    res = []
    for E, (_, part) in zip(engines, parts):
        st = torch.full((part.n,), RESULT_SENTINEL, dtype=torch.uint8, device="cuda")
        va = torch.zeros(part.n, dtype=torch.uint64, device="cuda")
        torch.cuda.synchronize()
        E.apply(part, st, va)
        E.sync()
        res.append((st, va))
    return res


def _split_apply_merge_device(b, world, engines, slots):
    own = shard.inst_owner_table(np.arange(slots), world)
    db = _upload(b)
    own_dev = _dev(shard._rank_table(own, world))
    parts = shard.split_batch_device(db, own_dev, world)
    for r, (_, part) in enumerate(parts):
        inst = _host(part.cols["inst"])
        known = inst < slots  # rows of unknown sessions (beyond the owner table) go to rank 0
        assert part.n and np.all(inst[known] % world == r) and (r == 0 or known.all())
    st, va = shard.merge_by_owner_device(db.cols["inst"], own_dev, world, _apply_parts(engines, parts))
    return _host(st), _host(va)


@pytest.mark.parametrize("world", [2, 4])
def test_device_split_apply_merge_values(world):
    """tests/test_gpu_shard.py's 400,000-row AtomicValue log over 4,096 slots, two batches, with the columns resident:
    upload, split on the device, per-rank Engine.apply, merge on the device == one replica; each slot's state from its
    owner."""
    from copycat_amd.workload import value_random_stream

    slots, max_inst = 4096, 4096 + 8
    types = np.full(slots, abi.CC_RES_VALUE, np.uint8)
    engines, O = _ranks(world, slots, max_inst, types), _oracle(slots, max_inst, types)
    for seed in (5, 6):
        b = value_random_stream(400_000, slots, max_inst, seed=seed, hot=8, p_hot=0.2)
        assert np.any(b.inst >= slots)  # unknown sessions among the rows
        st, va = _split_apply_merge_device(b, world, engines, slots)
        st1, va1 = O.apply(b)
        assert np.array_equal(st, st1) and np.array_equal(va, va1)
    tag1, val1, cur1 = O.value_state()
    for r, E in enumerate(engines):
        tag, val, cur = E.value_state()
        mine = np.arange(slots) % world == r
        assert np.array_equal(tag[mine], tag1[mine]) and np.array_equal(val[mine], val1[mine])
        assert np.array_equal(cur[mine], cur1[mine])


def test_device_split_apply_merge_maps():
    """tests/test_gpu_shard.py's 300,000-row MapState log over 64 maps on 4 ranks, with the columns resident."""
    from copycat_amd.workload import map_random_stream
    from tests.handles import register_key_strings

    world, slots = 4, 64
    types = np.full(slots, abi.CC_RES_MAP, np.uint8)
    engines = _ranks(world, slots, slots + 8, types, map_capacity=16384)
    O = _oracle(slots, slots + 8, types)
    for E in engines:
        register_key_strings(E)
    register_key_strings(None, O)  # String keys: java.util.HashMap places them by String.hashCode
    b = map_random_stream(300_000, slots, slots + 8, keys=256, seed=9, hot=2, p_hot=0.2)
    st, va = _split_apply_merge_device(b, world, engines, slots)
    st1, va1 = O.apply(b)
    assert np.array_equal(st, st1) and np.array_equal(va, va1)
    for m in range(slots):
        got, want = engines[m % world].map_entries(m), O.map_entries(m)
        for x, y in zip(got, want):
            assert np.array_equal(x, y), m


def test_from_the_wire():
    """The chain from log bytes: a front engine that knows every resource decodes AtomicValue entries on the GPU
    (WireDecoder.decode_to_device), the device columns are split for 2 ranks (index from a host arange), the per-rank
    engines apply their shares, and the merged results are the oracle's on the host-decoded log."""
    from copycat_amd.engine import Engine
    from copycat_amd.wire import Interner, WireDecoder
    from tests.golden.make_wire import instance_op

    world, slots, n = 2, 64, T + 500
    types = np.full(slots, abi.CC_RES_VALUE, np.uint8)
    front = Engine(slots, slots, 1 << 16)
    for g in range(slots):
        front.resource_create(g, abi.CC_RES_VALUE)
        front.instance_open(g, g, 1000 + g, 7)
    engines, O = _ranks(world, slots, slots, types), _oracle(slots, slots, types)
    rng = np.random.default_rng(21)
    entries = []
    for _ in range(n):
        iid = 1000 + int(rng.integers(0, slots))
        k = int(rng.integers(0, 4))
        val = lambda: None if rng.integers(0, 4) == 0 else ("LONG", int(rng.integers(0, 4)))  # noqa: E731
        if k == 0:
            entries.append(instance_op(iid, "VALUE_GET", [])[0])
        elif k == 1:
            entries.append(instance_op(iid, "VALUE_SET", [], a=val())[0])
        elif k == 2:
            entries.append(instance_op(iid, "VALUE_CAS", [], a=val(), b=val())[0])
        else:
            entries.append(instance_op(iid, "VALUE_GETANDSET", [], a=val())[0])
    bh, _, kind = WireDecoder(front, Interner(1)).decode(entries=entries)
    assert not kind.any() and np.all(bh.inst < slots)
    bh.index[:] = np.arange(1, n + 1, dtype=np.uint64)
    db, _, _, stats = WireDecoder(front, Interner(1)).decode_to_device(entries=entries)
    assert stats["device_rows"] == n
    db.cols["index"] = _dev(bh.index)
    own_dev = _dev(shard._rank_table(shard.inst_owner_table(np.arange(slots), world), world))
    parts = shard.split_batch_device(db, own_dev, world, rows=True)
    assert sum(p.n for _, p in parts) == n and all(p.n for _, p in parts)
    st, va = shard.merge_by_owner_device(db.cols["inst"], own_dev, world, _apply_parts(engines, parts))
    st1, va1 = O.apply(bh)
    assert np.array_equal(_host(st), st1) and np.array_equal(_host(va), va1)
    for r, (rows, part) in enumerate(parts):  # the rows output maps a rank's row back to the log
        assert np.array_equal(_host(part.cols["index"]), _host(rows) + 1)
