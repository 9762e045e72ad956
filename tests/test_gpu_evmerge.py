"""GPU: cc_merge_events_device (copycat_amd/csrc/evmerge_gpu.hip) against the host call, and the sharded loop with
engines: split on the device, one engine per rank, results and events merged back on the device.

1. Device against host, byte for byte, over the case grid of tests/evmerge_cases.py, plus the cases that straddle what
   the kernels have inside: k_evm_mark's wave (64 events) and workgroup step (256), k_evm_gather's window
   (CC_EVMERGE_WINDOW_EVENTS) and tile (CC_EVMERGE_TILE_ROWS).
2. The refusals of the host call, with the same code and total, outputs untouched.  These are argument errors answered
   by a status: every index is checked on the device before it addresses memory.
3. A coordination log (locks, elections, groups, value listeners) and a topic log through split_batch_device, `world`
   engines, merge_by_owner_device and merge_events_device: the merged stream equals one engine's, column for column."""
import ctypes as C
import functools

import numpy as np
import pytest

from copycat_amd import abi, shard
from tests import evmerge_cases as ec

pytestmark = pytest.mark.gpu

T, W = ec.T, abi.CC_EVMERGE_WINDOW_EVENTS
TDT = {"pos": "int32", "target": "int32", "code": "uint8", "src": "uint8", "tag": "uint8", "payload": "int64"}
NPV = {"pos": np.int32, "target": np.int32, "code": np.uint8, "src": np.uint8, "tag": np.uint8, "payload": np.int64}


def _up(a, view):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(view)).cuda()


def dev_merge(parts, rows, row_counts, n, out_capacity=None, extra=0, counts=None, stream=None, guard=3):
    """cc_merge_events_device over one upload per column (the parts are slices of it; each part has `extra` sentinel
    rows of capacity behind its events) into sentinel-filled columns -> (rc, total, out columns, *out.count)"""
    import torch

    from copycat_amd.engine import lib

    world = len(parts)
    lens = [len(p["pos"]) for p in parts]
    caps = [m + extra for m in lens]
    start = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    cols = {}
    for name in ec.COLS:
        full = np.full(max(int(start[-1]), 1), ec.SENTINEL[name], ec.DT[name])
        for r, p in enumerate(parts):
            full[start[r]:start[r] + lens[r]] = p[name]
        cols[name] = _up(full, NPV[name])
    cnt = _up(np.array(lens if counts is None else counts, np.uint64), np.int64)
    rstart = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64)
    allrows = _up(np.concatenate(list(rows) + [np.zeros(1, np.uint64)]), np.int64)
    pr = (abi.cc_events * world)()
    rowp = (C.c_void_p * world)()
    for r in range(world):
        for name in ec.COLS:
            setattr(pr[r], name, cols[name].data_ptr() + int(start[r]) * cols[name].element_size() if caps[r] else None)
        pr[r].capacity, pr[r].count = caps[r], cnt.data_ptr() + 8 * r
        rowp[r] = allrows.data_ptr() + 8 * int(rstart[r]) if len(rows[r]) else None
    cap = sum(lens) if out_capacity is None else out_capacity
    out = {name: _up(a, NPV[name]) for name, a in ec.sentinel_columns(max(cap, 1) + guard).items()}
    ocnt = _up(np.array([0x7777], np.uint64), np.int64)
    o = abi.cc_events(*[out[name].data_ptr() for name in ec.COLS], cap, ocnt.data_ptr())
    need = C.c_uint64()
    assert lib().cc_merge_events_device_bound(n, world, C.byref(need)) == abi.CC_OK
    work = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    tot = C.c_uint64(0x7777)
    rcs = np.ascontiguousarray(row_counts, np.uint64)
    torch.cuda.synchronize()
    rc = lib().cc_merge_events_device(pr, rowp, rcs.ctypes.data_as(C.c_void_p), n, world, C.byref(o), C.byref(tot),
                                      work.data_ptr(), work.numel(), C.c_void_p(stream.cuda_stream) if stream else None)
    torch.cuda.synchronize()
    host = {name: out[name].cpu().numpy().view(ec.DT[name]) for name in ec.COLS}
    return rc, tot.value, host, int(ocnt.cpu().numpy().view(np.uint64)[0])


def _same_as_host(case, threads=16, **kw):
    from copycat_amd.engine import lib

    rc, total, out, ocnt = dev_merge(case.parts, case.rows, case.row_counts, case.n, **kw)
    assert rc == abi.CC_OK, lib().cc_last_error()
    hrc, htotal, hout, hcnt = ec.host_merge(lib(), case.parts, case.rows, case.row_counts, case.n, threads)
    assert hrc == abi.CC_OK and total == htotal == case.total and ocnt == hcnt == total
    assert ec.equal_columns(out, hout, total) and ec.equal_columns(out, case.ref, total)
    assert ec.untouched(out, total)  # rows past the total keep their sentinel
    return out


# ---- 1. device against host ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", ec.WORLDS)
@pytest.mark.parametrize("events", ec.EVENTS)
def test_device_equals_host_on_the_grid(events, world):
    for n in ec.SIZES:
        for owner in ec.OWNERS:
            _same_as_host(ec.build(n, world, owner, events, seed=n + world))


def _runs(n, world, per_row, seed, owner="random"):
    rng = np.random.default_rng(seed)
    c = np.zeros(n, np.int64)
    c[:len(per_row)] = per_row
    return ec.Case(n, world, ec.owners(n, world, owner, rng), c, seed)


@pytest.mark.parametrize("world", [1, 2, 3])
def test_runs_across_wave_workgroup_and_window_boundaries(world):
    """runs of equal pos that lie across event 64 (a wave's step of k_evm_mark), 256 (its workgroup's step), 1024 (the
    gather window) and their multiples, in a rank's stream (world 1) and in the output (every world)"""
    per_row = [60, 10, 180, 12, 760, 9, 1, 1000, 70, 0, 0, 3, 250, 5, 2048, 1, 1, 62, 130]
    for n in (len(per_row), T + 5):
        _same_as_host(_runs(n, world, per_row, seed=21 + world))
    # every run exactly ends on, and starts at, a boundary
    _same_as_host(_runs(64, world, [64, 192, 768, 1024, 1, 255, 768], seed=31))


@pytest.mark.parametrize("total", [W - 1, W, W + 1, 2 * W + 1])
def test_tile_around_one_gather_window(total):
    """a tile whose events fill one window, lack one, exceed it by one; single events and one long run"""
    per_row = np.zeros(T, np.int64)
    per_row[:total] = 1
    _same_as_host(_runs(T, 2, per_row, seed=5))
    per_row[:] = 0
    per_row[T - 1] = total
    _same_as_host(_runs(T, 2, per_row, seed=6))


def test_long_runs_on_both_sides_of_a_tile_edge():
    n = 3 * T + 17
    per_row = np.random.default_rng(8).integers(0, 3, n)
    per_row[T - 1] = 65535   # a tile's last row
    per_row[T] = 65535       # the next tile's first
    per_row[n - 1] = 4097
    for world, owner in ((1, "round_robin"), (4, "round_robin"), (4, "random")):
        _same_as_host(_runs(n, world, per_row, seed=9, owner=owner))


def test_non_default_stream_slack_capacity_and_larger_output():
    import torch

    case = ec.build(3 * T + 17, 8, "random", "mixed", seed=13)
    st = torch.cuda.Stream()
    # parts whose capacity exceeds their count (sentinel rows behind the count must not appear), an output larger than
    # the total (rows past the total keep their sentinel), on a stream of the caller's
    out = _same_as_host(case, extra=777, out_capacity=case.total + 1000, stream=st, guard=1000)
    assert np.all(np.diff(out["pos"][:case.total].astype(np.int64)) >= 0)


def test_python_wrapper_returns_device_events():
    import torch

    from copycat_amd.engine import DeviceEvents

    case = ec.build(T + 65, 3, "random", "mixed", seed=4)
    parts = []
    for p in case.parts:
        d = DeviceEvents(len(p["pos"]) + 9)
        for name in ec.COLS:
            getattr(d, name)[:len(p["pos"])] = _up(p[name], NPV[name])
        d.count[0] = len(p["pos"])
        parts.append(d)
    rows = [_up(x, np.int64).view(torch.uint64) for x in case.rows]
    got = shard.merge_events_device(parts, rows, case.n).host()
    assert got["count"] == case.total and ec.equal_columns(got, case.ref, case.total)


# ---- 2. refusals, as the host's -----------------------------------------------------------------------------------------
def _refused(case, want, parts=None, rows=None, total=None, **kw):
    from copycat_amd.engine import lib

    args = (parts or case.parts, rows or case.rows, case.row_counts, case.n)
    rc, tot, out, ocnt = dev_merge(*args, **kw)
    msg = lib().cc_last_error().decode()
    hkw = {k: v for k, v in kw.items() if k in ("out_capacity", "counts")}
    if "counts" in kw:
        hkw["capacities"] = [len(p["pos"]) + kw.get("extra", 0) for p in args[0]]
    hrc, htot, hout, _ = ec.host_merge(lib(), *args, 16, **hkw)
    assert rc == hrc == want, (rc, hrc, msg)
    assert ec.untouched(out) and ocnt == 0x7777
    if total is not None:
        assert tot == htot == total
    return msg


def _base():
    return ec.build(T + 65, 3, "random", "mixed", seed=11)


def _with(case, r, name, j, value):
    parts = [dict(p) for p in case.parts]
    parts[r][name] = parts[r][name].copy()
    parts[r][name][j] = value
    return parts


def test_device_refusals():
    case = _base()
    j = len(case.parts[1]["pos"]) // 2
    msg = _refused(case, abi.CC_ERR_INVALID, parts=_with(case, 1, "pos", j, case.parts[1]["pos"][j - 1] - 1))
    assert "rank 1" in msg and f"event {j}" in msg  # pos decreasing at one event
    last = len(case.parts[2]["pos"]) - 1
    msg = _refused(case, abi.CC_ERR_INVALID, parts=_with(case, 2, "pos", last, int(case.row_counts[2])))
    assert "rank 2" in msg and f"event {last}" in msg  # pos == row_counts[r]: never used to address rows[r]
    parts = [dict(p) for p in case.parts]
    parts[0]["pos"] = np.full_like(parts[0]["pos"], 0xFFFFFFFF)  # a session-close stream
    assert "rank 0, event 0" in _refused(case, abi.CC_ERR_INVALID, parts=parts)
    rows = [x.copy() for x in case.rows]
    rows[1][int(case.parts[1]["pos"][-1])] = case.n  # a rows value == n: never used to address the per-row arrays
    assert "rank 1" in _refused(case, abi.CC_ERR_INVALID, rows=rows)
    counts = [len(p["pos"]) for p in case.parts]
    counts[1] += 5  # a part count above its capacity
    _refused(case, abi.CC_ERR_CAPACITY, counts=counts, total=case.total + 5)
    counts[1] += 95  # ... and beyond the sentinel rows that follow it
    _refused(case, abi.CC_ERR_CAPACITY, counts=counts, extra=20, total=case.total + 100)
    _refused(case, abi.CC_ERR_CAPACITY, out_capacity=case.total - 1, total=case.total)  # the output one event short


def test_no_events_stores_the_count_only():
    case = ec.build(T + 1, 3, "random", "none")
    rc, total, out, ocnt = dev_merge(case.parts, case.rows, case.row_counts, case.n, out_capacity=10)
    assert rc == abi.CC_OK and total == 0 and ocnt == 0 and ec.untouched(out)


# ---- 3. the loop with engines -------------------------------------------------------------------------------------------
KEYS = ("pos", "src", "target", "code", "tag", "payload")


def _sharded(b, own, world, make_engine, ev_capacity):
    """split_batch_device(rows=True) -> each rank's engine apply_events -> merge_by_owner_device, merge_events_device"""
    import torch

    from copycat_amd.engine import DeviceBatch, DeviceEvents

    db = DeviceBatch.upload(b)
    parts = shard.split_batch_device(db, own, world, rows=True)
    res, evs, keep = [], [], []
    for r, (rows, part) in enumerate(parts):
        E = make_engine(r)
        st = torch.empty(part.n, dtype=torch.uint8, device="cuda")
        va = torch.empty(part.n, dtype=torch.uint64, device="cuda")
        ev = DeviceEvents(ev_capacity)
        E.apply_events(part, st, va, ev)
        E.sync()
        res.append((st, va)), evs.append(ev), keep.append(E)
    st, va = shard.merge_by_owner_device(db.cols["inst"], own, world, res)
    merged = shard.merge_events_device(evs, [rows for rows, _ in parts], len(b))
    return st.cpu().numpy(), va.view(torch.int64).cpu().numpy().view(np.uint64), merged, keep


R_COORD, K_COORD = 64, 4
COORD_CAP = 4096  # lock() without a timeout queues for good: room for every lock row of one lock (about 940 here)


@functools.lru_cache(maxsize=None)
def _coord_reference():
    """the log, and one engine's and the oracle's answers for it (computed once for both worlds)"""
    from copycat_amd.workload import coord_random_stream
    from tests.test_gpu_coord import FLAGS, E_, G, L, V, _oracle_events, _setup

    types = np.array([L, E_, G, V] * (R_COORD // 4), np.uint8)
    E, O, max_inst = _setup(types, K_COORD, FLAGS, coord_cap=COORD_CAP)
    b = coord_random_stream(60_000, types, K_COORD, max_inst, seed=23)
    timed = (b.op == abi.CC_OP_LOCK_LOCK) & (b.aux.view(np.int64) > 0)
    b.aux[timed] = np.uint64(2**64 - 1)  # lock(timeout) -> lock(): no timer is armed
    s, v, ev = E.apply_host_events(b, capacity=1 << 20)
    s2, v2 = O.apply(b)
    assert np.array_equal(s, s2) and np.array_equal(v, v2)
    return types, max_inst, b, s, v, ev, _oracle_events(O)


@pytest.mark.parametrize("world", [2, 4])
def test_coordination_log_through_the_sharded_loop(world):
    from copycat_amd.engine import Engine
    from tests.test_gpu_coord import FLAGS, _canon

    types, max_inst, b, s1, v1, ev1, (oe, apos, amem) = _coord_reference()
    own = shard.inst_owner_table(np.arange(R_COORD * K_COORD) // K_COORD, world)

    def make_engine(rank):
        E = Engine(R_COORD, max_inst, 1 << 20, flags=FLAGS, max_events=1 << 22, coord_cap=COORD_CAP)
        for r in range(R_COORD):
            if r % world == rank:
                E.resource_create(r, int(types[r]))
                for k in range(K_COORD):
                    E.instance_open(r * K_COORD + k, r, 1000 + r * K_COORD + k, 7 + k)
        return E

    st, va, merged, engines = _sharded(b, own, world, make_engine, 1 << 20)
    ev = merged.host()
    assert np.array_equal(st, s1) and np.array_equal(va, v1)
    assert ev["count"] == ev1["count"] == len(ev1["pos"]) and ev["count"] > 1000
    for k in KEYS:  # one engine's stream, column for column in stream order
        assert np.array_equal(ev[k], ev1[k]), k
    assert np.all(np.diff(ev["pos"].astype(np.int64)) >= 0)
    # ... and the oracle's, by the canonical per-commit comparison (member rows against the oracle's aux stream)
    member = ev["code"] == abi.CC_EV_MEMBER
    assert _canon(*(ev[k][~member] for k in KEYS)) == _canon(*(oe[k] for k in KEYS))
    assert list(zip(ev["pos"][member].tolist(), ev["payload"][member].tolist())) == list(zip(apos.tolist(), amem.tolist()))
    # the merged stream through the packed D2H
    from copycat_amd.batch import unpack_events

    blob, count = engines[0].events_to_host_packed(merged)
    un = unpack_events(blob)
    assert count == ev["count"] and all(np.array_equal(un[k], ev[k]) for k in KEYS)


def test_topic_log_through_the_sharded_loop():
    """8 topics with 16 listeners each: the fan-out runs of real engines (tests/topic_model.py is the reference)"""
    from copycat_amd.batch import Batch
    from tests.test_gpu_topic import LISTEN, PUBLISH, UNLISTEN, World
    from tests.test_gpu_topic import T as TOPIC

    R, K, n = 8, 16, 5000
    w = World([TOPIC] * R, K, client=lambda s: 7 + s % 16)
    rng = np.random.default_rng(41)
    b = Batch(n)
    b.index[:] = np.arange(1, n + 1, dtype=np.uint64)
    b.time[:] = b.index
    b.inst[:] = rng.integers(0, R * K, n)
    u = rng.random(n)
    b.op[:] = np.where(u < 0.6, PUBLISH, np.where(u < 0.9, LISTEN, UNLISTEN))
    b.flags[:] = rng.integers(0, 5, n).astype(np.uint8)
    b.a[:] = rng.integers(0, 1 << 63, n, dtype=np.uint64)
    want = w.expect(b)
    s1, v1, ev1 = w.E.apply_host_events(b, capacity=1 << 18)
    w.check((s1, v1, ev1), want)
    assert len(ev1["pos"]) > 4 * n  # fan-out runs
    for world in (2, 4):
        own = shard.inst_owner_table(np.arange(R * K) // K, world)

        def make_engine(rank):
            E = w.fresh_engine()
            for r in range(R):
                if r % world == rank:
                    E.resource_create(r, int(TOPIC))
                    for s in w.inst[r]:
                        E.instance_open(s, r, w.iid(s), w.client(s))
            return E

        st, va, merged, _ = _sharded(b, own, world, make_engine, 1 << 18)
        ev = merged.host()
        w.check((st, va, ev), want)
        assert ev["count"] == len(ev1["pos"])
        for k in KEYS:
            assert np.array_equal(ev[k], ev1[k]), (world, k)
