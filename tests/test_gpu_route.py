"""GPU: cc_route_events_device (copycat_amd/csrc/route_gpu.hip) against the host call, and the way out with engines.

1. Device against host, byte for byte, over the case grid of tests/route_cases.py (sizes around the wave, the workgroup
   and CC_ROUTE_TILE_EVENTS; session counts around every power of 2^CC_ROUTE_DIGIT_BITS, up to a fourth round); rows
   past n_events and directory entries past the active sessions keep their sentinel.
2. The refusals of the host call, with the same codes and outputs untouched.  These are argument errors answered by a
   status: every index is checked on the device before it addresses memory.
3. A stream of the caller's, outputs that lack 16-byte alignment, a call without instance ids.
4. A coordination log (locks, elections, groups, value listeners) and a topic log over 12 clients through one engine
   and the route: each session's run, read through the directory, against the oracle's per-session event list.
5. The same logs through the sharded loop (split_batch_device, `world` engines, merge_events_device, route): the same
   routed stream and directory as the single engine's stream routed.
6. A cc_sessions_close stream (pos 0xFFFFFFFF) routes."""
import ctypes as C
import functools

import numpy as np
import pytest

from copycat_amd import abi, route, shard
from tests import route_cases as rc_

pytestmark = pytest.mark.gpu

T, D = rc_.T, rc_.D
NPV = {"pos": np.int32, "target": np.int32, "code": np.uint8, "src": np.uint8, "tag": np.uint8, "payload": np.int64}


def _up(a, view):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(view)).cuda()


def _down(t, dtype):
    return t.cpu().numpy().view(dtype)


def dev_route(case, out_capacity=None, dir_capacity=None, with_ids=True, ev=None, session_of_inst=None, n_sessions=None,
              stream=None, skew=0):
    """cc_route_events_device into sentinel-filled device outputs -> (rc, n_active, Outputs on the host).  skew: rows by
    which every output column starts behind its tensor's start (so the outputs lack 16-byte alignment)."""
    import torch

    from copycat_amd.engine import lib

    ev = ev or case.ev
    tab = case.session_of_inst if session_of_inst is None else session_of_inst
    n = case.n
    cap = n if out_capacity is None else out_capacity
    dcap = min(n, case.n_sessions) if dir_capacity is None else dir_capacity
    sessions = case.n_sessions if n_sessions is None else n_sessions
    o = rc_.Outputs(cap + skew, dcap + skew)
    d_in = {c: _up(ev[c] if n else np.zeros(1, rc_.DT[c]), NPV[c]) for c in rc_.COLS}
    d_tab, d_ids = _up(tab, np.int32), _up(case.id_of_inst, np.int64)
    d_out = {c: _up(o.cols[c], NPV[c]) for c in rc_.COLS}
    d_inst, d_ses, d_start = _up(o.inst, np.int64), _up(o.session, np.int32), _up(o.start, np.int32)
    d_cnt, d_dcnt = _up(o.count, np.int64), _up(o.dir_count, np.int64)
    at = lambda t: t.data_ptr() + skew * t.element_size()  # noqa: E731
    i_s = abi.cc_events(*[d_in[c].data_ptr() for c in rc_.COLS], n, None)
    o_s = abi.cc_events(*[at(d_out[c]) for c in rc_.COLS], cap, d_cnt.data_ptr())
    d_s = abi.cc_route_dir(at(d_ses), at(d_start), dcap, d_dcnt.data_ptr())
    need = C.c_uint64()
    assert lib().cc_route_events_device_bound(n, max(sessions, 1), C.byref(need)) == abi.CC_OK
    work = torch.empty(max(need.value, 16), dtype=torch.uint8, device="cuda")
    active = C.c_uint64(rc_.COUNT_SENTINEL)
    torch.cuda.synchronize()
    rc = lib().cc_route_events_device(C.byref(i_s), n, d_tab.data_ptr(), d_ids.data_ptr() if with_ids else None, len(tab),
                                      sessions, C.byref(o_s), at(d_inst) if with_ids else None, C.byref(d_s),
                                      C.byref(active), work.data_ptr(), work.numel(),
                                      C.c_void_p(stream.cuda_stream) if stream else None)
    torch.cuda.synchronize()
    for c in rc_.COLS:
        o.cols[c] = _down(d_out[c], rc_.DT[c])
    o.inst, o.session, o.start = _down(d_inst, np.uint64), _down(d_ses, np.uint32), _down(d_start, np.uint32)
    o.count, o.dir_count = _down(d_cnt, np.uint64), _down(d_dcnt, np.uint64)
    if skew:  # the rows before the skew must be untouched; then look at the outputs from where they start
        assert all(np.all(o.cols[c][:skew] == rc_.DT[c](rc_.SENTINEL[c])) for c in rc_.COLS)
        assert np.all(o.inst[:skew] == np.uint64(rc_.INST_SENTINEL))
        assert np.all(o.session[:skew] == rc_.DIR_SENTINEL) and np.all(o.start[:skew] == rc_.DIR_SENTINEL)
        o.cols = {c: o.cols[c][skew:] for c in rc_.COLS}
        o.inst, o.session, o.start = o.inst[skew:], o.session[skew:], o.start[skew:]
    return rc, active.value, o


def _same_as_host(case, **kw):
    from copycat_amd.engine import lib

    rc, active, out = dev_route(case, **kw)
    assert rc == abi.CC_OK, lib().cc_last_error()
    hkw = {k: v for k, v in kw.items() if k in ("out_capacity", "dir_capacity", "with_ids")}
    hrc, hactive, hout = rc_.host_route(lib(), case, 16, **hkw)
    assert hrc == abi.CC_OK and active == hactive == case.n_active, (case.n, case.n_sessions)
    ids = kw.get("with_ids", True)
    assert out.equals(case, with_ids=ids) and hout.equals(case, with_ids=ids), (case.n, case.n_sessions)
    return out


# ---- 1. device against host ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", rc_.DISTRIBUTIONS)
def test_device_equals_host_on_the_grid(pattern):
    for case in rc_.grid(pattern):
        _same_as_host(case)


def test_many_tiles_and_more_than_one_scan_chunk():
    """70 tiles: the (digit, tile) counters fill more than four scan chunks, and the tiles' heads more than one wave"""
    _same_as_host(rc_.build(70 * T + 5, D * D + 1, "zipf", seed=7))
    _same_as_host(rc_.build(70 * T, D + 1, "uniform", seed=8))


# ---- 2. refusals, as the host's -----------------------------------------------------------------------------------------
def _refused(case, want, active=rc_.COUNT_SENTINEL, **kw):
    from copycat_amd.engine import lib

    rc, act, out = dev_route(case, **kw)
    msg = lib().cc_last_error().decode()
    hrc, hact, hout = rc_.host_route(lib(), case, 16, **kw)
    assert rc == hrc == want, (rc, hrc, msg)
    assert out.untouched() and hout.untouched() and act == hact == active
    return msg


def test_device_refusals():
    case = rc_.build(T + 65, D + 1, "uniform", seed=11)
    ev = dict(case.ev)
    ev["target"] = ev["target"].copy()
    ev["target"][[case.n - 1, 77, 3000]] = (case.n_inst, 0xFFFFFFFF, case.n_inst + 1)  # never used to address the table
    msg = _refused(case, abi.CC_ERR_INVALID, ev=ev)
    assert "event 77:" in msg and "target" in msg
    tab = case.session_of_inst.copy()
    slot = int(case.ev["target"][500])
    tab[slot] = case.n_sessions  # an entry == n_sessions
    first = int(np.nonzero(case.ev["target"] == slot)[0][0])
    msg = _refused(case, abi.CC_ERR_INVALID, session_of_inst=tab)
    assert f"event {first}:" in msg and "session_of_inst" in msg
    ev = dict(case.ev)
    ev["target"] = ev["target"].copy()
    ev["target"][first + 1] = case.n_inst  # the lowest event wins between the two kinds
    assert f"event {first}:" in _refused(case, abi.CC_ERR_INVALID, ev=ev, session_of_inst=tab)
    _refused(case, abi.CC_ERR_INVALID, n_sessions=0)
    assert "output" in _refused(case, abi.CC_ERR_CAPACITY, out_capacity=case.n - 1)
    assert "directory" in _refused(case, abi.CC_ERR_CAPACITY, active=case.n_active, dir_capacity=case.n_active - 1)
    _refused(case, abi.CC_ERR_CAPACITY, active=case.n_active, dir_capacity=0)
    _same_as_host(case, dir_capacity=case.n_active)  # exactly enough


# ---- 3. stream, alignment, no ids ---------------------------------------------------------------------------------------
def test_non_default_stream_and_outputs_without_16_byte_alignment():
    import torch

    case = rc_.build(3 * T + 17, D * D + 1, "zipf", seed=13)
    _same_as_host(case, stream=torch.cuda.Stream())
    _same_as_host(case, skew=1, out_capacity=case.n + 100, dir_capacity=case.n_active + 9)
    _same_as_host(case, with_ids=False)


def test_python_wrapper_returns_device_tensors():
    from copycat_amd.engine import DeviceEvents

    case = rc_.build(T + 65, D * D, "uniform", seed=4)
    d = DeviceEvents(case.n + 9)
    for c in rc_.COLS:
        getattr(d, c)[:case.n] = _up(case.ev[c], NPV[c])
    d.count[0] = case.n
    out, inst, (session, start) = route.route_events_device(d, case.session_of_inst, case.n_sessions, case.id_of_inst)
    got = out.host()
    assert got["count"] == case.n and all(np.array_equal(got[c], case.ref[c]) for c in rc_.COLS)
    assert np.array_equal(_down(inst, np.uint64), case.ref_inst)
    assert np.array_equal(_down(session, np.uint32), case.ref_session) and np.array_equal(_down(start, np.uint32), case.ref_start)


# ---- 4. and 5. engines ---------------------------------------------------------------------------------------------------
KEYS = ("pos", "src", "target", "code", "tag", "payload")
CLIENTS = 12


def per_session(ev, session_of_inst, member_out=None):
    """tests/host_boundary_check.py's per_target, by owning session: session -> its events in stream order; the member
    rows of a join's result go to member_out per session"""
    out = {}
    for i in range(len(ev["pos"])):
        s = int(session_of_inst[int(ev["target"][i])])
        if int(ev["code"][i]) == abi.CC_EV_MEMBER:
            if member_out is not None:
                member_out.setdefault(s, []).append((int(ev["pos"][i]), int(ev["payload"][i])))
            continue
        out.setdefault(s, []).append(tuple(int(ev[k][i]) for k in KEYS))
    return out


def _routed(dev_events, tab, ids):
    """route on the device; the routed columns on the host, and each session's run read through the directory"""
    out, inst, (session, start) = route.route_events_device(dev_events, tab, CLIENTS, ids)
    got = out.host()
    session, start = _down(session, np.uint32), _down(start, np.uint32)
    assert np.array_equal(_down(inst, np.uint64), ids[got["target"]])
    runs = {int(s): {k: got[k][int(a):int(b)] for k in KEYS} for s, a, b in zip(session, start[:-1], start[1:])}
    return got, session, start, runs


def _device_events(ev):
    from copycat_amd.engine import DeviceEvents

    n = len(ev["pos"])
    d = DeviceEvents(n + 5)
    for c in rc_.COLS:
        getattr(d, c)[:n] = _up(ev[c], NPV[c])
    d.count[0] = n
    return d


def _sharded_events(b, own, world, make_engine, ev_capacity):
    """split_batch_device(rows=True) -> each rank's engine apply_events -> merge_events_device"""
    import torch

    from copycat_amd.engine import DeviceBatch, DeviceEvents

    db = DeviceBatch.upload(b)
    parts = shard.split_batch_device(db, own, world, rows=True)
    evs, keep = [], []
    for r, (rows, part) in enumerate(parts):
        E = make_engine(r)
        st = torch.empty(part.n, dtype=torch.uint8, device="cuda")
        va = torch.empty(part.n, dtype=torch.uint64, device="cuda")
        ev = DeviceEvents(ev_capacity)
        E.apply_events(part, st, va, ev)
        E.sync()
        evs.append(ev), keep.append(E)
    return shard.merge_events_device(evs, [rows for rows, _ in parts], len(b))


R_COORD, COORD_CAP = 16, 4096  # lock() without a timeout queues for good: room for every lock row of one lock


@functools.lru_cache(maxsize=None)
def _coord_log():
    """a coordination log over 12 clients, one engine's stream for it, and the oracle's events"""
    from copycat_amd.workload import coord_random_stream
    from tests.test_gpu_coord import FLAGS, E_, G, L, V, _oracle_events, _setup

    types = np.array([L, E_, G, V] * (R_COORD // 4), np.uint8)
    E, O, max_inst = _setup(types, CLIENTS, FLAGS, coord_cap=COORD_CAP)
    b = coord_random_stream(4000, types, CLIENTS, max_inst, seed=29)
    timed = (b.op == abi.CC_OP_LOCK_LOCK) & (b.aux.view(np.int64) > 0)
    b.aux[timed] = np.uint64(2**64 - 1)  # lock(timeout) -> lock(): no timer is armed
    s, v, ev = E.apply_host_events(b, capacity=1 << 18)
    s2, v2 = O.apply(b)
    assert np.array_equal(s, s2) and np.array_equal(v, v2)
    # _setup: instance r * K + k has id 1000 + r * K + k and belongs to client 7 + k: session ordinal k
    tab = (np.arange(max_inst) % CLIENTS).astype(np.uint32)
    ids = (1000 + np.arange(max_inst)).astype(np.uint64)
    return types, max_inst, b, ev, _oracle_events(O), tab, ids


def test_coordination_log_per_session_against_the_oracle():
    types, max_inst, b, ev, (oe, apos, amem), tab, ids = _coord_log()
    assert ev["count"] == len(ev["pos"]) > 1000
    got, session, start, runs = _routed(_device_events(ev), tab, ids)
    assert np.all(np.diff(session.astype(np.int64)) > 0) and start[0] == 0 and start[-1] == ev["count"]
    # a commit publishes at most one event per instance and a session holds one instance per resource, so the oracle's
    # events of one session, in its publish order, are that session's list; the member rows of a join's result
    # (ascending ids, target = the joiner) are the oracle's aux stream of the joins that session made
    got_mem, mine = {}, {}
    for s, run in runs.items():
        assert np.all(tab[run["target"]] == s)
        mine.update(per_session(run, tab, got_mem))
    want = per_session(oe, tab)
    assert mine == want and len(want) == CLIENTS
    want_mem = {}
    for p, m in zip(apos.tolist(), amem.tolist()):
        want_mem.setdefault(int(tab[int(b.inst[p])]), []).append((p, m))
    assert got_mem == want_mem and len(want_mem) > 0
    assert sum(len(r["pos"]) for r in runs.values()) == ev["count"]


@pytest.mark.parametrize("world", [2, 4])
def test_coordination_log_through_the_sharded_loop(world):
    from copycat_amd.engine import Engine
    from tests.test_gpu_coord import FLAGS

    types, max_inst, b, ev, _, tab, ids = _coord_log()
    one = _routed(_device_events(ev), tab, ids)
    own = shard.inst_owner_table(np.arange(R_COORD * CLIENTS) // CLIENTS, world)

    def make_engine(rank):
        E = Engine(R_COORD, max_inst, 1 << 20, flags=FLAGS, max_events=1 << 22, coord_cap=COORD_CAP)
        for r in range(R_COORD):
            if r % world == rank:
                E.resource_create(r, int(types[r]))
                for k in range(CLIENTS):
                    E.instance_open(r * CLIENTS + k, r, 1000 + r * CLIENTS + k, 7 + k)
        return E

    merged = _sharded_events(b, own, world, make_engine, 1 << 18)
    got = _routed(merged, tab, ids)
    assert all(np.array_equal(got[0][k], one[0][k]) for k in KEYS)
    assert np.array_equal(got[1], one[1]) and np.array_equal(got[2], one[2])


def test_topic_log_per_session_and_through_the_sharded_loop():
    """8 topics with 16 listeners each over 12 clients: a session owns up to two listeners of a topic, so a publish
    puts two rows of one fan-out into one session's run"""
    from copycat_amd.batch import Batch
    from tests.test_gpu_topic import LISTEN, PUBLISH, UNLISTEN, World, per_target
    from tests.test_gpu_topic import T as TOPIC

    R, K, n = 8, 16, 3000
    w = World([TOPIC] * R, K, client=lambda s: 7 + s % CLIENTS)
    rng = np.random.default_rng(43)
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
    w.check((s1, v1, ev1), want)  # the engine's stream is the model's, per target in publish order
    assert len(ev1["pos"]) > 4 * n
    tab = (np.arange(w.max_inst) % CLIENTS).astype(np.uint32)
    ids = np.array([w.iid(s) for s in range(w.max_inst)], np.uint64)
    got, session, start, runs = _routed(_device_events(ev1), tab, ids)
    assert len(session) == CLIENTS
    mev = want[2]
    model = per_target(*zip(*mev))
    for s, run in runs.items():
        assert np.all(tab[run["target"]] == s)
        assert np.all(np.diff(run["pos"].astype(np.int64)) >= 0)  # a session's run keeps the log order
        mine = per_target(run["pos"], run["target"], run["tag"], run["payload"])
        assert all(mine[t] == model[t] for t in mine)  # ... and every target's publish order, as the model gives it
    assert sorted(t for run in runs.values() for t in set(run["target"].tolist())) == sorted(model)
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

        again = _routed(_sharded_events(b, own, world, make_engine, 1 << 18), tab, ids)
        assert all(np.array_equal(again[0][k], got[k]) for k in KEYS), world
        assert np.array_equal(again[1], session) and np.array_equal(again[2], start)


# ---- 6. a close stream ---------------------------------------------------------------------------------------------------
def test_sessions_close_stream_routes():
    from copycat_amd.engine import DeviceEvents, _check, _np
    from copycat_amd.workload import coord_random_stream
    from tests.test_gpu_coord import FLAGS, E_, G, L, V, _setup

    types = np.array([L, E_, G, V] * 4, np.uint8)
    E, O, max_inst = _setup(types, CLIENTS, FLAGS, coord_cap=COORD_CAP)
    b = coord_random_stream(3000, types, CLIENTS, max_inst, seed=31)
    E.apply_host_events(b, capacity=1 << 18)
    clients = np.array([7 + 3, 7 + 8], np.uint64)
    evs = DeviceEvents(1 << 16)
    s = evs.struct()
    closed = C.c_uint64()
    _check(E.L.cc_sessions_close(E.h, _np(clients), len(clients), C.byref(s), None, C.byref(closed)))
    ev = evs.host()
    assert closed.value > 0 and ev["count"] > 0 and np.all(ev["pos"] == 0xFFFFFFFF) and np.all(ev["src"] == abi.CC_EVSRC_CLOSE)
    tab = (np.arange(max_inst) % CLIENTS).astype(np.uint32)
    ids = (1000 + np.arange(max_inst)).astype(np.uint64)
    got, session, start, runs = _routed(evs, tab, ids)
    ref, ref_inst, ref_session, ref_start = rc_.reference(ev, tab, ids)
    assert all(np.array_equal(got[k], ref[k]) for k in KEYS) and np.all(got["pos"] == 0xFFFFFFFF)
    assert np.array_equal(session, ref_session) and np.array_equal(start, ref_start)
    assert sum(len(r["pos"]) for r in runs.values()) == ev["count"]
