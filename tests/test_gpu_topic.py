"""GPU: the Topic state machine (CC_RES_TOPIC; apply_coord.hip's topic case, topic_fanout.hip, close.hip) against the
Python restatement of TopicState.java (tests/topic_model.py) and the hand-derived KATs (tests/golden/topic_kats.json);
locks and groups that share a walking wave with topics are checked against the oracle.

Events of a publish are compared per target session (each goes to a different session; tests/test_gpu_close.py
::_per_target); the engine's own order inside one publish, ascending listener instance id, is pinned by
test_list_lengths.  Integer equality only."""
import ctypes as C
import struct

import numpy as np
import pytest

from copycat_amd import abi
from copycat_amd.batch import Batch, pack
from tests.test_gpu_coord import _canon, _oracle_events
from tests.test_topic_model import KATS, topic_entry
from tests.topic_model import OK_NULL, TopicWorld, per_target

pytestmark = pytest.mark.gpu

T, G, L = abi.CC_RES_TOPIC, abi.CC_RES_GROUP, abi.CC_RES_LOCK
LISTEN, UNLISTEN, PUBLISH = abi.CC_OP_TOPIC_LISTEN, abi.CC_OP_TOPIC_UNLISTEN, abi.CC_OP_TOPIC_PUBLISH
FLAGS = abi.CC_CFG_TIMERS_DEFERRED
MSG = abi.CC_EV_MESSAGE


class World:
    """An engine, the topic model and (for the other types) the oracle over one registry: resource r of types[r] has
    the instance slots inst[r], instance id iid(slot), client client(slot)."""

    def __init__(self, types, K, iid=lambda s: 1000 + s, client=None, flags=FLAGS, **cfg):
        from oracle.oracle_py import Oracle

        self.types = list(types)
        self.K = K if isinstance(K, (list, tuple)) else [K] * len(types)
        self.iid, self.client = iid, client or (lambda s: 7 + s)
        self.max_inst = sum(self.K) + 8
        cfg.setdefault("max_events", 1 << 20)
        self.cfg = dict(max_resources=len(types), max_instances=self.max_inst, max_batch=cfg.pop("max_batch", 1 << 17),
                        flags=flags, **cfg)
        self.E = self.fresh_engine()
        self.W = TopicWorld()
        self.O = Oracle(len(types), self.max_inst, flags & abi.CC_CFG_TIMERS_DEFERRED)  # (the oracle's timer mode)
        self.inst, s = {}, 0
        for r, t in enumerate(self.types):
            self.inst[r] = list(range(s, s + self.K[r]))
            s += self.K[r]
            self.create(r)

    def create(self, r):
        t = self.types[r]
        self.E.resource_create(r, int(t))
        if t == T:
            self.W.create(r)
        else:
            self.O.resource_create(r, int(t))
        for s in self.inst[r]:
            self.E.instance_open(s, r, self.iid(s), self.client(s))
            if t == T:
                self.W.open(s, r, self.iid(s), self.client(s))
            else:
                self.O.instance_open(s, r, self.iid(s), self.client(s))

    def fresh_engine(self):
        from copycat_amd.engine import Engine

        c = dict(self.cfg)
        return Engine(c.pop("max_resources"), c.pop("max_instances"), c.pop("max_batch"), **c)

    def expect(self, b, lo=0, hi=None):
        """The model's / oracle's answer for rows [lo, hi) of b: status, value (the rows of b), message events as
        (row - lo, target, tag, payload), the other events as the oracle gives them."""
        hi = len(b) if hi is None else hi
        part = b.slice(lo, hi)
        s, v = self.O.apply(part)
        s, v = s.copy(), v.copy()
        oe = _oracle_events(self.O)
        res, ev = self.W.apply(part)
        for i, (st, val) in res.items():
            s[i], v[i] = st, val
        return s, v, ev, oe

    def check(self, got, want, n=None):
        """(status, value, events) of the engine against expect()'s answer for the same rows."""
        s, v, ev = got
        s2, v2, mev, (oe, apos, amem) = want
        n = len(s2) if n is None else n
        bad = np.nonzero((s[:n] != s2[:n]) | (v[:n] != v2[:n]))[0]
        assert len(bad) == 0, (bad[:5], s[bad[:5]], v[bad[:5]], s2[bad[:5]], v2[bad[:5]])
        assert np.all(np.diff(ev["pos"].astype(np.int64)) >= 0)  # the stream is ordered by log row
        m = ev["code"] == MSG
        assert (ev["src"][m] == abi.CC_EVSRC_COMMIT).all()
        assert per_target(ev["pos"][m], ev["target"][m], ev["tag"][m], ev["payload"][m]) == \
            per_target(*(zip(*mev) if mev else ([], [], [], [])))
        mem = ev["code"] == abi.CC_EV_MEMBER
        keys = ("pos", "src", "target", "code", "tag", "payload")
        assert _canon(*(ev[k][~m & ~mem] for k in keys)) == _canon(*(oe[k] for k in keys))
        assert list(zip(ev["pos"][mem].tolist(), ev["payload"][mem].tolist())) == list(zip(apos.tolist(), amem.tolist()))

    def apply(self, b, capacity=None):
        got = self.E.apply_host_events(b, capacity=capacity or max(70 * len(b), 1024))
        self.check(got, self.expect(b))
        return got

    def check_state(self, E=None):
        E = E or self.E
        for r, t in enumerate(self.types):
            if t != T:
                continue
            m = self.W.topics[r]
            assert E.topic_listeners(r) == m.listener_list(), r
            ret = [int(x) for x in E.retained(r)]
            assert ret == m.retained(), r
            held = sorted(i for _, i in E.topic_listeners(r))
            leak = sorted(ret)
            for i in held:
                leak.remove(i)
            assert leak == sorted(m.leaked), r  # the leak entries: retained but in no listener entry


def rows(spec, index0=1):
    """[(inst, op, tag, payload)] as a Batch (index and clock advance by one per row)"""
    n = len(spec)
    b = Batch(n)
    b.index[:] = np.arange(index0, index0 + n, dtype=np.uint64)
    b.time[:] = np.arange(index0, index0 + n, dtype=np.uint64)
    b.inst[:] = [x[0] for x in spec]
    b.op[:] = [x[1] for x in spec]
    b.flags[:] = [abi.cc_flags(x[2] if len(x) > 2 else 0) for x in spec]
    b.a[:] = np.array([x[3] if len(x) > 3 else 0 for x in spec], np.uint64)
    return b


# ---- 1. KATs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wire", [False, True], ids=["columns", "wire"])
@pytest.mark.parametrize("kat", KATS, ids=lambda k: k["name"])
def test_kats(kat, wire):
    """Every KAT through cc_apply_batch, on columns built directly and on columns decoded by cc_wire_decode from the
    entries' Catalyst bytes (make_wire's helpers; Delete has no wire id and keeps its direct row)."""
    from copycat_amd.wire import Interner, WireDecoder

    w = World([T if kat["type"] == "TOPIC" else G], kat["instances"])
    E = w.E
    for s in kat["steps"]:
        if "close" in s:
            closed, ev = E.sessions_close([s["close"]])
            assert closed == 1 and len(ev["pos"]) == 0
            continue
        b = rows([(s["k"], s["op"], s["tag"], s["payload"])], index0=s["index"])
        if wire and s["op"] != abi.CC_OP_DELETE:
            msg = {0: None, 1: ("LONG", s["payload"] - (1 << 64) if s["payload"] >> 63 else s["payload"]),
                   2: ("INT", struct.unpack("<i", struct.pack("<I", s["payload"] & 0xFFFFFFFF))[0]),
                   3: ("BOOL", bool(s["payload"]))}.get(s["tag"])
            if s["op"] == abi.CC_OP_GROUP_JOIN or s["tag"] == abi.CC_TAG_HANDLE:
                ent = None  # (no message object to build: a string message would need the interner's handle)
            else:
                ent = topic_entry(1000 + s["k"], s["op"], msg)
            if ent is not None:
                d, iid, kind = WireDecoder(engine=None, interner=Interner(1)).decode(entries=[ent])
                assert int(iid[0]) == 1000 + s["k"] and int(kind[0]) == 0
                b.op[:], b.flags[:], b.a[:] = d.op, d.flags, d.a
                assert int(b.op[0]) == s["op"] and abi.flag_tag_a(int(b.flags[0])) == s["tag"]
        st, v, ev = E.apply_host_events(b)
        assert (int(st[0]), int(v[0])) == (s["status"], s["value"]), s
        got = sorted(zip(ev["target"].tolist(), ev["tag"].tolist(), ev["payload"].tolist()))
        assert got == sorted(tuple(x) for x in s["events"]), s
        assert (ev["code"] == MSG).all() and (ev["src"] == abi.CC_EVSRC_COMMIT).all() and (ev["pos"] == 0).all()
    f = kat["final"]
    if f is not None:
        assert [list(x) for x in E.topic_listeners(0)] == f["listeners"]
        ret = [int(x) for x in E.retained(0)]
        assert ret == f["retained"]
        held = [i for _, i in f["listeners"]]
        assert sorted(set(ret) - set(held)) == f["leaked"]


# ---- 2. random parity -----------------------------------------------------------------------------------------------
def _mixed_world(**cfg):
    """8 topics, 4 locks and 4 groups on neighbouring slots (one walking wave): 64 instances of 16 clients."""
    types = [T, L, T, G, T, T, L, G, T, L, T, G, T, L, T, G]
    K = [6 if t == T else 2 for t in types]
    return World(types, K, client=lambda s: 7 + s % 16, **cfg)


def _mixed_stream(w, n, seed, index0=1):
    rng = np.random.default_rng(seed)
    b = Batch(n)
    b.index[:] = np.arange(index0, index0 + n, dtype=np.uint64)
    b.time[:] = np.arange(index0, index0 + n, dtype=np.uint64)
    tinst = np.array([s for r, t in enumerate(w.types) if t == T for s in w.inst[r]], np.uint32)
    linst = np.array([s for r, t in enumerate(w.types) if t == L for s in w.inst[r]], np.uint32)
    ginst = np.array([s for r, t in enumerate(w.types) if t == G for s in w.inst[r]], np.uint32)
    kind = rng.choice(3, n, p=[0.8, 0.1, 0.1])
    u = rng.random(n)
    top = kind == 0
    b.inst[:] = np.where(top, tinst[rng.integers(0, len(tinst), n)],
                         np.where(kind == 1, linst[rng.integers(0, len(linst), n)], ginst[rng.integers(0, len(ginst), n)]))
    b.op[:] = np.where(top, np.where(u < 0.7, PUBLISH, np.where(u < 0.85, LISTEN, UNLISTEN)),
                       np.where(kind == 1, np.where(u < 0.5, abi.CC_OP_LOCK_LOCK, abi.CC_OP_LOCK_UNLOCK),
                                np.where(u < 0.5, abi.CC_OP_GROUP_JOIN, abi.CC_OP_GROUP_LEAVE)))
    tag = rng.integers(0, 5, n)  # every tag, NULL included
    b.flags[:] = np.where(top, tag, 0).astype(np.uint8)
    pay = rng.integers(0, 1 << 63, n, dtype=np.uint64) | (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63))
    b.a[:] = np.where(top, pay, 0)
    # (lock rows are tryLock(), aux 0: they never queue, so random traffic cannot fill a lock's waiter block)
    return b


def test_random_parity():
    w = _mixed_world(sub_batch=16384)
    b = _mixed_stream(w, 50_000, 11)
    s, v, ev = w.apply(b)
    assert (s[b.op == PUBLISH] == OK_NULL).all()
    m = ev["code"] == MSG
    assert m.sum() > 50_000 and (ev["payload"][m] >> np.uint64(63)).any() and (ev["tag"][m] == 0).any()
    w.check_state()


# ---- 3. list lengths ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap,nl", [(64, 0), (64, 1), (64, 2), (64, 3), (64, 63), (64, 64), (128, 65), (128, 127),
                                    (128, 128)])
def test_list_lengths(cap, nl):
    """nl listeners (the register entry, the LDS entry, the global entries, the full block; past 64 an expansion of
    more than one wave), then 200 publishes: exactly nl events per publish, in ascending listener instance id.  The
    instance ids descend with the slot, so id order is not slot order."""
    w = World([T], nl + 1, iid=lambda s: 5000 - s, coord_cap=cap)
    order = np.random.default_rng(nl).permutation(nl).tolist()
    spec = [(s, LISTEN) for s in order] + [(nl, PUBLISH, abi.CC_TAG_LONG, 100 + i) for i in range(200)]
    s, v, ev = w.apply(rows(spec), capacity=200 * nl + 1024)
    assert len(ev["pos"]) == 200 * nl and (ev["code"] == MSG).all()
    want_t = np.tile(np.arange(nl - 1, -1, -1, dtype=np.uint32), 200)  # ascending id = descending slot
    assert np.array_equal(ev["target"], want_t)
    assert np.array_equal(ev["pos"], np.repeat(np.arange(nl, nl + 200, dtype=np.uint32), nl))
    assert np.array_equal(ev["payload"], np.repeat(np.arange(100, 300, dtype=np.uint64), nl))
    w.check_state()


# ---- 4. snapshot reuse ----------------------------------------------------------------------------------------------
def test_snapshot_reuse():
    """One topic: publish, publish, listen(new), publish, unlisten(same), publish, listen(existing), publish, 2,200
    times (2,000 repetitions are 16,000 rows, short of the 16,384-row sub-batch boundary).  The pattern is 8 rows and a
    chunk 512, so one extra publish after every 63 repetitions moves the pattern's phase by one against the 512-commit
    chunks and the sub-batch boundary: a chunk boundary falls at every phase.  A snapshot reused after the list
    changed, or one from an earlier launch, shows as a wrong target set."""
    w = World([T], 9, sub_batch=16384)
    pub = 8
    w.apply(rows([(0, LISTEN), (1, LISTEN), (2, LISTEN)]))
    spec, extra = [], 0
    for i in range(2200):
        new = 3 + i % 5
        m = (abi.CC_TAG_LONG, i)
        spec += [(pub, PUBLISH, *m), (pub, PUBLISH, *m), (new, LISTEN), (pub, PUBLISH, *m), (new, UNLISTEN),
                 (pub, PUBLISH, *m), (i % 3, LISTEN), (pub, PUBLISH, *m)]
        if i % 63 == 62:
            spec.append((pub, PUBLISH, abi.CC_TAG_INT, 7))
            extra += 1
    b = rows(spec, index0=10)
    assert len(b) > 16384 + 512 and extra >= 16
    s, v, ev = w.apply(b)
    assert len(ev["pos"]) == 2200 * (4 * 3 + 4) + extra * 3
    w.check_state()


# ---- 5. capacity ----------------------------------------------------------------------------------------------------
def _dev_prefix(E, b, capacity):
    import torch

    from copycat_amd.engine import RESULT_SENTINEL, DeviceBatch, DeviceEvents

    n = len(b)
    st = torch.full((n,), RESULT_SENTINEL, dtype=torch.uint8, device="cuda")
    va = torch.zeros(n, dtype=torch.int64, device="cuda")
    evs = DeviceEvents(capacity)
    applied = E.apply_prefix(DeviceBatch.upload(b), st, va, evs)
    return applied, st.cpu().numpy(), va.cpu().numpy().view(np.uint64), evs.host()


def _host_prefix(E, b, capacity):
    applied, s, v, ev = E.apply_host_prefix(b, capacity=capacity)
    return applied, s, v, ev


def test_capacity_listen_fails_the_batch():
    from copycat_amd.engine import EngineError

    w = World([T], 66)
    w.apply(rows([(s, LISTEN) for s in range(64)]))
    with pytest.raises(EngineError) as ei:
        w.E.apply_host_events(rows([(64, LISTEN)], index0=100))
    assert ei.value.rc == abi.CC_ERR_CAPACITY


@pytest.mark.parametrize("prefix", [_dev_prefix, _host_prefix], ids=["device", "host"])
def test_capacity_prefix_stops_at_the_65th_listen(prefix):
    """The prefix forms stop row-exactly before the listen the full block cannot hold; state, results and events are
    the model's after the prefix; after an unlisten the rest applies."""
    w = World([T], 66)
    m = (abi.CC_TAG_LONG, 5)
    spec = [(s, LISTEN) for s in range(64)] + [(65, PUBLISH, *m), (3, LISTEN), (64, LISTEN), (65, PUBLISH, *m)]
    b = rows(spec)
    stop = 66
    applied, s, v, ev = prefix(w.E, b, 1 << 12)
    assert applied == stop
    w.check((s, v, ev), w.expect(b, 0, stop), n=stop)
    w.check_state()
    rest = rows([(7, UNLISTEN)] + spec[stop:], index0=200)
    applied, s, v, ev = prefix(w.E, rest, 1 << 12)
    assert applied == len(rest)
    w.check((s, v, ev), w.expect(rest))
    assert len(ev["pos"]) == 64
    w.check_state()


@pytest.mark.parametrize("small", ["stream", "max_events"])
@pytest.mark.parametrize("prefix", [_dev_prefix, _host_prefix], ids=["device", "host"])
def test_capacity_no_partial_fanout(prefix, small):
    """An event stream (or max_events arena) of 100 rows and publishes of 64 events: the prefix forms stop before the
    second publish with the first one's 64 events whole; with room for less than one publish, before the first."""
    for cap, stop, nev in ((100, 65, 64), (40, 64, 0)):
        w = World([T], 65, max_events=cap if small == "max_events" else 1 << 20)
        m = (abi.CC_TAG_LONG, 9)
        b = rows([(s, LISTEN) for s in range(64)] + [(64, PUBLISH, *m), (64, PUBLISH, *m), (0, UNLISTEN)])
        applied, s, v, ev = prefix(w.E, b, cap if small == "stream" else 1 << 12)
        assert applied == stop and len(ev["pos"]) == nev
        w.check((s, v, ev), w.expect(b, 0, stop), n=stop)
        w.check_state()


# ---- 6. close -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["close", "expire"])
def test_close_drops_the_listener_and_leaks_its_commit(how):
    import torch

    w = World([T, T, T, G], 4, client=lambda s: 7 + s % 4)  # client 8 holds instance 1 of every resource
    w.apply(rows([(s, LISTEN) for s in range(12)] + [(2, PUBLISH, abi.CC_TAG_LONG, 1)]))
    if how == "close":
        closed, ev = w.E.sessions_close([8])
    else:
        bm = torch.zeros(1, dtype=torch.int64, device="cuda")
        bm[0] = 1 << 8
        closed, ev = w.E.sessions_expire(bm, 64)
    assert closed == 4 and not (ev["code"] == MSG).any()  # (instance 13 sits on the group: no member, no event)
    w.W.close_client(8)
    w.O.session_close(8)
    assert len(w.O.take_events()["pos"]) == 0
    for r in range(3):
        assert (1000 + 4 * r + 1) not in dict(w.E.topic_listeners(r))
        assert (4 * r + 1 + 1) in [int(x) for x in w.E.retained(r)]  # the listen commit's index (row + 1)
    w.check_state()
    s, v, ev = w.apply(rows([(0, PUBLISH, abi.CC_TAG_INT, 3), (4, PUBLISH), (10, PUBLISH, abi.CC_TAG_BOOL, 1),
                             (1, PUBLISH), (5, LISTEN)], index0=50))
    assert len(ev["pos"]) == 9 and not np.isin(ev["target"], [1, 5, 9]).any()
    assert abi.status_code(int(s[3])) == abi.CC_ST_UNKNOWN_SESSION == abi.status_code(int(s[4]))
    w.check_state()


# ---- 7. delete / recreate, snapshot / restore -----------------------------------------------------------------------
def test_delete_and_recreate_slot():
    w = World([T, T], 3)
    w.apply(rows([(0, LISTEN), (1, LISTEN), (3, LISTEN), (2, PUBLISH, abi.CC_TAG_LONG, 4)]))
    w.E.resource_delete(0)
    w.W.delete_resource(0)
    w.create(0)
    assert w.E.topic_listeners(0) == [] and [int(x) for x in w.E.retained(0)] == []
    s, v, ev = w.apply(rows([(2, PUBLISH, abi.CC_TAG_LONG, 5), (2, LISTEN), (0, PUBLISH), (5, PUBLISH)], index0=20))
    assert len(ev["pos"]) == 2
    w.check_state()


def test_snapshot_restore_mid_stream():
    """A snapshot taken mid-stream, restored into a fresh engine, and the stream continued there: results, events and
    final state equal the uninterrupted run (both equal the model)."""
    w = _mixed_world(sub_batch=16384)
    b = _mixed_stream(w, 6000, 5)
    w.apply(b.slice(0, 3000))
    w.E.sessions_close([9])  # a leaked listen commit travels with the snapshot
    w.W.close_client(9)
    w.O.session_close(9)
    w.O.take_events()
    F = w.fresh_engine()
    F.restore(w.E.snapshot())
    w.check_state(F)
    rest = b.slice(3000, 6000)
    want = w.expect(rest)
    got_e = w.E.apply_host_events(rest, capacity=1 << 18)
    got_f = F.apply_host_events(rest, capacity=1 << 18)
    w.check(got_e, want)
    w.check(got_f, want)
    for k in ("pos", "target", "code", "src", "tag", "payload"):
        assert np.array_equal(got_e[2][k], got_f[2][k]), k
    w.check_state()
    w.check_state(F)


# ---- 8. host boundary -----------------------------------------------------------------------------------------------
def test_host_entry_points_match_device_columns():
    """cc_apply_batch_host_events (host columns, host events) and cc_apply_batch_host_packed on topic rows: the results
    and events of the device-column path."""
    ws = [_mixed_world(sub_batch=16384) for _ in range(3)]
    b = _mixed_stream(ws[0], 20_000, 23)
    want = ws[0].expect(b)
    dev = ws[0].E.apply_host_events(b, capacity=1 << 19)
    ws[0].check(dev, want)
    # host columns, host event stream
    E = ws[1].E
    n, cap = len(b), 1 << 19
    st, va = np.zeros(n, np.uint8), np.zeros(n, np.uint64)
    cb = abi.cc_batch()
    for name, _ in abi.BATCH_COLUMNS:
        setattr(cb, name, getattr(b, name).ctypes.data)
    cols = {"pos": np.zeros(cap, np.uint32), "target": np.zeros(cap, np.uint32), "code": np.zeros(cap, np.uint8),
            "src": np.zeros(cap, np.uint8), "tag": np.zeros(cap, np.uint8), "payload": np.zeros(cap, np.uint64)}
    count = np.zeros(1, np.uint64)
    ev = abi.cc_events(*(cols[k].ctypes.data for k in ("pos", "target", "code", "src", "tag", "payload")), cap,
                       count.ctypes.data)
    r = abi.cc_results(st.ctypes.data, va.ctypes.data)
    assert E.L.cc_apply_batch_host_events(E.h, C.byref(cb), n, C.byref(r), C.byref(ev)) == abi.CC_OK
    host = (st, va, {k: x[:int(count[0])] for k, x in cols.items()})
    # packed blob
    s3, v3, e3, done = ws[2].E.apply_host_packed(pack(b), n, capacity=cap)
    assert done == n
    for got in (host, (s3, v3, e3)):
        assert np.array_equal(got[0], dev[0]) and np.array_equal(got[1], dev[1])
        for k in ("pos", "target", "code", "src", "tag", "payload"):
            assert np.array_equal(got[2][k], dev[2][k]), k
    for w in ws[1:]:
        w.W, w.O = ws[0].W, ws[0].O
        w.check_state()
