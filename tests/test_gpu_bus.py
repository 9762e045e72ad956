"""GPU: the MessageBus state machine (CC_RES_BUS; apply_coord.hip's bus case, topic_fanout.hip, close.hip) against the
Python restatement of MessageBusState.java (tests/bus_model.py) and the hand-derived KATs (tests/golden/bus_kats.json);
topics, locks and groups that share a walking wave with buses are checked against their own references.

Every test runs through the C-ABI on device columns with the result columns prefilled with the 0xFF sentinel
(Engine.apply_host_events) unless it is about another entry point, and compares statuses, values, events per target,
result rows per joiner, cc_read_bus_members / cc_read_bus_registrations and cc_read_retained with the model.  The
engine's own orders (ascending member id inside a fan-out, ascending topic inside a leave) are pinned by
test_list_lengths and test_leave_with_several_topics.  Integer equality only."""
import numpy as np
import pytest

from copycat_amd import abi
from copycat_amd.batch import Batch, events_check, pack, pack_events, unpack_events, unpack_results
from tests.bus_model import ILLEGAL_STATE, OK_MAP, OK_NULL, BusWorld, bus_rows, info
from tests.coord_bus_cases import BusTopicRows
from tests.test_bus_model import KATS
from tests.test_gpu_topic import World as TopicTestWorld
from tests.test_gpu_topic import _dev_prefix, _host_prefix

pytestmark = pytest.mark.gpu

B, T, G, L = abi.CC_RES_BUS, abi.CC_RES_TOPIC, abi.CC_RES_GROUP, abi.CC_RES_LOCK
JOIN, LEAVE, REG, UNREG, DELETE = (abi.CC_OP_BUS_JOIN, abi.CC_OP_BUS_LEAVE, abi.CC_OP_BUS_REGISTER,
                                   abi.CC_OP_BUS_UNREGISTER, abi.CC_OP_DELETE)
EV_REG, EV_UNREG, EV_LEAVE = abi.CC_EV_BUS_REGISTER, abi.CC_EV_BUS_UNREGISTER, abi.CC_EV_BUS_LEAVE
ROW_CODES = (abi.CC_EV_BUS_TOPIC, abi.CC_EV_BUS_ADDRESS)
KEYS = ("pos", "target", "code", "src", "tag", "payload")


def _by_target(ev):
    """{target: [(row, code, tag, payload)]} in stream order, from (row, target, code, tag, payload) tuples"""
    out = {}
    for r, t, c, g, p in ev:
        out.setdefault(int(t), []).append((int(r), int(c), int(g), int(p)))
    return out


class World(TopicTestWorld):
    """tests/test_gpu_topic.World with buses: resource r of type B lives in the bus model, the others where they did."""

    def __init__(self, types, K, **kw):
        self.BW = BusWorld()
        super().__init__(types, K, **kw)

    def create(self, r):
        if self.types[r] != B:
            return super().create(r)
        self.E.resource_create(r, int(B))
        self.BW.create(r)
        for s in self.inst[r]:
            self.E.instance_open(s, r, self.iid(s), self.client(s))
            self.BW.open(s, r, self.iid(s), self.client(s))

    def expect(self, b, lo=0, hi=None):
        hi = len(b) if hi is None else hi
        s, v, tev, oe = super().expect(b, lo, hi)
        res, bev, brows = self.BW.apply(b.slice(lo, hi))
        for i, (st, val) in res.items():
            s[i], v[i] = st, val
        return s, v, tev, oe, bev, brows

    def check(self, got, want, n=None):
        s, v, ev = got
        s2, v2, tev, oe, bev, brows = want
        bus = np.isin(ev["code"], (EV_REG, EV_UNREG))
        rw = np.isin(ev["code"], ROW_CODES)
        rest = {k: ev[k][~bus & ~rw] for k in KEYS}
        super().check((s, v, rest), (s2, v2, tev, oe), n)
        assert np.all(np.diff(ev["pos"].astype(np.int64)) >= 0)  # the whole stream is ordered by log row
        assert (ev["src"][bus] == abi.CC_EVSRC_COMMIT).all() and (ev["tag"][bus] == abi.CC_TAG_HANDLE).all()
        gb = zip(*(ev[k][bus].tolist() for k in ("pos", "target", "code", "tag", "payload")))
        assert _by_target(gb) == _by_target(bev)
        # a join's result rows: src RESULT, target = the joiner, in the model's order, right at the join's row
        assert (ev["src"][rw] == abi.CC_EVSRC_RESULT).all() and (ev["tag"][rw] == abi.CC_TAG_HANDLE).all()
        got_rows = {}
        for p, t, c, pl in zip(*(ev[k][rw].tolist() for k in ("pos", "target", "code", "payload"))):
            got_rows.setdefault((p, t), []).append((c, pl))
        assert got_rows == {(i, int(self.row_inst[i])): rr for i, rr in brows.items() if rr}
        for i, rr in brows.items():  # the status value is the topic count
            assert int(v[i]) == sum(1 for c, _ in rr if c == abi.CC_EV_BUS_TOPIC) and int(s[i]) == OK_MAP

    def apply(self, b, capacity=None):
        self.row_inst = b.inst
        return super().apply(b, capacity)

    def check_prefix(self, got, b, stop):
        self.row_inst = b.inst
        s, v, ev = got
        self.check((s, v, ev), self.expect(b, 0, stop), n=stop)

    def close(self, client):
        """cc_sessions_close of one client against the models: the bus "leave" events per target"""
        closed, ev = self.E.sessions_close([client])
        want = self.BW.close_client(client)
        self.W.close_client(client)
        self.O.session_close(client)
        self.O.take_events()
        m = ev["code"] == EV_LEAVE
        assert (ev["src"][m] == abi.CC_EVSRC_CLOSE).all() and (ev["pos"][m] == 0xFFFFFFFF).all()
        got = sorted(zip(ev["target"][m].tolist(), ev["code"][m].tolist(), ev["tag"][m].tolist(), ev["payload"][m].tolist()))
        assert got == sorted(want)
        return closed, ev

    def check_state(self, E=None):
        super().check_state(E)
        E = E or self.E
        for r, t in enumerate(self.types):
            if t != B:
                continue
            m = self.BW.buses[r]
            assert E.read_bus_members(r) == m.member_list(), r
            assert E.read_bus_registrations(r) == m.registration_list(), r
            assert [int(x) for x in E.retained(r)] == m.retained(), r


# ---- 1. KATs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kat", KATS, ids=lambda k: k["name"])
def test_kats(kat):
    ids = kat["instances"]
    w = World([B], len(ids), iid=lambda s: ids[s] if s < len(ids) else 9000 + s)
    E, slot = w.E, {m: s for s, m in enumerate(ids)}
    for st in kat["steps"]:
        if "close" in st:
            closed, ev = E.sessions_close([w.client(slot[st["close"]])])
            assert closed == 1
            assert (ev["src"] == abi.CC_EVSRC_CLOSE).all() and (ev["tag"] == abi.CC_TAG_LONG).all()
            got = sorted(zip(ev["target"].tolist(), ev["code"].tolist(), ev["payload"].tolist()))
            assert got == sorted((slot[t], c, p) for t, c, p in st["events"]), st
        else:
            spec = (slot[st["m"]], st["op"], st["a"]) if st["op"] in (JOIN, REG, UNREG) else (slot[st["m"]], st["op"])
            s, v, ev = E.apply_host_events(bus_rows([spec], index0=st["index"]))
            assert (int(s[0]), int(v[0])) == (st["status"], st["value"]), st
            fan = ev["src"] == abi.CC_EVSRC_COMMIT
            got = list(zip(ev["target"][fan].tolist(), ev["code"][fan].tolist(), ev["payload"][fan].tolist()))
            assert got == [(slot[t], c, p) for t, c, p in st["events"]], st  # (ascending member id, ascending topic)
            assert (ev["tag"] == abi.CC_TAG_HANDLE).all() and (ev["pos"] == 0).all()
            rw = ev["src"] == abi.CC_EVSRC_RESULT
            assert (ev["target"][rw] == slot[st["m"]]).all() and (fan | rw).all()
            assert [list(x) for x in zip(ev["code"][rw].tolist(), ev["payload"][rw].tolist())] == st["rows"], st
        if "retained" in st:
            assert [int(x) for x in E.retained(0)] == st["retained"], st
    f = kat["final"]
    assert [list(x) for x in E.read_bus_members(0)] == f["members"]
    assert [list(x) for x in E.read_bus_registrations(0)] == f["registrations"]
    assert [int(x) for x in E.retained(0)] == f["retained"]


# ---- 2. random parity -----------------------------------------------------------------------------------------------
NB, CLIENTS = 48, 12


def _mixed_world(**cfg):
    """48 buses of 12 instances (one per client) and, in the same 64-slot group, 4 topics, 4 groups and 4 locks."""
    types = [B] * NB + [T, G, L] * 4
    K = [CLIENTS] * NB + [4, 2, 2] * 4
    return World(types, K, client=lambda s: 7 + s % CLIENTS, **cfg)


def _mixed_stream(w, n, seed, index0=1, cap=64):
    """Random bus traffic (register / unregister heavy, with joins, leaves, a few Deletes and foreign ops) mixed with
    topic, group and lock rows.  The bus and topic rows are tests/coord_bus_cases.BusTopicRows's, whose scratch copy of
    the bus model walks the stream as it is drawn and turns a join or register that would take a bus past cap - 2
    entries into a leave, so the stream never fills a block."""
    rng = np.random.default_rng(seed)
    b = Batch(n)
    b.index[:] = np.arange(index0, index0 + n, dtype=np.uint64)
    b.time[:] = np.arange(index0, index0 + n, dtype=np.uint64)
    other = {t: np.array([s for r, x in enumerate(w.types) if x == t for s in w.inst[r]], np.uint32) for t in (G, L)}
    kind = rng.choice(4, n, p=[0.85, 0.05, 0.05, 0.05])
    u = rng.random(n)
    rows = BusTopicRows(w, rng, cap)
    for i in range(n):
        k, x = int(kind[i]), float(u[i])
        if k == 0:
            rows.bus(b, i, x)
        elif k == 1:
            rows.topic(b, i, x)
        elif k == 2:
            b.inst[i] = other[G][rng.integers(0, len(other[G]))]
            b.op[i] = abi.CC_OP_GROUP_JOIN if x < 0.5 else abi.CC_OP_GROUP_LEAVE
        else:  # tryLock() (aux 0) never queues
            b.inst[i] = other[L][rng.integers(0, len(other[L]))]
            b.op[i] = abi.CC_OP_LOCK_LOCK if x < 0.5 else abi.CC_OP_LOCK_UNLOCK
    return b


def test_random_parity():
    w = _mixed_world(sub_batch=16384)
    b = _mixed_stream(w, 20_000, 11)
    first = b.slice(0, 17_500)  # crosses the 16,384-row sub-batch boundary; ~300 commits per bus: past a 512-commit chunk
    s, v, ev = w.apply(first, capacity=1 << 19)
    assert (s == ILLEGAL_STATE).any() and (s == OK_MAP).any() and np.isin(ev["code"], ROW_CODES).sum() > 1000
    assert (ev["code"] == EV_REG).sum() > 10_000 and (ev["code"] == EV_UNREG).sum() > 5_000
    w.check_state()
    w.apply(b.slice(17_500, 20_000), capacity=1 << 18)
    w.check_state()
    assert any(x[2] == 0 for r in range(NB) for x in w.BW.buses[r].registration_list())  # empty-topic markers occurred
    assert any(len({m[1] for m in w.BW.buses[r].member_list()}) < len(w.BW.buses[r].members) for r in range(NB))


# ---- 3. list lengths ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap,nm", [(64, 0), (64, 1), (64, 2), (64, 3), (64, 8), (64, 9), (64, 63), (128, 65), (128, 127)])
def test_list_lengths(cap, nm):
    """nm members (at 63 and 127 the one registration fills the block), then the same register three times: nm events
    each, in ascending member instance id.  The instance ids descend with the slot, so id order is not slot order.  With
    no member the register is the ILLEGAL_STATE case."""
    w = World([B], nm + 1, iid=lambda s: 5000 - s, coord_cap=cap)
    order = np.random.default_rng(nm).permutation(nm).tolist()
    spec = [(s, JOIN, 500 + s % 7) for s in order] + [(0, REG, 7)] * 3
    s, v, ev = w.apply(bus_rows(spec), capacity=3 * nm + 1024)
    assert (s[nm:] == (OK_NULL if nm else ILLEGAL_STATE)).all()
    assert len(ev["pos"]) == 3 * nm and (ev["code"] == EV_REG).all()
    assert np.array_equal(ev["target"], np.tile(np.arange(nm - 1, -1, -1, dtype=np.uint32), 3))  # ascending id
    assert np.array_equal(ev["pos"], np.repeat(np.arange(nm, nm + 3, dtype=np.uint32), nm))
    assert (ev["payload"] == info(7, 500)).all()
    w.check_state()
    if nm:
        assert len(w.E.read_bus_registrations(0)) == 1 and len(w.E.retained(0)) == nm + 3  # two replaced Registers leaked


# ---- 4. snapshot reuse ----------------------------------------------------------------------------------------------
def test_snapshot_reuse_one_bus():
    """More than 256 fan records of one bus in one sub-batch (the expansion kernel takes 256 per chunk) against one
    member snapshot; then a join in the middle, after which the fan-outs reach the new member; then a leave."""
    w = World([B], 6, sub_batch=16384)
    spec = [(s, JOIN, 501 + s) for s in range(4)]
    spec += [(i % 4, REG if i % 2 == 0 else UNREG, 1 + (i // 2) % 3) for i in range(600)]
    spec += [(4, JOIN, 600)] + [(i % 5, REG, 1 + i % 3) for i in range(300)]
    spec += [(1, LEAVE)] + [(i % 5, UNREG, 1 + i % 3) for i in range(40)]
    s, v, ev = w.apply(bus_rows(spec), capacity=1 << 13)
    fan = np.isin(ev["code"], (EV_REG, EV_UNREG))
    after = ev["pos"] >= 4 + 600 + 1  # the rows after the fifth member's join
    assert (ev["target"][fan & after] == 4).sum() >= 300 and not (ev["target"][fan & ~after] == 4).any()
    w.check_state()


def test_snapshot_reuse_many_buses():
    """One fan record on each of 300 buses, twice, in one sub-batch: records of many resources in one expansion chunk,
    each against its own snapshot; a join on every bus in between."""
    nb = 300
    w = World([B] * nb, 3, sub_batch=16384, client=lambda s: 7 + s % 3)
    spec = [(3 * r + k, JOIN, 500 + k) for r in range(nb) for k in range(2)]
    spec += [(3 * r, REG, 1 + r % 4) for r in range(nb)]
    spec += [(3 * r + 2, JOIN, 500) for r in range(nb)]
    spec += [(3 * r + 1, REG, 1 + r % 4) for r in range(nb)] + [(3 * r, UNREG, 1 + r % 4) for r in range(nb)]
    s, v, ev = w.apply(bus_rows(spec), capacity=1 << 13)
    assert (ev["code"] == EV_REG).sum() == nb * 2 + nb * 3 and (ev["code"] == EV_UNREG).sum() == nb * 3
    w.check_state()


# ---- 5. a leave with several topics ---------------------------------------------------------------------------------
def test_leave_with_several_topics():
    """One member registered on 5 topics and 7 other members: its leave publishes 35 events, emission index 0..34,
    topic by topic in ascending handle and inside a topic in ascending member id (the stream is ordered by (row, k))."""
    w = World([B], 8, iid=lambda s: 5000 - s)
    topics = [9, 3, 7, 1, 5]
    spec = [(s, JOIN, 500 + s) for s in range(8)] + [(2, REG, t) for t in topics] + [(5, REG, 3), (2, LEAVE)]
    b = bus_rows(spec)
    s, v, ev = w.apply(b)
    row = len(spec) - 1
    m = ev["pos"] == row
    assert m.sum() == 35 and (ev["code"][m] == EV_UNREG).all()
    others = [x for x in range(7, -1, -1) if x != 2]  # ascending id = descending slot
    assert ev["target"][m].tolist() == others * 5
    assert ev["payload"][m].tolist() == [info(t, 502) for t in sorted(topics) for _ in others]
    w.check_state()
    assert w.E.read_bus_registrations(0) == [(3, 4995, 14)]  # (slot 5's Register; the leaver's emptied topics dropped)


# ---- 6. capacity ----------------------------------------------------------------------------------------------------
FULL = [(s, JOIN, 500) for s in range(60)] + [(0, REG, t) for t in (1, 2, 3, 4)]  # 60 members + 4 registrations = 64


def test_capacity_65th_entry_fails_the_batch():
    from copycat_amd.engine import EngineError

    for row in ((0, REG, 5), (60, JOIN, 500)):
        w = World([B], 62)
        w.apply(bus_rows(FULL))
        w.check_state()
        with pytest.raises(EngineError) as ei:
            w.E.apply_host_events(bus_rows([row], index0=100))
        assert ei.value.rc == abi.CC_ERR_CAPACITY


@pytest.mark.parametrize("prefix", [_dev_prefix, _host_prefix], ids=["device", "host"])
def test_capacity_prefix_stops_at_the_65th_entry(prefix):
    """The prefix forms stop row-exactly before the register the full block cannot hold (a re-register and a re-join
    before it add nothing and pass); after a leave the rest applies."""
    w = World([B], 62)
    spec = FULL + [(0, REG, 4), (3, JOIN, 501), (1, REG, 1), (0, REG, 2)]
    b = bus_rows(spec)
    stop = 66
    applied, s, v, ev = prefix(w.E, b, 1 << 12)
    assert applied == stop
    w.check_prefix((s, v, ev), b, stop)
    w.check_state()
    rest = bus_rows([(7, LEAVE)] + spec[stop:], index0=200)
    applied, s, v, ev = prefix(w.E, rest, 1 << 12)
    assert applied == len(rest)
    w.check_prefix((s, v, ev), rest, len(rest))
    assert len(ev["pos"]) == 2 * 59
    w.check_state()


def _product_world():
    """coord_cap 512: 256 members, and member 0 registered on 255 topics — 256 x 255 = 65,280, one entry short of the
    bound, with 511 of the 512 entries in use."""
    w = World([B], 257, coord_cap=512, max_events=1 << 17)
    w.apply(bus_rows([(s, JOIN, 500 + s % 5) for s in range(256)] + [(0, REG, 1 + t) for t in range(255)]), capacity=1 << 17)
    return w


def test_capacity_product_rule_refuses_65536():
    from copycat_amd.engine import EngineError

    w = _product_world()
    w.check_state()
    with pytest.raises(EngineError) as ei:  # 256 x 256 = 65,536: the block has room, the 16-bit event count has none
        w.E.apply_host_events(bus_rows([(1, REG, 1)], index0=1000))
    assert ei.value.rc == abi.CC_ERR_CAPACITY


def test_capacity_product_rule_largest_leave():
    """One entry earlier passes, and the largest leave it admits publishes every event: 255 topics x 255 remaining
    members = 65,025, emission indices up to 65,024."""
    w = _product_world()
    s, v, ev = w.apply(bus_rows([(0, LEAVE)], index0=1000), capacity=1 << 17)
    assert len(ev["pos"]) == 255 * 255 and (ev["code"] == EV_UNREG).all()
    assert ev["payload"].tolist() == [info(1 + t, 500) for t in range(255) for _ in range(255)]
    w.check_state()
    assert w.E.read_bus_registrations(0) == [] and len(w.E.retained(0)) == 255 + 255


@pytest.mark.parametrize("small", ["stream", "max_events"])
@pytest.mark.parametrize("prefix", [_dev_prefix, _host_prefix], ids=["device", "host"])
def test_capacity_no_partial_fanout(prefix, small):
    """An event stream (or max_events arena) of 100 rows and registers of 62 events: the prefix forms stop before the
    second register with the first one's 62 events whole; with room for less than one fan-out, before the first."""
    for cap, stop, nev in ((100, 63, 62), (40, 62, 0)):
        w = World([B], 63, max_events=cap if small == "max_events" else 1 << 20)
        b = bus_rows([(s, JOIN, 500) for s in range(62)] + [(0, REG, 7), (1, REG, 7), (0, LEAVE)])
        applied, s, v, ev = prefix(w.E, b, cap if small == "stream" else 1 << 12)
        assert applied == stop and len(ev["pos"]) == nev
        w.check_prefix((s, v, ev), b, stop)
        w.check_state()


# ---- 7. close and expire --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["close", "expire"])
def test_close_member_and_non_member(how):
    import torch

    # client 8 holds instance 1 of every bus: a registered member of bus 0, a plain member of bus 1, no member of bus 2
    w = World([B, B, B, G], 4, client=lambda s: 7 + s % 4)  # (its instance 13 sits on the group: no member, no event)
    w.apply(bus_rows([(0, JOIN, 500), (1, JOIN, 501), (2, JOIN, 500), (1, REG, 7), (2, REG, 7), (1, REG, 9),
                      (4, JOIN, 500), (5, JOIN, 501), (8, JOIN, 500), (10, JOIN, 502), (8, REG, 3)]))
    if how == "close":
        closed, ev = w.close(8)
    else:
        bm = torch.zeros(1, dtype=torch.int64, device="cuda")
        bm[0] = 1 << 8
        closed, ev = w.E.sessions_expire(bm, 64)
        want = w.BW.close_client(8)
        w.W.close_client(8)
        w.O.session_close(8)
        assert len(w.O.take_events()["pos"]) == 0
        got = sorted(zip(ev["target"].tolist(), ev["code"].tolist(), ev["tag"].tolist(), ev["payload"].tolist()))
        assert got == sorted(want) and (ev["src"] == abi.CC_EVSRC_CLOSE).all()
    assert closed == 4
    assert sorted(ev["target"].tolist()) == [0, 2, 4, 8, 10]  # bus 2: "leave"(1009) although 1009 never joined
    assert sorted(ev["payload"].tolist()) == [1001, 1001, 1005, 1009, 1009]
    w.check_state()
    ret = [int(x) for x in w.E.retained(0)]
    assert 2 in ret and 4 in ret and 6 in ret  # the leaked Join and the two stale Registers (row + 1)
    # the stale registrations are not reported: topic 9 has no member left among its registrants
    s, v, ev = w.apply(bus_rows([(3, JOIN, 777), (0, LEAVE), (2, LEAVE), (3, LEAVE)], index0=50))
    rw = ev["src"] == abi.CC_EVSRC_RESULT
    assert list(zip(ev["code"][rw].tolist(), ev["payload"][rw].tolist())) == [(12, 7), (13, 500), (12, 9)]
    assert w.E.read_bus_registrations(0) == [(7, 1001, 4), (9, 1001, 6)]  # they outlive every member
    w.check_state()


# ---- 8. delete ------------------------------------------------------------------------------------------------------
def test_delete_resource_and_recreate_slot():
    w = World([B, B], 3)
    w.apply(bus_rows([(0, JOIN, 500), (1, JOIN, 501), (3, JOIN, 500), (0, REG, 7), (0, UNREG, 7), (3, REG, 2)]))
    w.E.resource_delete(0)
    w.BW.delete_resource(0)
    w.create(0)
    assert w.E.read_bus_members(0) == [] and w.E.read_bus_registrations(0) == [] and len(w.E.retained(0)) == 0
    s, v, ev = w.apply(bus_rows([(0, REG, 7), (2, JOIN, 502), (2, REG, 7), (4, JOIN, 9), (0, DELETE), (2, REG, 8), (2, LEAVE)],
                                index0=20))
    assert int(s[0]) == ILLEGAL_STATE and len(ev["pos"]) == 1 + 2 + 1  # (bus 1's join reports its topic 2 and its address)
    w.check_state()


# ---- 9. snapshot / restore ------------------------------------------------------------------------------------------
def test_snapshot_restore_mid_stream():
    """A snapshot taken mid-stream (after a close, so a leak and stale registrations travel with it), restored into a
    fresh engine, and the stream continued on both: results, events and final state are equal and the model's."""
    w = _mixed_world(sub_batch=16384)
    b = _mixed_stream(w, 6000, 5)
    w.apply(b.slice(0, 3000), capacity=1 << 17)
    w.close(9)
    F = w.fresh_engine()
    F.restore(w.E.snapshot())
    w.check_state(F)
    rest = b.slice(3000, 6000)
    w.row_inst = rest.inst
    want = w.expect(rest)
    got_e = w.E.apply_host_events(rest, capacity=1 << 17)
    got_f = F.apply_host_events(rest, capacity=1 << 17)
    w.check(got_e, want)
    w.check(got_f, want)
    for k in KEYS:
        assert np.array_equal(got_e[2][k], got_f[2][k]), k
    w.check_state()
    w.check_state(F)


# ---- 10. host entry points ------------------------------------------------------------------------------------------
def test_host_entry_points_match_device_columns():
    """cc_apply_batch_host_packed_events on bus rows (packed batch in, packed results and packed events out) gives the
    device-column path's results and events, and cc_evpack_from_device packs the close fan-out; cc_evpack_check accepts
    both blobs."""
    from copycat_amd.engine import DeviceEvents

    ws = [_mixed_world(sub_batch=16384) for _ in range(2)]
    b = _mixed_stream(ws[0], 6000, 23)
    n, cap = len(b), 1 << 17
    dev = ws[0].apply(b, capacity=cap)
    res, evb, ev_count, done = ws[1].E.apply_host_packed_events(pack(b), n, capacity=cap, chunk_rows=4096)
    assert done == n and ev_count == len(dev[2]["pos"])
    assert events_check(evb) == ev_count
    s, v = unpack_results(res)
    assert np.array_equal(s, dev[0]) and np.array_equal(v, dev[1])
    got = unpack_events(evb)
    for k in KEYS:
        assert np.array_equal(got[k], dev[2][k]), k
    ws[1].BW, ws[1].W, ws[1].O = ws[0].BW, ws[0].W, ws[0].O
    ws[1].check_state()
    # the close fan-out through the packed event blob
    evs = DeviceEvents(1 << 12)
    st = evs.struct()
    import ctypes as C

    clients = np.array([9], np.uint64)
    closed = C.c_uint64()
    E = ws[1].E
    assert E.L.cc_sessions_close(E.h, clients.ctypes.data, 1, C.byref(st), None, C.byref(closed)) == abi.CC_OK
    blob, count = E.events_to_host_packed(evs)
    wide = evs.host()
    assert events_check(blob) == count == len(wide["pos"]) and np.array_equal(blob, pack_events(wide))
    _, wide0 = ws[0].close(9)  # (checks the "leave" events against the model)
    assert (wide0["code"] == EV_LEAVE).any()
    got = unpack_events(blob)
    for k in KEYS:
        assert np.array_equal(got[k], wide0[k]), k


# ---- 11. the two refusals -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [JOIN, REG, UNREG])
@pytest.mark.parametrize("bad", ["tag", "width"])
def test_operand_refusals(op, bad):
    """A Join / Register / Unregister whose operand is not a HANDLE, or is 2^32 or more, fails the call with
    CC_ERR_UNSUPPORTED; the largest handle below 2^32 passes."""
    from copycat_amd.engine import EngineError

    w = World([B], 2)
    top = (1 << 32) - 1
    s, v, ev = w.apply(bus_rows([(0, JOIN, top), (0, REG, top), (1, JOIN, 5)]))
    assert ev["payload"].tolist() == [info(top, top), top, top]  # the register's event, then the join's topic and address
    row = bus_rows([(0, op, 1 << 32)]) if bad == "width" else bus_rows([(0, op, 7)], tag=abi.CC_TAG_LONG)
    row.index[:] = 100
    row.time[:] = 100
    with pytest.raises(EngineError) as ei:
        w.E.apply_host_events(row)
    assert ei.value.rc == abi.CC_ERR_UNSUPPORTED
