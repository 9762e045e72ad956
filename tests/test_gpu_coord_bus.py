"""GPU: the coordination parity suite on engines that hold a MessageBus.

One bus in an engine makes cc_apply_batch launch k_apply_coord<true> for every coordination row of that engine: its
locks, elections, groups and values then run coord_apply<T, true> and op_registered<true>, the all-value wave takes
the generic copy, mixed waves walk twice and the stores at the end of the launch depend on the type.  The tests of
those four types elsewhere run on engines without a bus; here the same comparisons run with buses (and topics) in the
engine: the oracle for locks, elections, groups and values, tests/topic_model.py and tests/bus_model.py for the rest,
over one engine (tests/coord_bus_cases.CoordBusWorld), with value events, both timer modes and retained sets.
tests/test_coord_bus_cases.py asserts on the CPU that every stream used here is far from trivial.

Every comparison is integer equality: statuses, values, events (the oracle's as a multiset per commit, fan-outs per
target), lock / election / group / value state, the applied index, bus members and registrations, retained sets."""
import numpy as np
import pytest

from copycat_amd import abi
from tests import coord_bus_cases as cc
from tests.kat_runner import EngineBackend, KatRun, all_kats, gpu_eligible
from tests.test_gpu_topic import _dev_prefix, _host_prefix

pytestmark = pytest.mark.gpu

KEYS = ("pos", "target", "code", "src", "tag", "payload")
UNKNOWN_SESSION = abi.CC_ST_UNKNOWN_SESSION


# ---- 1. random parity -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,flags", cc.PARITY_CASES)
def test_random_parity(layout, flags):
    """40,000 rows over the layout in four calls (one row, a slice over the 16,384-row sub-batch boundary, no row, the
    rest), state after each, then the clock past the last deadline.  `module` has no CC_CFG_TIMERS_DEFERRED: the lock
    timeouts fire before the commit that moved the clock (A8), also when that commit is a bus row."""
    w = cc.parity_world(layout, flags)
    b = cc.parity_stream(w, layout)
    for lo, hi in cc.PARITY["slices"]:
        w.apply(b.slice(lo, hi), capacity=1 << 20)
        w.check_state()
    w.advance(int(b.time[-1]) + 1000)
    w.check_state()


# ---- 2. values without value events next to a bus -------------------------------------------------------------------
def test_values_plain():
    """600 values and no CC_CFG_VALUE_EVENTS: the values of the bus's super-bucket run in k_apply_coord<true>, the
    others in k_apply_value_v3; statuses, values and the final state of every slot, the bus against its model."""
    w = cc.values_plain_world()
    b = cc.values_plain_stream(w)
    cuts = cc.VALUES_PLAIN["cuts"]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        w.apply(b.slice(lo, hi))
    w.check_state()
    ty = cc.row_types(w, b)
    res = np.full(w.max_inst, -1, np.int64)
    for r in range(len(w.types)):
        res[w.inst[r]] = r
    sb = np.where(b.inst < w.max_inst, res[np.minimum(b.inst, w.max_inst - 1)], -256) // 256
    assert cc.VALUES_PLAIN_BUS // 256 == 1
    assert ((sb == 1) & (ty == cc.V)).sum() > 5000 and ((sb == 0) & (ty == cc.V)).sum() > 5000 and (ty == cc.B).sum() > 2000


# ---- 3. large blocks ------------------------------------------------------------------------------------------------
def test_large_blocks():
    """coord_cap 256 and 200 instances per resource: lock queues, election listener lists, group member lists and the
    bus's member list all pass the two entries a walking lane caches; the rest of a block lives in global memory."""
    w = cc.large_world()
    b = cc.large_stream(w)
    w.apply(b, capacity=1 << 23)
    w.check_state()
    longest = {cc.L: 0, cc.E_: 0, cc.G: 0}
    for r in w.own:
        t = w.types[r]
        if t == cc.L:
            longest[t] = max(longest[t], len(w.O.lock_state(r)[3]))
        elif t == cc.E_:
            longest[t] = max(longest[t], len(w.O.election_state(r)[2]))
        elif t == cc.G:
            longest[t] = max(longest[t], len(w.O.group_members(r)))
    assert min(longest.values()) > 2, longest
    assert max(len(m.members) for m in w.BW.buses.values()) > 2


# ---- 4. instantiation switches --------------------------------------------------------------------------------------
def test_instantiation_switches():
    """An engine changes kernel instantiation with its first bus and with its last: phase 1 has no bus and no topic
    (<false>, no fan-out pass), phase 2 creates both topics and both buses (<true>), phase 3 deletes both buses (<false>
    with topics), phase 4 creates one bus again.  One index sequence and one clock run through the phases; state, events
    and retained sets after each.  A snapshot after phase 2 goes into a fresh engine in which no bus was ever created
    (the restore has to turn the bus walk on); it runs phases 3 and 4 to the same events, column by column."""
    w = cc.switch_world()
    base = cc.switch_base(w)
    F = None
    for phase in (1, 2, 3, 4):
        cc.switch_enter(w, phase)
        if F is not None and phase == 3:
            for r in cc.SWITCH["buses"]:
                F.resource_delete(r)
        if F is not None and phase == 4:
            r = cc.SWITCH["buses"][0]
            F.resource_create(r, int(cc.B))
            for s in w.inst[r]:
                F.instance_open(s, r, w.iid(s), w.client(s))
        b = cc.switch_stream(w, base, phase)
        w.row_inst = b.inst
        want = w.expect(b)
        got = w.E.apply_host_events(b, capacity=1 << 20)
        w.check(got, want)
        w.check_state()
        if F is not None:
            got_f = F.apply_host_events(b, capacity=1 << 20)
            w.check(got_f, want)
            w.check_state(F)
            assert np.array_equal(got[0], got_f[0]) and np.array_equal(got[1], got_f[1])
            for k in KEYS:
                assert np.array_equal(got[2][k], got_f[2][k]), (phase, k)
        if phase == 2:
            assert (np.isin(got[2]["code"], (abi.CC_EV_BUS_REGISTER, abi.CC_EV_BUS_UNREGISTER))).sum() >= 500
            F = w.fresh_engine()
            F.restore(w.E.snapshot())
            w.check_state(F)
        if phase == 3:
            assert not np.isin(got[2]["code"], (abi.CC_EV_BUS_REGISTER, abi.CC_EV_BUS_UNREGISTER)).any()
            assert (got[2]["code"] == abi.CC_EV_MESSAGE).any()


# ---- 5. close and expire under a bus --------------------------------------------------------------------------------
def test_close_and_expire_under_a_bus():
    """tests/test_gpu_close.test_close_fanout_random at (R = 64, K = 5, n = 20,000) with two buses and two topics in the
    first quarter: the closed clients hold an instance on every resource, the buses included.  Events per target
    against the oracle and the bus model together, the instances that left the table, then a batch on the same
    instances: UNKNOWN_SESSION on the closed ones of every type."""
    w = cc.close_world()
    b = cc.coord_bus_stream(w, cc.CLOSE["n"], cc.CLOSE["seed"], cc.CLOSE["p_bus"])
    w.apply(b, capacity=1 << 21)
    w.check_state()
    before = w.open_slots()
    total = leaves = 0
    for group, expire in cc.close_clients():
        now = w.open_slots()
        closed, _, n_leave = w.close(group, expire)
        assert closed == len(now) - len(w.open_slots())
        total += closed
        leaves += n_leave
    assert total > 0 and leaves > 0
    w.check_state()
    closed_slots = np.setdiff1d(np.array(before), np.array(w.open_slots()))
    b2 = cc.close_follow_up(w, b)
    s, _, _ = w.apply(b2, capacity=1 << 21)
    ty = cc.row_types(w, b2)
    on_closed = np.isin(b2.inst, closed_slots)
    for t in (cc.L, cc.E_, cc.G, cc.V, cc.B, cc.T):
        m = on_closed & (ty == t)
        assert m.any() and (abi.status_code(s[m]) == UNKNOWN_SESSION).all(), t
    w.check_state()
    closed, _, _ = w.close([999])  # a client with no instance closes nothing
    assert closed == 0


# ---- 6. retained sets -----------------------------------------------------------------------------------------------
def test_retained_sets():
    """tests/test_gpu_retained.test_retained_coordination_parity at (n = 2,000, R = 16, K = 3) with schedule rows and two
    buses: the retained set of every slot (check_state compares cc_read_retained of the oracle's slots with the oracle
    and of the buses with the model) after each batch, after two closes, in a restored snapshot and after the timers."""
    w = cc.retain_world()
    b = cc.retain_stream(w)
    n = len(b)
    cuts = [0, n // 3, n // 3 + 1, n]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        w.apply(b.slice(lo, hi))
        w.check_state()
    assert sum(len(w.O.retained(r)) for r in w.own) > cc.RETAIN["R"] // 2
    for client in (7, 8):
        w.close([client])
        w.check_state()
    F = w.fresh_engine()
    F.restore(w.E.snapshot())
    w.check_state(F)
    assert w.O.pending_timers() > 0
    oe = w.advance(int(b.time[-1]) + 1000)
    assert (oe["code"] == abi.CC_EV_EXECUTE).any()
    w.check_state()


# ---- 7. both prefix forms -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix", [_dev_prefix, _host_prefix], ids=["device", "host"])
def test_prefix_stops_at_a_full_lock_queue_after_a_bus_fanout(prefix):
    """coord_cap 64 and one lock with 64 waiters: the prefix forms stop row-exactly before the 65th waiter, whose row
    follows a bus register's fan-out; results, events and state are the references' after the rows before it, the rest
    keeps the caller's prefill, and after an unlock the remainder applies."""
    w = cc.prefix_world()
    fill, b, stop, rest = cc.prefix_batches(w)
    w.apply(fill)
    w.check_state()
    applied, s, v, ev = prefix(w.E, b, 1 << 18)
    assert applied == stop
    w.check_prefix((s, v, ev), b, stop)
    assert (s[stop:] == 0xFF).all()
    fan = ev["pos"] == stop - 1
    assert fan.any() and (ev["code"][fan] == abi.CC_EV_BUS_REGISTER).all()
    w.check_state()
    applied, s, v, ev = prefix(w.E, rest, 1 << 18)
    assert applied == len(rest)
    w.check_prefix((s, v, ev), rest, len(rest))
    w.check_state()
    assert len(w.O.lock_state(cc.PREFIX["lock"])[3]) == cc.PREFIX["cap"]


# ---- 8. the KATs with a bystander bus -------------------------------------------------------------------------------
KATS = [k for k in all_kats() if gpu_eligible(k)]
BUS_SLOT, BUS_CLIENT, BUS_IID = 63, 1 << 40, 1 << 41


class BystanderBackend(EngineBackend):
    """EngineBackend whose engine also holds one bus at resource slot 63 (the quarter of almost every KAT's resources)
    with two instances, in the two highest instance slots, of a client no KAT uses; it never gets a row."""

    def __init__(self, kat):
        super().__init__(kat)
        self.E.resource_create(BUS_SLOT, int(cc.B))
        top = self.E.max_instances
        for k, s in enumerate((top - 2, top - 1)):
            self.E.instance_open(s, BUS_SLOT, BUS_IID + k, BUS_CLIENT)


@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_kat_with_a_bystander_bus(kat):
    used_res = {r[0] for r in kat["resources"]}
    used_inst = {i[0] for i in kat["instances"]}
    assert BUS_SLOT not in used_res and not used_inst & {62, 63}
    assert max([i[2] for i in kat["instances"]] + [0]) < BUS_IID and BUS_CLIENT not in {i[3] for i in kat["instances"]}
    backend = BystanderBackend(kat)
    KatRun(kat, backend).run()
    E = backend.E
    assert E.read_bus_members(BUS_SLOT) == [] and E.read_bus_registrations(BUS_SLOT) == []
    assert [int(x) for x in E.retained(BUS_SLOT)] == []
    assert E.instance_slot(BUS_IID) == E.max_instances - 2 and E.instance_slot(BUS_IID + 1) == E.max_instances - 1
