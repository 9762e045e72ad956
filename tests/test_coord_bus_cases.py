"""The streams of tests/test_gpu_coord_bus.py walked through the references alone (the oracle, tests/bus_model.py,
tests/topic_model.py; no engine): the preconditions that make the GPU comparisons meaningful, so that no stream passes
there by being trivial.  Every (layout, n, seed) of the GPU file is built by the same function of
tests/coord_bus_cases.py and has to show: no bus block full, no lock queue past K, every status class the oracle can
return for locks, elections, groups and values, a lock with two waiters, a waiter expired by its timeout, an election
that promoted a listener, an execute that reached a member, a "change" to a value listener, bus op codes on rows of the
other types, and enough bus traffic.  A seed that misses a condition is replaced in coord_bus_cases.py; no condition is
loosened."""
import numpy as np
import pytest

from copycat_amd import abi
from tests import coord_bus_cases as cc

COORD_STATUS = {abi.CC_ST_OK, abi.CC_ST_UNKNOWN_SESSION, abi.CC_ST_UNKNOWN_OP, abi.CC_ST_ILLEGAL_STATE,
                abi.CC_ST_ILLEGAL_ARGUMENT}  # (NULL_POINTER needs a failed deleteResource: the manager's KATs)
VALUE_STATUS = {abi.CC_ST_OK, abi.CC_ST_UNKNOWN_SESSION, abi.CC_ST_UNKNOWN_OP}


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_lib):
    return oracle_lib


def _coordination_facts(f, K, cap=64, fan=500, joins=100):
    assert f.max_entries < cap, f.max_entries
    assert f.max_queue <= K, f.max_queue
    assert f.status == COORD_STATUS, f.status
    assert f.max_queue >= 2 and f.expired >= 1 and f.promoted >= 1 and f.executed >= 1 and f.changes >= 1, vars(f)
    assert f.bus_ops_on_oracle >= 1
    assert f.fan_events >= fan and f.join_rows >= joins, (f.fan_events, f.join_rows)


def test_mixed_stream_of_the_bus_tests_is_unchanged():
    """tests/test_gpu_bus._mixed_stream draws its bus and topic rows through BusTopicRows now: the rows of its seeds are
    the ones it drew before (the digest was taken from the earlier function)."""
    import hashlib

    from tests.bus_model import BusWorld
    from tests.test_gpu_bus import CLIENTS, NB, _mixed_stream
    from tests.topic_model import TopicWorld

    class Fake:  # the registry of test_gpu_bus._mixed_world, without an engine
        def __init__(self):
            self.types = [cc.B] * NB + [cc.T, cc.G, cc.L] * 4
            K = [CLIENTS] * NB + [4, 2, 2] * 4
            self.BW, self.W, self.inst, s = BusWorld(), TopicWorld(), {}, 0
            for r, t in enumerate(self.types):
                self.inst[r] = list(range(s, s + K[r]))
                s += K[r]
                if t in (cc.B, cc.T):
                    m = self.BW if t == cc.B else self.W
                    m.create(r)
                    for x in self.inst[r]:
                        m.open(x, r, 1000 + x, 7 + x % CLIENTS)

    digests = {}
    for n, seed in ((20_000, 11), (6000, 5), (6000, 23)):
        b = _mixed_stream(Fake(), n, seed)
        h = hashlib.sha256()
        for name, _ in abi.BATCH_COLUMNS:
            h.update(getattr(b, name).tobytes())
        digests[(n, seed)] = h.hexdigest()[:16]
    assert digests == MIXED_STREAM_DIGESTS


MIXED_STREAM_DIGESTS = {(20_000, 11): "ccb0b95ee5622905", (6000, 5): "28117ec410d72b81", (6000, 23): "adf2602b103aaf73"}


@pytest.mark.parametrize("layout,flags", cc.PARITY_CASES)
def test_parity_streams(layout, flags):
    w = cc.parity_world(layout, flags, engine=False)
    b = cc.parity_stream(w, layout)
    f = cc.Facts()
    for lo, hi in cc.PARITY["slices"]:
        cc.walk(w, b.slice(lo, hi), f)
    assert f.rows == cc.PARITY["n"]
    _coordination_facts(f, cc.PARITY["K"])
    ty = cc.row_types(w, b)
    for t in (cc.L, cc.E_, cc.G, cc.V, cc.B) + ((cc.T,) if layout == "mixed" else ()):
        assert (ty == t).sum() > 1000, t
    if layout == "mixed":  # both quarters take rows of every oracle type
        res = {s: r for r in range(len(w.types)) for s in w.inst[r]}
        quarter = np.array([res.get(int(s), -64) // 64 for s in b.inst])
        for q in (0, 1):
            assert {int(t) for t in ty[quarter == q]} >= set(cc.ORACLE_TYPES)


def test_values_plain_stream():
    w = cc.values_plain_world(engine=False)
    b = cc.values_plain_stream(w)
    f = cc.Facts()
    cuts = cc.VALUES_PLAIN["cuts"]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        cc.walk(w, b.slice(lo, hi), f)
    assert f.status == VALUE_STATUS and f.max_entries < 64
    assert f.bus_ops_on_oracle == 0  # (the value generator's foreign ops are map ops)
    assert f.fan_events >= 500 and f.join_rows >= 100, (f.fan_events, f.join_rows)
    ty = cc.row_types(w, b)
    bus_rows = (ty == cc.B).sum()
    assert 0.04 * len(b) < bus_rows < 0.06 * len(b)
    # values of super-bucket 1 (resource slots 256..511) share the bus's kernel, the others keep the value kernel
    res = {s: r for r in range(len(w.types)) for s in w.inst[r]}
    sb = np.array([res.get(int(s), -256) // 256 for s in b.inst])
    for k in (0, 1, 2):
        assert ((sb == k) & (ty == cc.V)).sum() > 5000, k
    assert abi.CC_OP_VALUE_CAS in b.op[(sb == 1) & (ty == cc.V)]


def test_large_stream():
    w = cc.large_world(engine=False)
    f = cc.walk(w, cc.large_stream(w))
    _coordination_facts(f, cc.LARGE["K"], cap=cc.LARGE["cap"])
    assert min(f.max_list.values()) > 2, f.max_list  # past the two cached entries: the rest live in global memory
    assert f.max_entries > 64  # the bus block too is past the default capacity


def test_switch_streams():
    w = cc.switch_world(engine=False)
    base = cc.switch_base(w)
    total = cc.Facts()
    for phase in (1, 2, 3, 4):
        cc.switch_enter(w, phase)
        b = cc.switch_stream(w, base, phase)
        f = cc.walk(w, b)
        ty = cc.row_types(w, b)
        on_bus = (ty == cc.B) & np.isin(b.inst, list(w.BW.inst))
        assert on_bus.any() == (phase in (2, 4)) and ((ty == cc.T).any() == (phase > 1))
        assert f.max_queue <= cc.SWITCH["K"] and f.max_entries < 64
        assert f.status == COORD_STATUS, (phase, f.status)
        assert f.max_queue >= 2 and f.promoted >= 1 and f.executed >= 1 and f.changes >= 1, (phase, vars(f))
        if phase in (2, 4):
            assert f.fan_events >= 500 and f.join_rows >= 100, (phase, f.fan_events, f.join_rows)
        for k in ("expired", "bus_ops_on_oracle"):
            setattr(total, k, getattr(total, k) + getattr(f, k))
    assert total.expired >= 1 and total.bus_ops_on_oracle >= 1
    assert int(base.index[-1]) == len(base) and (np.diff(base.time.astype(np.int64)) >= 0).all()  # one sequence, one clock


def test_close_streams():
    w = cc.close_world(engine=False)
    b = cc.coord_bus_stream(w, cc.CLOSE["n"], cc.CLOSE["seed"], cc.CLOSE["p_bus"])
    f = cc.walk(w, b)
    _coordination_facts(f, cc.CLOSE["K"])
    before = w.open_slots()
    oracle_events = bus_events = 0
    for group, expire in cc.close_clients():
        _, oe, leaves = w.close(group, expire)
        oracle_events += len(oe["pos"])
        bus_events += leaves
    after = w.open_slots()
    closed = sorted(set(before) - set(after))
    assert {int(t) for t in cc.row_types(w, b)[np.isin(b.inst, closed)]} >= {cc.L, cc.E_, cc.G, cc.V, cc.B, cc.T}
    assert oracle_events > 0 and bus_events > 0
    b2 = cc.close_follow_up(w, b)
    s = w.expect(b2)[0]
    ty = cc.row_types(w, b2)
    on_closed = np.isin(b2.inst, closed)
    for t in (cc.L, cc.E_, cc.G, cc.V, cc.B, cc.T):
        m = on_closed & (ty == t)
        assert m.any() and (abi.status_code(s[m]) == abi.CC_ST_UNKNOWN_SESSION).all(), t
    assert (abi.status_code(s[~on_closed & (ty != 0)]) != abi.CC_ST_UNKNOWN_SESSION).all()


def test_retained_stream():
    w = cc.retain_world(engine=False)
    b = cc.retain_stream(w)
    f = cc.walk(w, b)
    _coordination_facts(f, cc.RETAIN["K"])
    assert (b.op == abi.CC_OP_GROUP_SCHEDULE).sum() == cc.RETAIN["schedules"]
    assert sum(len(w.O.retained(r)) for r in w.own) > cc.RETAIN["R"] // 2
    assert w.O.pending_timers() > 0  # schedule commits still retained: the timers have yet to fire


def test_prefix_batches():
    w = cc.prefix_world(engine=False)
    fill, b, stop, rest = cc.prefix_batches(w)
    cap, lock = cc.PREFIX["cap"], cc.PREFIX["lock"]
    w.expect(fill)
    assert len(w.O.lock_state(lock)[3]) == cap  # a holder and 64 waiters
    f = cc.walk(w, b.slice(0, stop - 1))
    fan = w.expect(b, stop - 1, stop)[4]
    assert len(fan) >= 1 and int(b.op[stop - 1]) == cc.REG  # the register on the row before the stop fans out
    assert len(w.O.lock_state(lock)[3]) == cap  # still full: row `stop` is the 65th waiter
    assert int(b.op[stop]) == abi.CC_OP_LOCK_LOCK and int(b.inst[stop]) in w.inst[lock] and int(b.aux[stop]) == 2**64 - 1
    assert (b.op[:stop][np.isin(b.inst[:stop], w.inst[lock])] == abi.CC_OP_ELECT_ISLEADER).all()
    assert len(rest) == len(b) - stop + 1 and int(rest.index[0]) == int(b.index[stop - 1]) + 1
    assert (np.diff(rest.index.astype(np.int64)) == 1).all() and (np.diff(rest.time.astype(np.int64)) >= 0).all()
    cc.walk(w, rest.slice(0, 2), f)
    assert len(w.O.lock_state(lock)[3]) == cap  # the unlock made room for exactly that waiter
    cc.walk(w, rest.slice(2, len(rest)), f)
    assert f.queues.pop(lock) == cap
    f.max_queue = max(f.queues.values())  # (the other locks: the generator's clients bound them)
    _coordination_facts(f, cc.PREFIX["K"])
