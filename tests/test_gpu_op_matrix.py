"""GPU: every op byte x flags byte on every resource type (tests/abi_cases.sweep_rows).

Op dispatch is spread over value_encode, op_registered<kBus>, op_on_gpu, set_as_map_op / mmap_as_map_op, map_key_op and
the two k_apply_coord instantiations, which must all agree with ResourceStateMachineExecutor.java:78 ("unknown operation
type") on ranges that are adjacent or have holes: MultiMap is 75 and 78-84 (76 / 77 have no handler), Bus 85-88, 89 is
no op, Queue 90-99, Set 100-105.  Here each resource gets every op 0..255 with operand tags a, b in 0..4 and key tags
0..3, wrong-typed and null operands included, the unused columns scribbled, the rows permuted and applied twice in one
batch so every op also meets populated state.  Expected: the oracle, or tests/topic_model.py / tests/bus_model.py.
Integer equality only."""
import numpy as np
import pytest

from copycat_amd import abi
from tests import abi_cases as ac

pytestmark = pytest.mark.gpu

V, M, L, E_, G, S, Q, MM = (abi.CC_RES_VALUE, abi.CC_RES_MAP, abi.CC_RES_LOCK, abi.CC_RES_ELECTION, abi.CC_RES_GROUP,
                            abi.CC_RES_SET, abi.CC_RES_QUEUE, abi.CC_RES_MULTIMAP)
ORACLE_TYPES = (V, M, L, E_, G, S, Q, MM)  # every type the oracle has
FLAGS = abi.CC_CFG_TIMERS_DEFERRED | abi.CC_CFG_VALUE_EVENTS
COORD_CAP = 256
UNKNOWN_SESSION = abi.cc_status(abi.CC_ST_UNKNOWN_SESSION, abi.CC_TAG_NULL)
EV_KEYS = ("pos", "src", "target", "code", "tag", "payload")


def _mixed(K=2, extra=0, **cfg):
    """One resource of every oracle type with K instances each (resource r: slots r * K .. r * K + K - 1, ids 1000 +
    slot, instance k of client 7 + k), `extra` instance slots left unopened below max_instances."""
    from copycat_amd.engine import Engine
    from oracle.oracle_py import Oracle
    from tests.handles import register_key_strings

    R = len(ORACLE_TYPES)
    max_inst = R * K + extra
    E = Engine(R, max_inst, 1 << 19, flags=FLAGS, map_capacity=4096, coord_cap=COORD_CAP, max_events=1 << 21,
               sub_batch=65536, **cfg)
    O = Oracle(R, max_inst, FLAGS & abi.CC_CFG_TIMERS_DEFERRED)
    for r, t in enumerate(ORACLE_TYPES):
        E.resource_create(r, int(t))
        O.resource_create(r, int(t))
        for k in range(K):
            s = r * K + k
            E.instance_open(s, r, 1000 + s, 7 + k)
            O.instance_open(s, r, 1000 + s, 7 + k)
    register_key_strings(E, O, 16)  # the sweep's HANDLE keys are 0..3
    return E, O, max_inst


def _lengths(O):
    """every collection the engine keeps in a coord_cap block: lock waiters, election listeners, group members, value
    listeners (retained: current + listeners) and queue elements (retained + the cleaned head)"""
    def read():
        out = []
        for r, t in enumerate(ORACLE_TYPES):
            if t == L:
                out.append(len(O.lock_state(r)[3]))
            elif t == E_:
                out.append(len(O.election_state(r)[2]))
            elif t == G:
                out.append(len(O.group_members(r)))
            elif t in (V, Q):
                out.append(len(O.retained(r)) + 1)
        return out
    return read


def _check_rows(b, got, want):
    s, v, ev = got
    s2, v2, oe, (apos, amem) = want
    bad = np.nonzero((s != s2) | (v != v2))[0]
    assert len(bad) == 0, (f"{len(bad)} rows differ; first {bad[:8]}: inst {b.inst[bad[:8]]} ops {b.op[bad[:8]]} flags "
                           f"{b.flags[bad[:8]]} gpu {s[bad[:8]]},{v[bad[:8]]} oracle {s2[bad[:8]]},{v2[bad[:8]]}")
    from tests.test_gpu_coord import _canon

    member = ev["code"] == abi.CC_EV_MEMBER
    g = _canon(*(ev[k][~member] for k in EV_KEYS))
    w = _canon(*(oe[k] for k in EV_KEYS))
    assert len(g) == len(w), f"{len(g)} events vs oracle {len(w)}"
    assert g == w, next(((i, x, y) for i, (x, y) in enumerate(zip(g, w)) if x != y), None)
    assert list(zip(ev["pos"][member].tolist(), ev["payload"][member].tolist())) == list(zip(apos.tolist(), amem.tolist()))
    assert np.all(np.diff(ev["pos"].astype(np.int64)) >= 0)


def test_mixed_engine_every_op_and_flags_byte():
    """Eight types x 256 ops x 100 flags bytes, twice: 409,600 rows in one call on an engine with a map table,
    coord_cap 256 and value events.  No collection may fill: the oracle's state, read every 64 rows, bounds every
    peak below coord_cap.  Then the state of every resource."""
    from tests.test_gpu_coord import _check_state

    K = 2
    E, O, max_inst = _mixed(K)
    res = [([r * K + k for k in range(K)], [1000 + r * K + k for k in range(K)]) for r in range(len(ORACLE_TYPES))]
    b = ac.sweep_rows(res, seed=701)
    assert len(b) == 8 * 256 * 100 * 2
    s2, v2, oe, aux, peak = ac.peak_lengths(O, b, _lengths(O), step=64)
    assert peak < COORD_CAP, peak
    codes = np.bincount(abi.status_code(s2), minlength=9)
    assert codes[abi.CC_ST_UNKNOWN_OP] > 300_000 and codes[abi.CC_ST_OK] > 5_000
    assert all(codes[c] > 20 for c in (abi.CC_ST_ILLEGAL_STATE, abi.CC_ST_ILLEGAL_ARGUMENT, abi.CC_ST_NULL_POINTER,
                                       abi.CC_ST_NO_SUCH_ELEMENT)), codes
    got = E.apply_host_events(b, capacity=1 << 21)
    _check_rows(b, got, (s2, v2, oe, aux))
    _check_state(E, O, list(ORACLE_TYPES))
    for r, t in enumerate(ORACLE_TYPES):
        if t in (M, S, MM):
            for x, y in zip(E.map_entries(r), O.map_entries(r)):
                assert np.array_equal(x, y), r
        if t != V:  # (a value's retained set needs CC_CFG_VALUE_RETAINED; its state is compared above)
            assert E.retained(r) == O.retained(r), r


def test_rows_that_resolve_to_nothing():
    """The sweep on instances at and past max_instances, on slots never opened and on instances closed by
    cc_sessions_close before the batch: every row is UNKNOWN_SESSION whatever its op and flags, nothing is published
    and no state moves."""
    K, extra = 3, 4
    E, O, max_inst = _mixed(K, extra)
    R = len(ORACLE_TYPES)
    live = ac.sweep_rows([([r * K], [1000 + r * K]) for r in range(R)], seed=711, tags_a=(1, 4), tags_b=(0,), ktags=(0,),
                         repeat=1)
    got = E.apply_host_events(live, capacity=1 << 20)  # populated state for the closed instances to leave behind
    s2, v2 = O.apply(live)
    assert np.array_equal(got[0], s2) and np.array_equal(got[1], v2)
    O.take_events()
    O.take_aux()
    closed, _ =E.sessions_close([7 + 2], capacity=1 << 16)  # instance 2 of every resource
    O.session_close(7 + 2)
    O.take_events()
    assert closed == R
    before = [E.retained(r) for r in range(R) if ORACLE_TYPES[r] != V]
    gone = [r * K + 2 for r in range(R)]
    never = list(range(R * K, R * K + extra))
    past = [max_inst, max_inst + 1, 1 << 31, (1 << 32) - 1]
    slots = gone + never + past
    b = ac.sweep_rows([(slots, [1000 + s for s in gone])], seed=712, index0=int(live.index[-1]) + 1)
    assert len(b) == 256 * 100 * 2 and set(b.inst.tolist()) == set(slots)
    s, v, ev = E.apply_host_events(b, capacity=1 << 16)
    assert (s == UNKNOWN_SESSION).all() and not v.any() and len(ev["pos"]) == 0
    os_, ov = O.apply(b)
    assert np.array_equal(os_, s) and np.array_equal(ov, v)
    assert E.applied_index() == O.applied_index()
    assert before == [E.retained(r) for r in range(R) if ORACLE_TYPES[r] != V]


def test_topic_and_bus_every_op_and_flags_byte():
    """The sweep on a Topic and on a MessageBus against their models.  Join, Register and Unregister carry a HANDLE
    operand below 2^32 (anything else fails the call: test_gpu_bus.py::test_operand_refusals)."""
    from tests.test_gpu_bus import World

    T, B = abi.CC_RES_TOPIC, abi.CC_RES_BUS
    K = 2
    w = World([T, B], K, coord_cap=COORD_CAP, max_batch=1 << 17, max_events=1 << 21)
    res = [(w.inst[r], [w.iid(s) for s in w.inst[r]]) for r in range(2)]
    needs_handle = (abi.CC_OP_BUS_JOIN, abi.CC_OP_BUS_REGISTER, abi.CC_OP_BUS_UNREGISTER)
    b = ac.sweep_rows(res, seed=721, handle_a=lambda r, op: r == 1 and op in needs_handle)
    assert len(b) == 2 * 256 * 100 * 2
    s, v, ev = w.apply(b, capacity=1 << 21)
    w.check_state()
    # no block can fill: listeners and members are keyed by instance (K of them), registrations by (topic 0..3, instance)
    assert len(w.W.topics[0].listener_list()) <= K and w.BW.buses[1].entries() <= K + 4 * K + 4 < COORD_CAP
    codes = np.bincount(abi.status_code(s), minlength=9)
    assert codes[abi.CC_ST_UNKNOWN_OP] > 90_000 and codes[abi.CC_ST_OK] > 1_000 and codes[abi.CC_ST_ILLEGAL_STATE] > 20
    fan = np.isin(ev["code"], (abi.CC_EV_BUS_REGISTER, abi.CC_EV_BUS_UNREGISTER))
    assert (ev["code"] == abi.CC_EV_MESSAGE).sum() > 50 and fan.sum() > 100 and np.isin(ev["code"], (12, 13)).sum() > 50


def test_value_only_engine_every_op_and_flags_byte():
    """The sweep on value resources of an engine without maps and without coordination (k_part_v4 / value_encode),
    less ops 54 / 55, which are CC_ERR_UNSUPPORTED there (test_gpu_value_apply.py)."""
    from copycat_amd.engine import Engine
    from oracle.oracle_py import Oracle
    from tests.test_gpu_value import _assert_same

    R, K = 4, 2
    E = Engine(R, R * K + 8, 1 << 18, sub_batch=ac.SUB_BATCH)
    O = Oracle(R, R * K + 8)
    for r in range(R):
        E.resource_create(r, V)
        O.resource_create(r, V)
        for k in range(K):
            E.instance_open(r * K + k, r, 1000 + r * K + k, 7 + k)
            O.instance_open(r * K + k, r, 1000 + r * K + k, 7 + k)
    res = [([r * K + k for k in range(K)], [1000 + r * K + k for k in range(K)]) for r in range(R)]
    listen = (abi.CC_OP_VALUE_LISTEN, abi.CC_OP_VALUE_UNLISTEN)
    b = ac.sweep_rows(res, seed=731, skip=lambda r, op: op in listen)
    assert len(b) == R * 254 * 100 * 2 and not np.isin(b.op, listen).any()
    gs, gv = E.apply_host(b)
    os_, ov = O.apply(b)
    _assert_same(E, O, gs, gv, os_, ov, R)
    assert (abi.status_code(os_) == abi.CC_ST_OK).sum() > 2_000
