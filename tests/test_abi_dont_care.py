"""CPU: "Columns an op does not use may hold anything" (include/copycat_apply.h, cc_batch) in the references.

tests/abi_cases.USED is the statement of the promise.  It is the wire decoder's carried-fields contract
(tests/test_wire.py::_carried) for every op that function names, and the oracle, tests/topic_model.py and
tests/bus_model.py give identical results, events and final state for a batch b and for scribble(b) on every stream of
tests/test_gpu_dont_care.py: that is what licenses comparing the engine on scribble(b) with the references on b.  The
allowed difference is 0 rows.  No GPU."""
import re
import os

import numpy as np
import pytest

from copycat_amd import abi
from tests import abi_cases as ac

EV_KEYS = ("pos", "target", "code", "src", "tag", "payload")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "copycat_apply.h")


def test_used_is_the_wire_decoders_carried_fields():
    from tests.golden.make_wire import OP
    from tests.test_wire import _carried

    named = 0
    for name in OP:
        if not hasattr(abi, "CC_OP_" + name):
            continue
        carried = _carried(name)
        if carried:
            named += 1
        if name in ac.USED_BY_NAME and not carried:
            assert name.startswith(("TOPIC_", "BUS_")), name  # (_carried names no topic / bus op: their operand is a)
            continue
        assert ac.USED[getattr(abi, "CC_OP_" + name)] == carried, name
    assert named >= 30
    for name in ac.USED_BY_NAME:
        assert _carried(name) in (ac.USED_BY_NAME[name], set()), name


def test_used_covers_exactly_the_ops_of_the_header():
    ops = {v for k, v in vars(abi).items() if k.startswith("CC_OP_")}
    assert {o for o, cols in ac.USED.items() if cols} <= ops
    assert all(ac.USED[o] == frozenset() for o in range(256) if o not in ops)


def test_header_carries_the_table():
    """The cc_batch comment holds the table of abi_cases._TABLE, row for row."""
    text = open(HEADER).read()
    lo = text.index("Columns an op does not use may hold anything")
    comment = re.sub(r"[\s*/,]+", " ", text[lo:text.index("typedef struct cc_batch", lo)])
    for cols, names in ac._TABLE:
        row = cols + " | " + " ".join(names.split())
        assert row in comment, row


def test_scribble_changes_only_unused_cells():
    from copycat_amd.workload import map_random_stream

    b = map_random_stream(20_000, 8, 16, keys=64, seed=3)
    s = ac.scribble(b, 9)
    use = ac.used_mask(b.op)
    for name, shift, bits in (("a", 0, 7), ("b", 3, 7), ("key", 6, 3)):
        u = use[name]
        assert np.array_equal(getattr(b, name)[u], getattr(s, name)[u])
        assert np.array_equal((b.flags[u] >> shift) & bits, (s.flags[u] >> shift) & bits)
        assert (getattr(b, name)[~u] != getattr(s, name)[~u]).mean() > 0.99
    assert np.array_equal(b.aux[use["aux"]], s.aux[use["aux"]])
    for name in ("index", "time", "inst", "op"):
        assert np.array_equal(getattr(b, name), getattr(s, name))
    free_a = ~use["a"]
    assert set(np.unique(s.flags[free_a] & 7).tolist()) == set(range(8))  # the result-only tags 5..7 occur
    assert set(np.unique(s.flags[~use["key"]] >> 6).tolist()) == set(range(4))  # and the HANDLE key tag


@pytest.mark.parametrize("replicas", [1, 2, 3, 4, 5, 6, 7, 8, 15, 16])
def test_quorum_oracle_is_the_numpy_rule_on_the_edge_inputs(replicas):
    """The reference of tests/test_gpu_quorum.py's edge cases: the oracle equals "sort descending, take entry R / 2" on
    inputs at 0, 2^63 and 2^64 - 1, and a fair share of the groups advance."""
    from oracle.oracle_py import quorum_commit

    for groups in (4097, 4098):
        match, ts, ci = ac.quorum_edge_groups(groups, replicas, seed=groups * 31 + replicas)
        want = ac.quorum_numpy(match, ts, ci)
        assert np.array_equal(quorum_commit(match, ts, ci), want)
        assert 0.05 < (want != ci).mean() < 0.5
        assert (match >= np.uint64(1 << 63)).any() and (match < np.uint64(3)).any()


@pytest.mark.parametrize("now", [10_000_000, (1 << 63) + 5, 3])
def test_expiry_oracle_takes_the_timeout_as_signed(now):
    from oracle.oracle_py import expire_sweep

    last = ac.expiry_edge_sessions(1001, now, seed=now % 1000 + 1)
    with np.errstate(over="ignore"):
        diff = (np.uint64(now) - last).view(np.int64)
    for timeout in ac.EXPIRY_TIMEOUTS + (5000,):
        signed = timeout - (1 << 64) if timeout >> 63 else timeout
        want = diff > signed
        bm, count = expire_sweep(last, now, timeout)
        bits = np.unpackbits(bm.view(np.uint8), bitorder="little")[:1001].astype(bool)
        assert np.array_equal(bits, want) and count == int(want.sum())
    assert 0 < (diff > 5000).sum() < 1001


def _same_rows(x, y):
    s, v = x
    s2, v2 = y
    bad = np.nonzero((s != s2) | (v != v2))[0]
    assert len(bad) == 0, (len(bad), bad[:5])


def test_oracle_ignores_unused_columns_value_stream():
    from oracle.oracle_py import Oracle

    b = ac.value_stream()
    sb = ac.scribble(b, 1)
    assert ac.changed_share(b, sb) > 0.5
    R = ac.VALUE["resources"]
    Os = [Oracle(R, R + 8) for _ in range(2)]
    for O in Os:
        for r in range(R):
            O.resource_create(r, abi.CC_RES_VALUE)
            O.instance_open(r, r, 1000 + r, 7)
    _same_rows(Os[0].apply(b), Os[1].apply(sb))
    for x, y in zip(Os[0].value_state(), Os[1].value_state()):
        assert np.array_equal(x, y)
    assert np.array_equal(Os[0].value_retained(), Os[1].value_retained())
    assert Os[0].applied_index() == Os[1].applied_index()


def table_oracle(flags):
    from oracle.oracle_py import Oracle
    from tests.handles import register_key_strings

    types = ac.table_types()
    R = len(types)
    O = Oracle(R, R + 8, flags & abi.CC_CFG_TIMERS_DEFERRED)
    for r, t in enumerate(types):
        O.resource_create(r, int(t))
        O.instance_open(r, r, 1000 + r, 7)
    register_key_strings(None, O)
    return O


@pytest.mark.parametrize("ttl,flags", [(False, abi.CC_CFG_TIMERS_DEFERRED), (True, abi.CC_CFG_TIMERS_DEFERRED), (True, 0)],
                         ids=["plain", "ttl-manager", "ttl-module"])
def test_oracle_ignores_unused_columns_table_stream(ttl, flags):
    b = ac.table_stream(ttl)
    sb = ac.scribble(b, 2)
    assert len(b) == 60_000 and ac.changed_share(b, sb) > 0.5
    types = ac.table_types()
    Os = [table_oracle(flags) for _ in range(2)]
    got = Os[0].apply(b)
    _same_rows(got, Os[1].apply(sb))
    keyed = [r for r, t in enumerate(types) if t != abi.CC_RES_VALUE]
    for r in keyed:
        for x, y in zip(Os[0].map_entries(r), Os[1].map_entries(r)):
            assert np.array_equal(x, y), r
        assert Os[0].retained(r) == Os[1].retained(r), r
    for x, y in zip(Os[0].value_state(0, ac.TABLE["values"]), Os[1].value_state(0, ac.TABLE["values"])):
        assert np.array_equal(x, y)
    # the stream is far from trivial: barrier rows, containsValue answers of both kinds, live entries at the end
    s, v = got
    cv = (b.op == abi.CC_OP_MAP_CONTAINSVALUE) & (s == abi.cc_status(abi.CC_ST_OK, abi.CC_TAG_BOOL))
    assert (v[cv] == 1).sum() > 20 and (v[cv] == 0).sum() > 20
    assert sum(len(Os[0].map_entries(r)[0]) for r in keyed) > 1000
    assert (b.op == abi.CC_OP_DELETE).sum() > 10 and ((b.op == abi.CC_OP_MAP_CLEAR).sum() > 10) == (not ttl)


@pytest.mark.parametrize("bus", [False, True], ids=["no-bus", "bus-and-topic"])
def test_references_ignore_unused_columns_coord_stream(bus):
    from tests.coord_bus_cases import B, E_, G, L, T

    ws = [ac.coord_world(bus, engine=False) for _ in range(2)]
    b = ac.coord_stream(ws[0], bus)
    sb = ac.scribble(b, 3)
    assert len(b) == ac.COORD["n"] and ac.changed_share(b, sb) > 0.5
    s, v, tev, (oe, apos, amem), bev, brows = ws[0].expect(b)
    s2, v2, tev2, (oe2, apos2, amem2), bev2, brows2 = ws[1].expect(sb)
    _same_rows((s, v), (s2, v2))
    assert tev == tev2 and bev == bev2 and brows == brows2
    for k in EV_KEYS:
        assert np.array_equal(oe[k], oe2[k]), k
    assert np.array_equal(apos, apos2) and np.array_equal(amem, amem2)
    w, w2 = ws
    for r, t in enumerate(w.types):
        if t == L:
            assert w.O.lock_state(r) == w2.O.lock_state(r)
        elif t == E_:
            assert w.O.election_state(r) == w2.O.election_state(r)
        elif t == G:
            assert w.O.group_members(r) == w2.O.group_members(r)
        elif t == T:
            assert w.W.topics[r].listener_list() == w2.W.topics[r].listener_list()
        elif t == B:
            assert w.BW.buses[r].member_list() == w2.BW.buses[r].member_list()
            assert w.BW.buses[r].registration_list() == w2.BW.buses[r].registration_list()
        if t not in (T, B):
            assert w.O.retained(r) == w2.O.retained(r), r
    # far from trivial: schedule rows that armed timers, queue answers, and with a bus its fan-outs and topic messages
    assert (b.op == abi.CC_OP_GROUP_SCHEDULE).sum() == ac.COORD["schedules"]
    assert len(oe["pos"]) > 5000 and (oe["src"] == abi.CC_EVSRC_TIMER).any()
    drain = s[-ac.COORD["queues"] * abi.CC_QUEUE_CAP:]
    assert (abi.status_tag(drain) != abi.CC_TAG_NULL).sum() > 10  # the queues held elements at the end
    if bus:
        assert len(bev) > 1000 and len(tev) > 1000
