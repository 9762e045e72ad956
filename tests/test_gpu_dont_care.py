"""GPU: "Columns an op does not use may hold anything" (include/copycat_apply.h, cc_batch; the table is
tests/abi_cases.USED).

The engine applies scribble(b): every cell outside USED holds a random u64, every unused tag field random bits (the
result-only tags 5..7 and an unregistered HANDLE key tag among them).  The expected results, events and final state are
the references' on the clean b, which tests/test_abi_dont_care.py shows to be the references' on scribble(b) too.  The
partitions read every column of every row (k_part_v4 decides per row whether a record fits 8 bytes, k_part_ext and
k_hot_sample hash the key and its tag, value_encode canonicalises by tag), so a kernel that lets an unused cell reach a
record, a hash or an error bit fails here.

Three engine configurations, each a different kernel route, each through three entry points: device columns
(cc_apply_batch), host columns (cc_apply_batch_host / _host_events) and a packed blob of all nine columns
(cc_apply_batch_host_packed).  Bit-exact, by the helpers of the parity tests."""
import ctypes as C
import functools

import numpy as np
import pytest

from copycat_amd import abi
from copycat_amd.batch import pack
from tests import abi_cases as ac

pytestmark = pytest.mark.gpu

ENTRIES = ("device", "host", "packed")
EV_KEYS = ("pos", "target", "code", "src", "tag", "payload")
EV_CAP = 1 << 20


# ---- the three entry points ------------------------------------------------------------------------------------------
def _apply(E, b, entry):
    """(status, value) of b through one entry point, no event stream"""
    import torch

    from copycat_amd.engine import RESULT_SENTINEL, DeviceBatch

    n = len(b)
    if entry == "device":
        st = torch.full((n,), RESULT_SENTINEL, dtype=torch.uint8, device="cuda")
        va = torch.full((n,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda")
        E.apply(DeviceBatch.upload(b), st, va)
        E.sync()
        s, v = st.cpu().numpy(), va.cpu().numpy().view(np.uint64)
    elif entry == "host":
        s, v = E.apply_host(b)
    else:
        s, v, _, done = E.apply_host_packed(pack(b), n, events=False, chunk_rows=ac.SUB_BATCH)
        assert done == n
    assert not np.any(s == RESULT_SENTINEL), "rows left unwritten"
    return s, v


def _apply_events(E, b, entry):
    """(status, value, events) of b through one entry point with an event stream"""
    n = len(b)
    if entry == "device":
        return E.apply_host_events(b, capacity=EV_CAP)  # (device columns in, a device event stream out)
    if entry == "packed":
        s, v, ev, done = E.apply_host_packed(pack(b), n, capacity=EV_CAP, chunk_rows=ac.SUB_BATCH)
        assert done == n and ev["count"] == len(ev["pos"])
        return s, v, {k: ev[k] for k in EV_KEYS}
    st, va = np.full(n, 0xFF, np.uint8), np.zeros(n, np.uint64)
    cb = abi.cc_batch()
    for name, _ in abi.BATCH_COLUMNS:
        setattr(cb, name, getattr(b, name).ctypes.data)
    cols = {"pos": np.zeros(EV_CAP, np.uint32), "target": np.zeros(EV_CAP, np.uint32), "code": np.zeros(EV_CAP, np.uint8),
            "src": np.zeros(EV_CAP, np.uint8), "tag": np.zeros(EV_CAP, np.uint8), "payload": np.zeros(EV_CAP, np.uint64)}
    count = np.zeros(1, np.uint64)
    ev = abi.cc_events(*(cols[k].ctypes.data for k in EV_KEYS), EV_CAP, count.ctypes.data)
    r = abi.cc_results(st.ctypes.data, va.ctypes.data)
    rc = E.L.cc_apply_batch_host_events(E.h, C.byref(cb), n, C.byref(r), C.byref(ev))
    assert rc == abi.CC_OK, (rc, E.L.cc_last_error())
    assert int(count[0]) <= EV_CAP
    return st, va, {k: x[:int(count[0])] for k, x in cols.items()}


# ---- 1. the value-only engine ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _value_case():
    """the stream, its scribbled copy and the oracle after the clean stream (computed once, never changed)"""
    from oracle.oracle_py import Oracle

    R = ac.VALUE["resources"]
    b = ac.value_stream()
    O = Oracle(R, R + 8)
    for r in range(R):
        O.resource_create(r, abi.CC_RES_VALUE)
        O.instance_open(r, r, 1000 + r, 7)
    os_, ov = O.apply(b)
    return b, ac.scribble(b, 1), O, os_, ov


@pytest.mark.parametrize("retained", [False, True], ids=["plain", "retained"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_value_only_engine(entry, retained):
    """k_part_v4 -> k_apply_value_v3 -> k_unpermute_v3 over three segments of one group with a ragged last tile: the
    unused a / b of a Get or a Delete, a key, an aux and tags 5..7 never reach a record.  With CC_CFG_VALUE_RETAINED
    the retained commit of every slot too."""
    from copycat_amd.engine import Engine
    from tests.test_gpu_value import _assert_same

    R = ac.VALUE["resources"]
    b, sb, O, os_, ov = _value_case()
    assert len(b) == 2 * ac.SUB_BATCH + 8192 + 37 and ac.changed_share(b, sb) > 0.5
    flags = abi.CC_CFG_TIMERS_DEFERRED | (abi.CC_CFG_VALUE_RETAINED if retained else 0)
    E = Engine(R, R + 8, len(b), sub_batch=ac.SUB_BATCH, flags=flags)
    E.resource_create_range(0, R, abi.CC_RES_VALUE)
    E.instance_open_range(0, R, 0, 1000, 7)
    gs, gv = _apply(E, sb, entry)
    _assert_same(E, O, gs, gv, os_, ov, R)
    if retained:
        assert np.array_equal(E.value_retained(), O.value_retained())


# ---- 2. values, maps, sets and multimaps in one table ----------------------------------------------------------------
TABLE_MODES = {"plain": (False, abi.CC_CFG_TIMERS_DEFERRED), "ttl-manager": (True, abi.CC_CFG_TIMERS_DEFERRED),
               "ttl-module": (True, 0)}


@functools.lru_cache(maxsize=None)
def _table_case(mode):
    from tests.test_abi_dont_care import table_oracle

    ttl, flags = TABLE_MODES[mode]
    b = ac.table_stream(ttl)
    O = table_oracle(flags)
    os_, ov = O.apply(b)
    return b, ac.scribble(b, 2), O, os_, ov


@pytest.mark.parametrize("mode", list(TABLE_MODES))
@pytest.mark.parametrize("entry", ENTRIES)
def test_table_engine(entry, mode):
    """k_part_ext -> k_apply_map (+ the hot-key scan, map_cv, the barrier rows of map_wide) next to k_apply_value_v3:
    60,000 rows over values, 64-key and 1,024-key maps, sets and multimaps, with in-stream containsValue, clear, size
    and Delete rows; TTL mode in both timer orders.  A HANDLE key tag scribbled into a row that reads no key is never
    registered and must not raise CC_ERR_STATE; the key and aux of a value row and of a whole-map row never reach the
    table."""
    from copycat_amd.engine import Engine
    from tests.handles import register_key_strings
    from tests.test_gpu_map import _assert_maps, _assert_rows

    ttl, flags = TABLE_MODES[mode]
    b, sb, O, os_, ov = _table_case(mode)
    types = ac.table_types()
    R = len(types)
    E = Engine(R, R + 8, len(b), map_capacity=ac.TABLE["map_capacity"], sub_batch=ac.SUB_BATCH, flags=flags)
    for r, t in enumerate(types):
        E.resource_create(r, int(t))
        E.instance_open(r, r, 1000 + r, 7)
    register_key_strings(E)
    gs, gv = _apply(E, sb, entry)
    _assert_rows(gs, gv, os_, ov)
    keyed = [r for r, t in enumerate(types) if t != abi.CC_RES_VALUE]
    _assert_maps(E, O, keyed)
    for r in keyed:
        if types[r] == abi.CC_RES_MULTIMAP:
            assert E.retained(r) == O.retained(r), r
    nv = ac.TABLE["values"]
    for x, y in zip(E.value_state(0, nv), O.value_state(0, nv)):
        assert np.array_equal(x, y)
    c = E.counters()
    assert c[0] > 0 and c[2] >= 4  # barrier rows and at least four sub-batches


# ---- 3. coordination -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bus", [False, True], ids=["no-bus", "bus-and-topic"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_coordination_engine(entry, bus):
    """k_part_ext -> k_apply_coord<false> (no bus in the engine) and k_apply_coord<true> (+ k_topic_fanout) at
    coord_cap 256: locks, elections, groups, values with listeners, queues, GROUP_SCHEDULE barrier rows; with a bus a
    Topic and a MessageBus and their traffic.  Every status, value and event and the final state of every resource."""
    w = ac.coord_world(bus)
    b = ac.coord_stream(w, bus)
    sb = ac.scribble(b, 3)
    assert ac.changed_share(b, sb) > 0.5
    want = w.expect(b)
    w.row_inst = b.inst
    got = _apply_events(w.E, sb, entry)
    w.check(got, want)
    w.check_state()
