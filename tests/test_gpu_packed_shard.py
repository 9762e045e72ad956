"""GPU: the sharded loop with only narrow bytes between the coordinator and the ranks.

A coordinator holds the log in HBM and splits it there; every share leaves the GPU as a batch blob
(cc_pack_from_device), the rank applies the blob and answers with a result blob and an event blob
(cc_apply_batch_host_packed_events), the coordinator decodes both straight into device columns (cc_respack_to_device,
cc_evpack_to_device), merges them on the device and sends the merged answer out packed again:

  split_batch_device(rows) -> per rank batch_to_host_packed -> per rank apply_host_packed_events
    -> results_to_device, events_to_device -> merge_by_owner_device, merge_events_device
    -> results_to_host_packed, events_to_host_packed

The final blobs, decoded, equal what one engine applying the whole log returns, every result row and every event
column, and the oracle's per commit (the checks of tests/test_gpu_shard.py and tests/test_gpu_evmerge.py).  The world's
engines and the coordinator's share this box's one GPU, as in those tests."""
import functools

import numpy as np
import pytest

from copycat_amd import abi, shard
from copycat_amd.batch import events_check, pack, results_check, unpack_events, unpack_results

pytestmark = pytest.mark.gpu

B = abi.CC_PACK_BLOCK_ROWS
KEYS = ("pos", "src", "target", "code", "tag", "payload")


def _chain(b, own, world, make_engine, ev_capacity):
    """-> (status, value, events) decoded from the coordinator's final blobs, and the per-rank share sizes"""
    import torch

    from copycat_amd.engine import DeviceBatch, DeviceEvents, Engine

    coord = Engine(16, 16, 4096)  # the coordinator: staging and error store of the pack / unpack calls, no resources
    db = DeviceBatch.upload(b)
    parts = shard.split_batch_device(db, own, world, rows=True)                       # 1
    host_parts = shard.split_batch(b, own, world, rows=False)
    res, evs, sizes, wire = [], [], [], 0
    for r, (rows, part) in enumerate(parts):
        blob = coord.batch_to_host_packed(part)                                       # 2
        if part.n:  # the share's blob is the one the host encoder writes for the host split's share
            assert np.array_equal(blob, pack(host_parts[r][1])), f"rank {r}: the share's blob"
        E = make_engine(r)
        rblob, eblob, ev_count, done = E.apply_host_packed_events(blob, part.n, capacity=ev_capacity)   # 3
        assert done == part.n and results_check(rblob) == part.n and events_check(eblob) == ev_count
        E.close()
        st = torch.full((part.n,), 0xFF, dtype=torch.uint8, device="cuda")
        va = torch.zeros(part.n, dtype=torch.uint64, device="cuda")
        ev = DeviceEvents(max(ev_count, 1))
        ev.capacity = ev_count
        ev.count[0] = 0x7777
        coord.results_to_device(rblob, st, va)                                        # 4
        torch.cuda.synchronize()  # (the two decoders share one staging: the engine is synchronised between them)
        coord.events_to_device(eblob, ev)
        torch.cuda.synchronize()
        assert int(ev.count.item()) == ev_count
        res.append((st, va)), evs.append(ev), sizes.append(part.n)
        wire += len(blob) + len(rblob) + len(eblob)
    st, va = shard.merge_by_owner_device(db.cols["inst"], own, world, res)            # 5
    merged = shard.merge_events_device(evs, [rows for rows, _ in parts], len(b))
    final_res = coord.results_to_host_packed(st, va)                                  # 6
    final_ev, count = coord.events_to_host_packed(merged)
    coord.close()
    s, v = unpack_results(final_res)
    ev = unpack_events(final_ev)
    ev["count"] = count
    wide = sum(len(b) * np.dtype(dt).itemsize for _, dt in abi.BATCH_COLUMNS) + 9 * len(b) + 19 * count
    print(f"world {world}: {wire} B packed between coordinator and ranks, {wide} B wide")
    return s, v, ev, sizes


# ---- a coordination log with events ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 4])
def test_coordination_log_through_the_packed_loop(world):
    """Fails without the feature: Engine.batch_to_host_packed does not exist."""
    from copycat_amd.engine import Engine
    from tests.test_gpu_coord import FLAGS, _canon
    from tests.test_gpu_evmerge import COORD_CAP, K_COORD, R_COORD, _coord_reference

    types, max_inst, b, s1, v1, ev1, (oe, apos, amem) = _coord_reference()  # 60,000 rows; one engine's answers = the oracle's
    own = shard.inst_owner_table(np.arange(R_COORD * K_COORD) // K_COORD, world)

    def make_engine(rank):
        E = Engine(R_COORD, max_inst, 1 << 20, flags=FLAGS, max_events=1 << 22, coord_cap=COORD_CAP)
        for r in range(R_COORD):
            if r % world == rank:
                E.resource_create(r, int(types[r]))
                for k in range(K_COORD):
                    E.instance_open(r * K_COORD + k, r, 1000 + r * K_COORD + k, 7 + k)
        return E

    s, v, ev, sizes = _chain(b, own, world, make_engine, len(ev1["pos"]) + 64)
    assert sum(sizes) == len(b) == 60_000 and all(sizes)
    assert np.array_equal(s, s1) and np.array_equal(v, v1)  # every result row
    assert ev["count"] == ev1["count"] == len(ev1["pos"]) and ev["count"] > 1000
    for k in KEYS:  # one engine's stream, column for column in stream order
        assert np.array_equal(ev[k], ev1[k]), k
    # ... and the oracle's, by the canonical per-commit comparison (member rows against the oracle's aux stream)
    member = ev["code"] == abi.CC_EV_MEMBER
    assert _canon(*(ev[k][~member] for k in KEYS)) == _canon(*(oe[k] for k in KEYS))
    assert list(zip(ev["pos"][member].tolist(), ev["payload"][member].tolist())) == list(zip(apos.tolist(), amem.tolist()))


# ---- a value log -----------------------------------------------------------------------------------------------------------
SLOTS, MAX_INST = 4096, 4096 + 8
N_VALUE = 50_001


def _value_engine(owned):
    from copycat_amd.engine import Engine

    E = Engine(SLOTS, MAX_INST, 1 << 20, flags=abi.CC_CFG_TIMERS_DEFERRED)
    if owned.all():
        E.resource_create_range(0, SLOTS, abi.CC_RES_VALUE)
        E.instance_open_range(0, SLOTS, 0, 1000, 7)
        return E
    for g in np.nonzero(owned)[0].tolist():  # a rank hosts the slots it owns (the others stay unused)
        E.resource_create(g, abi.CC_RES_VALUE)
        E.instance_open(g, g, 1000 + g, 7)
    return E


@functools.lru_cache(maxsize=None)
def _value_reference():
    """the log, and one engine's answers for it, checked against the oracle's (computed once for every world)"""
    from copycat_amd.workload import value_random_stream
    from oracle.oracle_py import Oracle

    b = value_random_stream(N_VALUE, SLOTS, MAX_INST, seed=5, hot=8, p_hot=0.2)
    assert np.any(b.inst >= SLOTS)  # unknown sessions among the rows: they go to rank 0
    E = _value_engine(np.ones(SLOTS, bool))
    s, v = E.apply_host(b)
    E.close()
    O = Oracle(SLOTS, MAX_INST, abi.CC_CFG_TIMERS_DEFERRED)
    for g in range(SLOTS):
        O.resource_create(g, abi.CC_RES_VALUE)
        O.instance_open(g, g, 1000 + g, 7)
    s2, v2 = O.apply(b)
    assert np.array_equal(s, s2) and np.array_equal(v, v2)
    return b, s, v


def _value_chain(world, owner_of_slot):
    b, s1, v1 = _value_reference()
    own = np.asarray(owner_of_slot, np.int32)
    s, v, ev, sizes = _chain(b, own, world, lambda rank: _value_engine(own == rank), 1024)
    assert np.array_equal(s, s1) and np.array_equal(v, v1)
    assert ev["count"] == 0 and all(len(ev[k]) == 0 for k in KEYS)  # no listeners: header-only event blobs all the way
    return sizes


@pytest.mark.parametrize("world", [2, 4])
def test_value_log_through_the_packed_loop(world):
    sizes = _value_chain(world, shard.inst_owner_table(np.arange(SLOTS), world))
    assert sum(sizes) == N_VALUE
    for m in sizes:  # every share is more than one block and one split tile, and ends inside one
        assert m > B and m % B and m > abi.CC_SPLIT_TILE_ROWS and m % abi.CC_SPLIT_TILE_ROWS


def test_value_log_with_an_empty_share():
    """world 3, rank 1 owns nothing: its share is a header-only blob in and two header-only blobs out"""
    sizes = _value_chain(3, np.where(np.arange(SLOTS) % 2 == 0, 0, 2))
    assert sizes[1] == 0 and sizes[0] > B and sizes[2] > B
