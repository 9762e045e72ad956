"""GPU parity: a batch that lists more in-stream rows than a list's first allocation holds (2^20 rows).

The listing pass of cc_apply_batch counts the batch's map size / isEmpty rows, its in-stream clear rows and its
containsValue candidates into lists of 2^20 rows; a batch with more of one kind regrows that list and scans again.
Each case applies a first batch of 1.2 M rows with more than 2^20 rows of one kind, puts between them, then a smaller
second batch on the same engine (which reuses the grown list).

Bar: bit-exact per-commit status/value against the CPU oracle, sampled maps' final entries, and no barrier row."""
import numpy as np
import pytest

from copycat_amd import abi
from copycat_amd.batch import Batch

pytestmark = pytest.mark.gpu

N1, LISTED1 = 1_200_000, 1_100_000  # LISTED1 > 2^20
N2, LISTED2 = 60_000, 50_000


def _batch(kind, n, listed, maps, index0, seed):
    rng = np.random.default_rng(seed)
    op = np.full(n, abi.CC_OP_MAP_PUT, np.uint8)
    inst = rng.integers(0, maps, n).astype(np.uint32)
    key = rng.integers(0, 48, n).astype(np.uint64)
    a = rng.integers(1, 4, n).astype(np.uint64)  # stored values 1..3, never null
    rows = np.sort(rng.choice(n, size=listed, replace=False))
    if kind == "size":
        op[rows] = np.where(np.arange(listed) % 2 == 0, abi.CC_OP_MAP_SIZE, abi.CC_OP_MAP_ISEMPTY).astype(np.uint8)
    elif kind == "clear":  # spread evenly: fewer than 128 clears of any map, so no sub-batch is cut for one
        op[rows] = abi.CC_OP_MAP_CLEAR
        inst[rows] = (np.arange(listed) % maps).astype(np.uint32)
        assert -(-listed // maps) < 128
    else:  # containsValue: operands 0..4 against stored values 1..3
        op[rows] = abi.CC_OP_MAP_CONTAINSVALUE
        a[rows] = rng.integers(0, 5, listed).astype(np.uint64)
    b = Batch.from_columns(index=np.arange(index0, index0 + n, dtype=np.uint64), inst=inst, op=op,
                           flags=np.full(n, abi.cc_flags(abi.CC_TAG_LONG, 0, 0), np.uint8), key=key, a=a)
    return b, rows


@pytest.mark.parametrize("kind,maps", [("size", 256), ("clear", 16384), ("cv", 256)])
def test_stream_list_regrown_past_first_allocation(kind, maps):
    from copycat_amd.engine import Engine
    from oracle.oracle_py import Oracle

    assert LISTED1 > 1 << 20
    E = Engine(maps, maps, N1, map_capacity=1 << 18, flags=abi.CC_CFG_TIMERS_DEFERRED)
    O = Oracle(maps, maps, abi.CC_CFG_TIMERS_DEFERRED)
    E.resource_create_range(0, maps, abi.CC_RES_MAP)
    E.instance_open_range(0, maps, 0, 1000, 7)
    for m in range(maps):
        O.resource_create(m, abi.CC_RES_MAP)
        O.instance_open(m, m, 1000 + m, 7)
    c0 = E.counters()
    for n, listed, index0, seed in ((N1, LISTED1, 1, 11), (N2, LISTED2, N1 + 1, 12)):
        b, rows = _batch(kind, n, listed, maps, index0, seed)
        gs, gv = E.apply_host(b)
        os_, ov = O.apply(b)
        bad = np.nonzero((gs != os_) | (gv != ov))[0]
        assert len(bad) == 0, (f"{len(bad)} of {n} rows differ; first {bad[:5]}: gpu {gs[bad[:5]]},{gv[bad[:5]]} "
                               f"oracle {os_[bad[:5]]},{ov[bad[:5]]}")
        if kind != "clear":
            assert len(np.unique(gv[rows])) > 1  # the puts between them: the answers differ
    for m in range(0, maps, max(1, maps // 64)):
        for x, y, what in zip(E.map_entries(m), O.map_entries(m), ("key tag", "key", "value tag", "value", "index")):
            assert np.array_equal(x, y), f"map {m}: {what} differs"
    assert E.applied_index() == O.applied_index() == N1 + N2
    c1 = E.counters()
    assert c1[0] == c0[0] == 0  # no barrier row: every listed row was answered in the stream
    if kind == "cv":
        assert c1[1] - c0[1] == LISTED1 + LISTED2
