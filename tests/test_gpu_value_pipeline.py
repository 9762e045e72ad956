"""GPU parity of the value-only apply where k_apply_value_v3's chunk pipeline is deep: a chunk is ranked and scanned
one workgroup barrier before it is placed, so its ranks and placement bases live across a barrier, the walkers' run
starts sit in three buffers, and one loader wave per chunk (in rotation) scans.  Lists of four and more chunks, more
than twelve chunks, workgroups of 0, 1, 2 and 5 chunks in one launch, a CAS chain across the chunk seams, escaped
records and results at the seams, and state carried over launches.

Bar: bit-exact per-commit status / value, value_state and applied index against the CPU oracle (integer path, no
tolerance); result columns prefilled with the 0xFF sentinel status (Engine.apply_host).  Geometry as in
test_gpu_value_apply.py: resource r is slot r & 255 of super-bucket r >> 8; a super-bucket's list is its rows in log
order, walked in 3072-record chunks."""
import numpy as np
import pytest

from copycat_amd import abi
from tests.test_gpu_value_apply import CHUNK, SLOTS, L, _batch, _escapes, _mixed_ops, _run_both

pytestmark = pytest.mark.gpu

SUB = 16384  # the smallest sub-batch (one launch of the three kernels each)


def _one_bucket(n, one_slot, seed):
    rng = np.random.default_rng(seed)
    inst = np.full(n, 37, np.uint32) if one_slot else rng.integers(0, SLOTS, n).astype(np.uint32)
    return _mixed_ops(rng, inst)


@pytest.mark.parametrize("one_slot", [False, True])
@pytest.mark.parametrize("n", [1] + [CHUNK * k + d for k in (4, 5) for d in (-1, 0, 1)])
def test_pipeline_depth(n, one_slot):
    """One super-bucket, one record and lists that end one short of, at and one past four and five chunks: the
    rank-ahead state is live across two and more barriers.  With one_slot every rank of a full chunk (0..3071) is
    used, on one counter half."""
    b = _one_bucket(n, one_slot, 2000 + n)
    assert np.all(b.inst >> 8 == 0) and (not one_slot or np.all(b.inst == 37))
    _run_both(b, SLOTS, SLOTS)


def test_scan_wave_rotation():
    """More than twelve chunks in one list: every loader wave scans once and the rotation wraps."""
    n = 13 * CHUNK + 5
    b = _one_bucket(n, False, 2100)
    assert (n + CHUNK - 1) // CHUNK > 12 and n < 50_000
    _run_both(b, SLOTS, SLOTS)


@pytest.mark.parametrize("resources,deep_at,others", [(512, 0, (0,)), (512, 1, (1,)), (512, 0, (CHUNK + 1,)),
                                                      (768, 0, (0, 1)), (768, 1, (1, CHUNK + 1)),
                                                      (768, 2, (CHUNK + 1, 0))])
def test_uneven_workgroups(resources, deep_at, others):
    """Two and three super-buckets in one launch: one holds 4 * 3072 + 1 records (five chunks), the others 0, 1 and
    3073 (no chunk, one, two), their rows interleaved at random."""
    nsb = resources // SLOTS
    counts = list(others)
    counts.insert(deep_at, 4 * CHUNK + 1)
    assert len(counts) == nsb
    rng = np.random.default_rng(2200 + resources + 7 * deep_at + sum(others))
    sb = rng.permutation(np.repeat(np.arange(nsb), counts))
    inst = (sb * SLOTS + rng.integers(0, SLOTS, len(sb))).astype(np.uint32)
    b = _mixed_ops(rng, inst)
    assert [int(np.sum(b.inst >> 8 == k)) for k in range(nsb)] == counts and len(b) < 50_000
    _run_both(b, resources, resources)


def test_cas_chain_across_chunk_boundaries():
    """Slot 5: a set, then CASes that each expect exactly what the one before wrote, in a list that crosses six chunk
    seams (the chain itself lies on both sides of each).  Slot 9, interleaved row by row: the same CASes against a
    value that never matches.  A chunk handed over wrongly, or walked out of order, fails a CAS of the chain."""
    k = 3 * CHUNK + 10  # CASes per slot; the list holds 2 k + 2 records
    inst = np.empty(2 * k + 2, np.uint32)
    inst[0::2], inst[1::2] = 5, 9
    op = np.full(2 * k + 2, abi.CC_OP_VALUE_CAS, np.uint8)
    op[:2] = abi.CC_OP_VALUE_SET
    a = np.repeat(np.arange(100, 100 + k + 1, dtype=np.uint64), 2)  # row pair j: expected 100 + j ...
    bb = a + 1                                                      # ... update 101 + j
    a[:2], bb[:2] = (101, 7), 0                                     # the sets: slot 5 holds 101, slot 9 holds 7
    b = _batch(inst, op, np.full(2 * k + 2, L | (L << 3), np.uint8), a, bb)
    assert len(b) > 6 * CHUNK and len(b) < 50_000
    gs, gv = _run_both(b, SLOTS, SLOTS)
    assert np.all(gv[2::2] == 1), np.nonzero(gv[2::2] != 1)[0][:5]  # every CAS of the chain succeeded
    assert np.all(gv[3::2] == 0)                                    # none of the stale ones did


def _seams(n):
    """First and last position of every chunk and of the list."""
    edges = {0, n - 1}
    for c in range(CHUNK, n, CHUNK):
        edges |= {c - 1, c}
    return sorted(edges)


@pytest.mark.parametrize("kind", ["getandset", "cas_get"])
def test_escapes_at_the_seams(kind):
    """Slot 250 holds a value past 56 bits (set by a call of its own).  At the first and last position of every chunk
    and of the list: getAndSet of another such value (an escaped record whose result escapes too), or in turn a CAS
    from the held value (expected past 32 bits: escaped record) and a get (plain record, escaped result).  Every other
    row is a small plain record on slots 0..199."""
    n = 4 * CHUNK + 7
    big = lambda p: (1 << 60) + 12345 * p
    rng = np.random.default_rng(2300)
    body = _mixed_ops(rng, rng.integers(0, 200, n).astype(np.uint32))
    inst, op, flags = body.inst.copy(), body.op.copy(), body.flags.copy()
    a, bcol = [int(x) for x in body.a], [int(x) for x in body.b]
    cur = big(0)
    for q, p in enumerate(_seams(n)):
        inst[p], flags[p] = 250, L | (L << 3)
        if kind == "getandset":
            op[p], a[p], bcol[p] = abi.CC_OP_VALUE_GETANDSET, big(p + 1), 0
            cur = big(p + 1)
        elif q % 2 == 0:
            op[p], a[p], bcol[p] = abi.CC_OP_VALUE_CAS, cur, cur + (1 << 20)  # update - expected past 14 bits too
            cur += 1 << 20
        else:
            op[p], a[p], bcol[p] = abi.CC_OP_VALUE_GET, 0, 0
    # row 0 (a call of its own): slot 250 <- big(0)
    b = _batch(np.concatenate([[250], inst]), np.concatenate([[abi.CC_OP_VALUE_SET], op]),
               np.concatenate([[L], flags]), [big(0)] + a, [0] + bcol)
    seams = np.array(_seams(n)) + 1  # batch rows
    esc = np.array([_escapes(int(b.op[i]), int(b.flags[i]), int(b.a[i]), int(b.b[i])) for i in range(len(b))])
    plain_get = (b.op[seams] == abi.CC_OP_VALUE_GET)
    assert np.all(esc[seams] | plain_get) and esc[seams].any() and not esc[np.setdiff1d(np.arange(1, n + 1), seams)].any()
    assert len(seams) == 10 and len(b) < 50_000
    gs, gv = _run_both(b, SLOTS, SLOTS, split=[(0, 1), (1, n + 1)])
    ret = np.isin(b.op[seams], (abi.CC_OP_VALUE_GET, abi.CC_OP_VALUE_GETANDSET))
    assert ret.any() and np.all(gv[seams][ret] >= np.uint64(1 << 60))  # results past the packed word's 56 bits
    if kind == "cas_get":
        assert np.all(gv[seams][~ret] == 1)  # every escaped CAS met the value it expected


@pytest.mark.parametrize("one_slot", [False, True])
@pytest.mark.parametrize("launches", [2, 3])
def test_state_across_launches(launches, one_slot):
    """Two and three sub-batches of one call: in each, super-bucket 0 holds 4 * 3072 + 1 records (the rest of a full
    sub-batch goes to super-bucket 1).  The walkers' registers and the loaders' rank-ahead state start fresh with every
    launch; the slots' values carry over."""
    deep = 4 * CHUNK + 1
    rng = np.random.default_rng(2400 + launches)
    sbs = []
    for k in range(launches):
        rows = SUB if k + 1 < launches else deep
        sbs.append(rng.permutation(np.repeat([0, 1], [deep, rows - deep])))
    sb = np.concatenate(sbs)
    slot = np.full(len(sb), 37) if one_slot else rng.integers(0, SLOTS, len(sb))
    b = _mixed_ops(rng, (sb * SLOTS + slot).astype(np.uint32))
    for k in range(launches):
        assert int(np.sum(b.inst[k * SUB:(k + 1) * SUB] >> 8 == 0)) == deep
    assert len(b) == (launches - 1) * SUB + deep < 50_000
    _run_both(b, 2 * SLOTS, 2 * SLOTS, sub_batch=SUB)
