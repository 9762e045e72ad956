"""GPU parity of the value-only apply (k_part_v4 -> k_apply_value_v3 -> k_unpermute_v3, map_capacity = 0) at the
shapes where k_apply_value_v3 changes path: chunk and wave edges, run windows (dense, sparse, with empty runs), grid
sizes of the XCD-affine super-bucket order, every record class mixed with escaped operands and results, and state
carried across sub-batches and calls.

Bar: bit-exact per-commit status / value, value_state and applied index against the CPU oracle (integer path, no
tolerance).  Geometry the inputs are built for (value_path.hip): resource r is slot r & 255 of super-bucket r >> 8;
row i is in partition tile i // 8192; a super-bucket's list is its rows in log order, walked in 3072-record chunks
that twelve loader waves load in 256-record spans of four 64-record groups."""
import numpy as np
import pytest

from copycat_amd import abi
from copycat_amd.batch import Batch

pytestmark = pytest.mark.gpu

TILE, CHUNK, SPAN, GROUP, SLOTS = 8192, 3072, 256, 64, 256
L, I, N = abi.CC_TAG_LONG, abi.CC_TAG_INT, abi.CC_TAG_NULL
M64 = 1 << 64


def _batch(inst, op, flags, a, b):
    n = len(op)
    u64 = lambda x: np.array([int(v) % M64 for v in x], np.uint64) if not isinstance(x, np.ndarray) else x.astype(np.uint64)
    return Batch.from_columns(index=np.arange(1, n + 1, dtype=np.uint64), time=np.arange(1, n + 1, dtype=np.uint64),
                              inst=np.asarray(inst, np.uint32), op=np.asarray(op, np.uint8),
                              flags=np.asarray(flags, np.uint8), a=u64(a), b=u64(b))


def _run_both(b, resources, max_inst, sub_batch=0, split=None):
    from copycat_amd.engine import Engine
    from oracle.oracle_py import Oracle

    E = Engine(resources, max_inst, max(len(b), 1), sub_batch=sub_batch, map_capacity=0)
    O = Oracle(resources, max_inst)
    E.resource_create_range(0, resources, abi.CC_RES_VALUE)
    E.instance_open_range(0, resources, 0, 1000, 7)
    for r in range(resources):
        O.resource_create(r, abi.CC_RES_VALUE)
        O.instance_open(r, r, 1000 + r, 7)
    gs, gv, os_, ov = [], [], [], []
    for lo, hi in (split or [(0, len(b))]):
        part = b.slice(lo, hi)
        s, v = E.apply_host(part)
        s2, v2 = O.apply(part)
        gs.append(s); gv.append(v); os_.append(s2); ov.append(v2)
    gs, gv, os_, ov = (np.concatenate(x) for x in (gs, gv, os_, ov))
    bad = np.nonzero((gs != os_) | (gv != ov))[0]
    assert len(bad) == 0, (f"{len(bad)} rows differ; first {bad[:5]}: gpu {gs[bad[:5]]},{gv[bad[:5]]} "
                           f"oracle {os_[bad[:5]]},{ov[bad[:5]]}")
    for x, y in zip(E.value_state(0, resources), O.value_state(0, resources)):
        assert np.array_equal(x, y)
    assert E.applied_index() == O.applied_index()
    return gs, gv


def _mixed_ops(rng, inst):
    """get / set / CAS / getAndSet (and a few deletes) with values 0..3, so CASes both succeed and fail."""
    n = len(inst)
    k = rng.integers(0, 100, n)
    op = np.select([k < 30, k < 50, k < 80, k < 98], [abi.CC_OP_VALUE_GET, abi.CC_OP_VALUE_SET, abi.CC_OP_VALUE_CAS,
                                                      abi.CC_OP_VALUE_GETANDSET], abi.CC_OP_DELETE).astype(np.uint8)
    flags = np.full(n, L | (L << 3), np.uint8)
    return _batch(inst, op, flags, rng.integers(0, 4, n).astype(np.uint64), rng.integers(0, 4, n).astype(np.uint64))


@pytest.mark.parametrize("one_slot", [False, True])
@pytest.mark.parametrize("n", [255, 256, 257, 3071, 3072, 3073, 6144, 6145, 9217])
def test_chunk_and_wave_edges(n, one_slot):
    """One super-bucket takes every row: lists that end one short of, at and one past a 256-record span and a
    3072-record chunk, and at two and three chunks.  With one_slot, one walker lane walks every record of a chunk."""
    rng = np.random.default_rng(1000 + n)
    inst = np.full(n, 37, np.uint32) if one_slot else rng.integers(0, SLOTS, n).astype(np.uint32)
    b = _mixed_ops(rng, inst)
    assert np.all(b.inst >> 8 == 0)
    if one_slot:
        assert np.all(b.inst == 37)
    _run_both(b, SLOTS, SLOTS)


def _spans_of(rows):
    """(tiles spanned first..last, distinct tiles, tiles of that range without a record) of every aligned 256-record
    span of a super-bucket's list (rows = its batch rows in log order)."""
    out = []
    for c in range(0, len(rows), SPAN):
        tl = rows[c:c + SPAN] // TILE
        out.append((int(tl[-1] - tl[0] + 1), len(np.unique(tl)), int(tl[-1] - tl[0] + 1 - len(np.unique(tl)))))
    return out


def test_sparse_runs_and_empty_runs():
    """One hot slot takes >= 99.8 % of ~4M rows; cold super-bucket 5 has ~3 records per tile (its 256-record spans
    cover more than 64 runs, some tiles none: the per-wave search), cold super-bucket 9 has ~6 per tile but none in
    every 20th tile (spans of at most 64 runs with an empty run among them: the run window gives way to the search),
    cold super-bucket 12 has ~5 in every tile (the run window with short runs)."""
    R, n = 4096, 512 * TILE
    rng = np.random.default_rng(77)
    inst = np.full(n, 3, np.uint32)  # the hot slot: super-bucket 0, slot 3
    tile = np.arange(n) // TILE
    u = rng.random(n)
    c5 = u < 3.0 / TILE
    c9 = (u >= 0.25) & (u < 0.25 + 6.0 / TILE) & (tile % 20 != 7)
    c12 = (u >= 0.5) & (u < 0.5 + 4.0 / TILE)
    inst[c5] = 5 * SLOTS + rng.integers(0, SLOTS, int(c5.sum()))
    inst[c9] = 9 * SLOTS + rng.integers(0, SLOTS, int(c9.sum()))
    inst[c12] = 12 * SLOTS + rng.integers(0, SLOTS, int(c12.sum()))
    for k in range(512):  # super-bucket 12 has a record in every tile
        inst[k * TILE + 11] = 12 * SLOTS + k % SLOTS
    b = _mixed_ops(rng, inst)
    assert np.mean(b.inst == 3) >= 0.998
    sb = b.inst >> 8
    s5, s9, s12 = (_spans_of(np.nonzero(sb == k)[0]) for k in (5, 9, 12))
    assert int(np.sum(sb == 5)) >= 257
    assert any(distinct > 64 for _, distinct, _ in s5)
    assert len(np.unique(tile[sb == 5])) < 512 and any(empty > 0 for _, _, empty in s5)
    assert any(span <= 64 and empty > 0 for span, _, empty in s9)
    assert all(empty == 0 for _, _, empty in s12) and len(s12) > 4
    _run_both(b, R, R)


@pytest.mark.parametrize("resources,n", [(256, 20_000), (1000, 60_000), (1792, 100_000), (2304, 120_000),
                                         (131072, 400_000)])
def test_grid_sizes_of_the_super_bucket_order(resources, n):
    """1, 4 (the last one ragged), 7, 9 and 512 super-buckets: grids below, at one short of, one past and far past
    the eight XCDs the workgroup -> super-bucket order deals over."""
    from copycat_amd.workload import value_random_stream

    assert (resources + SLOTS - 1) // SLOTS in (1, 4, 7, 9, 512)
    max_inst = resources + 8
    b = value_random_stream(n, resources, max_inst, seed=resources, hot=2, p_hot=0.05)
    _run_both(b, resources, max_inst)


def _escapes(op, flags, a, b):
    """The record's escape rule (value_path.hip v3_encode): a set / getAndSet value past 46 bits, a CAS whose expected
    value is past 32 bits or whose update - expected is past 14 bits (NULL operands count as 0)."""
    fits = lambda x, bits: -(1 << (bits - 1)) <= ((x + (1 << 63)) % M64) - (1 << 63) < (1 << (bits - 1))
    ta, tb = flags & 7, (flags >> 3) & 7
    pa, pb = (a if ta else 0), (b if tb else 0)
    if op in (abi.CC_OP_VALUE_SET, abi.CC_OP_VALUE_GETANDSET):
        return not fits(pa, 46)
    if op == abi.CC_OP_VALUE_CAS:
        return not (fits(pa, 32) and fits((pb - pa) % M64, 14))
    return False


def test_every_class_and_tag_mixed_with_escapes():
    """get, set, CAS, getAndSet, delete and an unknown op; null tags on either operand; instances past max_instances
    and never opened; operands on both sides of 2^31 (expected), 2^13 (update - expected) and 2^45 (set values);
    results on both sides of 2^55.  Eight slots of one super-bucket take the templates in turn, so escaped and plain
    records alternate inside every 64-record group, across the 3072-record chunk edge too."""
    R, max_inst = SLOTS, SLOTS + 4
    vals = [0, 1, -1, (1 << 31) - 1, 1 << 31, -(1 << 31), -(1 << 31) - 1, (1 << 45) - 1, 1 << 45, -(1 << 45),
            -(1 << 45) - 1, (1 << 55) - 1, 1 << 55, -(1 << 55), -(1 << 55) - 1, (1 << 63) - 1, -(1 << 63)]
    dels = [0, 1, -1, 8191, 8192, -8192, -8193, 1 << 20]
    rng = np.random.default_rng(5)
    cur, ctag = [0] * 8, [N] * 8
    rows = []
    for k in range(560):
        for s in range(8):
            slot = 29 * s + 3
            v, d = vals[(k + 2 * s) % len(vals)], dels[(k + s) % len(dels)]
            kind = (k * 5 + s * 3) % 16
            if kind in (0, 1):
                rows.append((slot, abi.CC_OP_VALUE_GET, 0, 0, 0))
            elif kind in (2, 3):  # set (Long; an Integer or null now and then)
                t = L if kind == 2 else (I if k % 2 else N)
                v2 = v & 0x7FFFFFFF if t == I else v
                rows.append((slot, abi.CC_OP_VALUE_SET, t, v2, 0))
                cur[s], ctag[s] = (v2 if t != N else 0), t
            elif kind in (4, 5, 6, 7):  # a CAS from the value the slot holds: succeeds
                nt = L if kind != 7 else N
                upd = (cur[s] + d) if nt != N else 0
                rows.append((slot, abi.CC_OP_VALUE_CAS, ctag[s] | (nt << 3), cur[s], upd))
                cur[s], ctag[s] = upd, nt
            elif kind in (8, 9):  # a CAS from another value: fails (both sides of every boundary)
                rows.append((slot, abi.CC_OP_VALUE_CAS, L | (L << 3), v + 7, v + 7 + d))
            elif kind in (10, 11):
                rows.append((slot, abi.CC_OP_VALUE_GETANDSET, L, v, 0))
                cur[s], ctag[s] = v, L
            elif kind == 12:
                rows.append((slot, abi.CC_OP_DELETE, 0, 0, 0))
                cur[s], ctag[s] = 0, N
            elif kind == 13:
                rows.append((slot, 99, L, v, 0))  # no AtomicValue operation
            elif kind == 14:
                rows.append((max_inst + s, abi.CC_OP_VALUE_SET, L, v, 0))  # past max_instances
            else:
                rows.append((R + s % 4, abi.CC_OP_VALUE_GET, 0, 0, 0))  # below max_instances, never opened
    arr = np.array(rows, dtype=object)
    b = _batch([int(x) for x in arr[:, 0]], [int(x) for x in arr[:, 1]], [int(x) for x in arr[:, 2]],
               list(arr[:, 3]), list(arr[:, 4]))
    # the super-bucket's list = the rows of opened instances, in log order
    listed = np.nonzero(b.inst < R)[0]
    esc = np.array([_escapes(int(b.op[i]), int(b.flags[i]), int(b.a[i]), int(b.b[i])) for i in listed])
    assert len(listed) > CHUNK + 2 * GROUP and np.all(b.inst[listed] >> 8 == 0)
    groups = [esc[c:c + GROUP] for c in range(0, len(listed) - GROUP + 1, GROUP)]
    assert all(g.any() and not g.all() for g in groups)  # every full group mixes escaped and plain records
    edge = esc[CHUNK - GROUP:CHUNK + GROUP]
    assert edge[:GROUP].any() and not edge[:GROUP].all() and edge[GROUP:].any() and not edge[GROUP:].all()
    for op in (abi.CC_OP_VALUE_GET, abi.CC_OP_VALUE_SET, abi.CC_OP_VALUE_CAS, abi.CC_OP_VALUE_GETANDSET,
               abi.CC_OP_DELETE, 99):
        assert np.any(b.op[listed] == op), op
    cas = listed[b.op[listed] == abi.CC_OP_VALUE_CAS]
    assert np.any((b.flags[cas] & 7) == N) and np.any(((b.flags[cas] >> 3) & 7) == N)  # null expected / null update
    assert np.any(b.inst >= max_inst) and np.any((b.inst >= R) & (b.inst < max_inst))
    gs, gv = _run_both(b, R, max_inst)
    got = gv[listed].view(np.int64)
    ret = np.isin(b.op[listed], (abi.CC_OP_VALUE_GET, abi.CC_OP_VALUE_GETANDSET))
    for x in ((1 << 55) - 1, 1 << 55, -(1 << 55), -(1 << 55) - 1):  # results on both sides of the packed word
        assert np.any(got[ret] == x), x
    okc = gv[cas] == 1
    assert okc.any() and not okc.all()  # both CAS outcomes


def test_state_across_sub_batches_and_calls():
    """Three sub-batches and five rows in all, applied in three calls, one of them empty."""
    from copycat_amd.workload import value_random_stream

    R, sub = 1000, 16384
    n = 3 * sub + 5
    b = value_random_stream(n, R, R + 8, seed=31, hot=4, p_hot=0.3)
    _run_both(b, R, R + 8, sub_batch=sub, split=[(0, 2 * sub + 1), (2 * sub + 1, 2 * sub + 1), (2 * sub + 1, n)])
