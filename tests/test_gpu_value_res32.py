"""GPU parity of the value-only pipeline's 4-byte result word (value_path.hip: 24-bit payload | 7-bit status | escape
bit, one word per staging position in an array of its own; a payload outside [-2^23, 2^23) goes whole to the escape
column): tile and sub-batch edges of the unpermute's 32 KB tile image, every payload on both sides of the word's and of
the former 56-bit word's limits under every value tag, every status the path produces, tiles whose every get escapes
beside tiles where none does, and lists that end inside a chunk beside an empty super-bucket.

Bar: bit-exact per-commit status / value, value_state and applied index against the CPU oracle (integer path, no
tolerance).  The result columns are device tensors prefilled with status 0xFF and value -1; no row may keep the 0xFF.
Geometry as in test_gpu_value_apply.py: resource r is slot r & 255 of super-bucket r >> 8; row i is in tile
i // 8192."""
import numpy as np
import pytest

from copycat_amd import abi
from tests.test_gpu_value_apply import CHUNK, SLOTS, TILE, L, I, N, _batch, _mixed_ops

pytestmark = pytest.mark.gpu

B, H = abi.CC_TAG_BOOL, abi.CC_TAG_HANDLE
SUB = 16384  # the smallest sub-batch the engine accepts
GET, SET, CAS, GAS, DEL = (abi.CC_OP_VALUE_GET, abi.CC_OP_VALUE_SET, abi.CC_OP_VALUE_CAS, abi.CC_OP_VALUE_GETANDSET,
                           abi.CC_OP_DELETE)
UNKNOWN_OP = 99  # no AtomicValue operation
I64 = lambda x: ((int(x) + (1 << 63)) % (1 << 64)) - (1 << 63)
INLINE = lambda x: -(1 << 23) <= I64(x) < (1 << 23)  # the word holds the payload


def _run(b, resources, max_inst, sub_batch=0, split=None):
    """Engine (device columns, prefilled results) against the oracle -> (status, value) of every row."""
    import torch

    from copycat_amd.engine import DeviceBatch, Engine
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
        status = torch.full((hi - lo,), 0xFF, dtype=torch.uint8, device="cuda")
        value = torch.full((hi - lo,), -1, dtype=torch.int64, device="cuda")
        E.apply(DeviceBatch.upload(part), status, value)
        E.sync()
        s2, v2 = O.apply(part)
        gs.append(status.cpu().numpy()); gv.append(value.cpu().numpy().view(np.uint64)); os_.append(s2); ov.append(v2)
    gs, gv, os_, ov = (np.concatenate(x) for x in (gs, gv, os_, ov))
    assert not np.any(gs == 0xFF), f"rows left unwritten: {np.nonzero(gs == 0xFF)[0][:5]}"
    bad = np.nonzero((gs != os_) | (gv != ov))[0]
    assert len(bad) == 0, (f"{len(bad)} rows differ; first {bad[:5]}: gpu {gs[bad[:5]]},{gv[bad[:5]]} "
                           f"oracle {os_[bad[:5]]},{ov[bad[:5]]}")
    for x, y in zip(E.value_state(0, resources), O.value_state(0, resources)):
        assert np.array_equal(x, y)
    assert E.applied_index() == O.applied_index()
    return gs, gv


def _rows(rows):
    """(inst, op, flags, a, b) tuples -> Batch."""
    c = list(zip(*rows))
    return _batch(list(c[0]), list(c[1]), list(c[2]), list(c[3]), list(c[4]))


@pytest.mark.parametrize("sub_batch", [0, SUB])
@pytest.mark.parametrize("n", [1, 3, TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
def test_tile_and_sub_batch_edges(n, sub_batch):
    """300 resources (two super-buckets, the second partial), batches that end one short of, at and one past a tile,
    a 1- and a 3-row tail group, and three tiles and a tail: one sub-batch, or two of the smallest.  A few rows are of
    unknown sessions, and slot 17's gets return a value the word cannot hold."""
    R, max_inst = 300, 304
    rng = np.random.default_rng(3000 + n)
    inst = rng.integers(0, max_inst, n).astype(np.uint32)
    b = _mixed_ops(rng, inst)
    big = b.inst == 17
    b.a[big & (b.op != CAS)] += np.uint64(1 << 40)
    if sub_batch and n > 3 * TILE:
        assert n > sub_batch  # more than one sub-batch
    _run(b, R, max_inst, sub_batch=sub_batch)


BOUNDARY = [-(1 << 23) - 1, -(1 << 23), -1, 0, (1 << 23) - 1, 1 << 23, (1 << 55) - 1, 1 << 55, -(1 << 55) - 1,
            -(1 << 63), (1 << 63) - 1]


def test_payload_boundary_under_every_tag():
    """Per boundary value v and tag (Long and handle: every v; Integer: those an int holds; Boolean: 0 and 1), on a
    slot of its own kind: set v / get / getAndSet(v + 1) (returns v) / CAS(v + 1 -> v) succeeds / CAS again fails /
    get / getAndSet(null) / get (a slot holding null) / delete / get (after delete).  Before any of it, a get on every
    slot (no value yet)."""
    slots = {L: 3, H: 70, I: 130, B: 251}
    rows = [(s, GET, 0, 0, 0) for s in slots.values()]
    expect = []  # (row, returned value, tag)
    for v in BOUNDARY:
        for t, s in slots.items():
            if (t == I and not -(1 << 31) <= v < (1 << 31)) or (t == B and v not in (0, 1)):
                continue
            w = v + 1 if v != (1 << 63) - 1 else v - 1  # a neighbour that is a legal i64
            if t == B:
                w = 1 - v
            rows.append((s, SET, t, v, 0))
            expect.append((len(rows), v, t)); rows.append((s, GET, 0, 0, 0))
            expect.append((len(rows), v, t)); rows.append((s, GAS, t, w, 0))
            rows.append((s, CAS, t | (t << 3), w, v))
            rows.append((s, CAS, t | (t << 3), w, v))
            expect.append((len(rows), v, t)); rows.append((s, GET, 0, 0, 0))
            expect.append((len(rows), v, t)); rows.append((s, GAS, N, 0, 0))
            expect.append((len(rows), 0, N)); rows.append((s, GET, 0, 0, 0))
            rows.append((s, DEL, 0, 0, 0))
            expect.append((len(rows), 0, N)); rows.append((s, GET, 0, 0, 0))
    b = _rows(rows)
    gs, gv = _run(b, SLOTS, SLOTS)
    ok = abi.CC_ST_OK
    for s in range(4):
        assert gs[s] == ok | (N << 4) and gv[s] == 0  # no value yet
    for row, v, t in expect:
        assert I64(gv[row]) == v and gs[row] == ok | (t << 4), (row, v, t, gs[row], gv[row])
    got = {(I64(gv[row]), t) for row, v, t in expect}
    for v in BOUNDARY:
        assert (v, L) in got and (v, H) in got, v
    assert any(not INLINE(v) for v in BOUNDARY) and any(INLINE(v) for v in BOUNDARY)
    cas = np.nonzero(b.op == CAS)[0]
    assert np.all(gs[cas] == ok | (B << 4)) and np.all(gv[cas[0::2]] == 1) and np.all(gv[cas[1::2]] == 0)


def test_statuses():
    """CAS success and failure, set, getAndSet, get, delete, an unknown op, and rows of unknown sessions (an instance
    past max_instances, one never opened), with small and escaping values, spread over two super-buckets."""
    R, max_inst = 300, 306
    rng = np.random.default_rng(3100)
    n = 6000
    inst = rng.integers(0, R, n).astype(np.uint32)
    b = _mixed_ops(rng, inst)
    op, flags, a = b.op.copy(), b.flags.copy(), b.a.copy()
    k = rng.integers(0, 20, n)
    op[k == 0] = UNKNOWN_OP
    a[k == 1] += np.uint64(1 << 40)
    inst[k == 2] = max_inst + 5   # past max_instances
    inst[k == 3] = R + 2          # below max_instances, never opened
    flags[k == 4] = N | (N << 3)  # null operands
    b = _batch(inst, op, flags, a, b.b)
    gs, gv = _run(b, R, max_inst)
    unknown_session = abi.CC_ST_UNKNOWN_SESSION | (N << 4)
    assert np.all(gs[b.inst >= R] == unknown_session) and np.all(gv[b.inst >= R] == 0)
    live = b.inst < R
    assert np.all(gs[live & (b.op == UNKNOWN_OP)] == abi.CC_ST_UNKNOWN_OP | (N << 4))
    cas = live & (b.op == CAS)
    assert np.any(gv[cas] == 1) and np.any(gv[cas] == 0) and np.all(gs[cas] == abi.CC_ST_OK | (B << 4))
    for o in (GET, SET, GAS, DEL):
        assert np.any(live & (b.op == o)), o
    ret = live & np.isin(b.op, (GET, GAS))
    assert np.any(gv[ret] >= np.uint64(1 << 40)) and np.any((gs[ret] >> 4) == N) and np.any((gs[ret] >> 4) == L)


def test_dense_escapes_then_none():
    """Tile 0: 24 slots hold values offset by 2^40 and every other row is a get (all escape), the rows between are
    CASes (booleans, inline), so escaped and inline words alternate inside every 128-byte line.  Tile 1: the same slots
    reset to small values and read again: no escape."""
    rng = np.random.default_rng(3200)
    slots = (np.arange(24) * 10 + 1).astype(np.uint32)
    rows = [(int(s), SET, L, (1 << 40) + 7 * int(s), 0) for s in slots]
    while len(rows) < TILE:
        s = int(slots[rng.integers(0, 24)])
        rows.append((s, GET, 0, 0, 0) if len(rows) % 2 == 0 else (s, CAS, L | (L << 3), 5, 6))
    rows += [(int(s), SET, L, 3 * int(s), 0) for s in slots]
    while len(rows) < 2 * TILE:
        s = int(slots[rng.integers(0, 24)])
        rows.append((s, GET, 0, 0, 0) if len(rows) % 2 == 0 else (s, CAS, L | (L << 3), 5, 6))
    b = _rows(rows)
    gs, gv = _run(b, SLOTS, SLOTS)
    get = b.op == GET
    assert np.all(gv[:TILE][get[:TILE]] >= np.uint64(1 << 40)) and int(get[:TILE].sum()) > TILE // 2 - 30
    assert np.all(gv[TILE:][get[TILE:]] < np.uint64(1 << 23)) and int(get[TILE:].sum()) > TILE // 2 - 30


@pytest.mark.parametrize("tail", [1, 100, CHUNK - 1])
def test_list_end_inside_a_chunk_and_an_empty_super_bucket(tail):
    """Three super-buckets: 0 holds a chunk and `tail` records (its list ends inside its second chunk: the loaders'
    records past the end go to the dummy words), 1 holds none, 2 holds 70 (less than one chunk, a partial last
    64-record group).  The engine's own arrays hold the words; the whole output and state are compared."""
    R = 3 * SLOTS
    counts = [CHUNK + tail, 0, 70]
    rng = np.random.default_rng(3300 + tail)
    sb = rng.permutation(np.repeat(np.arange(3), counts))
    inst = (sb * SLOTS + rng.integers(0, SLOTS, len(sb))).astype(np.uint32)
    b = _mixed_ops(rng, inst)
    b.a[(b.inst & 7) == 0] += np.uint64(1 << 40)  # some results escape, at the list ends too
    assert [int(np.sum(b.inst >> 8 == k)) for k in range(3)] == counts
    _run(b, R, R)
