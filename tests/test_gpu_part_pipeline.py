"""GPU parity of the value-only apply where k_part_v4's tile pipeline changes path: a workgroup of the persistent
grid (256 workgroups, 8192-commit tiles) reaches a second tile -- and with it the loads issued a tile early and the
records encoded before the rank -- only from 257 tiles up, so every batch here is 2-6M rows.

Bar: bit-exact per-commit status / value, value_state and applied index against the CPU oracle (integer path, no
tolerance); result columns are prefilled with the sentinel, so a row no kernel writes differs.  Geometry
(value_path.hip): row i is in tile i // 8192; workgroup g takes tiles g, g + 256, g + 512, ...; resource r is slot
r & 255 of super-bucket r >> 8."""
import numpy as np
import pytest

from copycat_amd import abi
from tests.test_gpu_value_apply import TILE, L, _batch, _escapes, _mixed_ops, _run_both

pytestmark = pytest.mark.gpu

GRID = 256  # persistent workgroups
R = 512     # resources (two super-buckets)


def _random_batch(n, seed, resources=R):
    rng = np.random.default_rng(seed)
    return _mixed_ops(rng, rng.integers(0, resources, n).astype(np.uint32))


@pytest.mark.parametrize("n", [GRID * TILE, GRID * TILE + 1, (GRID + 1) * TILE - 1, (GRID + 1) * TILE,
                               2 * GRID * TILE + 100, 300 * TILE + 4097])
def test_tile_counts_per_workgroup(n):
    """No workgroup with a second tile; workgroup 0's second tile one row long (the next tile's loads are issued
    beside a full tile's records); one row short of a full second tile and a full one; three tiles for workgroup 0,
    the last partial; 44 workgroups with a second tile, the last of them partial."""
    _run_both(_random_batch(n, 4000 + n % 1000), R, R)


@pytest.mark.parametrize("n", [GRID * TILE + 1, 2 * GRID * TILE + 100])
def test_byte_path_across_the_prefetch(n):
    """op / flags columns that start one element into their buffers: unaligned, so every tile loads them as bytes."""
    import torch

    from copycat_amd.engine import RESULT_SENTINEL, DeviceBatch, Engine
    from oracle.oracle_py import Oracle

    b = _random_batch(n, 4100 + n % 1000)
    db = DeviceBatch.upload(b, device="cuda:0")
    for name in ("op", "flags"):
        buf = torch.empty(n + 1, dtype=torch.uint8, device="cuda:0")
        buf[1:].copy_(db.cols[name])
        db.cols[name] = buf[1:]
        assert db.cols[name].data_ptr() % 4 == 1
    E = Engine(R, R, n, map_capacity=0)
    O = Oracle(R, R)
    E.resource_create_range(0, R, abi.CC_RES_VALUE)
    E.instance_open_range(0, R, 0, 1000, 7)
    for r in range(R):
        O.resource_create(r, abi.CC_RES_VALUE)
        O.instance_open(r, r, 1000 + r, 7)
    st = torch.full((n,), RESULT_SENTINEL, dtype=torch.uint8, device="cuda:0")
    va = torch.full((n,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda:0")
    E.apply(db, st, va)
    E.sync()
    gs, gv = st.cpu().numpy(), va.cpu().numpy().view(np.uint64)
    os_, ov = O.apply(b)
    bad = np.nonzero((gs != os_) | (gv != ov))[0]
    assert len(bad) == 0, f"{len(bad)} rows differ; first {bad[:5]}: gpu {gs[bad[:5]]},{gv[bad[:5]]} oracle {os_[bad[:5]]},{ov[bad[:5]]}"
    for x, y in zip(E.value_state(0, R), O.value_state(0, R)):
        assert np.array_equal(x, y)
    assert E.applied_index() == O.applied_index()


def test_escaped_and_dropped_rows_at_the_tile_edges():
    """Around the first row, row 4095 and the last row of tiles 0, 256 and 512 (workgroup 0's first, second and third
    tile, the third 100 rows long): a set value past 46 bits, a CAS expected value past 32 bits, a CAS delta past 14
    bits (records that keep their row), an instance past max_instances and a never-opened one (rows that are encoded
    and dropped).  The five kinds take turns on the anchor row itself."""
    n = 2 * GRID * TILE + 100
    max_inst = R + 8
    b = _random_batch(n, 4200)
    inst, op, flags, a, bb = (x.copy() for x in (b.inst, b.op, b.flags, b.a, b.b))
    LL = L | (L << 3)
    kinds = [
        (11, abi.CC_OP_VALUE_SET, L, 1 << 45, 0),                       # set value past 46 bits (signed)
        (12, abi.CC_OP_VALUE_CAS, LL, 1 << 31, (1 << 31) + 1),          # expected past 32 bits
        (13, abi.CC_OP_VALUE_CAS, LL, 5, 5 + (1 << 13)),                # update - expected past 14 bits
        (max_inst + 3, abi.CC_OP_VALUE_SET, L, 9, 0),                   # past max_instances
        (R + 2, abi.CC_OP_VALUE_GET, 0, 0, 0),                          # below max_instances, never opened
    ]
    anchors = []
    for tile in (0, GRID, 2 * GRID):
        rows = min(TILE, n - tile * TILE)
        anchors += [tile * TILE + p for p in (0, 4095, rows - 1) if p < rows]
    assert len(anchors) == 8
    planted = {k: [] for k in range(5)}
    for i, p in enumerate(anchors):
        start = p if p + 5 <= min(n, (p // TILE + 1) * TILE) else p - 4  # the block stays inside the anchor's tile
        for d in range(5):
            k = (i + d - (p - start)) % 5  # kind i % 5 lands on the anchor row
            row = start + d
            inst[row], op[row], flags[row], a[row], bb[row] = kinds[k]
            planted[k].append(row)
        assert (i % 5) == [k for k in range(5) if p in planted[k]][0]
    b = _batch(inst, op, flags, a, bb)
    for k in (0, 1, 2):
        for row in planted[k]:
            assert _escapes(int(b.op[row]), int(b.flags[row]), int(b.a[row]), int(b.b[row])), (k, row)
    gs, gv = _run_both(b, R, max_inst)
    for k in (3, 4):
        assert (abi.status_code(gs[planted[k]]) == abi.CC_ST_UNKNOWN_SESSION).all()


def test_state_across_launches_with_a_cas_chain_over_the_seams():
    """Three sub-batches of 257 tiles in one call: in each launch workgroup 0 takes tiles 0 and 256.  One slot's CAS
    chain (each link expects what the link before wrote) has links on both sides of every seam of workgroup 0's tiles
    -- the end of tile 0, the start and the end of tile 256, the start of the next launch's tile 0 -- and of the
    neighbouring tiles."""
    sub = (GRID + 1) * TILE
    n = 3 * sub
    rng = np.random.default_rng(4300)
    chain = 77
    inst = rng.integers(0, R - 1, n).astype(np.uint32)
    inst[inst >= chain] += 1  # the chain's slot is the chain's alone
    b = _mixed_ops(rng, inst)
    inst, op, flags, a, bb = (x.copy() for x in (b.inst, b.op, b.flags, b.a, b.b))
    links = []
    for s in range(3):
        for edge in (0, TILE, GRID * TILE, sub):  # tile 0 | tile 1, tile 255 | tile 256, and the launch's two ends
            links += [s * sub + edge + d for d in (-3, -2, -1, 0, 1, 2) if 0 <= s * sub + edge + d < n]
    links = sorted(set(links))
    assert len(links) == 3 * 4 * 6 - 6 - 2 * 6
    cur = 1000
    for k, row in enumerate(links):
        inst[row], flags[row] = chain, (L if k == 0 else L | (L << 3))
        if k == 0:
            op[row], a[row], bb[row] = abi.CC_OP_VALUE_SET, cur, 0
        else:
            op[row], a[row], bb[row] = abi.CC_OP_VALUE_CAS, cur, cur + 3
            cur += 3
    b = _batch(inst, op, flags, a, bb)
    assert np.array_equal(np.nonzero(b.inst == chain)[0], np.array(links))
    gs, gv = _run_both(b, R, R, sub_batch=sub)
    assert (gv[links[1:]] == 1).all()  # every link found the value its predecessor wrote
