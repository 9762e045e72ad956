"""The group / segment arithmetic of the value-only apply (copycat_amd/csrc/value_group.h) through its host entry points,
on CPU: CC_VALUE_GROUP_TILES as text, rows per group, groups per call, staging size, every segment's rows, tiles and
dummy position, and the 2^29-position bound refused with CC_ERR_CAPACITY instead of wrapping into 32 bits.

Checked against the rules restated here: a tile is 8192 rows; a segment is the engine's sub-batch (whole tiles, at most
3072 of them); a group is whole segments, at least one, at most 2^29 - 4096 positions and at most the knob's tiles; the
staging holds min(n, max_batch, group) rows in whole tiles; segment j starts at row j * sub_batch of its group and its
dummy position is the staging size counted from its own first tile."""
import ctypes as C

import numpy as np
import pytest

from copycat_amd import abi

TILE, MAX_TILES = 8192, 3072
LIMIT = (1 << 29) - 4096
NO_CAP = (1 << 64) - 1


def _lib():
    from copycat_amd.engine import lib

    L = lib()
    for name in ("cc_value_group_knob", "cc_value_group_plan", "cc_value_group_segment"):
        assert getattr(L, name).argtypes is not None, f"{name}: the library has no value-group arithmetic"
    return L


def _knob(text):
    out = C.c_uint64(123)
    rc = _lib().cc_value_group_knob(None if text is None else text.encode(), C.byref(out))
    return rc, out.value


def _plan(n, sub, max_batch, knob):
    out = np.zeros(3, np.uint64)
    rc = _lib().cc_value_group_plan(n, sub, max_batch, knob, out.ctypes.data)
    return rc, [int(x) for x in out]


def _segment(rows, sub, staging, j):
    out = np.zeros(5, np.uint64)
    rc = _lib().cc_value_group_segment(rows, sub, staging, j, out.ctypes.data)
    return rc, [int(x) for x in out]


def test_knob_text():
    assert _knob(None) == (abi.CC_OK, NO_CAP)
    assert _knob("") == (abi.CC_OK, NO_CAP)
    assert _knob("0") == (abi.CC_OK, 0)
    assert _knob("4") == (abi.CC_OK, 4)
    assert _knob("0012") == (abi.CC_OK, 12)
    assert _knob("4294967295") == (abi.CC_OK, (1 << 32) - 1)
    for bad in ("-1", "+4", "4k", " 4", "4 ", "0x10", "1.5", "4294967296", "99999999999999999999999"):
        assert _knob(bad)[0] == abi.CC_ERR_INVALID, bad


@pytest.mark.parametrize("sub_tiles", [2, 3, 1024, 3071, MAX_TILES])
@pytest.mark.parametrize("knob", [NO_CAP, 0, 1, 2, 4, 5, 6144, 1 << 20])
def test_rows_per_group(sub_tiles, knob):
    sub = sub_tiles * TILE
    rc, (group_rows, groups, staging) = _plan(10 * sub + 5, sub, 0, knob)
    assert rc == abi.CC_OK
    if knob == 0:
        assert (group_rows, groups, staging) == (0, 0, 0)
        return
    segs = LIMIT // sub
    if knob != NO_CAP:
        segs = min(segs, knob // sub_tiles)
    segs = max(segs, 1)
    assert group_rows == segs * sub and group_rows % sub == 0
    assert group_rows <= max(LIMIT, sub)
    assert groups == -(-(10 * sub + 5) // group_rows)
    want = min(10 * sub + 5, group_rows)
    assert staging == -(-want // TILE) * TILE and staging >= want


def test_plan_sizes():
    sub = 2 * TILE
    # the staging follows the call up to the group, and max_batch when that is smaller
    assert _plan(sub + 1, sub, 0, NO_CAP) == (abi.CC_OK, [LIMIT // sub * sub, 1, 3 * TILE])
    assert _plan(5 * sub + 4097, sub, 0, NO_CAP)[1][1:] == [1, 11 * TILE]
    assert _plan(5 * sub + 4097, sub, 3 * sub, NO_CAP)[1][2] == 3 * sub
    assert _plan(5 * sub + 5, sub, 0, 4) == (abi.CC_OK, [2 * sub, 3, 2 * sub])
    assert _plan(0, sub, 0, 4) == (abi.CC_OK, [2 * sub, 0, 0])
    # c2: 100M rows in 24 Mi sub-batches are one group of five segments, 22 B a position
    rc, (group_rows, groups, staging) = _plan(100_000_000, MAX_TILES * TILE, 100_000_000, NO_CAP)
    assert rc == abi.CC_OK and groups == 1 and group_rows == 21 * MAX_TILES * TILE
    assert staging == -(-100_000_000 // TILE) * TILE and 2.1e9 < 22 * staging < 2.3e9
    # a sub-batch that is no whole number of tiles, or past the run table, makes no plan
    assert _plan(10, TILE + 1, 0, NO_CAP)[0] == abi.CC_ERR_INVALID
    assert _plan(10, 0, 0, NO_CAP)[0] == abi.CC_ERR_INVALID
    assert _plan(10, (MAX_TILES + 1) * TILE, 0, NO_CAP)[0] == abi.CC_ERR_INVALID


@pytest.mark.parametrize("rows", [1, 16384, 16385, 32768, 32769, 5 * 16384 + 4097, 6 * 16384])
def test_segments_tile_the_group(rows):
    sub = 2 * TILE
    staging = -(-rows // TILE) * TILE
    nseg = -(-rows // sub)
    at = 0
    for j in range(nseg):
        rc, (row0, n, tile0, tiles, dummy) = _segment(rows, sub, staging, j)
        assert rc == abi.CC_OK
        assert row0 == at == j * sub and tile0 == j * 2
        assert n == min(sub, rows - row0) and tiles == -(-n // TILE) and 1 <= tiles <= 2
        assert dummy == staging - tile0 * TILE and dummy >= n  # every live position is below the dummy rows
        at += n
    assert at == rows
    assert _segment(rows, sub, staging, nseg)[0] == abi.CC_ERR_INVALID
    # a larger staging (reused after a longer call) moves only the dummy position
    assert _segment(rows, sub, staging + 4 * TILE, 0)[1] == [0, min(sub, rows), 0, -(-min(sub, rows) // TILE), staging + 4 * TILE]


def test_position_bound_is_refused_not_wrapped():
    sub = MAX_TILES * TILE
    top = (1 << 29) - TILE  # the largest whole-tile staging whose 1024 dummy rows end at or below 2^29
    rc, (row0, n, tile0, tiles, dummy) = _segment(top, sub, top, top // sub)
    assert rc == abi.CC_OK and row0 == (top // sub) * sub and dummy == top - row0 and dummy + 1024 <= 1 << 29
    assert _segment(top, sub, 1 << 29, 0)[0] == abi.CC_ERR_CAPACITY
    assert _segment(1 << 29, sub, 1 << 29, 0)[0] == abi.CC_ERR_CAPACITY
    # 2^32 + 8192 positions would read as 8192 in 32 bits
    assert _segment(TILE, sub, (1 << 32) + TILE, 0)[0] == abi.CC_ERR_CAPACITY
    assert _segment((1 << 32) + TILE, sub, (1 << 32) + TILE, 0)[0] == abi.CC_ERR_CAPACITY
    # a group longer than its staging
    assert _segment(3 * TILE, 2 * TILE, 2 * TILE, 0)[0] == abi.CC_ERR_CAPACITY
    # every plan's staging passes the bound: the largest group of every segment size
    for sub_tiles in (2, 5, 1000, MAX_TILES):
        s = sub_tiles * TILE
        rc, (group_rows, _, staging) = _plan(1 << 40, s, 0, NO_CAP)
        assert rc == abi.CC_OK and staging == group_rows <= LIMIT
        assert _segment(group_rows, s, staging, group_rows // s - 1)[0] == abi.CC_OK
