"""Packed event blobs on the CPU (copycat_amd/csrc/evpack.cpp): the reference encoder, the validator and the decoder.

Bar: exact.  A decoded blob equals the six event columns byte for byte; the blob is the same for every thread count and
equals the one the format's rules demand (tests/evpack_cases.py restates them in Python); the directory carries the
width and mode each case was built to get; the validator refuses every malformed blob and the decoder then writes
nothing."""
import ctypes as C

import numpy as np
import pytest

from copycat_amd import abi
from copycat_amd.batch import _aligned_bytes, events_bound, events_check, events_info, pack_events, unpack_events
from copycat_amd.engine import EngineError, lib
from tests import evpack_cases as ec
from tests.pack_cases import B

HEADER, ENTRY = ec.HEADER, ec.ENTRY
FOR, BY_POS = ec.FOR, ec.BY_POS


def _aligned_copy(blob):
    out = _aligned_bytes(len(blob))
    out[:] = blob
    return out


def _struct(ev, capacity=None, count=None):
    return abi.cc_events(*(ev[k].ctypes.data for k in ec.NAMES), len(ev["pos"]) if capacity is None else capacity, count)


def test_struct_sizes():
    assert C.sizeof(abi.cc_evpack_block) == ENTRY == 112
    assert C.sizeof(abi.cc_pack_header) == HEADER == 64
    assert abi.cc_evpack_block.col.offset == 16 and C.sizeof(abi.cc_pack_col) == 16
    assert abi.CC_EVPACK_MAGIC == int.from_bytes(b"CCPE", "little") and abi.CC_PK_BY_POS == 2


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 4095, 4096, 4097, 12293])
def test_round_trip_and_thread_independence(n):
    ev = ec.random_events(n, seed=n + 1)
    blobs = [pack_events(ev, threads=t) for t in (1, 3, 0)]
    assert all(np.array_equal(blobs[0], b) for b in blobs[1:]), "the blob depends on the thread count"
    blob = blobs[0]
    assert blob.ctypes.data % 16 == 0 and len(blob) <= events_bound(n)
    assert np.array_equal(blob, ec.encode(ev)), "not the blob the format's rules demand"
    assert events_check(blob) == n
    for t in (1, 3, 0):
        assert ec.same(unpack_events(blob, threads=t), ev)
    info = events_info(blob)
    assert info["n"] == n and info["blocks"] == (n + B - 1) // B and info["bytes"] == len(blob)
    if n == 0:
        assert len(blob) == HEADER


def test_width_selection_per_column_and_width():
    cases = ec.width_cases()
    seen = {k: set() for k in ec.NAMES}
    for name, ev, expect in cases:
        blob = pack_events(ev)
        info = events_info(blob)
        for k in ec.NAMES:
            got = info["columns"][k]["blocks"][0]
            if k in expect:
                assert got == expect[k], (name, k, got)
            assert got[0] == FOR, (name, k)
            seen[k].add(got[1])
        assert np.array_equal(blob, ec.encode(ev)), name
        assert ec.same(unpack_events(blob), ev), name
    assert seen == {"pos": {0, 1, 2, 4}, "target": {0, 1, 2, 4}, "code": {0, 1}, "src": {0, 1}, "tag": {0, 1},
                    "payload": {0, 1, 2, 4, 8}}  # every (column, width) the format allows


@pytest.mark.parametrize("name,ev,expect", ec.by_pos_cases(), ids=[c[0] for c in ec.by_pos_cases()])
def test_by_pos_selection(name, ev, expect):
    blob = pack_events(ev)
    info = events_info(blob)
    assert info["columns"]["payload"]["blocks"][0] == expect
    assert ec.block_entries(ev)[5] == expect  # (the restated rules agree with the hand-written entry)
    assert np.array_equal(blob, ec.encode(ev))
    assert ec.same(unpack_events(blob), ev)


def test_by_pos_table_entries_no_row_refers_to_are_zero():
    ev = [c[1] for c in ec.by_pos_cases() if c[0] == "fanout_gaps"][0]
    blob = pack_events(ev)
    blk = abi.cc_evpack_block.from_buffer_copy(blob[HEADER:HEADER + ENTRY].tobytes())
    e = blk.col[5]
    assert (e.mode, e.width, e.reserved16) == (BY_POS, 8, 190)
    table = blob[blk.offset + e.offset:blk.offset + e.offset + 190 * 8].view(np.uint64)
    first = int(ev["pos"].min())
    rows = {int(p) - first: int(v) for p, v in zip(ev["pos"], ev["payload"])}
    assert len(rows) == 64
    for i in range(190):
        assert int(table[i]) == rows.get(i, 0), i
    assert len(blob) == HEADER + ENTRY + B * 1 + B * 2 + ec.r16(190 * 8)  # pos 1 byte, target 2, the table


def test_all_cases_in_one_stream_each():
    for ev in ec.all_case_blocks():
        blob = pack_events(ev, threads=2)
        assert np.array_equal(blob, ec.encode(ev))
        assert ec.same(unpack_events(blob), ev)


# ---- refusals -------------------------------------------------------------------------------------------------------------
def _put(blob, at, value, size):
    blob[at:at + size] = np.frombuffer(int(value).to_bytes(size, "little"), np.uint8)


def _get(blob, at, size):
    return int.from_bytes(blob[at:at + size].tobytes(), "little")


E0, E1 = HEADER, HEADER + ENTRY  # the two directory entries of the blob below
COL = lambda c: 16 + 16 * c  # a column's entry inside a directory entry: mode, width, reserved16, offset, base
MUTATIONS = [
    ("magic", lambda b: _put(b, 0, abi.CC_RESPACK_MAGIC, 4), "bad magic"),
    ("version", lambda b: _put(b, 4, 2, 4), "version"),
    ("present", lambda b: _put(b, 32, 3, 4), "present"),
    ("n", lambda b: _put(b, 8, _get(b, 8, 8) + 1, 8), "rows"),
    ("blocks", lambda b: _put(b, 16, 3, 8), "block count"),
    ("bytes", lambda b: _put(b, 24, len(b) + 16, 8), "larger than the buffer"),
    ("header_block_rows", lambda b: _put(b, 36, 2048, 4), "block_rows"),
    ("block_rows", lambda b: _put(b, E0, B - 1, 4), "rows"),
    ("misaligned_offset", lambda b: _put(b, E0 + COL(1) + 4, _get(b, E0 + COL(1) + 4, 4) + 8, 4), "not 16-byte aligned"),
    ("area_misaligned", lambda b: _put(b, E1 + 8, _get(b, E1 + 8, 8) + 8, 8), "not 16-byte aligned"),
    ("area_outside", lambda b: _put(b, E1 + 8, _get(b, 24, 8), 8), "outside the blob"),
    ("area_overlaps", lambda b: _put(b, E1 + 8, _get(b, E0 + 8, 8), 8), "overlaps"),
    ("column_outside", lambda b: _put(b, E0 + COL(1) + 4, _get(b, E0 + 4, 4), 4), "outside its block"),
    ("columns_overlap", lambda b: _put(b, E0 + COL(1) + 4, 0, 4), "overlap"),
    ("payload_width_3", lambda b: _put(b, E1 + COL(5) + 1, 3, 1), "width is not"),
    ("pos_width_8", lambda b: _put(b, E0 + COL(0) + 1, 8, 1), "native width"),
    ("code_width_2", lambda b: _put(b, E0 + COL(2) + 1, 2, 1), "native width"),
    ("mode_rel_a", lambda b: _put(b, E0 + COL(5), abi.CC_PK_REL_A, 1), "mode"),
    ("by_pos_entries_0", lambda b: _put(b, E0 + COL(5) + 2, 0, 2), "table of no entry"),
    ("by_pos_entries_4097", lambda b: _put(b, E0 + COL(5) + 2, 4097, 2), "table of no entry or of more than 4096"),
    ("by_pos_entries_below_a_pos_offset", lambda b: _put(b, E0 + COL(5) + 2, 63, 2), "pos offset outside"),
    ("by_pos_on_target", lambda b: _put(b, E0 + COL(1), BY_POS, 1), "other than payload"),
    ("by_pos_with_pos_width_4", lambda b: _put(b, E1 + COL(5), BY_POS, 1), "wider than 2 bytes"),
    ("by_pos_width_0", lambda b: _put(b, E0 + COL(5) + 1, 0, 1), "width 0"),
]


@pytest.fixture(scope="module")
def good_blob():
    """Two blocks: a fan-out (pos 1 byte, target 2, payload a table of 64 entries, every table entry referred to), then a
    tail of 100 rows with pos 4 bytes wide, target 2, the three byte columns raw and payload 2."""
    rng = np.random.default_rng(11)
    mixed = (np.arange(100) % 3).astype(np.uint8)
    tail = ec.events(np.array([5, 90000] * 50, np.uint32), target=ec.spread(7, 300, 100, 2).astype(np.uint32), code=mixed,
                     src=mixed, tag=mixed, payload=np.uint64(1 << 33) + rng.integers(0, 50000, 100, dtype=np.uint64))
    ev = ec.concat([ec.fanout(64, 64, seed=9), tail])
    blob = pack_events(ev)
    cols = events_info(blob)["columns"]
    assert cols["pos"]["blocks"] == [(FOR, 1, 100, 0), (FOR, 4, 0, 0)]
    assert [b[:2] for b in cols["target"]["blocks"]] == [(FOR, 2), (FOR, 2)]
    assert [b[:2] for b in cols["payload"]["blocks"]] == [(BY_POS, 8), (FOR, 2)] and cols["payload"]["blocks"][0][3] == 64
    return ev, blob


def _refused(blob, what):
    L = lib()
    with pytest.raises(EngineError) as e:
        events_check(blob)
    assert e.value.rc == abi.CC_ERR_INVALID
    assert "event blob" in str(e.value) and what in str(e.value), str(e.value)
    # the decoder refuses the same blob and touches no output
    out = {k: np.full(2 * B, 0xEE, np.dtype(dt)) for k, dt in abi.EVENT_COLUMNS}
    count = np.full(1, 0xEE, np.uint64)
    s = _struct(out, count=count.ctypes.data)
    assert L.cc_evpack_unpack(blob.ctypes.data, blob.nbytes, C.byref(s), 1) == abi.CC_ERR_INVALID
    assert all((v == 0xEE).all() for v in out.values()) and count[0] == 0xEE


@pytest.mark.parametrize("name,mutate,what", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_validator_refuses(good_blob, name, mutate, what):
    ev, blob = good_blob
    bad = _aligned_copy(blob)
    mutate(bad)
    _refused(bad, what)
    assert events_check(blob) == len(ev["pos"])  # (the fixture itself is intact)


def test_validator_refuses_truncation_null_and_misaligned(good_blob):
    ev, blob = good_blob
    _refused(_aligned_copy(blob)[:len(blob) - 16], "larger than the buffer")
    _refused(_aligned_copy(blob)[:48], "shorter than its header")
    shifted = _aligned_bytes(len(blob) + 16)[8:8 + len(blob)]
    shifted[:] = blob
    _refused(shifted, "not 16-byte aligned")
    L = lib()
    assert L.cc_evpack_check(None, 64, None) == abi.CC_ERR_INVALID
    assert "event blob" in L.cc_last_error().decode()
    s = _struct(ev)
    size = C.c_uint64()
    assert L.cc_evpack_pack(C.byref(s), len(ev["pos"]), shifted.ctypes.data, shifted.nbytes, 1, C.byref(size)) == abi.CC_ERR_INVALID
    assert L.cc_evpack_pack(None, 0, shifted.ctypes.data, 0, 1, C.byref(size)) == abi.CC_ERR_INVALID


def test_unpack_needs_the_capacity_and_writes_the_count(good_blob):
    L = lib()
    ev, blob = good_blob
    n = len(ev["pos"])
    out = {k: np.full(n, 0xEE, np.dtype(dt)) for k, dt in abi.EVENT_COLUMNS}
    count = np.zeros(1, np.uint64)
    s = _struct(out, capacity=n - 1, count=count.ctypes.data)
    assert L.cc_evpack_unpack(blob.ctypes.data, blob.nbytes, C.byref(s), 1) == abi.CC_ERR_CAPACITY
    assert all((v == 0xEE).all() for v in out.values())
    s = _struct(out, capacity=n, count=count.ctypes.data)
    assert L.cc_evpack_unpack(blob.ctypes.data, blob.nbytes, C.byref(s), 1) == abi.CC_OK
    assert count[0] == n and ec.same(out, ev)
    s = _struct(out, capacity=n + 5, count=None)  # (count is optional)
    assert L.cc_evpack_unpack(blob.ctypes.data, blob.nbytes, C.byref(s), 1) == abi.CC_OK


def test_pack_ignores_capacity_and_count():
    L = lib()
    ev = ec.random_events(500, seed=2)
    blob = pack_events(ev)
    for capacity, count in ((0, None), (7, None), (1 << 40, 12345)):  # (count: never dereferenced)
        s = _struct(ev, capacity=capacity, count=count)
        buf, size = _aligned_bytes(len(blob)), C.c_uint64()
        assert L.cc_evpack_pack(C.byref(s), 500, buf.ctypes.data, buf.nbytes, 1, C.byref(size)) == abi.CC_OK
        assert np.array_equal(buf, blob)


def test_short_cap_returns_the_size_and_writes_nothing():
    L = lib()
    n = 3 * B + 17
    ev = ec.random_events(n, seed=5)
    blob = pack_events(ev)
    s = _struct(ev)
    for cap in (0, HEADER, HEADER + 4 * ENTRY, len(blob) - 16, len(blob) - 1):
        buf = _aligned_bytes(len(blob))
        buf[:] = 0xEE
        size = C.c_uint64()
        assert L.cc_evpack_pack(C.byref(s), n, buf.ctypes.data, cap, 2, C.byref(size)) == abi.CC_ERR_CAPACITY
        assert size.value == len(blob)
        assert (buf == 0xEE).all(), f"cap {cap}: the encoder wrote into a buffer it refused"
    buf = _aligned_bytes(len(blob))  # the exact size is enough
    size = C.c_uint64()
    assert L.cc_evpack_pack(C.byref(s), n, buf.ctypes.data, len(blob), 2, C.byref(size)) == abi.CC_OK
    assert np.array_equal(buf, blob)
    bound = C.c_uint64()
    assert L.cc_evpack_bound(n, C.byref(bound)) == abi.CC_OK and bound.value >= len(blob)
    assert L.cc_evpack_bound(n, None) == abi.CC_ERR_INVALID


def test_fan_out_streams_pack_to_the_size_the_format_gives():
    """Full blocks of a fan-out (one code / src / tag, targets inside a span below 65,536, one random 64-bit payload per
    publishing row, consecutive rows).  64 events per row: per block 4,096 B of pos (1 byte), 8,192 B of target (2 bytes),
    a 512 B payload table and 112 B of directory, 3.15 B per event; the pin is 3.25 B against 19 B wide.  8 events per
    row: pos takes 2 bytes and the table 4,096 B, 5.03 B per event; the pin is 7.25 B."""
    for per_row, pin in ((64, 3.25), (8, 7.25)):
        n = 16 * B
        ev = ec.fanout(n // per_row, per_row, seed=per_row)
        blob = pack_events(ev)
        info = events_info(blob)
        print(per_row, {k: (v["rows"], v["bytes_per_row"]) for k, v in info["columns"].items()}, info["bytes_per_row"])
        assert ec.same(unpack_events(blob), ev)
        assert set(info["columns"]["payload"]["rows"]) == {(BY_POS, 8)}
        assert len(blob) / n <= pin
