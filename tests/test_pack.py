"""Packed host batches on the CPU (copycat_amd/csrc/pack.cpp): cc_pack_batch / cc_pack_check / cc_unpack_batch.

The format (include/copycat_apply.h "packed host batches") is exact: decoding gives the caller's columns back byte for
byte.  Checked here: the round trip on ragged sizes, every thread count and every kind of stream; the deterministic
encoder rule (the narrowest exact encoding per block and column, pinned through the directory); every refusal of the
validator; and the size of the project's own c2 workload."""
import ctypes as C

import numpy as np
import pytest

from copycat_amd import abi, workload
from copycat_amd.batch import pack, pack_check, pack_info, unpack
from copycat_amd.engine import EngineError, lib
from tests import pack_cases as pc

HDR = C.sizeof(abi.cc_pack_header)
BLK = C.sizeof(abi.cc_pack_block)


def _same(b, u, columns):
    for name, _ in abi.BATCH_COLUMNS:
        got, want = getattr(u, name), getattr(b, name)
        assert got.dtype == want.dtype and len(got) == len(want)
        if name in columns:
            assert got.tobytes() == want.tobytes(), name
        else:
            assert not got.any(), name  # an absent column: unpack() leaves zeros


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 4095, 4096, 4097, 12288 + 5])
def test_round_trip(n):
    for name, b, columns in pc.streams(n):
        blobs = []
        for threads in (1, 3, 0):
            blob = pack(b, columns=columns, threads=threads)
            blobs.append(blob.tobytes())
            got_n, present = pack_check(blob)
            assert got_n == n
            assert present == sum(1 << c for c, (col, _) in enumerate(abi.BATCH_COLUMNS) if col in columns)
            _same(b, unpack(blob, threads=threads), columns)
        assert blobs[0] == blobs[1] == blobs[2], f"{name}: the blob depends on the thread count"
        info = pack_info(blob)
        assert info["n"] == n and info["blocks"] == (n + pc.B - 1) // pc.B and info["bytes"] == len(blob)


def test_struct_layouts():
    assert (HDR, C.sizeof(abi.cc_pack_col), BLK, C.sizeof(abi.cc_packed_opts)) == (64, 16, 160, 32)


@pytest.mark.parametrize("name,b,expect", pc.width_cases(), ids=[c[0] for c in pc.width_cases()])
def test_width_selection(name, b, expect):
    blob = pack(b)
    info = pack_info(blob)
    for col, _ in abi.BATCH_COLUMNS:
        blocks = info["columns"][col]["blocks"]
        want = expect.get(col)
        if want is None:
            if not getattr(b, col).any():
                assert all(e == (pc.FOR, 0, 0) for e in blocks), (col, blocks)
            continue
        assert len(blocks) == len(want)
        for got, (mode, width, base) in zip(blocks, want):
            assert got[:2] == (mode, width), (col, got, (mode, width))
            if base is not None:
                assert got[2] == base, (col, got, base)
    _same(b, unpack(blob), pc.ALL)
    # the size follows from the widths: header, directory, and per block each column's rows rounded up to 16 bytes
    size = HDR + BLK * info["blocks"]
    for col, _ in abi.BATCH_COLUMNS:
        left = len(b)
        for _, width, _ in info["columns"][col]["blocks"]:
            rows = min(left, pc.B)
            size += (rows * width + 15) // 16 * 16
            left -= rows
    assert size == len(blob) == info["bytes"]


def test_every_width_occurs():
    """The cases above cover every (column kind, mode, width) the format allows."""
    seen = set()
    for _, b, _ in pc.width_cases():
        info = pack_info(pack(b))
        for col, dt in abi.BATCH_COLUMNS:
            kind = "b" if col == "b" else dt
            seen |= {(kind, m, w) for m, w, _ in info["columns"][col]["blocks"]}
    want = {("u8", pc.FOR, w) for w in (0, 1, 2, 4, 8)} | {("b", pc.FOR, w) for w in (0, 1, 2, 8)}
    want |= {("b", pc.REL, w) for w in (1, 2, 4)} | {("u4", pc.FOR, w) for w in (0, 1, 2, 4)}
    want |= {("u1", pc.FOR, w) for w in (0, 1)}
    assert want <= seen, want - seen


# ---- refusals ----------------------------------------------------------------------------------------------------------
def _aligned_copy(blob, extra=0):
    buf = np.zeros(len(blob) + extra + 64, np.uint8)
    off = (-buf.ctypes.data) % 64
    out = buf[off:off + len(blob) + extra]
    out[:len(blob)] = blob
    return out


def _refused(blob, nbytes=None):
    """cc_pack_check and cc_unpack_batch both answer CC_ERR_INVALID (no output column is touched)."""
    L = lib()
    nbytes = len(blob) if nbytes is None else nbytes
    n, present = C.c_uint64(), C.c_uint32()
    assert L.cc_pack_check(blob.ctypes.data, nbytes, C.byref(n), C.byref(present)) == abi.CC_ERR_INVALID
    assert b"packed blob" in L.cc_last_error()
    cols = [np.zeros(3 * pc.B, np.dtype(dt)) for _, dt in abi.BATCH_COLUMNS]
    out = abi.cc_batch_out(*(c.ctypes.data for c in cols))
    assert L.cc_unpack_batch(blob.ctypes.data, nbytes, C.byref(out), 1) == abi.CC_ERR_INVALID
    with pytest.raises(EngineError):
        pack_check(blob[:nbytes])


def _good(columns=pc.ALL, n=2 * pc.B + 77):
    b = pc.random_batch(n, 11)
    b.inst[:] = b.inst % 1000 + 5  # (inst at width 2, so a wider width can be written into its entry)
    b.op[:] = 52
    blob = _aligned_copy(pack(b, columns=columns))
    pack_check(blob)
    return blob


def _hdr(blob):
    return abi.cc_pack_header.from_buffer(blob, 0)


def _blk(blob, k):
    return abi.cc_pack_block.from_buffer(blob, HDR + BLK * k)


COL = {name: c for c, (name, _) in enumerate(abi.BATCH_COLUMNS)}


def test_check_refuses_truncation():
    blob = _good()
    blocks = _hdr(blob).blocks
    cuts = {0, 1, HDR - 1, HDR, len(blob) - 1, len(blob) - 16} | {HDR + BLK * k for k in range(blocks + 1)}
    cuts |= {HDR + BLK * k - 1 for k in range(1, blocks + 1)} | {_blk(blob, k).offset for k in range(blocks)}
    for cut in sorted(cuts):
        _refused(blob, cut)
        _refused(_aligned_copy(blob[:cut]))  # (an exact-size copy: nothing readable past the cut)
    pack_check(blob)


def _mutations():
    def magic(b):
        _hdr(b).magic ^= 1

    def version(b):
        _hdr(b).version = abi.CC_PACK_VERSION + 1

    def block_rows(b):
        _hdr(b).block_rows = 2048

    def present_bit(b):
        _hdr(b).present |= 1 << 9

    def inst_width_8(b):
        _blk(b, 0).col[COL["inst"]].width = 8

    def op_width_2(b):
        _blk(b, 1).col[COL["op"]].width = 2

    def width_3(b):
        _blk(b, 0).col[COL["key"]].width = 3

    def mode_2(b):
        _blk(b, 0).col[COL["key"]].mode = 2

    def rel_on_a(b):
        e = _blk(b, 0).col[COL["a"]]
        e.mode, e.width = abi.CC_PK_REL_A, 4

    def rel_on_key(b):
        e = _blk(b, 2).col[COL["key"]]
        e.mode, e.width = abi.CC_PK_REL_A, 1

    def rel_width_8(b):
        _blk(b, 0).col[COL["b"]].mode = abi.CC_PK_REL_A  # (b is raw here: width 8)

    def col_unaligned(b):
        _blk(b, 1).col[COL["key"]].offset += 8

    def col_outside(b):
        _blk(b, 1).col[COL["aux"]].offset = _blk(b, 1).bytes

    def col_overlap(b):
        _blk(b, 0).col[COL["a"]].offset = _blk(b, 0).col[COL["index"]].offset

    def area_unaligned(b):
        _blk(b, 1).offset += 8

    def area_overlap(b):
        _blk(b, 1).offset = _blk(b, 0).offset

    def area_in_directory(b):
        _blk(b, 0).offset = HDR

    def area_outside(b):
        _blk(b, 2).offset = _hdr(b).bytes

    def area_length(b):
        _blk(b, 2).bytes += 16

    def rows_short(b):
        _blk(b, 0).rows = pc.B - 1

    def rows_tail(b):
        _blk(b, 2).rows += 1

    def n_more(b):
        _hdr(b).n += 1

    def blocks_more(b):
        _hdr(b).blocks += 1

    def bytes_more(b):
        _hdr(b).bytes += 16

    def bytes_tiny(b):
        _hdr(b).bytes = 32

    return [v for v in locals().values() if callable(v)]


@pytest.mark.parametrize("mutate", _mutations(), ids=[f.__name__ for f in _mutations()])
def test_check_refuses(mutate):
    blob = _good()
    mutate(blob)
    _refused(blob)


def test_check_refuses_rel_a_without_a_and_misalignment():
    blob = _good(columns=("inst", "op", "flags", "b"))
    e = _blk(blob, 0).col[COL["b"]]
    e.mode, e.width = abi.CC_PK_REL_A, 1
    _refused(blob)
    good = _good()
    shifted = _aligned_copy(good, extra=8)
    shifted[8:8 + len(good)] = good
    _refused(shifted[8:8 + len(good)])  # not 16-byte aligned


def test_pack_short_capacity():
    L = lib()
    b = pc.random_batch(pc.B + 9, 3)
    full = pack(b)
    s = abi.cc_batch(*(getattr(b, name).ctypes.data for name, _ in abi.BATCH_COLUMNS))
    for cap in (0, HDR - 1, HDR + BLK, len(full) - 1):
        buf = _aligned_copy(np.full(len(full), 0xEE, np.uint8))
        need = C.c_uint64()
        assert L.cc_pack_batch(C.byref(s), len(b), buf.ctypes.data, cap, 2, C.byref(need)) == abi.CC_ERR_CAPACITY
        assert need.value == len(full)
        assert (buf == 0xEE).all()  # a refused encode writes nothing
    buf = _aligned_copy(np.zeros(len(full), np.uint8))
    assert L.cc_pack_batch(C.byref(s), len(b), buf.ctypes.data, len(full), 2, C.byref(need)) == abi.CC_OK
    assert buf.tobytes() == full.tobytes()
    bound = C.c_uint64()
    assert L.cc_pack_bound(len(b), 0x1FF, C.byref(bound)) == abi.CC_OK and bound.value >= len(full)
    assert L.cc_pack_bound(len(b), 0x200, C.byref(bound)) == abi.CC_ERR_INVALID


def test_c2_step_packs_to_12_bytes_per_row():
    """The third 4M-row AtomicLongClients step (65,536 resources, default seed), columns index / inst / op / flags /
    a / b: at most 12 B per row, header and directory included (30 B wide)."""
    clients = workload.AtomicLongClients(resources=65536)
    for _ in range(3):
        b = clients.next(4 << 20)
    blob = pack(b, columns=pc.VALUE_COLS)
    info = pack_info(blob)
    print({k: (v["rows"], v["bytes_per_row"]) for k, v in info["columns"].items()}, info["bytes_per_row"])
    assert len(blob) / len(b) <= 12.0
    _same(b, unpack(blob), pc.VALUE_COLS)
