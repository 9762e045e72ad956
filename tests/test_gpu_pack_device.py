"""cc_pack_from_device on the MI355X: the batch encoder kernels (pack_enc.hip) against the host encoder.

Bar: bit-exact.  The blob equals cc_pack_batch's byte for byte (header, directory, data areas, paddings), whatever the
column set; the bytes behind it keep their sentinel; the device columns are read only.  The REL_A and signed-base
boundaries are built explicitly and also checked against the directory entry the format's rule demands."""
import ctypes as C

import numpy as np
import pytest

from copycat_amd import abi
from copycat_amd.batch import Batch, _aligned_bytes, pack, pack_bound, pack_check, pack_info
from tests import pack_cases as pc

pytestmark = pytest.mark.gpu

B = pc.B
FOR, REL = pc.FOR, pc.REL
M64 = pc.M64
INST_ONLY = ("inst",)
PLACE_PASS = 256  # blocks one pass of k_pack_place holds (one per lane)
SIZES = (1, 15, 16, 17, 255, 256, 257, B - 1, B, B + 1, 2 * B + 33)
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


@pytest.fixture(scope="module")
def small_engine():
    from copycat_amd.engine import Engine

    E = Engine(16, 16, 4096)
    yield E
    E.close()


def _encode(E, b, columns, name, stream=None):
    """the device encoder on an upload of `b`: the blob equals the host encoder's, nothing else is written"""
    import torch

    from copycat_amd.engine import DeviceBatch

    n = len(b)
    want = pack(b, columns=columns, threads=1)
    db = DeviceBatch.upload(b, columns=columns)
    assert all(t.data_ptr() % 16 == 0 for t in db.cols.values())
    out = _aligned_bytes(pack_bound(n, columns) + 64)
    out[:] = 0xCD
    torch.cuda.synchronize()
    got = E.batch_to_host_packed(db, out=out[:len(out) - 64], stream=stream)
    assert len(got) == len(want), f"{name}: {len(got)} bytes, the host encoder writes {len(want)}"
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{name}: the blob differs from the host encoder's first at byte {bad[0]}"
    assert (out[len(got):] == 0xCD).all(), f"{name}: bytes after the blob were written"
    present = sum(1 << c for c, (col, _) in enumerate(abi.BATCH_COLUMNS) if col in columns)
    assert pack_check(got) == (n, present)
    for col, t in db.cols.items():  # the device columns are read only
        assert t.cpu().numpy().tobytes() == getattr(b, col).tobytes(), f"{name}: column {col} was written"
    return got


def _entries(blob, col):
    return pack_info(blob)["columns"][col]["blocks"]


# ---- the case grid ------------------------------------------------------------------------------------------------------
def test_width_cases(small_engine):
    """every (column kind, mode, width) of tests/pack_cases.py, with the entry the rule demands"""
    for name, b, expect in pc.width_cases():
        got = _encode(small_engine, b, pc.ALL, name)
        for col, blocks in expect.items():
            have = _entries(got, col)
            for k, (mode, width, base) in enumerate(blocks):
                assert have[k][:2] == (mode, width), (name, col, k, have[k])
                assert base is None or have[k][2] == base, (name, col, k, have[k])


@pytest.mark.parametrize("n", SIZES)
def test_streams_and_column_sets(small_engine, n):
    """Fails without the feature: cc_pack_from_device does not exist."""
    for name, b, columns in pc.streams(n):
        _encode(small_engine, b, columns, f"{name}/{n}")
    r = pc.random_batch(n, n + 7)
    _encode(small_engine, r, INST_ONLY, f"inst_only/{n}")
    _encode(small_engine, r, pc.VALUE_COLS, f"value_cols/{n}")
    _encode(small_engine, r, pc.ALL, f"all/{n}")


def _mixed(n, seed):
    """n rows whose blocks take different widths and modes on every column"""
    rng = np.random.default_rng(seed)
    b = pc.random_batch(n, seed)
    for lo in range(0, n, B):
        m = min(B, n - lo)
        s = slice(lo, lo + m)
        style = int(rng.integers(0, 4))
        if style == 0:  # a run of a log: indices in order, few instances, operands near each other
            b.index[s] = np.uint64(lo + 1) + np.arange(m, dtype=np.uint64)
            b.time[s] = np.uint64(1 << 40) + (np.arange(m, dtype=np.uint64) >> np.uint64(3))
            b.inst[s] = 1000 + rng.integers(0, 200, m)
            b.op[s], b.flags[s] = 52, rng.integers(0, 3, m)
            b.a[s] = np.uint64(1 << 50) + rng.integers(0, 60000, m, dtype=np.uint64)
            b.b[s] = b.a[s] + pc.u64(rng.integers(-100, 100, m))
            b.key[s], b.aux[s] = 0, pc.u64(rng.integers(-5, 300, m))
        elif style == 1:  # wide a, b close to it
            b.b[s] = b.a[s] + pc.u64(rng.integers(-30000, 30000, m))
            b.inst[s] = rng.integers(0, 60000, m)
        elif style == 2:  # constants
            for col in ("time", "key", "aux", "inst", "op", "flags"):
                getattr(b, col)[s] = 7
    return b


def test_one_block_more_than_a_placement_pass(small_engine):
    """257 blocks: k_pack_place takes a second pass with a carry"""
    n = PLACE_PASS * B + 1
    b = _mixed(n, 3)
    got = _encode(small_engine, b, pc.ALL, f"mixed/{n}")
    info = pack_info(got)
    assert info["blocks"] == PLACE_PASS + 1
    assert {(FOR, 8), (REL, 1), (REL, 2)} <= set(info["columns"]["b"]["rows"])
    _encode(small_engine, b, pc.VALUE_COLS, f"mixed_value_cols/{n}")
    _encode(small_engine, b, INST_ONLY, f"mixed_inst_only/{n}")


# ---- REL_A on b, built explicitly ----------------------------------------------------------------------------------------
def _ab(d, a=None, n=1000, seed=1):
    """a: full-range counters (FOR needs 8 bytes for a and for b); b = a + d modulo 2^64, d reaching both its ends"""
    if a is None:
        a = np.random.default_rng(seed).integers(0, M64, n, dtype=np.uint64, endpoint=True)
    return a, a + pc.u64(d)


def _between(lo, hi, n=1000, seed=2):
    d = np.random.default_rng(seed).integers(lo, hi, n, endpoint=True).astype(object)
    for k in range(0, n - 1, B):  # every block reaches both ends
        d[k + (n - 1 - k) // 2], d[min(k + B, n) - 1] = lo, hi
    return [int(x) for x in d]


REL_CASES = [  # (name, lowest and highest b - a, the entry of b)
    ("fits_1", -128, 127, (REL, 1)),
    ("low_past_1", -129, 127, (REL, 2)),
    ("high_past_1", -128, 128, (REL, 2)),
    ("fits_2", -32768, 32767, (REL, 2)),
    ("low_past_2", -32769, 32767, (REL, 4)),
    ("high_past_2", -32768, 32768, (REL, 4)),
    ("fits_4", I32_MIN, I32_MAX, (REL, 4)),
    ("low_past_4", I32_MIN - 1, I32_MAX, (FOR, 8)),
    ("high_past_4", I32_MIN, I32_MAX + 1, (FOR, 8)),
]


@pytest.mark.parametrize("name,lo,hi,entry", REL_CASES, ids=[c[0] for c in REL_CASES])
def test_rel_a_boundaries(small_engine, name, lo, hi, entry):
    for n in (1000, B + 1000):  # one tail block; a full block and a tail
        a, b = _ab(_between(lo, hi, n), n=n)
        got = _encode(small_engine, Batch.from_columns(op=np.zeros(n, np.uint8), a=a, b=b), pc.ALL, name)
        assert all(e[:2] == entry for e in _entries(got, "b")), (name, _entries(got, "b"))
        assert all(e[:2] == (FOR, 8) for e in _entries(got, "a"))


def test_rel_a_rule_corners(small_engine):
    n = 1000
    op = np.zeros(n, np.uint8)
    # REL_A ties FOR at two bytes: stays FOR
    mid = pc.spread(1 << 20, 30000, n, 8)
    got = _encode(small_engine, Batch.from_columns(op=op, a=mid, b=mid + pc.u64(_between(-200, 200, n))), pc.ALL, "tie_2")
    assert _entries(got, "b")[0][:2] == (FOR, 2)
    # ... and at four bytes
    big = pc.spread(1 << 40, 1 << 30, n, 9)
    got = _encode(small_engine, Batch.from_columns(op=op, a=big, b=big + pc.u64(_between(-40000, 40000, n))), pc.ALL, "tie_4")
    assert _entries(got, "b")[0][:2] == (FOR, 4)
    # choose64's width is 1: REL_A is never taken, though b - a is 0 on every row (it would not be narrower than 1)
    small = pc.spread(5000, 200, n, 7)
    got = _encode(small_engine, Batch.from_columns(op=op, a=small, b=small.copy()), pc.ALL, "for_1")
    assert _entries(got, "b")[0][:2] == (FOR, 1)
    # ... and width 0
    got = _encode(small_engine, Batch.from_columns(op=op, a=small, b=np.full(n, 9, np.uint64)), pc.ALL, "for_0")
    assert _entries(got, "b")[0] == (FOR, 0, 9)
    # b - a wraps modulo 2^64: a = 2^64 - 1 and 2^63, b = a + 1
    wrap = pc.u64([M64, 1 << 63] * (n // 2))
    got = _encode(small_engine, Batch.from_columns(op=op, a=wrap, b=wrap + np.uint64(1)), pc.ALL, "wraps")
    assert _entries(got, "b")[0][:2] == (REL, 1)
    # a difference of 2^63 (the most negative): no REL_A
    a, b = _ab([0, -(1 << 63)] * (n // 2), n=n)
    got = _encode(small_engine, Batch.from_columns(op=op, a=a, b=b), pc.ALL, "int64_min")
    assert _entries(got, "b")[0][:2] == (FOR, 8)
    # b present with a absent: b - a would take one byte, but there is no a in the blob
    a, b = _ab(_between(-100, 100, n), n=n)
    got = _encode(small_engine, Batch.from_columns(op=op, a=a, b=b), ("index", "inst", "op", "flags", "b"), "no_a")
    assert _entries(got, "b")[0][:2] == (FOR, 8)
    # one block REL_A, the next one not, the tail REL_A at another width
    d = _between(-100, 100, B) + _between(-1 << 40, 1 << 40, B) + _between(-30000, 30000, 77)
    a, b = _ab(d, n=2 * B + 77)
    got = _encode(small_engine, Batch.from_columns(op=np.zeros(2 * B + 77, np.uint8), a=a, b=b), pc.ALL, "three_blocks")
    assert [e[:2] for e in _entries(got, "b")] == [(REL, 1), (FOR, 8), (REL, 2)]


# ---- the signed and the unsigned base ------------------------------------------------------------------------------------
def test_signed_and_unsigned_base(small_engine):
    n = 1000
    op = np.zeros(n, np.uint8)
    cases = [
        # both bases give one byte (all values negative): the entry carries the unsigned minimum
        ("all_negative", pc.u64(-300 + np.arange(n) % 201), (FOR, 1, (-300) & M64)),
        # across 2^63 the unsigned base takes one byte, the signed one eight
        ("straddles_2^63", pc.u64([(1 << 63) - 1, 1 << 63] * (n // 2)), (FOR, 1, (1 << 63) - 1)),
        # across zero the signed base is narrower
        ("straddles_zero", pc.u64(np.arange(n) % 254 - 3), (FOR, 1, (-3) & M64)),
        ("straddles_zero_2", pc.u64(np.arange(n) * 13 % 60000 - 31528), (FOR, 2, (-31528) & M64)),
        ("straddles_zero_4", pc.u64(np.arange(n) * 1000003 % (1 << 31) - (1 << 30)), (FOR, 4, None)),
        # both spans need eight bytes: the raw column, base 0
        ("raw", pc.u64([0, M64, 1 << 63, 5] * (n // 4)), (FOR, 8, 0)),
    ]
    for name, v, entry in cases:
        for col in ("index", "time", "key", "a", "b", "aux"):
            got = _encode(small_engine, Batch.from_columns(op=op, **{col: v}), pc.ALL, f"{name}/{col}")
            have = _entries(got, col)[0]
            assert have[:2] == entry[:2] and (entry[2] is None or have[2] == entry[2]), (name, col, have)


def test_inst_widths(small_engine):
    n = B + 1000
    op = np.zeros(n, np.uint8)
    seen = set()
    for span in (0, 1, 255, 256, 65535, 65536, (1 << 32) - 501):
        inst = pc.spread(500, span, n, span + 1).astype(np.uint32)
        inst[5], inst[6] = 500, 500 + span  # (the first block reaches both ends; the tail holds the highest value)
        for columns in (INST_ONLY, pc.VALUE_COLS, pc.ALL):
            got = _encode(small_engine, Batch.from_columns(op=op, inst=inst), columns, f"inst_span_{span}")
            for k, e in enumerate(_entries(got, "inst")):
                blk = inst[k * B:(k + 1) * B].astype(np.int64)
                d = int(blk.max() - blk.min())
                w = 0 if d == 0 else 1 if d <= 0xFF else 2 if d <= 0xFFFF else 4  # choose_small: base 0 at width 4
                assert e == (FOR, w, 0 if w == 4 else int(blk.min())), (span, k, e)
                seen.add(w)
    assert seen == {0, 1, 2, 4}


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_blob_untouched(small_engine):
    from copycat_amd.engine import DeviceBatch

    n = B + 9
    b = pc.random_batch(n, 4)
    db = DeviceBatch.upload(b)
    bound = pack_bound(n)
    blob = _aligned_bytes(bound + 16)
    blob[:] = 0xCD
    size = C.c_uint64(7)
    L = small_engine.L

    def call(s, ptr, cap):
        return L.cc_pack_from_device(small_engine.h, C.byref(s), n, ptr, cap, C.byref(size), None)

    for name, off in (("key", 8), ("inst", 4), ("flags", 1)):  # a misaligned device column
        s = db.struct()
        setattr(s, name, getattr(s, name) + off)
        assert call(s, blob.ctypes.data, bound) == abi.CC_ERR_INVALID, name
    assert call(db.struct(), blob.ctypes.data + 8, bound) == abi.CC_ERR_INVALID  # a misaligned blob
    assert size.value == 7
    assert call(db.struct(), blob.ctypes.data, bound - 1) == abi.CC_ERR_CAPACITY and size.value == bound
    assert (blob == 0xCD).all()
    assert call(db.struct(), blob.ctypes.data, bound) == abi.CC_OK  # and the engine is as good as new
    assert np.array_equal(blob[:size.value], pack(b))


# ---- a stream of the caller's, and the round trip ------------------------------------------------------------------------
def test_non_default_stream_and_staging_reuse(small_engine):
    import torch

    st = torch.cuda.Stream()
    for n in (3 * B + 5, 100, 5 * B):  # the staging grows, is reused smaller, grows again
        _encode(small_engine, _mixed(n, n), pc.ALL, f"stream/{n}", stream=st)


def test_round_trip_through_unpack_to_device(small_engine):
    import torch

    from copycat_amd.engine import DeviceBatch

    n = 3 * B + 77
    b = _mixed(n, 12)
    for columns in (pc.ALL, pc.VALUE_COLS):
        db = DeviceBatch.upload(b, columns=columns)
        blob = small_engine.batch_to_host_packed(db)
        back = {col: torch.zeros_like(t) for col, t in db.cols.items()}
        small_engine.unpack_to_device(blob, back)
        torch.cuda.synchronize()
        for col, t in back.items():
            assert t.cpu().numpy().tobytes() == getattr(b, col).tobytes(), col
