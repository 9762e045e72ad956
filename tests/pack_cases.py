"""Batches for the packed-batch tests (tests/test_pack.py on the CPU, tests/test_gpu_pack.py on the GPU): the
width-selection cases with the directory entries the encoder rule demands, and the round-trip streams."""
import numpy as np

from copycat_amd import abi, workload
from copycat_amd.batch import Batch

FOR, REL = abi.CC_PK_FOR, abi.CC_PK_REL_A
B = abi.CC_PACK_BLOCK_ROWS
ALL = tuple(name for name, _ in abi.BATCH_COLUMNS)
VALUE_COLS = ("index", "inst", "op", "flags", "a", "b")  # key / aux / time NULL (a value batch)
M64 = (1 << 64) - 1


def u64(values):
    return np.array([int(v) & M64 for v in values], dtype=np.uint64)


def spread(lo, span, n, seed):
    """n values in [lo, lo + span] (mod 2^64) that reach both ends."""
    rng = np.random.default_rng(seed)
    off = rng.integers(0, span, n, dtype=np.uint64, endpoint=True)
    off[0], off[-1] = 0, span
    return (np.uint64(lo & M64) + off).astype(np.uint64)


def random_batch(n, seed):
    """Uniformly random full-range columns (the generator of tests/test_split.py)."""
    rng = np.random.default_rng(seed)
    b = Batch(n)
    for name in Batch.__slots__:
        a = getattr(b, name)
        a[:] = rng.integers(0, np.iinfo(a.dtype).max, n, dtype=a.dtype, endpoint=True)
    return b


def width_cases():
    """[(name, Batch, {column: [(mode, width, base or None) per block]})]: every (column kind, mode, width) that can
    occur.  Columns a case does not name are all zero (width 0, base 0)."""
    out = []
    n = 1000

    def case(name, expect, rows=n, **cols):
        out.append((name, Batch.from_columns(op=cols.pop("op", np.zeros(rows, np.uint8)), **cols), expect))

    case("constant", {"key": [(FOR, 0, 77)], "a": [(FOR, 0, M64)], "inst": [(FOR, 0, 9)], "op": [(FOR, 0, 52)]},
         key=np.full(n, 77, np.uint64), a=np.full(n, M64, np.uint64), inst=np.full(n, 9, np.uint32),
         op=np.full(n, 52, np.uint8))
    for span, w in ((255, 1), (256, 2), (65535, 2), (65536, 4), ((1 << 32) - 1, 4), (1 << 32, 8)):
        case(f"span_{span}", {"key": [(FOR, w, 0 if w == 8 else 1 << 40)]}, key=spread(1 << 40, span, n, span))
    # a signed span: {-3 .. 250} takes 1 byte from the signed minimum (8 from the unsigned one)
    case("signed_span", {"a": [(FOR, 1, (-3) & M64)]}, a=u64(np.arange(n) % 254 - 3))
    v = list(range(-31528, 26803, 60))
    case("signed_span_2", {"aux": [(FOR, 2, (-31528) & M64)]}, aux=u64(v + [26803] * (n - len(v))))
    case("raw", {"b": [(FOR, 8, 0)]}, rows=3, b=u64([0, M64, 1 << 63]))
    case("inst_1", {"inst": [(FOR, 1, 500)]}, inst=spread(500, 200, n, 1).astype(np.uint32))
    case("inst_2", {"inst": [(FOR, 2, 500)]}, inst=spread(500, 60000, n, 2).astype(np.uint32))
    case("inst_4", {"inst": [(FOR, 4, 0)]}, inst=spread(500, 1 << 31, n, 3).astype(np.uint32))
    case("op_flags_raw", {"op": [(FOR, 1, 0)], "flags": [(FOR, 1, 0)]}, op=(np.arange(n) % 7 + 50).astype(np.uint8),
         flags=(np.arange(n) % 200).astype(np.uint8))
    wide = random_batch(n, 5).a  # full-range counters: FOR needs 8 bytes for a and for b
    for lo, hi, w in ((-128, 127, 1), (-128, 128, 2), (-32768, 32767, 2), (-32769, 0, 4), (0, (1 << 31) - 1, 4)):
        d = np.random.default_rng(w).integers(lo, hi, n, endpoint=True)
        d[0], d[-1] = lo, hi
        case(f"rel_a_{lo}_{hi}", {"a": [(FOR, 8, 0)], "b": [(REL, w, 0)]}, a=wide, b=wide + d.astype(np.uint64))
    d = np.zeros(n, np.int64)
    d[-1] = 1 << 31
    case("rel_a_too_wide", {"b": [(FOR, 8, 0)]}, a=wide, b=wide + d.astype(np.uint64))
    wrap = u64([M64, 1 << 63] * (n // 2))
    case("rel_a_wraps", {"b": [(REL, 1, 0)]}, a=wrap, b=wrap + np.uint64(1))
    # REL_A is never chosen when FOR is as narrow
    small = spread(0, 200, n, 7)
    case("for_beats_rel_1", {"b": [(FOR, 1, None)]}, a=small, b=small + u64(np.arange(n) % 11 - 5 + 5))
    mid = spread(0, 30000, n, 8)
    case("for_beats_rel_2", {"b": [(FOR, 2, None)]}, a=mid, b=mid + u64(np.arange(n) % 401 - 200))
    # two consecutive blocks, the same column at different widths (and a tail block)
    two = np.concatenate([spread(10, 100, B, 9), spread(1 << 20, 70000, 100, 10)])
    case("two_blocks", {"key": [(FOR, 1, 10), (FOR, 4, 1 << 20)], "index": [(FOR, 2, 1), (FOR, 1, B + 1)]}, rows=B + 100,
         key=two, index=np.arange(1, B + 101, dtype=np.uint64))
    return out


def coord_types(res=24):
    return np.array([abi.CC_RES_LOCK, abi.CC_RES_ELECTION, abi.CC_RES_GROUP] * (res // 3), np.uint8)


def streams(n):
    """[(name, Batch of n rows, columns packed)]: the round-trip data of test 1."""
    return [
        ("random", random_batch(n, n + 1), ALL),
        ("value", workload.value_random_stream(max(n, 1), 300, 400, seed=3).slice(0, n), ALL),
        ("map", workload.map_random_stream(max(n, 1), 40, 64, seed=4).slice(0, n), ALL),
        ("coord", workload.coord_random_stream(max(n, 1), coord_types(), 4, 96, seed=5).slice(0, n), ALL),
        ("value_cols", workload.value_random_stream(max(n, 1), 300, 400, seed=6).slice(0, n), VALUE_COLS),
        ("random_value_cols", random_batch(n, n + 2), VALUE_COLS),
    ]
