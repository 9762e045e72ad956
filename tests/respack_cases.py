"""Result columns for the packed-result-blob tests (tests/test_respack.py on the CPU, tests/test_gpu_respack.py on the
GPU): one block per width-selection case, with the directory entry the encoder rule demands, and random result rows."""
import numpy as np

from copycat_amd import abi
from tests.pack_cases import B, M64, spread, u64

FOR = abi.CC_PK_FOR
HEADER, ENTRY = 64, 48


def r16(x):
    return (x + 15) & ~15


def width_cases():
    """[(name, status rows, value rows, (status width, status base), (value width, value base))], B rows each but the
    last (a tail): every (column, width) the format allows.

    A tie between the two bases: when a block's unsigned and signed minimum differ, its values lie on both sides of
    zero AND of 2^63, so one of the two spans is at least 2^63 and the widths differ unless both are 8 (written raw,
    base 0).  Below width 8 a tie therefore has one base; "all_negative" pins that the entry carries it as the unsigned
    minimum, "straddles_2^63" that the unsigned base wins where the signed one needs 8 bytes."""
    ok = np.full(B, 0x10, np.uint8)
    mixed = (np.arange(B) % 3 * 0x10).astype(np.uint8)
    out = [
        ("constant", ok, np.full(B, 7, np.uint64), (0, 0x10), (0, 7)),
        ("prefill", np.full(B, 0xFF, np.uint8), np.full(B, 0xA5A5A5A5A5A5A5A5, np.uint64), (0, 0xFF), (0, 0xA5A5A5A5A5A5A5A5)),
        ("status_mixed", mixed, np.zeros(B, np.uint64), (1, 0), (0, 0)),
    ]
    for span, w in ((255, 1), (256, 2), (65535, 2), (65536, 4), ((1 << 32) - 1, 4), (1 << 32, 8)):
        out.append((f"span_{span}", mixed, spread(1 << 40, span, B, span), (1, 0), (w, 0 if w == 8 else 1 << 40)))
    # a block straddling zero: 1 byte from the signed minimum, 8 from the unsigned one
    out.append(("straddles_zero", ok, u64(np.arange(B) % 254 - 3), (0, 0x10), (1, (-3) & M64)))
    out.append(("straddles_zero_2", mixed, u64(np.arange(B) * 13 % 60000 - 31528), (1, 0), (2, (-31528) & M64)))
    out.append(("all_negative", ok, u64(-300 + np.arange(B) % 201), (0, 0x10), (1, (-300) & M64)))
    out.append(("straddles_2^63", ok, u64([(1 << 63) - 1, 1 << 63] * (B // 2)), (0, 0x10), (1, (1 << 63) - 1)))
    out.append(("raw", mixed, u64([0, M64, 1 << 63, 5] * (B // 4)), (1, 0), (8, 0)))
    # the tail: 1,003 rows (neither column's bytes a multiple of 16)
    out.append(("tail", mixed[:1003], spread(99, 40000, 1003, 4), (1, 0), (2, 99)))
    return out


def width_rows():
    """The cases laid out one per block: (status, value, [(status entry, value entry) per block])."""
    cases = width_cases()
    return (np.concatenate([c[1] for c in cases]), np.concatenate([c[2] for c in cases]), [(c[3], c[4]) for c in cases])


def blob_bytes(rows_and_widths):
    """The size the widths demand: [(rows, status width, value width)] per block."""
    return HEADER + ENTRY * len(rows_and_widths) + sum(r16(m * sw) + r16(m * vw) for m, sw, vw in rows_and_widths)


def random_results(n, seed):
    """n result rows whose blocks take different widths: per block a random span for the values (at times around zero)
    and statuses that are constant in some blocks."""
    rng = np.random.default_rng(seed)
    status, value = np.zeros(n, np.uint8), np.zeros(n, np.uint64)
    for lo in range(0, n, B):
        m = min(B, n - lo)
        span = (0, 200, 60000, 1 << 30, M64)[int(rng.integers(0, 5))]
        base = int(rng.integers(0, 1 << 62)) if rng.random() < 0.5 else -int(rng.integers(0, min(span, 1 << 20) + 1))
        value[lo:lo + m] = np.uint64(base & M64) + rng.integers(0, span, m, dtype=np.uint64, endpoint=True)
        status[lo:lo + m] = 0x10 if rng.random() < 0.5 else rng.integers(0, 255, m, dtype=np.uint8, endpoint=True)
    return status, value
