"""Event columns for the packed-event-blob tests (tests/test_evpack.py on the CPU, tests/test_gpu_evpack.py on the GPU),
and the format's rules restated in Python: `encode` builds the blob the rules of include/copycat_apply.h "packed event
blobs" demand, from the event columns alone, without a look at the C code.  The encoders (cc_evpack_pack, the gfx950
kernels, the pipelined call) are compared with it byte for byte; the named cases below also carry the directory entry
each of them was built to get, written out by hand."""
import numpy as np

from copycat_amd import abi
from tests.pack_cases import B, M64, spread, u64

FOR, BY_POS = abi.CC_PK_FOR, abi.CC_PK_BY_POS
HEADER, ENTRY = 64, 112
NAMES = tuple(name for name, _ in abi.EVENT_COLUMNS)
NATIVE = {"pos": 4, "target": 4, "code": 1, "src": 1, "tag": 1, "payload": 8}


def r16(x):
    return (x + 15) & ~15


def width_of(span):
    return 0 if span == 0 else 1 if span <= 0xFF else 2 if span <= 0xFFFF else 4 if span <= 0xFFFFFFFF else 8


def events(pos, target=None, code=None, src=None, tag=None, payload=None):
    """Six event columns of len(pos) rows; a scalar or None column is constant."""
    n = len(pos)

    def col(v, dt, default):
        if v is None:
            v = default
        return np.full(n, v, dt) if np.isscalar(v) else np.ascontiguousarray(v, dtype=dt)

    return {"pos": col(pos, np.uint32, 0), "target": col(target, np.uint32, 9), "code": col(code, np.uint8, 3),
            "src": col(src, np.uint8, 1), "tag": col(tag, np.uint8, 2), "payload": col(payload, np.uint64, 0)}


def concat(parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in NAMES}


def take(ev, lo, hi):
    return {k: ev[k][lo:hi] for k in NAMES}


def same(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in NAMES)


# ---- the rules ---------------------------------------------------------------------------------------------------------
def choose(name, v):
    """(width, base) of one block's column in mode FOR."""
    v = [int(x) for x in v]
    lo, hi = min(v), max(v)
    native = NATIVE[name]
    if native == 1:
        return (1, 0) if hi != lo else (0, lo)
    w, base = width_of(hi - lo), lo
    if native == 8:
        s = [x - (1 << 64) if x >> 63 else x for x in v]
        ws = width_of(max(s) - min(s))
        if ws < w:  # (a tie goes to the unsigned base)
            w, base = ws, min(s) & M64
    return (w, 0) if w == native else (w, base)


def block_entries(ev):
    """[(mode, width, base, entries)] of one block's six columns, in cc_events order."""
    m = len(ev["pos"])
    out = [(FOR, *choose(k, ev[k]), 0) for k in NAMES]
    pw, (_, vw, vbase, _) = out[0][1], out[5]
    pos, pay = ev["pos"].astype(np.int64), ev["payload"]
    ok = bool((pos[1:] >= pos[:-1]).all()) and bool((pay[1:] == pay[:-1])[pos[1:] == pos[:-1]].all())
    if ok and vw > 0 and pw <= 2:
        E = int(pos.max() - pos.min()) + 1
        if r16(E * vw) < r16(m * vw):
            out[5] = (BY_POS, vw, vbase, E)
    return out


def _narrow(v, base, w, units):
    if w == 0:
        return b""
    off = (np.asarray(v, np.uint64) - np.uint64(base)).astype({1: "<u1", 2: "<u2", 4: "<u4", 8: "<u8"}[w])
    raw = off.tobytes()
    assert len(raw) == units * w
    return raw + bytes(r16(len(raw)) - len(raw))


def encode(ev):
    """The blob the format's rules demand of these event columns (a uint8 array)."""
    n = len(ev["pos"])
    blocks = (n + B - 1) // B
    at = HEADER + ENTRY * blocks
    directory, data = [], []
    for k in range(blocks):
        blk = take(ev, k * B, min(n, (k + 1) * B))
        m = len(blk["pos"])
        area, cols = b"", b""
        for name, (mode, w, base, entries) in zip(NAMES, block_entries(blk)):
            off = len(area)
            if mode == BY_POS:
                table = np.zeros(entries, np.uint64)
                table[(blk["pos"] - blk["pos"].min()).astype(np.int64)] = blk["payload"] - np.uint64(base)
                area += _narrow(table + np.uint64(base), base, w, entries)
            else:
                area += _narrow(blk[name], base, w, m)
            cols += bytes([mode, w]) + entries.to_bytes(2, "little") + off.to_bytes(4, "little") + base.to_bytes(8, "little")
        directory.append(m.to_bytes(4, "little") + len(area).to_bytes(4, "little") + at.to_bytes(8, "little") + cols)
        data.append(area)
        at += len(area)
    header = (abi.CC_EVPACK_MAGIC.to_bytes(4, "little") + (1).to_bytes(4, "little") + n.to_bytes(8, "little")
              + blocks.to_bytes(8, "little") + at.to_bytes(8, "little") + (0x3F).to_bytes(4, "little")
              + B.to_bytes(4, "little") + bytes(24))
    return np.frombuffer(header + b"".join(directory) + b"".join(data), np.uint8)


# ---- the named cases ---------------------------------------------------------------------------------------------------
def fanout(rows, per_row, first_row=100, seed=1, target_span=60000, step=1):
    """`rows` publishing rows (`step` apart) with `per_row` events each: one random 64-bit payload per row, targets
    inside a span below 65,536, one code / src / tag."""
    rng = np.random.default_rng(seed)
    pos = np.repeat(first_row + step * np.arange(rows, dtype=np.uint32), per_row)
    pay = np.repeat(rng.integers(0, M64, rows, dtype=np.uint64, endpoint=True), per_row)
    tgt = 1000 + rng.integers(0, target_span, len(pos), dtype=np.uint32, endpoint=True)
    tgt[0], tgt[-1] = 1000, 1000 + target_span
    return events(pos, target=tgt, payload=pay)


def width_cases():
    """[(name, events of one block, {column: (mode, width, base, entries)})]: every (column, width) the format allows
    in mode FOR; pos is constant or decreases somewhere unless the case is about pos, so no table is taken."""
    desc = np.arange(B, 0, -1, dtype=np.uint32)  # strictly decreasing: never BY_POS
    out = [("constant", events(np.full(B, 7, np.uint32), payload=5),
            {"pos": (FOR, 0, 7, 0), "target": (FOR, 0, 9, 0), "code": (FOR, 0, 3, 0), "src": (FOR, 0, 1, 0),
             "tag": (FOR, 0, 2, 0), "payload": (FOR, 0, 5, 0)})]
    for span, w in ((255, 1), (256, 2), (65535, 2), (65536, 4), ((1 << 32) - 1, 4)):
        v = ((1 << 20) + spread(0, span, B, span)).astype(np.uint32) if w < 4 else spread(5, span, B, span).astype(np.uint32)
        lo = int(v.min())
        out.append((f"pos_span_{span}", events(v[::-1].copy() if w < 4 else v, payload=np.arange(B)),
                    {"pos": (FOR, w, 0 if w == 4 else lo, 0)}))
        out.append((f"target_span_{span}", events(desc, target=v), {"target": (FOR, w, 0 if w == 4 else lo, 0)}))
    mixed = (np.arange(B) % 3).astype(np.uint8)
    out.append(("bytes_mixed", events(desc, code=mixed, src=mixed + 1, tag=mixed * 7),
                {"code": (FOR, 1, 0, 0), "src": (FOR, 1, 0, 0), "tag": (FOR, 1, 0, 0)}))
    for span, w in ((255, 1), (256, 2), (65535, 2), (65536, 4), ((1 << 32) - 1, 4), (1 << 32, 8)):
        out.append((f"payload_span_{span}", events(desc, payload=spread(1 << 40, span, B, span)),
                    {"payload": (FOR, w, 0 if w == 8 else 1 << 40, 0)}))
    # a block straddling zero: 1 byte from the signed minimum, 8 from the unsigned one
    out.append(("payload_straddles_zero", events(desc, payload=u64(np.arange(B) % 254 - 3)), {"payload": (FOR, 1, (-3) & M64, 0)}))
    out.append(("payload_straddles_zero_2", events(desc, payload=u64(np.arange(B) * 13 % 60000 - 31528)),
                {"payload": (FOR, 2, (-31528) & M64, 0)}))
    # ties: both bases give the width; the entry carries the unsigned minimum
    out.append(("payload_all_negative", events(desc, payload=u64(-300 + np.arange(B) % 201)), {"payload": (FOR, 1, (-300) & M64, 0)}))
    out.append(("payload_straddles_2^63", events(desc, payload=u64([(1 << 63) - 1, 1 << 63] * (B // 2))),
                {"payload": (FOR, 1, (1 << 63) - 1, 0)}))
    out.append(("payload_raw", events(desc, payload=u64([0, M64, 1 << 63, 5] * (B // 4))), {"payload": (FOR, 8, 0, 0)}))
    # the tail: 1,003 rows (no column's bytes a multiple of 16)
    out.append(("tail", events(desc[:1003], target=spread(7, 300, 1003, 2).astype(np.uint32), code=mixed[:1003],
                               payload=spread(99, 40000, 1003, 4)),
                {"pos": (FOR, 2, B - 1002, 0), "target": (FOR, 2, 7, 0), "code": (FOR, 1, 0, 0), "payload": (FOR, 2, 99, 0)}))
    return out


def by_pos_cases():
    """[(name, events of one block, the payload's (mode, width, base, entries))]."""
    out = []
    f = fanout(64, 64, seed=3)
    out.append(("fanout", f, (BY_POS, 8, 0, 64)))
    g = fanout(64, 64, seed=4, step=3)  # rows three apart: two of three table entries are referred to by no row
    out.append(("fanout_gaps", g, (BY_POS, 8, 0, 190)))
    small = fanout(32, 128, seed=5)
    small["payload"] = (np.uint64(1 << 50) + (small["payload"] % np.uint64(200))).astype(np.uint64)
    small["payload"][:128], small["payload"][-128:] = (1 << 50), (1 << 50) + 199
    out.append(("fanout_one_byte", small, (BY_POS, 1, 1 << 50, 32)))
    d = fanout(64, 64, seed=6)
    d["pos"] = d["pos"].copy()
    d["pos"][2000] -= 1  # (row 2000 starts no run: its pos is now below the row before it)
    out.append(("pos_decreases_once", d, (FOR, 8, 0, 0)))
    p = fanout(64, 64, seed=7)
    p["payload"] = p["payload"].copy()
    p["payload"][1001] ^= np.uint64(1)
    out.append(("one_pos_two_payloads", p, (FOR, 8, 0, 0)))
    # the size tie: 17 rows one byte wide are 32 bytes, and so is a table of 32 entries; 16 entries are 16 bytes
    pay17 = u64([500 + (i * 7) % 100 for i in range(17)])
    pos_tie = np.array(list(range(16)) + [31], np.uint32)
    pay17[0], pay17[1] = 500, 599
    out.append(("size_tie", events(pos_tie, payload=pay17), (FOR, 1, 500, 0)))
    pos_win = np.array([0] + list(range(16)), np.uint32)
    pay_win = pay17.copy()
    pay_win[1] = pay_win[0]
    pay_win[2] = 599
    out.append(("one_entry_less_than_the_tie", events(pos_win, payload=pay_win), (BY_POS, 1, 500, 16)))
    out.append(("payload_width_0", events(np.repeat(np.arange(64, dtype=np.uint32), 64), payload=77), (FOR, 0, 77, 0)))
    wide = events(np.repeat(np.array([5, 70005], np.uint32), B // 2), payload=np.repeat(u64([1, 2]), B // 2))
    out.append(("pos_width_4", wide, (FOR, 1, 1, 0)))
    out.append(("tail_of_1_row", events(np.array([12], np.uint32), payload=1 << 40), (FOR, 0, 1 << 40, 0)))
    return out


def closed_sessions(n=300, seed=8):
    """Events as cc_sessions_close writes them: pos 0xFFFFFFFF on every row, payloads that differ."""
    rng = np.random.default_rng(seed)
    return events(np.full(n, 0xFFFFFFFF, np.uint32), target=rng.integers(0, 500, n, dtype=np.uint32),
                  payload=rng.integers(0, 1 << 40, n, dtype=np.uint64))


def all_case_blocks():
    """Every named case, one per block (cases shorter than a block go last in their own stream): [events, ...]."""
    full = [c[1] for c in width_cases() + by_pos_cases() if len(c[1]["pos"]) == B]
    tails = [c[1] for c in width_cases() + by_pos_cases() if len(c[1]["pos"]) != B]
    return [concat(full)] + [concat(full[:2] + [t]) for t in tails] + [closed_sessions()]


def random_events(n, seed):
    """n events whose blocks take different widths and modes: per block a style for pos (a fan-out, sorted rows,
    random rows), a span for the targets and the payloads, byte columns that are constant in some blocks."""
    rng = np.random.default_rng(seed)
    ev = events(np.zeros(n, np.uint32))
    for lo in range(0, n, B):
        m = min(B, n - lo)
        style = int(rng.integers(0, 4))
        if style == 0:  # a fan-out: the payload is a function of a non-decreasing pos
            per = int(rng.choice([1, 3, 8, 64, 200]))
            pos = lo + np.arange(m, dtype=np.uint32) // per
            pay = rng.integers(0, M64, m // per + 1, dtype=np.uint64, endpoint=True)[(pos - lo).astype(np.int64)]
        elif style == 1:  # sorted rows, payloads of their own
            pos = np.sort(rng.integers(0, 50000, m, dtype=np.uint32))
            pay = np.uint64(1 << 33) + rng.integers(0, 60000, m, dtype=np.uint64)
        elif style == 2:
            pos = rng.integers(0, 1 << 32, m, dtype=np.uint32)
            pay = u64(rng.integers(-100, 100, m))
        else:
            pos = np.full(m, 0xFFFFFFFF, np.uint32)
            pay = rng.integers(0, (0, 200, 1 << 30)[int(rng.integers(0, 3))], m, dtype=np.uint64, endpoint=True)
        ev["pos"][lo:lo + m], ev["payload"][lo:lo + m] = pos, pay
        ev["target"][lo:lo + m] = 40 + rng.integers(0, (0, 200, 60000, 1 << 31)[int(rng.integers(0, 4))], m, dtype=np.uint32,
                                                    endpoint=True)
        for k in ("code", "src", "tag"):
            ev[k][lo:lo + m] = 4 if rng.random() < 0.6 else rng.integers(0, 255, m, dtype=np.uint8, endpoint=True)
    return ev
