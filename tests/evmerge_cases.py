"""Shared case builder of the event-merge tests (cc_merge_events / cc_merge_events_device; numpy only).

A case is a sharded log seen from the merge: `n` log rows, an owner per row, and a number of events per row.  From these
the builder makes what a split and `world` engines would leave behind: rows[r] (the log rows of rank r, increasing),
row_counts[r], and rank r's event stream, whose pos is a row of the rank's share.  Target, code, src, tag and payload
differ from event to event (drawn per rank from a seeded generator), so a misplaced event shows in every column.

The reference is independent of both implementations: the parts concatenated, pos mapped through rows, and a stable
argsort by log row."""
import ctypes as C

import numpy as np

from copycat_amd import abi

T = abi.CC_EVMERGE_TILE_ROWS
COLS = tuple(name for name, _ in abi.EVENT_COLUMNS)
DT = {"pos": np.uint32, "target": np.uint32, "code": np.uint8, "src": np.uint8, "tag": np.uint8, "payload": np.uint64}
SENTINEL = {"pos": 0xDEADBEEF, "target": 0xFEEDFACE, "code": 0xA5, "src": 0x5A, "tag": 0xC3, "payload": 0xDEADBEEFCAFEF00D}

SIZES = (1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17)
WORLDS = (1, 2, 3, 8, 256)
OWNERS = ("round_robin", "one_rank", "blocks", "random")
EVENTS = ("none", "one_per_row", "first_and_last_row", "run_65535", "mixed")


def owners(n, world, pattern, rng):
    if pattern == "round_robin":
        return (np.arange(n) % world).astype(np.int64)
    if pattern == "one_rank":  # every other rank has no rows (and NULL columns)
        return np.full(n, world - 1, np.int64)
    if pattern == "blocks":
        return ((np.arange(n) // 37) % world).astype(np.int64)
    if pattern == "random":
        return rng.integers(0, world, n)
    raise ValueError(pattern)


def events_per_row(n, pattern, rng):
    c = np.zeros(n, np.int64)
    if pattern == "none":
        pass
    elif pattern == "one_per_row":
        c[:] = 1
    elif pattern == "first_and_last_row":
        c[0] = 2
        c[-1] += 3
    elif pattern == "run_65535":
        c[n // 2] = 65535
        c[:: max(1, n // 7)] += 1
    elif pattern == "mixed":
        c[:] = rng.integers(0, 4, n)
        c[rng.integers(0, n, max(1, n // 1000))] = 300
    else:
        raise ValueError(pattern)
    return c


class Case:
    """parts[r]: dict of numpy columns; rows[r]: uint64 log rows; row_counts; ref: the merged columns"""

    def __init__(self, n, world, own, per_row, seed=0):
        rng = np.random.default_rng(seed + 1000)
        self.n, self.world = int(n), int(world)
        own = np.asarray(own, np.int64)
        per_row = np.asarray(per_row, np.int64)
        self.rows, self.parts = [], []
        for r in range(world):
            mine = np.nonzero(own == r)[0].astype(np.uint64)
            k = per_row[mine.astype(np.int64)]
            m = int(k.sum())
            part = {"pos": np.repeat(np.arange(len(mine), dtype=np.uint32), k),
                    "target": rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32),
                    "code": rng.integers(1, 14, m).astype(np.uint8),
                    "src": rng.integers(0, 4, m).astype(np.uint8),
                    "tag": rng.integers(0, 8, m).astype(np.uint8),
                    "payload": rng.integers(0, 1 << 63, m, dtype=np.uint64) * np.uint64(2) + np.uint64(r & 1)}
            self.rows.append(mine)
            self.parts.append(part)
        self.row_counts = np.array([len(x) for x in self.rows], np.uint64)
        self.total = int(per_row.sum())
        self.ref = reference(self.parts, self.rows)


def reference(parts, rows):
    log_row = np.concatenate([rows[r][p["pos"].astype(np.int64)] if len(p["pos"]) else np.zeros(0, np.uint64)
                              for r, p in enumerate(parts)])
    order = np.argsort(log_row, kind="stable")
    ref = {name: np.concatenate([p[name] for p in parts])[order] for name in COLS if name != "pos"}
    ref["pos"] = log_row[order].astype(np.uint32)
    return ref


def build(n, world, owner, events, seed=0):
    rng = np.random.default_rng(seed)
    return Case(n, world, owners(n, world, owner, rng), events_per_row(n, events, rng), seed)


def sentinel_columns(capacity):
    return {name: np.full(capacity, SENTINEL[name], DT[name]) for name in COLS}


def equal_columns(got, want, m):
    return all(np.array_equal(got[name][:m], want[name][:m]) for name in COLS)


def untouched(out, start=0):
    return all(np.all(out[name][start:] == DT[name](SENTINEL[name])) for name in COLS)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and len(a) else None


def host_structs(parts, rows, capacities=None, counts=None):
    """(cc_events[world], rows pointer array, keep-alive) over numpy columns; empty columns become NULL"""
    world = len(parts)
    pr = (abi.cc_events * world)()
    rowp = (C.c_void_p * world)()
    keep = []
    for r, p in enumerate(parts):
        cnt = np.array([len(p["pos"]) if counts is None else counts[r]], np.uint64)
        keep.append(cnt)
        for name in COLS:
            setattr(pr[r], name, _p(p[name]))
        pr[r].capacity = len(p["pos"]) if capacities is None else capacities[r]
        pr[r].count = cnt.ctypes.data_as(C.c_void_p)
        rowp[r] = _p(rows[r])
    return pr, rowp, keep


def host_merge(lib, parts, rows, row_counts, n, threads=1, out_capacity=None, capacities=None, counts=None):
    """cc_merge_events into sentinel-filled columns -> (rc, total, out columns, *out.count)"""
    world = len(parts)
    pr, rowp, keep = host_structs(parts, rows, capacities, counts)
    total_in = sum(len(p["pos"]) for p in parts)
    cap = total_in if out_capacity is None else out_capacity
    out = sentinel_columns(max(cap, 1) + 3)  # three guard rows behind the capacity
    ocnt = np.array([0x7777], np.uint64)
    o = abi.cc_events(*[_p(out[name]) for name in COLS], cap, ocnt.ctypes.data_as(C.c_void_p))
    tot = C.c_uint64(0x7777)
    rc_ = np.ascontiguousarray(row_counts, np.uint64)
    rc = lib.cc_merge_events(pr, rowp, rc_.ctypes.data_as(C.c_void_p), n, world, threads, C.byref(o), C.byref(tot))
    return rc, tot.value, out, int(ocnt[0])
