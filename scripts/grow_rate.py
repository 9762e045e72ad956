#!/usr/bin/env python3
"""Time of cc_snapshot_restore_grow against cc_snapshot_restore of the same snapshot, and of grow.hip's three kernels.

Two engines, one per kind of growth (each is timed against a plain restore into an engine of its own configuration):

  maps   map_capacity 1,048,576 -> 2,097,152 (1,024 -> 2,048 table regions, one more bit; the compacted-key set doubles
         with the table), `--entries` live entries (500,000) of 64 maps, a tenth of them removed again (tombstones)
  coord  coord_cap 64 -> 256 on 32,768 coordination slots: 16,384 locks with a holder and 3 waiters whose ring has
         moved on (head 1), 16,384 queues of 40 elements (head 10)

Each restore is repeated `--runs` times after `--warmup` runs, host wall clock around the call (it returns after its
last device wait); the kernel times come from separate runs with cc_snapshot_grow_timing on (HIP events around each
kernel).  Before anything is timed the grown engine's readers are compared with the source engine's: the whole map
table (cc_read_map_table), and the lock state of every 64th lock.

Prints one JSON line.

    python scripts/grow_rate.py [--entries 500000] [--runs 5] [--warmup 1]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def timed(fn, warmup, runs):
    ms = []
    for k in range(warmup + runs):
        t = time.perf_counter()
        fn()
        if k >= warmup:
            ms.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def kernel_ms(E, snap, runs):
    """per-kernel milliseconds of `runs` grown restores: [table, compacted-key set, coordination blocks]"""
    ms = (C.c_float * 3)()
    out = [[], [], []]
    E.L.cc_snapshot_grow_timing(1, None)
    for _ in range(runs):
        E.restore(snap, grow=True)
        E.L.cc_snapshot_grow_timing(1, ms)
        for k in range(3):
            out[k].append(float(ms[k]))
    E.L.cc_snapshot_grow_timing(0, None)
    return [{"median_ms": round(statistics.median(x), 3), "min_ms": round(min(x), 3), "max_ms": round(max(x), 3)} for x in out]


def maps_case(args):
    from copycat_amd import abi
    from copycat_amd.batch import Batch
    from copycat_amd.engine import Engine

    M, n = 64, args.entries
    rng = np.random.default_rng(1)
    keys = rng.permutation(4 * n)[:n].astype(np.uint64)
    gone = n // 10
    rows = n + gone
    b = Batch.from_columns(index=np.arange(1, rows + 1, dtype=np.uint64),
                           inst=np.concatenate([np.arange(n) % M, np.arange(gone) % M]).astype(np.uint32),
                           op=np.concatenate([np.full(n, abi.CC_OP_MAP_PUT), np.full(gone, abi.CC_OP_MAP_REMOVE)]).astype(np.uint8),
                           flags=np.full(rows, abi.cc_flags(abi.CC_TAG_LONG, 0, 0), np.uint8),
                           key=np.concatenate([keys, keys[:gone]]), a=np.concatenate([keys, keys[:gone]]) + np.uint64(1))

    def engine(cap):
        return Engine(M, M + 8, rows, map_capacity=cap)

    E = engine(1 << 20)
    E.resource_create_range(0, M, abi.CC_RES_MAP)
    E.instance_open_range(0, M, 0, 1000, 7)
    E.apply_host(b)
    snap = E.snapshot()
    P, Gr = engine(1 << 20), engine(1 << 21)
    Gr.restore(snap, grow=True)
    ok = all(np.array_equal(x, y) for x, y in zip(Gr.map_table(), E.map_table())) and Gr.applied_index() == E.applied_index()
    out = {"live_entries": int(len(E.map_table()[0])), "snapshot_mib": round(len(snap) / 2**20, 1), "readers_equal": bool(ok),
           "restore": timed(lambda: P.restore(snap), args.warmup, args.runs),
           "restore_grow": timed(lambda: Gr.restore(snap, grow=True), args.warmup, args.runs)}
    k = kernel_ms(Gr, snap, args.runs)
    out["k_grow_table"], out["k_grow_cset"] = k[0], k[1]
    return out


def coord_case(args):
    from copycat_amd import abi
    from copycat_amd.batch import Batch
    from copycat_amd.engine import Engine

    NL = NQ = 16384
    R, KL = NL + NQ, 4
    insts = NL * KL + NQ  # lock r's instance k: k * NL + r; queue q's instance: NL * KL + q
    LOCK, UNLOCK, ADD, POLL = abi.CC_OP_LOCK_LOCK, abi.CC_OP_LOCK_UNLOCK, abi.CC_OP_QUEUE_ADD, abi.CC_OP_QUEUE_POLL
    rounds = [(np.arange(NL) + k * NL, LOCK, -1) for k in range(KL)]
    rounds += [(np.arange(NL), UNLOCK, 0), (np.arange(NL), LOCK, -1)]  # the ring moves on: head 1, 3 waiters
    q = np.arange(NQ) + NL * KL
    rounds += [(q, ADD, 0)] * 40 + [(q, POLL, 0)] * 10 + [(q, ADD, 0)] * 10
    rows = sum(len(r[0]) for r in rounds)
    b = Batch(rows)
    b.index[:] = np.arange(1, rows + 1, dtype=np.uint64)
    b.time[:] = 1
    b.inst[:] = np.concatenate([r[0] for r in rounds])
    b.op[:] = np.concatenate([np.full(len(r[0]), r[1], np.uint8) for r in rounds])
    b.aux[:] = np.concatenate([np.full(len(r[0]), r[2], np.int64) for r in rounds]).view(np.uint64)
    b.flags[:] = np.where(b.op == ADD, abi.cc_flags(abi.CC_TAG_LONG), 0).astype(np.uint8)
    b.a[:] = b.index

    def engine(cap):
        return Engine(R, insts, rows, flags=abi.CC_CFG_TIMERS_DEFERRED, max_events=1 << 20, coord_cap=cap)

    E = engine(64)
    E.resource_create_range(0, NL, abi.CC_RES_LOCK)
    E.resource_create_range(NL, NQ, abi.CC_RES_QUEUE)
    for k in range(KL):
        E.instance_open_range(k * NL, NL, 0, 1000 + k * NL, 7 + k)
    E.instance_open_range(NL * KL, NQ, NL, 1000 + NL * KL, 7)
    E.apply_host_events(b, capacity=1 << 18)
    snap = E.snapshot()
    P, Gr = engine(64), engine(256)
    Gr.restore(snap, grow=True)
    ok = all(Gr.lock_state(r) == E.lock_state(r) for r in range(0, NL, 64)) and Gr.applied_index() == E.applied_index()
    out = {"slots": R, "snapshot_mib": round(len(snap) / 2**20, 1), "readers_equal": bool(ok),
           "lock_waiters": len(E.lock_state(0)[3]),
           "restore": timed(lambda: P.restore(snap), args.warmup, args.runs),
           "restore_grow": timed(lambda: Gr.restore(snap, grow=True), args.warmup, args.runs)}
    out["k_grow_coord"] = kernel_ms(Gr, snap, args.runs)[2]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--entries", type=int, default=500_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(HERE))
    import torch

    out = {"workload": "snapshot_restore_grow", "runs": args.runs, "maps": maps_case(args), "coord": coord_case(args),
           "gpu": torch.cuda.get_device_name(0)}
    print(json.dumps(out))
    return 0 if out["maps"]["readers_equal"] and out["coord"]["readers_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
