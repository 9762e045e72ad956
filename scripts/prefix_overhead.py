#!/usr/bin/env python3
"""What cc_apply_batch_prefix costs over cc_apply_batch when nothing stops it.

Two engines of one build get the same resident batches in the same order: one through apply() / apply_events()
followed by sync(), the other through apply_prefix() (which is synchronous).  Shapes: a c2 value-only engine (no scan,
no checkpoint: the ratio should be 1 up to the final sync) and a c5 coordination engine with its event stream (one scan
of inst / op / aux, the per-resource pass, the checkpoint copy and the copy of the caller's result rows).  Per shape:
--warmup untimed steps, then --repeats timed steps per engine, interleaved (plain, prefix, plain, ...) so that clock
and thermal drift hit both alike; host wall clock around the synchronous call; the median is reported, with min / max.
Prints one JSON line.

    python scripts/prefix_overhead.py [--rows 10000000] [--warmup 2] [--repeats 7] [--shapes c2,c5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from copycat_amd import abi  # noqa: E402
from copycat_amd.batch import Batch  # noqa: E402
from copycat_amd.engine import RESULT_SENTINEL, DeviceBatch, DeviceEvents, Engine  # noqa: E402
from copycat_amd.workload import SEED_C2, AtomicLongClients, CoordClients  # noqa: E402

STREAMS = 2  # distinct resident batches per shape, applied in turn (as bench.py cycles its resident streams)


def _results(n, dev):
    return (torch.full((n,), RESULT_SENTINEL, dtype=torch.uint8, device=dev),
            torch.full((n,), -1, dtype=torch.int64, device=dev))


def _time(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def _measure(plain, prefix, streams, warmup, repeats):
    """plain(k) / prefix(k) apply resident batch k on their own engine and return with the stream drained."""
    ms = {"plain": [], "prefix": []}
    for step in range(warmup + repeats):
        k = step % len(streams)
        a, b = _time(lambda: plain(k)), _time(lambda: prefix(k))
        if step >= warmup:
            ms["plain"].append(a)
            ms["prefix"].append(b)
    out = {}
    for name, v in ms.items():
        out[name] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
    out["ratio"] = round(out["prefix"]["median_ms"] / out["plain"]["median_ms"], 4)
    return out


def run_c2(n, dev, warmup, repeats):
    R = 65536
    cols = ("index", "inst", "op", "flags", "a", "b")
    clients = AtomicLongClients(resources=R, seed=SEED_C2)
    host = Batch(n)
    streams = []
    for _ in range(STREAMS):
        clients.next(n, out=host)
        streams.append(DeviceBatch.upload(host, device=dev, columns=cols))
    engines = []
    for _ in range(2):
        E = Engine(R, R, n, device=dev.index, flags=abi.CC_CFG_TIMERS_DEFERRED)
        E.resource_create_range(0, R, abi.CC_RES_VALUE)
        E.instance_open_range(0, R, 0, 1, 1)
        engines.append((E, _results(n, dev)))
    (EA, (sa, va)), (EB, (sb, vb)) = engines

    def plain(k):
        EA.apply(streams[k], sa, va)
        EA.sync()

    def prefix(k):
        assert EB.apply_prefix(streams[k], sb, vb) == n

    out = _measure(plain, prefix, streams, warmup, repeats)
    assert torch.equal(sa, sb) and torch.equal(va, vb), "c2: the two paths' results differ"
    return out


def run_c5(n, dev, warmup, repeats):
    R = 262_144 // 8
    kinds = np.array([abi.CC_RES_LOCK, abi.CC_RES_ELECTION, abi.CC_RES_GROUP], np.uint8)
    types = np.resize(kinds, R)
    clients = CoordClients(types, K=1, max_inst=R, seed=0xA700000 + 5)
    host = Batch(n)
    streams = []
    for _ in range(STREAMS):
        clients.next(n, out=host)
        streams.append(DeviceBatch.upload(host, device=dev))
    engines = []
    for _ in range(2):
        E = Engine(R + 256, R, n, device=dev.index, flags=abi.CC_CFG_TIMERS_DEFERRED, max_events=2 * n)
        for r in range(R):
            E.resource_create(r, int(types[r]))
        E.instance_open_range(0, R, 0, 1000, 1)
        engines.append((E, _results(n, dev), DeviceEvents(2 * n, device=dev)))
    (EA, (sa, va), ea), (EB, (sb, vb), eb) = engines

    def plain(k):
        EA.apply_events(streams[k], sa, va, ea)
        EA.sync()

    def prefix(k):
        assert EB.apply_prefix(streams[k], sb, vb, eb) == n

    out = _measure(plain, prefix, streams, warmup, repeats)
    assert torch.equal(sa, sb) and torch.equal(va, vb), "c5: the two paths' results differ"
    assert int(ea.count.item()) == int(eb.count.item()) > 0, "c5: the two paths' event counts differ"
    out["events_last_step"] = int(eb.count.item())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--shapes", default="c2,c5")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"rows": args.rows, "warmup": args.warmup, "repeats": args.repeats, "gpu": torch.cuda.get_device_name(0)}
    for shape in args.shapes.split(","):
        res[shape] = {"c2": run_c2, "c5": run_c5}[shape](args.rows, dev, args.warmup, args.repeats)
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
