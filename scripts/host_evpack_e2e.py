#!/usr/bin/env python3
"""The PCIe-inclusive step of an event-heavy stream from host memory: a packed batch in and a packed result blob out in
both calls, the events as a wide page-locked host stream (cc_apply_batch_host_packed_results, 19 B per event) against a
packed event blob (cc_apply_batch_host_packed_events).

Workloads (scripts/topic_rate.py's): topic publish fan-out at 64 and at 8 listeners (4,096 topics, 98 % publishes, rows
for --events events per step) and the c5 stream (bench.py's mixed coordination: locks, elections and groups a third each
over 32,768 resources, --c5-rows rows per step).

The two calls run in two worker processes, one engine each, driven in lockstep by this process: per step each worker
builds the same batch (same seeds), packs it (untimed) and times its call, host wall clock around the synchronous call.
--baseline-root DIR imports the wide worker's package from another checkout (the parent commit's build), so old and new
code are measured interleaved in one session; the default is this checkout.  --warmup untimed steps, then --repeats
timed ones; medians with [min, max].  Every step the event worker decodes its blob on the host (cc_evpack_unpack, timed
on its own) and both workers report the event count and a CRC-32 per decoded column: any difference fails the run.  Per
chunk of every timed event-blob call the stage times come from HIP events (CC_PACKED_TIMELINE).
encode_over_d2h_saved is the event encode time over the D2H time the blob saves: the bytes it does not send (19 B per
event less the blob) at the rate its own D2H ran at.  Prints one JSON line per workload (and writes them to --out).

    python scripts/host_evpack_e2e.py [--events 100000000] [--c5-rows 8388608] [--warmup 2] [--repeats 7]
                                      [--baseline-root DIR] [--workloads topic64,topic8,c5] [--out profiles/evpack/e2e.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TOPICS = 4096
EV_COLS = (("pos", np.uint32), ("target", np.uint32), ("code", np.uint8), ("src", np.uint8), ("tag", np.uint8),
           ("payload", np.uint64))


def _stat(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}


# ---- a worker: one engine, one of the two calls -----------------------------------------------------------------------
def worker(args):
    sys.path.insert(0, os.path.abspath(args.root))
    sys.path.insert(1, HERE)
    import torch  # noqa: F401

    from copycat_amd import abi
    from copycat_amd.batch import Batch, _aligned_bytes, pack, pack_bound, results_bound
    from copycat_amd.engine import Engine, _check, host_register

    w = args.workload
    if w.startswith("topic"):
        from topic_rate import topic_rows

        L = int(w[5:])
        n = int(args.events / (0.98 * L)) + 1
        K, bound = L + 3, L + 2
        sub = min(1 << 22, -(-n // 16384) * 16384)
        E = Engine(TOPICS, TOPICS * K, max(n, TOPICS * K), flags=abi.CC_CFG_TIMERS_DEFERRED, sub_batch=sub,
                   max_events=sub * bound + 1024, coord_cap=max(64, 1 << (L + 2).bit_length()))
        E.resource_create_range(0, TOPICS, abi.CC_RES_TOPIC)
        for k in range(K):
            E.instance_open_range(k * TOPICS, TOPICS, 0, 1000 + k * TOPICS, 7 + k)
        s0 = Batch(TOPICS * L)
        s0.index[:] = np.arange(1, TOPICS * L + 1, dtype=np.uint64)
        s0.inst[:] = np.arange(TOPICS * L)
        s0.op[:] = abi.CC_OP_TOPIC_LISTEN
        E.apply_host_events(s0, capacity=1024)
        index0 = [TOPICS * L + 1]
        cap = n * bound + 1024

        def batch(step):
            b = topic_rows(step, n, TOPICS, L, index0[0])
            index0[0] += n
            return b
    else:
        from copycat_amd.workload import CoordClients

        n, R = args.c5_rows, 32768
        types = np.resize(np.array([abi.CC_RES_LOCK, abi.CC_RES_ELECTION, abi.CC_RES_GROUP], np.uint8), R)
        E = Engine(R + 256, R, n, flags=abi.CC_CFG_TIMERS_DEFERRED, max_events=2 * n)
        for r in range(R):
            E.resource_create(r, int(types[r]))
        E.instance_open_range(0, R, 0, 1000, 1)
        clients = CoordClients(types, K=1, max_inst=R, seed=0xA700000 + 5)
        host = Batch(n)
        cap = 2 * n

        def batch(step):
            clients.next(n, out=host)
            return host

    res_buf = _aligned_bytes(results_bound(n))
    host_register(res_buf)
    cols = {k: np.zeros(cap, dt) for k, dt in EV_COLS}  # wide: the host event stream; events: the decoded blob
    count = np.zeros(1, np.uint64)
    blob_buf = None
    if args.worker == "wide":
        for a in cols.values():
            host_register(a)
    else:
        from copycat_amd.batch import events_bound

        ev_buf = _aligned_bytes(events_bound(cap))
        host_register(ev_buf)
    print(json.dumps({"ready": True, "rows": n, "capacity": cap}), flush=True)
    for line in sys.stdin:
        if line.strip() == "quit":
            break
        step = int(line)
        b = batch(step)
        if blob_buf is None:
            blob_buf = _aligned_bytes(pack_bound(n))
            host_register(blob_buf)
        blob = pack(b, threads=16, out=blob_buf)
        out = {"step": step}
        if args.worker == "wide":
            ev = abi.cc_events(*(cols[k].ctypes.data for k, _ in EV_COLS), cap, count.ctypes.data)
            opts = abi.cc_packed_opts(chunk_rows=args.chunk_rows, flags=0)
            size, done = C.c_uint64(), C.c_uint64()
            t = time.perf_counter()
            rc = E.L.cc_apply_batch_host_packed_results(E.h, blob.ctypes.data, blob.nbytes, res_buf.ctypes.data, res_buf.nbytes,
                                                        C.byref(size), C.byref(ev), C.byref(opts), C.byref(done))
            out["ms"] = (time.perf_counter() - t) * 1e3
            _check(rc)
            m = int(count[0])
            out["res_crc"] = zlib.crc32(res_buf[:size.value])
        else:
            t = time.perf_counter()
            res, evb, m, done = E.apply_host_packed_events(blob, n, capacity=cap, chunk_rows=args.chunk_rows, out=res_buf,
                                                           ev_out=ev_buf, timeline=True)
            out["ms"] = (time.perf_counter() - t) * 1e3
            assert done == n
            out["blob_bytes"] = len(evb)
            out["timeline"] = E.packed_events_timeline().tolist()
            s = abi.cc_events(*(cols[k].ctypes.data for k, _ in EV_COLS), cap, count.ctypes.data)
            t = time.perf_counter()
            _check(E.L.cc_evpack_unpack(evb.ctypes.data, evb.nbytes, C.byref(s), 16))
            out["ms_unpack"] = (time.perf_counter() - t) * 1e3
            assert int(count[0]) == m
            out["res_crc"] = zlib.crc32(res)
        out["events"] = m
        out["crc"] = [zlib.crc32(cols[k][:m]) for k, _ in EV_COLS]
        print(json.dumps(out), flush=True)


# ---- the driver ---------------------------------------------------------------------------------------------------------
def _spawn(mode, root, workload, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--root", root, "--workload", workload,
           "--events", str(args.events), "--c5-rows", str(args.c5_rows), "--chunk-rows", str(args.chunk_rows)]
    return subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, bufsize=1)


def _ask(p, line):
    if line is not None:
        p.stdin.write(line + "\n")
        p.stdin.flush()
    reply = p.stdout.readline()
    if not reply:
        raise RuntimeError(f"a worker ended (exit {p.wait()})")
    return json.loads(reply)


def measure(workload, args):
    wide, new = _spawn("wide", args.baseline_root, workload, args), _spawn("events", ROOT, workload, args)
    try:
        info = _ask(wide, None)
        assert _ask(new, None)["rows"] == info["rows"]
        ms_w, ms_n, ms_u, per_ev, lines, events = [], [], [], [], [], []
        for step in range(args.warmup + args.repeats):
            a, b = _ask(wide, str(step)), _ask(new, str(step))
            same = a["events"] == b["events"] and a["crc"] == b["crc"] and a["res_crc"] == b["res_crc"]
            print(f"{workload} step {step}: wide {a['ms']:.2f} ms, event blob {b['ms']:.2f} ms (+ unpack {b['ms_unpack']:.2f}), "
                  f"{b['events']} events, {b['blob_bytes'] / max(b['events'], 1):.3f} B per event, same {same}", file=sys.stderr,
                  flush=True)
            if not same:
                raise RuntimeError(f"{workload} step {step}: the decoded events or the results differ from the wide call's")
            if step >= args.warmup:
                ms_w.append(a["ms"]), ms_n.append(b["ms"]), ms_u.append(b["ms_unpack"])
                per_ev.append(b["blob_bytes"] / max(b["events"], 1)), lines.append(b), events.append(b["events"])
    finally:
        for p in (wide, new):
            try:
                p.stdin.write("quit\n")
                p.stdin.flush()
            except OSError:
                pass
            p.wait(timeout=120)
    out = {"workload": workload, "rows": info["rows"], "events_per_step": statistics.median(events), "warmup": args.warmup,
           "repeats": args.repeats, "baseline_root": os.path.relpath(os.path.abspath(args.baseline_root), ROOT), "ms_wide_events": _stat(ms_w),
           "ms_event_blob": _stat(ms_n), "ms_unpack_events": _stat(ms_u), "bytes_per_event": round(statistics.median(per_ev), 3),
           "wide_bytes_per_event": 19}
    out["blob_median_over_wide_min"] = round(out["ms_event_blob"]["median_ms"] / out["ms_wide_events"]["min_ms"], 4)
    out["blob_median_below_wide_min"] = out["ms_event_blob"]["median_ms"] < out["ms_wide_events"]["min_ms"]
    mid = sorted(lines, key=lambda x: x["ms"])[len(lines) // 2]
    out["chunks_ms_h2d_decode_apply_encode_d2h_evencode_evd2h"] = [[round(x, 3) for x in c] for c in mid["timeline"]]
    enc, d2h = mid["timeline"][0][5], mid["timeline"][0][6]
    saved = (19 * mid["events"] - mid["blob_bytes"]) / (mid["blob_bytes"] / d2h) if d2h > 0 and mid["blob_bytes"] else None
    out["ms_event_encode"], out["ms_event_d2h"] = round(enc, 3), round(d2h, 3)
    out["ms_d2h_saved_at_the_blob_rate"] = round(saved, 3) if saved else None
    out["encode_over_d2h_saved"] = round(enc / saved, 4) if saved else None
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--events", type=float, default=100e6)
    ap.add_argument("--c5-rows", type=int, default=1 << 23)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--chunk-rows", type=int, default=0)
    ap.add_argument("--baseline-root", default=ROOT)
    ap.add_argument("--workloads", default="topic64,topic8,c5")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", choices=("wide", "events"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--workload", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    lines = []
    for w in args.workloads.split(","):
        lines.append(json.dumps(measure(w, args)))
        print(lines[-1], flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
