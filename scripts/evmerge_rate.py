"""Rate of the device event merge (cc_merge_events_device, copycat_amd/csrc/evmerge_gpu.hip) beside the host call
(cc_merge_events) in the same process (DESIGN.md §6 "The event merge").

Workload: synthetic per-rank event streams of a log of N rows split round-robin over `world` ranks: 22 % of the rows
publish one event, one row in 4,000 is a fan-out of 120 events (0.25 events per row in all, as c5's 24.6M events per
100M rows).  Target, code, src, tag and payload differ from event to event.  Streams, row ids, output and workspace
are resident; a device call is timed with device events around it (its one host wait included, then the gather it
enqueued), 2 warm-ups and 7 timed calls, the host call on 16 threads alternating with it.  The kernels are timed from
events the library records around its launches (cc_merge_events_device_timing) in 7 further calls.  After the timed
calls the device output is compared with the host call's in full; any difference makes the exit status nonzero.
Settings: world 8 and world 2.

Usage: python scripts/evmerge_rate.py [--rows N] [--out profiles/evmerge/rate.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from copycat_amd import abi  # noqa: E402

COPY_TBPS = 6.29  # the measured copy rate MI355X_MICROARCH.md records
PEAK_TBPS = 8.0   # the HBM3E peak
PCIE_D2H_GBPS = 57.0  # the measured D2H rate of this box
EVENT_BYTES = 19
WARM, TIMED = 2, 7
COLS = [name for name, _ in abi.EVENT_COLUMNS]
NPDT = {"u4": np.uint32, "u1": np.uint8, "u8": np.uint64}
VIEW = {"u4": np.int32, "u1": np.uint8, "u8": np.int64}


def algorithmic_bytes(n, events, runs, long_runs):
    """what each step must move: per log row, per event, per run of equal pos, per run of two or more"""
    return {"clear": 8 * n,
            "mark": 4 * events + runs * (8 + 8) + long_runs * (8 + 4),  # pos read; per run: row id read, record stored;
                                                                         # a long run's tail: row id read, end stored
            "scan": 8 * n + 4 * long_runs + 16 * ((n + abi.CC_EVMERGE_TILE_ROWS - 1) // abi.CC_EVMERGE_TILE_ROWS),
            "gather": 8 * n + 4 * long_runs + 2 * (EVENT_BYTES - 4) * events + 4 * events,  # records; five columns in, six out
            }


def build(n, world, seed):
    rng = np.random.default_rng(seed)
    per_row = (rng.random(n) < 0.22).astype(np.uint16)
    per_row[rng.integers(0, n, n // 4000)] = 120
    parts, rows = [], []
    for r in range(world):
        k = per_row[r::world]
        pos = np.repeat(np.arange(len(k), dtype=np.uint32), k)
        j = np.arange(len(pos), dtype=np.uint64)
        x = (j + np.uint64((r * 0x9E3779B97F4A7C15) & (2**64 - 1))) * np.uint64(0xD6E8FEB86659FD93)  # (wraps)
        parts.append({"pos": pos, "target": (x >> np.uint64(17)).astype(np.uint32), "code": (x >> np.uint64(5)).astype(np.uint8),
                      "src": (x >> np.uint64(43)).astype(np.uint8), "tag": (x >> np.uint64(29)).astype(np.uint8), "payload": x})
        rows.append(np.arange(r, n, world, dtype=np.uint64))
    return parts, rows, int(per_row.astype(np.int64).sum()), int(np.count_nonzero(per_row)), int(np.count_nonzero(per_row > 1))


def med(xs):
    return float(np.median(xs))


def rates(ms, events, nbytes):
    tbps = nbytes / (ms * 1e-3) / 1e12
    return {"ms": round(ms, 4), "events_per_s": round(events / (ms * 1e-3), 1), "algorithmic_bytes": int(nbytes),
            "achieved_TBps": round(tbps, 3), "share_of_measured_copy_rate_6.29TBps": round(tbps / COPY_TBPS, 3),
            "share_of_hbm_peak_8TBps": round(tbps / PEAK_TBPS, 3)}


def setting(n, world, threads):
    import torch

    from copycat_amd.engine import _check, _np, lib

    L = lib()
    parts, rows, events, runs, long_runs = build(n, world, 7 + world)
    row_counts = np.array([len(x) for x in rows], np.uint64)
    # ---- host side
    hpr, hrow, hcnt = (abi.cc_events * world)(), (C.c_void_p * world)(), []
    for r, p in enumerate(parts):
        c = np.array([len(p["pos"])], np.uint64)
        hcnt.append(c)
        hpr[r] = abi.cc_events(*[_np(p[name]) for name in COLS], len(p["pos"]), _np(c))
        hrow[r] = _np(rows[r])
    hout = {name: np.zeros(events, NPDT[dt]) for name, dt in abi.EVENT_COLUMNS}
    hocnt = np.zeros(1, np.uint64)
    ho = abi.cc_events(*[_np(hout[name]) for name in COLS], events, _np(hocnt))
    htot = C.c_uint64()
    # ---- device side, all resident
    dkeep, dpr, drow = [], (abi.cc_events * world)(), (C.c_void_p * world)()
    for r, p in enumerate(parts):
        t = {name: torch.from_numpy(p[name].view(VIEW[dt])).cuda() for name, dt in abi.EVENT_COLUMNS}
        c = torch.tensor([len(p["pos"])], dtype=torch.int64, device="cuda")
        rw = torch.from_numpy(rows[r].view(np.int64)).cuda()
        dkeep.append((t, c, rw))
        dpr[r] = abi.cc_events(*[t[name].data_ptr() for name in COLS], len(p["pos"]), c.data_ptr())
        drow[r] = rw.data_ptr()
    dout = {name: torch.zeros(events, dtype=getattr(torch, np.dtype(VIEW[dt]).name), device="cuda")
            for name, dt in abi.EVENT_COLUMNS}
    docnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    do = abi.cc_events(*[dout[name].data_ptr() for name in COLS], events, docnt.data_ptr())
    need = C.c_uint64()
    _check(L.cc_merge_events_device_bound(n, world, C.byref(need)))
    work = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    dtot = C.c_uint64()
    stream = torch.cuda.current_stream()
    sp = C.c_void_p(stream.cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def dev():
        e0.record(stream)
        _check(L.cc_merge_events_device(dpr, drow, _np(row_counts), n, world, C.byref(do), C.byref(dtot),
                                        C.c_void_p(work.data_ptr()), work.numel(), sp))
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def host():
        t0 = time.perf_counter()
        _check(L.cc_merge_events(hpr, hrow, _np(row_counts), n, world, threads, C.byref(ho), C.byref(htot)))
        return (time.perf_counter() - t0) * 1e3

    torch.cuda.synchronize()
    ds, hs = [], []
    for it in range(WARM + TIMED):
        d, h = dev(), host()
        if it >= WARM:
            ds.append(d), hs.append(h)
    kern = []
    _check(L.cc_merge_events_device_timing(1, None))
    for it in range(TIMED):
        dev()
        ms = (C.c_float * 4)()
        _check(L.cc_merge_events_device_timing(1, ms))
        kern.append(list(ms))
    _check(L.cc_merge_events_device_timing(0, None))
    parity = dtot.value == htot.value == events and int(docnt.item()) == int(hocnt[0]) == events
    for name, dt in abi.EVENT_COLUMNS:
        parity = parity and bool(np.array_equal(dout[name].cpu().numpy().view(NPDT[dt]), hout[name]))
    parity = parity and bool(np.all(np.diff(hout["pos"].astype(np.int64)) >= 0))
    ab = algorithmic_bytes(n, events, runs, long_runs)
    call_bytes = sum(ab.values())
    steps = ("clear", "mark", "scan", "gather")
    out = {"label": f"world {world}", "rows": n, "world": world, "events": events, "runs_of_equal_pos": runs, "runs_of_two_or_more": long_runs,
           "events_per_row": round(events / n, 4), "host_threads": threads, "workspace_bytes": need.value,
           "algorithmic_bytes": ab,
           "algorithmic_bytes_per_row_and_event": {"per_row": 8 + 8 + 8, "per_event": 4 + 4 + 2 * (EVENT_BYTES - 4),
                                                   "per_run": 16, "per_run_of_two_or_more": 20},
           "device_call": dict(rates(med(ds), events, call_bytes), all_ms=[round(x, 4) for x in ds],
                               rows_per_s=round(n / (med(ds) * 1e-3), 1),
                               what="events around the call: clear, mark, scans, the host wait, gather"),
           "device_steps_ms": {s: dict(rates(med([k[i] for k in kern]), events, ab[s]), all_ms=[round(k[i], 4) for k in kern])
                               for i, s in enumerate(steps)},
           "host_call": {"ms": round(med(hs), 3), "all_ms": [round(x, 3) for x in hs],
                         "events_per_s": round(events / (med(hs) * 1e-3), 1)},
           "host_merging_deployment_today": {
               "d2h_of_six_columns_ms_at_57GBps": round(events * EVENT_BYTES / (PCIE_D2H_GBPS * 1e9) * 1e3, 3),
               "host_merge_ms": round(med(hs), 3),
               "note": "the D2H time is computed from the measured PCIe rate, not measured here"},
           "parity": bool(parity)}
    print(json.dumps({"label": out["label"], "parity": out["parity"], "events": events, "device_ms": out["device_call"]["ms"],
                      "host_ms": out["host_call"]["ms"],
                      "steps_ms": {s: out["device_steps_ms"][s]["ms"] for s in steps}}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=100e6)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join("profiles", "evmerge", "rate.json"))
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("evmerge_rate.py measures on the GPU: no device found")
    n = int(args.rows)
    results = []
    for world in (8, 2):
        results.append(setting(n, world, args.threads))
        torch.cuda.empty_cache()
    parity = all(r["parity"] for r in results)
    doc = {"script": "scripts/evmerge_rate.py", "rows": n, "device": torch.cuda.get_device_name(0), "warmups": WARM,
           "timed_calls": TIMED, "reference_rates": {"measured_copy_TBps": COPY_TBPS, "hbm_peak_TBps": PEAK_TBPS,
                                                      "pcie_d2h_GBps": PCIE_D2H_GBPS},
           "settings": results, "parity": parity}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out, "parity": parity}))
    sys.exit(0 if parity else 1)


if __name__ == "__main__":
    main()
