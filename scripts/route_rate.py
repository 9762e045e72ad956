"""Rate of the device route (cc_route_events_device, copycat_amd/csrc/route_gpu.hip) beside the host call
(cc_route_events) in the same process (DESIGN.md §6 "The route").

Workload: a synthetic stream of N events (25M: the merged stream of profiles/evmerge/rate.json) whose targets are drawn
uniformly from 2 S instance slots owned by S client sessions (the slots in scrambled order), for S = 4,096, 65,536 and
1M: two and three rounds of the device's 8-bit digit.  Pos, code, src, tag and payload differ from event to event.
Stream, tables, outputs and workspace are resident; a device call is timed with device events around it (its one host
wait at the end included), 2 warm-ups and 7 timed calls, the host call on 16 threads alternating with it.  The kernels
are timed from events the library records around its launches (cc_route_events_device_timing) in 7 further calls.
After the timed calls the device outputs are compared with the host call's in full; any difference makes the exit
status nonzero.

Usage: python scripts/route_rate.py [--events N] [--out profiles/route/rate.json]
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
WARM, TIMED = 2, 7
COLS = [name for name, _ in abi.EVENT_COLUMNS]
NPDT = {"u4": np.uint32, "u1": np.uint8, "u8": np.uint64}
VIEW = {"u4": np.int32, "u1": np.uint8, "u8": np.int64}
STEPS = ("key", "count", "scan", "scatter", "directory", "gather")


def algorithmic_bytes(n, rounds, active):
    """what each step must move: the key kernel reads the target and stores a key and a permutation
    entry (the table reads hit a cache); a round reads and stores a (key, permutation) pair per event, the count reads
    the key once more; the directory reads the sorted keys; the gather reads 19 B and stores 19 + 8 B per event and
    reads the permutation and the instance id"""
    return {"key": (4 + 8) * n, "count": 4 * n * rounds, "scan": 0, "scatter": 16 * n * rounds,
            "directory": 2 * 4 * n + 8 * active, "gather": (4 + 19 + 8 + 27) * n}


def build(n, sessions, seed):
    rng = np.random.default_rng(seed)
    n_inst = 2 * sessions
    j = np.arange(n, dtype=np.uint64)
    x = (j + np.uint64(0x9E3779B97F4A7C15)) * np.uint64(0xD6E8FEB86659FD93)  # (wraps)
    ev = {"pos": (x >> np.uint64(31)).astype(np.uint32), "target": rng.integers(0, n_inst, n).astype(np.uint32),
          "code": (x >> np.uint64(5)).astype(np.uint8), "src": (x >> np.uint64(43)).astype(np.uint8),
          "tag": (x >> np.uint64(29)).astype(np.uint8), "payload": x}
    tab = (np.arange(n_inst, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(sessions)).astype(np.uint32)
    ids = np.arange(n_inst, dtype=np.uint64) * np.uint64(7) + np.uint64(1 << 40)
    return ev, tab, ids


def med(xs):
    return float(np.median(xs))


def rates(ms, events, nbytes):
    tbps = nbytes / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
    return {"ms": round(ms, 4), "events_per_s": round(events / (ms * 1e-3), 1) if ms > 0 else None,
            "algorithmic_bytes": int(nbytes), "achieved_TBps": round(tbps, 3),
            "share_of_measured_copy_rate_6.29TBps": round(tbps / COPY_TBPS, 3), "share_of_hbm_peak_8TBps": round(tbps / PEAK_TBPS, 3)}


def setting(n, sessions, threads):
    import torch

    from copycat_amd.engine import _check, _np, lib

    L = lib()
    ev, tab, ids = build(n, sessions, 7)
    n_inst = len(tab)
    cap = min(n, sessions)
    # ---- host side
    hout = {name: np.zeros(n, NPDT[dt]) for name, dt in abi.EVENT_COLUMNS}
    hinst, hses, hstart = np.zeros(n, np.uint64), np.zeros(cap, np.uint32), np.zeros(cap + 1, np.uint32)
    hocnt, hdcnt = np.zeros(1, np.uint64), np.zeros(1, np.uint64)
    hi = abi.cc_events(*[_np(ev[name]) for name in COLS], n, None)
    ho = abi.cc_events(*[_np(hout[name]) for name in COLS], n, _np(hocnt))
    hd = abi.cc_route_dir(_np(hses), _np(hstart), cap, _np(hdcnt))
    hact = C.c_uint64()
    # ---- device side, all resident
    tdt = lambda dt: getattr(torch, np.dtype(VIEW[dt]).name)  # noqa: E731
    din = {name: torch.from_numpy(ev[name].view(VIEW[dt])).cuda() for name, dt in abi.EVENT_COLUMNS}
    dtab, dids = torch.from_numpy(tab.view(np.int32)).cuda(), torch.from_numpy(ids.view(np.int64)).cuda()
    dout = {name: torch.zeros(n, dtype=tdt(dt), device="cuda") for name, dt in abi.EVENT_COLUMNS}
    dinst = torch.zeros(n, dtype=torch.int64, device="cuda")
    dses, dstart = torch.zeros(cap, dtype=torch.int32, device="cuda"), torch.zeros(cap + 1, dtype=torch.int32, device="cuda")
    docnt, ddcnt = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    di = abi.cc_events(*[din[name].data_ptr() for name in COLS], n, None)
    do = abi.cc_events(*[dout[name].data_ptr() for name in COLS], n, docnt.data_ptr())
    dd = abi.cc_route_dir(dses.data_ptr(), dstart.data_ptr(), cap, ddcnt.data_ptr())
    need = C.c_uint64()
    _check(L.cc_route_events_device_bound(n, sessions, C.byref(need)))
    work = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    dact = C.c_uint64()
    stream = torch.cuda.current_stream()
    sp = C.c_void_p(stream.cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def dev():
        e0.record(stream)
        _check(L.cc_route_events_device(C.byref(di), n, C.c_void_p(dtab.data_ptr()), C.c_void_p(dids.data_ptr()), n_inst,
                                        sessions, C.byref(do), C.c_void_p(dinst.data_ptr()), C.byref(dd), C.byref(dact),
                                        C.c_void_p(work.data_ptr()), work.numel(), sp))
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def host():
        t0 = time.perf_counter()
        _check(L.cc_route_events(C.byref(hi), n, _np(tab), _np(ids), n_inst, sessions, threads, C.byref(ho), _np(hinst),
                                 C.byref(hd), C.byref(hact)))
        return (time.perf_counter() - t0) * 1e3

    torch.cuda.synchronize()
    ds, hs = [], []
    for it in range(WARM + TIMED):
        d, h = dev(), host()
        if it >= WARM:
            ds.append(d), hs.append(h)
    kern = []
    _check(L.cc_route_events_device_timing(1, None))
    for it in range(TIMED):
        dev()
        ms = (C.c_float * abi.CC_ROUTE_TIMING_SLOTS)()
        _check(L.cc_route_events_device_timing(1, ms))
        kern.append(list(ms))
    _check(L.cc_route_events_device_timing(0, None))
    active = int(hact.value)
    parity = dact.value == active and int(docnt.item()) == int(hocnt[0]) == n and int(ddcnt.item()) == int(hdcnt[0]) == active
    for name, dt in abi.EVENT_COLUMNS:
        parity = parity and bool(np.array_equal(dout[name].cpu().numpy().view(NPDT[dt]), hout[name]))
    parity = parity and bool(np.array_equal(dinst.cpu().numpy().view(np.uint64), hinst))
    parity = parity and bool(np.array_equal(dses.cpu().numpy().view(np.uint32)[:active], hses[:active]))
    parity = parity and bool(np.array_equal(dstart.cpu().numpy().view(np.uint32)[:active + 1], hstart[:active + 1]))
    parity = parity and bool(np.all(np.diff(tab[hout["target"]].astype(np.int64)) >= 0))
    rounds = (max(sessions - 1, 0).bit_length() + abi.CC_ROUTE_DIGIT_BITS - 1) // abi.CC_ROUTE_DIGIT_BITS
    ab = algorithmic_bytes(n, rounds, active)
    call_bytes = sum(ab.values())
    out = {"label": f"{sessions} sessions", "events": n, "sessions": sessions, "active_sessions": active, "instances": n_inst,
           "rounds": rounds, "host_threads": threads, "workspace_bytes": need.value, "algorithmic_bytes": ab,
           "algorithmic_bytes_per_event": {"key": 12, "per_round": 16 + 4, "directory": 8, "gather_in": 4 + 19 + 8, "gather_out": 27},
           "device_call": dict(rates(med(ds), n, call_bytes), all_ms=[round(x, 4) for x in ds],
                               what="events around the call: every kernel and the one host wait at the end"),
           "device_steps_ms": {s: dict(rates(med([k[i] for k in kern]), n, ab[s]), all_ms=[round(k[i], 4) for k in kern])
                               for i, s in enumerate(STEPS)},
           "host_call": {"ms": round(med(hs), 3), "all_ms": [round(x, 3) for x in hs],
                         "events_per_s": round(n / (med(hs) * 1e-3), 1)},
           "host_over_device": round(med(hs) / med(ds), 2),
           "parity": bool(parity)}
    print(json.dumps({"label": out["label"], "parity": out["parity"], "device_ms": out["device_call"]["ms"],
                      "host_ms": out["host_call"]["ms"], "steps_ms": {s: out["device_steps_ms"][s]["ms"] for s in STEPS}}),
          flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=float, default=25e6)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--sessions", type=int, nargs="*", default=[4096, 65536, 1 << 20])
    ap.add_argument("--out", default=os.path.join("profiles", "route", "rate.json"))
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("route_rate.py measures on the GPU: no device found")
    n = int(args.events)
    results = []
    for sessions in args.sessions:
        results.append(setting(n, sessions, args.threads))
        torch.cuda.empty_cache()
    parity = all(r["parity"] for r in results)
    doc = {"script": "scripts/route_rate.py", "events": n, "device": torch.cuda.get_device_name(0), "warmups": WARM,
           "timed_calls": TIMED, "reference_rates": {"measured_copy_TBps": COPY_TBPS, "hbm_peak_TBps": PEAK_TBPS},
           "settings": results, "parity": parity}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out, "parity": parity}))
    sys.exit(0 if parity else 1)


if __name__ == "__main__":
    main()
