"""Rate of the device split and merge (cc_split_batch_device / cc_merge_results_device, copycat_amd/csrc/split_gpu.hip)
beside the host calls (cc_split_batch / cc_merge_results) in the same process (DESIGN.md §6 "The split on the device").

Workload: bench.py's global_log_split log (atomic_long_stream, same seed): N rows over world x 65,536 resources,
owner = slot % world.  Columns, outputs and the workspace are resident; a call is timed with device events around it
(its one host wait included, then the scatter / gather it enqueued), 2 warm-ups and 7 timed calls, the host call of the
same setting alternating with it.  The three kernels are timed from events the library records around its launches
(cc_split_device_timing) in 7 further calls.  After the timed calls every device output is compared with the host
call's; any difference makes the exit status nonzero.  Settings: world 8 with every column, world 2 with every column,
world 8 with the c2 value batch's columns (inst, op, flags, a, b).

Usage: python scripts/split_rate.py [--rows N] [--out profiles/split_gpu/rate.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from copycat_amd import abi, shard  # noqa: E402
from copycat_amd.batch import Batch  # noqa: E402

COPY_TBPS = 6.29  # the measured copy rate MI355X_MICROARCH.md records
PEAK_TBPS = 8.0   # the HBM3E peak
WIDTH = {"index": 8, "time": 8, "inst": 4, "op": 1, "flags": 1, "key": 8, "a": 8, "b": 8, "aux": 8}
WARM, TIMED = 2, 7


def split_bytes_per_row(names, rows=False):
    """count pass: inst read, owner byte written; scatter pass: owner byte + the columns read, the columns written"""
    cols = sum(WIDTH[c] for c in names)
    return {"count": 4 + 1, "scatter": 1 + cols + cols + (8 if rows else 0), "total": 4 + 1 + 1 + 2 * cols + (8 if rows else 0)}


def merge_bytes_per_row():
    """count pass as the split's; gather pass: owner byte + status and value read, status and value written"""
    return {"count": 4 + 1, "gather": 1 + 9 + 9, "total": 4 + 1 + 1 + 9 + 9}


def rates(ms, n, bytes_per_row):
    tbps = n * bytes_per_row / (ms * 1e-3) / 1e12
    return {"ms": round(ms, 4), "rows_per_s": round(n / (ms * 1e-3), 1), "bytes_per_row": bytes_per_row,
            "achieved_TBps": round(tbps, 3), "share_of_measured_copy_rate_6.29TBps": round(tbps / COPY_TBPS, 3),
            "share_of_hbm_peak_8TBps": round(tbps / PEAK_TBPS, 3)}


def med(xs):
    return float(np.median(xs))


def host_view(t):
    import torch

    w = t.element_size()
    return t.view({8: torch.int64, 4: torch.int32, 1: torch.uint8}[w]).cpu().numpy().view(
        {8: np.uint64, 4: np.uint32, 1: np.uint8}[w])


def setting(b, world, names, threads, label):
    import time

    import torch

    from copycat_amd.engine import DeviceBatch, _check, _np, lib

    L = lib()
    n = len(b)
    R = 65536 * world
    tab = (np.arange(R) % world).astype(np.uint8)
    present = lambda name: name in names  # noqa: E731
    # ---- host side: columns, outputs (allocated once, pages faulted in by the warm-up calls)
    hcols = abi.cc_batch(**{name: _np(getattr(b, name)) if present(name) else None for name in Batch.__slots__})
    counts = np.zeros(world, np.uint64)
    _check(L.cc_split_batch(C.byref(hcols), n, _np(tab), R, world, threads, None, None, _np(counts), None))
    cap = counts.copy()
    hsub = [Batch(int(c)) for c in counts]
    houts = (abi.cc_batch_out * world)()
    for r in range(world):
        for name in names:
            setattr(houts[r], name, _np(getattr(hsub[r], name)))
    # ---- device side: columns, outputs, workspace, all resident
    db = DeviceBatch.upload(b, columns=names)
    dtab = torch.from_numpy(tab).cuda()
    need = C.c_uint64()
    _check(L.cc_split_device_bound(n, world, C.byref(need)))
    work = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    dsub = [{name: torch.empty(int(c), dtype=db.cols[name].dtype, device="cuda") for name in names} for c in counts]
    douts = (abi.cc_batch_out * world)()
    for r in range(world):
        for name in names:
            setattr(douts[r], name, dsub[r][name].data_ptr())
    dcols = db.struct()
    dcounts = np.zeros(world, np.uint64)
    stream = torch.cuda.current_stream()
    sp = C.c_void_p(stream.cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def dev_split():
        e0.record(stream)
        _check(L.cc_split_batch_device(C.byref(dcols), n, C.c_void_p(dtab.data_ptr()), R, world, douts, _np(cap),
                                       _np(dcounts), None, C.c_void_p(work.data_ptr()), work.numel(), sp))
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def host_split():
        t0 = time.perf_counter()
        _check(L.cc_split_batch(C.byref(hcols), n, _np(tab), R, world, threads, houts, _np(cap), _np(counts), None))
        return (time.perf_counter() - t0) * 1e3

    torch.cuda.synchronize()
    ds, hs = [], []
    for it in range(WARM + TIMED):
        d, h = dev_split(), host_split()
        if it >= WARM:
            ds.append(d), hs.append(h)
    assert dcounts.tolist() == counts.tolist()
    kern = []
    _check(L.cc_split_device_timing(1, None))
    for it in range(TIMED):
        dev_split()
        ms = (C.c_float * 3)()
        _check(L.cc_split_device_timing(1, ms))
        kern.append(list(ms))
    _check(L.cc_split_device_timing(0, None))
    parity = True
    for r in range(world):
        for name in names:
            parity &= bool(np.array_equal(host_view(dsub[r][name]), getattr(hsub[r], name)))
    bpr = split_bytes_per_row(names)
    out = {"label": label, "rows": n, "world": world, "columns": list(names), "host_threads": threads,
           "bytes_per_row": bpr,
           "device_split": dict(rates(med(ds), n, bpr["total"]), all_ms=[round(x, 4) for x in ds],
                                what="events around the call: count, scan, the host wait, scatter"),
           "device_split_kernels_ms": {
               "k_split_count": dict(rates(med([k[0] for k in kern]), n, bpr["count"]), all_ms=[round(k[0], 4) for k in kern]),
               "k_split_scan": {"ms": round(med([k[1] for k in kern]), 4), "all_ms": [round(k[1], 4) for k in kern]},
               "k_split_scatter": dict(rates(med([k[2] for k in kern]), n, bpr["scatter"]),
                                       all_ms=[round(k[2], 4) for k in kern])},
           "host_split": {"ms": round(med(hs), 3), "all_ms": [round(x, 3) for x in hs],
                          "rows_per_s": round(n / (med(hs) * 1e-3), 1)},
           "split_parity": parity}
    # ---- merge: synthetic per-rank results (status = a byte of the row's a column, value = its index, or a without one)
    val = "index" if present("index") else "a"
    hres = [((getattr(hsub[r], "a") & 0xFF).astype(np.uint8), getattr(hsub[r], val).copy()) for r in range(world)]
    hpr = (abi.cc_results * world)()
    dpr = (abi.cc_results * world)()
    dres = []
    for r, (s, v) in enumerate(hres):
        hpr[r].status, hpr[r].value = _np(s), _np(v)
        ts, tv = torch.from_numpy(s).cuda(), torch.from_numpy(v.view(np.int64)).cuda()
        dres.append((ts, tv))
        dpr[r].status, dpr[r].value = ts.data_ptr(), tv.data_ptr()
    hst, hva = np.empty(n, np.uint8), np.empty(n, np.uint64)
    hout = abi.cc_results(_np(hst), _np(hva))
    dst, dva = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.int64, device="cuda")
    dout = abi.cc_results(dst.data_ptr(), dva.data_ptr())
    dinst = C.c_void_p(db.cols["inst"].data_ptr())

    def dev_merge():
        e0.record(stream)
        _check(L.cc_merge_results_device(dinst, n, C.c_void_p(dtab.data_ptr()), R, world, dpr, C.byref(dout),
                                         C.c_void_p(work.data_ptr()), work.numel(), sp))
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def host_merge():
        t0 = time.perf_counter()
        _check(L.cc_merge_results(_np(b.inst), n, _np(tab), R, world, threads, hpr, C.byref(hout)))
        return (time.perf_counter() - t0) * 1e3

    torch.cuda.synchronize()
    dm, hm = [], []
    for it in range(WARM + TIMED):
        d, h = dev_merge(), host_merge()
        if it >= WARM:
            dm.append(d), hm.append(h)
    kern = []
    _check(L.cc_split_device_timing(1, None))
    for it in range(TIMED):
        dev_merge()
        ms = (C.c_float * 3)()
        _check(L.cc_split_device_timing(1, ms))
        kern.append(list(ms))
    _check(L.cc_split_device_timing(0, None))
    mpar = bool(np.array_equal(host_view(dst), hst) and np.array_equal(host_view(dva), hva)
                and np.array_equal(hva, getattr(b, val)) and np.array_equal(hst, (b.a & 0xFF).astype(np.uint8)))
    mb = merge_bytes_per_row()
    out.update({
        "merge_bytes_per_row": mb,
        "device_merge": dict(rates(med(dm), n, mb["total"]), all_ms=[round(x, 4) for x in dm],
                             what="events around the call: count, scan, the host wait, gather"),
        "device_merge_kernels_ms": {
            "k_split_count": {"ms": round(med([k[0] for k in kern]), 4), "all_ms": [round(k[0], 4) for k in kern]},
            "k_split_scan": {"ms": round(med([k[1] for k in kern]), 4), "all_ms": [round(k[1], 4) for k in kern]},
            "k_merge_gather": dict(rates(med([k[2] for k in kern]), n, mb["gather"]), all_ms=[round(k[2], 4) for k in kern])},
        "host_merge": {"ms": round(med(hm), 3), "all_ms": [round(x, 3) for x in hm],
                       "rows_per_s": round(n / (med(hm) * 1e-3), 1)},
        "merge_parity": mpar})
    print(json.dumps({k: out[k] for k in ("label", "split_parity", "merge_parity")} |
                     {"device_split_ms": out["device_split"]["ms"], "host_split_ms": out["host_split"]["ms"],
                      "device_merge_ms": out["device_merge"]["ms"], "host_merge_ms": out["host_merge"]["ms"]}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=100e6)
    ap.add_argument("--out", default=os.path.join("profiles", "split_gpu", "rate.json"))
    args = ap.parse_args()
    import torch

    from copycat_amd.workload import atomic_long_stream

    if not torch.cuda.is_available():
        sys.exit("split_rate.py measures on the GPU: no device found")
    n = int(args.rows)
    threads = shard._threads(0)
    all_cols = tuple(Batch.__slots__)
    results = []
    for world, names, label in ((8, all_cols, "world 8, every column"), (2, all_cols, "world 2, every column"),
                                (8, ("inst", "op", "flags", "a", "b"), "world 8, the c2 value batch's columns")):
        b = atomic_long_stream(n, 65536 * world)  # (bench.py global_log_split's log for this world)
        results.append(setting(b, world, names, threads, label))
        del b
        torch.cuda.empty_cache()
    parity = all(r["split_parity"] and r["merge_parity"] for r in results)
    doc = {"script": "scripts/split_rate.py", "rows": n, "device": torch.cuda.get_device_name(0),
           "warmups": WARM, "timed_calls": TIMED, "reference_rates_TBps": {"measured_copy": COPY_TBPS, "hbm_peak": PEAK_TBPS},
           "expectation_from_bytes_ms": {"split_every_column": round(n * split_bytes_per_row(all_cols)["total"] / (COPY_TBPS * 1e12) * 1e3, 3),
                                         "merge": round(n * merge_bytes_per_row()["total"] / (COPY_TBPS * 1e12) * 1e3, 3)},
           "settings": results, "parity": parity}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out, "parity": parity}))
    sys.exit(0 if parity else 1)


if __name__ == "__main__":
    main()
