#!/usr/bin/env python3
"""The PCIe-inclusive c2 step from host memory: wide columns (cc_apply_batch_host) against a packed blob
(cc_apply_batch_host_packed) against a packed blob in and a packed result blob out (cc_apply_batch_host_packed_results).

Three engines of one build get the same AtomicLongClients steps over 65,536 resources.  The baseline engine takes the six
wide columns (30 B per commit) from page-locked host memory through cc_apply_batch_host: the same code as before the
packed path existed, measured in the same run on the same box.  The other engine takes the step packed
(cc_pack_batch, --threads host threads, timed on its own) through cc_apply_batch_host_packed, blob and result rows
page-locked.  --warmup untimed steps, then --repeats timed steps per engine, interleaved; host wall clock around the
synchronous calls; medians with min / max.  Every step's results are compared between the two paths.  Per chunk of
every timed packed call the H2D, decode, apply and D2H times come from HIP events (CC_PACKED_TIMELINE).  Both paths
also run once from pageable memory.  The third engine takes the same blob through cc_apply_batch_host_packed_results
into a page-locked result blob (ms_packed_both; its baseline is ms_packed_call of the same run); the blob is decoded on
the host (cc_respack_unpack, --threads threads, timed on its own as ms_unpack_results) and compared with the other two
paths every step; per chunk its H2D, decode, apply, encode and D2H times come from HIP events, and
encode_over_d2h_saved is the largest encode time over the D2H time the chunk saves against the wide-result call of the
same step.  Prints one JSON line (and writes it to --out).

    python scripts/host_packed_e2e.py [--rows 100000000] [--warmup 2] [--repeats 7] [--threads 16] [--chunk-rows 0]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from copycat_amd import abi  # noqa: E402
from copycat_amd.batch import Batch, _aligned_bytes, pack, pack_bound, pack_info, results_bound, results_check  # noqa: E402
from copycat_amd.engine import RESULT_SENTINEL, Engine, _check, host_register, host_unregister  # noqa: E402
from copycat_amd.workload import SEED_C2, AtomicLongClients  # noqa: E402

COLS = ("index", "inst", "op", "flags", "a", "b")
R = 65536


def _ms(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def _stat(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}


def _engine(n):
    E = Engine(R, R, n, flags=abi.CC_CFG_TIMERS_DEFERRED)
    E.resource_create_range(0, R, abi.CC_RES_VALUE)
    E.instance_open_range(0, R, 0, 1, 1)
    return E


def _wide(E, b, status, value):
    s = abi.cc_batch()
    for name in COLS:
        setattr(s, name, getattr(b, name).ctypes.data)
    r = abi.cc_results(status.ctypes.data, value.ctypes.data)
    _check(E.L.cc_apply_batch_host(E.h, C.byref(s), len(b), C.byref(r)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--chunk-rows", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.rows
    clients = AtomicLongClients(resources=R, seed=SEED_C2, threads=args.threads)
    EW, EP, EB = _engine(n), _engine(n), _engine(n)
    host = Batch(n)
    blob_buf = _aligned_bytes(pack_bound(n, COLS))  # (below the bound cc_pack_batch sizes the blob first: a second pass)
    res = [(np.full(n, RESULT_SENTINEL, np.uint8), np.zeros(n, np.uint64)) for _ in range(2)]
    res_buf = _aligned_bytes(results_bound(n))
    ds, dv = np.zeros(n, np.uint8), np.zeros(n, np.uint64)  # the result blob decoded on the host
    pinned = [getattr(host, c) for c in COLS] + [blob_buf, res_buf] + [a for pair in res for a in pair]
    for a in pinned:
        host_register(a)
    (sw, vw), (sp, vp) = res
    ms = {"wide": [], "pack": [], "packed_call": [], "packed_both": [], "unpack_results": []}
    chunks, bytes_per_row = [], []
    chunks_both, result_bytes_per_row = [], []
    try:
        for step in range(args.warmup + args.repeats):
            clients.next(n, out=host)
            tw = _ms(lambda: _wide(EW, host, sw, vw))
            blob = None

            def do_pack():
                nonlocal blob
                blob = pack(host, columns=COLS, threads=args.threads, out=blob_buf)

            tp = _ms(do_pack)
            tc = _ms(lambda: EP.apply_host_packed(blob, n, events=False, chunk_rows=args.chunk_rows, out=(sp, vp),
                                                  timeline=True))
            assert np.array_equal(sw, sp) and np.array_equal(vw, vp), f"step {step}: the two paths' results differ"
            rblob = None

            def do_both():
                nonlocal rblob
                rblob = EB.apply_host_packed_results(blob, n, events=False, chunk_rows=args.chunk_rows, out=res_buf,
                                                     timeline=True)[0]

            tb = _ms(do_both)
            assert results_check(rblob) == n
            rr = abi.cc_results(ds.ctypes.data, dv.ctypes.data)
            tu = _ms(lambda: _check(EB.L.cc_respack_unpack(rblob.ctypes.data, rblob.nbytes, C.byref(rr), args.threads)))
            assert np.array_equal(sw, ds) and np.array_equal(vw, dv), f"step {step}: the decoded result blob differs"
            print(f"step {step}: wide {tw:.2f} pack {tp:.2f} packed_call {tc:.2f} packed_both {tb:.2f} "
                  f"unpack_results {tu:.2f} ms", file=sys.stderr, flush=True)
            if step >= args.warmup:
                ms["wide"].append(tw), ms["pack"].append(tp), ms["packed_call"].append(tc)
                ms["packed_both"].append(tb), ms["unpack_results"].append(tu)
                chunks.append(EP.packed_timeline().tolist())
                chunks_both.append(EB.packed_results_timeline().tolist())
                bytes_per_row.append(len(blob) / n)
                result_bytes_per_row.append(len(rblob) / n)
        last_info = pack_info(blob) if n <= (1 << 24) else None
        # once more from pageable memory: fresh copies nobody registered
        clients.next(n, out=host)
        cold = Batch(0)
        for name in COLS:
            setattr(cold, name, getattr(host, name).copy())
        cold_blob = pack(cold, columns=COLS, threads=args.threads)
        cs, cv = np.full(n, RESULT_SENTINEL, np.uint8), np.zeros(n, np.uint64)
        cs2, cv2 = cs.copy(), cv.copy()
        pageable = {"ms_wide": round(_ms(lambda: _wide(EW, cold, cs, cv)), 3),
                    "ms_packed_call": round(_ms(lambda: EP.apply_host_packed(cold_blob, n, events=False,
                                                                               chunk_rows=args.chunk_rows,
                                                                               out=(cs2, cv2))), 3)}
        assert np.array_equal(cs, cs2) and np.array_equal(cv, cv2), "pageable: the two paths' results differ"
    finally:
        for a in pinned:
            host_unregister(a)
    out = {"rows": n, "resources": R, "warmup": args.warmup, "repeats": args.repeats, "pack_threads": args.threads,
           "chunk_rows": args.chunk_rows or (16 << 20), "gpu": torch.cuda.get_device_name(0),
           "ms_wide": _stat(ms["wide"]), "ms_pack": _stat(ms["pack"]), "ms_packed_call": _stat(ms["packed_call"]),
           "bytes_per_row": round(statistics.median(bytes_per_row), 3), "wide_bytes_per_row": 30}
    out["packed_over_wide"] = round(out["ms_packed_call"]["median_ms"] / out["ms_wide"]["median_ms"], 4)
    out["pack_plus_call_over_wide"] = round((out["ms_pack"]["median_ms"] + out["ms_packed_call"]["median_ms"]) /
                                            out["ms_wide"]["median_ms"], 4)
    # per chunk of the median-time packed call: [H2D, decode, apply, D2H] ms; over every timed call: decode < H2D
    order = sorted(range(len(chunks)), key=lambda i: ms["packed_call"][i])
    out["chunks_ms_h2d_decode_apply_d2h"] = [[round(x, 3) for x in c] for c in chunks[order[len(order) // 2]]]
    out["decode_below_h2d_every_chunk"] = all(c[1] < c[0] for call in chunks for c in call)
    out["max_decode_over_h2d"] = round(max(c[1] / c[0] for call in chunks for c in call), 4)
    out["pageable"] = pageable
    # packed results: per chunk of the median-time call [H2D, decode, apply, encode, D2H] ms; over every timed call and
    # chunk, the encode time over the D2H time it saves against the wide-result call of the same step
    out["ms_packed_both"] = _stat(ms["packed_both"])
    out["ms_unpack_results"] = _stat(ms["unpack_results"])
    out["result_bytes_per_row"] = round(statistics.median(result_bytes_per_row), 3)
    out["wide_result_bytes_per_row"] = 9
    out["packed_both_over_packed_call"] = round(out["ms_packed_both"]["median_ms"] / out["ms_packed_call"]["median_ms"], 4)
    order = sorted(range(len(chunks_both)), key=lambda i: ms["packed_both"][i])
    out["chunks_ms_h2d_decode_apply_encode_d2h"] = [[round(x, 3) for x in c] for c in chunks_both[order[len(order) // 2]]]
    saved = [(cb[3], cw[3] - cb[4]) for wide_call, both_call in zip(chunks, chunks_both) for cw, cb in zip(wide_call, both_call)]
    out["encode_below_d2h_saved_every_chunk"] = all(d > 0 and e < d for e, d in saved)
    out["encode_over_d2h_saved"] = round(max(e / d for e, d in saved), 4) if all(d > 0 for _, d in saved) else None
    if last_info:
        out["columns_bytes_per_row"] = {k: v["bytes_per_row"] for k, v in last_info["columns"].items()}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
