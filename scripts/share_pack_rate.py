"""Time of the packed blobs on the device (cc_pack_from_device, cc_respack_to_device, cc_evpack_to_device;
copycat_amd/csrc/pack_enc.hip, unpack_res.hip) beside the wide PCIe copies they replace, in the same process
(DESIGN.md §4.13.1).

Workload: one share of bench.py's global c2 log (atomic_long_stream, N rows over 8 x 65,536 resources, owner = slot % 8,
rank 0's share, the c2 value batch's columns index / inst / op / flags / a / b: 30 B per row wide); that share's real
results (an engine applies the share's blob); and rank 0's event stream of scripts/evmerge_rate.py (c5-like: 0.25
events per row).  Three comparisons, the legs of each alternating, 2 warm-ups and the median of 7 timed calls, device
events around each leg:
  1. cc_pack_from_device                            against a wide D2H of the same six columns into pinned memory;
  2. cc_pack_from_device                            against that wide D2H followed by cc_pack_batch on 16 threads;
  3. cc_respack_to_device + cc_evpack_to_device     against cc_respack_unpack + cc_evpack_unpack on 16 threads followed by
                                                    a wide H2D of the eight columns from pinned memory.
Blobs and wide host columns are page-locked.  A plain D2H / H2D of the blob's bytes alone is timed too: what a packed
call takes beyond it is its kernels, its staging and its synchronisation.  After the timed calls the device encoder's
blob is compared with cc_pack_batch's and every decoded device column with the host decoder's, in full; any difference
makes the exit status nonzero.

Usage: python scripts/share_pack_rate.py [--rows N] [--out profiles/share_pack/rate.json]
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
from copycat_amd.batch import (Batch, _aligned_bytes, events_bound, pack, pack_bound, pack_events,  # noqa: E402
                               results_bound, unpack_events, unpack_results)

WORLD = 8
VALUE_COLS = ("index", "inst", "op", "flags", "a", "b")
WARM, TIMED = 2, 7
THREADS = 16
NPDT = {"u4": np.uint32, "u1": np.uint8, "u8": np.uint64}


def med(xs):
    return float(np.median(xs))


def leg(ms, nbytes=None):
    out = {"ms": round(med(ms), 4), "all_ms": [round(x, 4) for x in ms]}
    if nbytes is not None:
        out["bytes"] = int(nbytes)
        out["GBps"] = round(nbytes / (med(ms) * 1e-3) / 1e9, 2)
    return out


def pinned(a):
    from copycat_amd.engine import host_register

    host_register(a)
    return a


def alternate(*legs):
    """[[ms of the timed calls] per leg]: one call of every leg per round, 2 warm-up rounds and 7 timed ones"""
    out = [[] for _ in legs]
    for it in range(WARM + TIMED):
        for k, f in enumerate(legs):
            ms = f()
            if it >= WARM:
                out[k].append(ms)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=100e6)
    ap.add_argument("--out", default=os.path.join("profiles", "share_pack", "rate.json"))
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("share_pack_rate.py measures on the GPU: no device found")
    from evmerge_rate import build as build_events

    from copycat_amd.engine import DeviceBatch, DeviceEvents, Engine
    from copycat_amd.workload import atomic_long_stream

    n_log = int(args.rows)
    R = 65536 * WORLD
    log = atomic_long_stream(n_log, R)
    mine = log.inst % WORLD == 0
    share = Batch.from_columns(**{name: getattr(log, name)[mine] for name in VALUE_COLS})
    del log, mine
    n = len(share)
    stream = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(f):
        def run():
            e0.record(stream)
            f()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)
        return run

    coord = Engine(16, 16, 4096)  # the coordinator's engine: staging and error store only
    # ---- 1, 2: the share out ---------------------------------------------------------------------------------------------
    db = DeviceBatch.upload(share, columns=VALUE_COLS)
    wide_bytes = sum(getattr(share, name).nbytes for name in VALUE_COLS)
    hwide = {name: pinned(np.empty_like(getattr(share, name))) for name in VALUE_COLS}
    hbatch = Batch.from_columns(**hwide)  # (the same arrays: what cc_pack_batch reads after the wide D2H)
    L = coord.L
    sp = C.c_void_p(stream.cuda_stream)

    def copy(dst, src, nbytes, kind):  # hipMemcpyAsync on the stream and its synchronisation (cc_memcpy)
        assert L.cc_memcpy(C.c_void_p(dst), C.c_void_p(src), nbytes, kind, sp) == abi.CC_OK

    blob_dev = pinned(_aligned_bytes(pack_bound(n, VALUE_COLS)))
    blob_host = pinned(_aligned_bytes(pack_bound(n, VALUE_COLS)))
    size = {}

    def pack_device():
        size["device"] = len(coord.batch_to_host_packed(db, out=blob_dev))

    def wide_d2h():
        for name in VALUE_COLS:
            copy(hwide[name].ctypes.data, db.cols[name].data_ptr(), hwide[name].nbytes, abi.CC_MEMCPY_D2H)

    def wide_d2h_then_host_pack():
        wide_d2h()
        size["host"] = len(pack(hbatch, columns=VALUE_COLS, threads=THREADS, out=blob_host))

    t_pack, t_wide, t_wide_pack = alternate(timed(pack_device), timed(wide_d2h), timed(wide_d2h_then_host_pack))
    encode_parity = bool(size["device"] == size["host"] and np.array_equal(blob_dev[:size["device"]], blob_host[:size["host"]])
                         and all(np.array_equal(hwide[name], getattr(share, name)) for name in VALUE_COLS))
    blob = blob_dev[:size["device"]]
    dblob = torch.empty(len(blob), dtype=torch.uint8, device="cuda")
    (t_blob_d2h,) = alternate(timed(lambda: copy(blob_host.ctypes.data, dblob.data_ptr(), len(blob), abi.CC_MEMCPY_D2H)))
    # ---- 3: the answers back ---------------------------------------------------------------------------------------------
    # the share's real results: rank 0's engine holds its 65,536 resources under local slots (global slot / 8)
    local = Batch.from_columns(**{name: getattr(share, name) for name in VALUE_COLS})
    local.inst = (share.inst // WORLD).astype(np.uint32)
    rank = Engine(R // WORLD, R // WORLD, 1 << 24, flags=abi.CC_CFG_TIMERS_DEFERRED)
    rank.resource_create_range(0, R // WORLD, abi.CC_RES_VALUE)
    rank.instance_open_range(0, R // WORLD, 0, 1000, 7)
    res_blob = pinned(_aligned_bytes(results_bound(n)))
    rblob, _, done = rank.apply_host_packed_results(pack(local, columns=VALUE_COLS, threads=THREADS), n, events=False,
                                                    out=res_blob)
    del local
    assert done == n
    rank.close()
    parts, _, _, _, _ = build_events(n_log, WORLD, 7 + WORLD)
    ev = parts[0]
    del parts
    m = len(ev["pos"])
    eblob = pack_events(ev, threads=THREADS, out=pinned(_aligned_bytes(events_bound(m))))
    dst = torch.empty(n, dtype=torch.uint8, device="cuda")
    dva = torch.empty(n, dtype=torch.int64, device="cuda")
    dev = DeviceEvents(m)
    hst, hva = pinned(np.empty(n, np.uint8)), pinned(np.empty(n, np.uint64))
    hev = {name: pinned(np.empty(m, NPDT[dt])) for name, dt in abi.EVENT_COLUMNS}
    dst2, dva2 = torch.empty_like(dst), torch.empty_like(dva)
    dev2 = DeviceEvents(m)
    hres = abi.cc_results(hst.ctypes.data, hva.ctypes.data)
    hcnt = np.zeros(1, np.uint64)
    hevs = abi.cc_events(*[hev[name].ctypes.data for name, _ in abi.EVENT_COLUMNS], m, hcnt.ctypes.data)
    wide_back = 9 * n + 19 * m
    host_ms = []

    def packed_in():
        coord.results_to_device(rblob, dst, dva)
        stream.synchronize()  # (the two decoders share one staging: the engine is synchronised between them)
        coord.events_to_device(eblob, dev)

    def host_unpack_then_wide_h2d():
        t0 = time.perf_counter()
        assert L.cc_respack_unpack(rblob.ctypes.data, rblob.nbytes, C.byref(hres), THREADS) == abi.CC_OK
        assert L.cc_evpack_unpack(eblob.ctypes.data, eblob.nbytes, C.byref(hevs), THREADS) == abi.CC_OK
        host_ms.append((time.perf_counter() - t0) * 1e3)
        wide_h2d()

    def wide_h2d():
        copy(dst2.data_ptr(), hst.ctypes.data, hst.nbytes, abi.CC_MEMCPY_H2D)
        copy(dva2.data_ptr(), hva.ctypes.data, hva.nbytes, abi.CC_MEMCPY_H2D)
        for name, _ in abi.EVENT_COLUMNS:
            copy(getattr(dev2, name).data_ptr(), hev[name].ctypes.data, hev[name].nbytes, abi.CC_MEMCPY_H2D)

    t_in, t_host_in = alternate(timed(packed_in), timed(host_unpack_then_wide_h2d))
    (t_wide_h2d,) = alternate(timed(wide_h2d))
    both = pinned(np.concatenate([rblob, eblob]))
    dboth = torch.empty(len(both), dtype=torch.uint8, device="cuda")
    (t_blob_h2d,) = alternate(timed(lambda: copy(dboth.data_ptr(), both.ctypes.data, len(both), abi.CC_MEMCPY_H2D)))
    rs, rv = unpack_results(rblob)
    rev = unpack_events(eblob)
    decode_parity = bool(np.array_equal(dst.cpu().numpy(), rs) and np.array_equal(dva.cpu().numpy().view(np.uint64), rv)
                         and int(dev.count.item()) == m
                         and all(np.array_equal(getattr(dev, name).cpu().numpy().view(NPDT[dt]), rev[name])
                                 for name, dt in abi.EVENT_COLUMNS)
                         and all(np.array_equal(rev[name], ev[name]) for name, _ in abi.EVENT_COLUMNS)
                         and np.array_equal(hst, rs) and np.array_equal(hva, rv))
    coord.close()
    parity = encode_parity and decode_parity
    doc = {
        "script": "scripts/share_pack_rate.py", "device": torch.cuda.get_device_name(0), "log_rows": n_log, "world": WORLD,
        "share_rows": n, "share_events": m, "warmups": WARM, "timed_calls": TIMED, "host_threads": THREADS,
        "what": "device events around each leg, legs alternating in one process; blobs and wide host columns page-locked; "
                "a plain copy is one hipMemcpyAsync per column on the stream, each with its synchronisation (cc_memcpy)",
        "share_out": {
            "columns": list(VALUE_COLS), "wide_bytes": int(wide_bytes), "wide_bytes_per_row": round(wide_bytes / n, 2),
            "blob_bytes": int(len(blob)), "blob_bytes_per_row": round(len(blob) / n, 2),
            "cc_pack_from_device": leg(t_pack),
            "wide_d2h": leg(t_wide, wide_bytes),
            "wide_d2h_then_cc_pack_batch_16_threads": leg(t_wide_pack),
            "d2h_of_the_blob_bytes_alone": leg(t_blob_d2h, len(blob)),
            "packed_call_over_wide_d2h": round(med(t_pack) / med(t_wide), 3),
            "packed_call_over_wide_d2h_then_host_pack": round(med(t_pack) / med(t_wide_pack), 3),
            "packed_call_beyond_its_d2h_ms": round(med(t_pack) - med(t_blob_d2h), 4),
        },
        "answers_back": {
            "wide_bytes": int(wide_back), "result_blob_bytes": int(len(rblob)), "event_blob_bytes": int(len(eblob)),
            "result_blob_bytes_per_row": round(len(rblob) / n, 2), "event_blob_bytes_per_event": round(len(eblob) / m, 2),
            "cc_respack_to_device_and_cc_evpack_to_device": leg(t_in),
            "host_unpack_16_threads_then_wide_h2d": leg(t_host_in),
            "host_unpack_alone": leg(host_ms[WARM:]),
            "wide_h2d_alone": leg(t_wide_h2d, wide_back),
            "h2d_of_the_blob_bytes_alone": leg(t_blob_h2d, len(both)),
            "packed_calls_over_wide_h2d": round(med(t_in) / med(t_wide_h2d), 3),
            "packed_calls_over_host_unpack_then_wide_h2d": round(med(t_in) / med(t_host_in), 3),
            "packed_calls_beyond_their_h2d_ms": round(med(t_in) - med(t_blob_h2d), 4),
        },
        "encode_parity": encode_parity, "decode_parity": decode_parity, "parity": parity,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out, "parity": parity, "share_rows": n, "events": m,
                      "pack_from_device_ms": doc["share_out"]["cc_pack_from_device"]["ms"],
                      "wide_d2h_ms": doc["share_out"]["wide_d2h"]["ms"],
                      "wide_d2h_then_host_pack_ms": doc["share_out"]["wide_d2h_then_cc_pack_batch_16_threads"]["ms"],
                      "packed_in_ms": doc["answers_back"]["cc_respack_to_device_and_cc_evpack_to_device"]["ms"],
                      "host_unpack_then_wide_h2d_ms": doc["answers_back"]["host_unpack_16_threads_then_wide_h2d"]["ms"],
                      "wide_h2d_ms": doc["answers_back"]["wide_h2d_alone"]["ms"]}))
    sys.exit(0 if parity else 1)


if __name__ == "__main__":
    main()
