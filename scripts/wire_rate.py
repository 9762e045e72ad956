#!/usr/bin/env python3
"""Decode rate of the Catalyst log: cc_wire_decode on one host thread against cc_wire_decode_to_device (k_wire_decode).

The stream is c2-shaped: `--rows` InstanceCommand{CompareAndSet(expect Long, update Long)} entries of 34 bytes each over
`--instances` open instances, built vectorised in numpy (2 B top id, 8 B instance id, 2 B op id, 2 x (3 B Long id + 8 B
value), big-endian, the default codec).  Every entry is plain, so no row escapes to the host.  The device columns of the
first call are checked against the host decoder's before anything is timed.

Reports, as one JSON line (also written to --out): cc_wire_decode rows/s on one thread of this machine's CPU; the new
call's total time (host wall clock around the synchronous call: offsets scan, H2D from pageable memory, kernel, escape
count back); its H2D, kernel and escape round trip from HIP events (cc_wire_timeline); and the kernel's bytes/s over
its algorithmic bytes (entry bytes + 8 B offset + 38 B of columns per row).  Median of --steps calls after --warmup.

    python scripts/wire_rate.py [--rows 16777216] [--instances 65536] [--steps 5] [--warmup 2] [--out FILE]

--strings: the device String dictionary (cc_wire_dict_attach).  `--rows` MapCommands.Put entries of 53 bytes: a String
key of 16 bytes drawn uniformly from `--keys` keys, a Long value, a ttl.  Two decoders on one engine hold the same
Strings in two interners; one is attached as the dictionary, the other is not, and a call that passes an interner other
than the attached one decodes as an unattached engine does (every row escapes to the host decoder: the behaviour before
the dictionary).  After the parity check against cc_wire_decode the two are timed alternately in one run; one JSON line
is appended to profiles/wire_gpu/rate_strings.json.

--plain-ab: the default all-plain leg on the same engine through the attached and through the other decoder,
alternating, --steps timed calls each: the attach must not move the plain kernel's time beyond the spread (max - min)
of the unattached repeats.  One JSON line, profiles/wire_gpu/rate_plain_ab.json.

--pipeline: cc_apply_wire_host against cc_apply_wire_host_packed on the default segment, every host buffer page-locked,
on one engine pair (the serial call on one, the pipelined call on the other, both fed the same rows).  The two are
called alternately, --steps timed calls each after --warmup; after every pair the unpacked results equal the serial
call's rows, and at the end the two engines' values and applied indices are equal.  The pipelined call runs at the
default chunk_rows and, as a second setting reported beside it, at --chunk-rows (default 2 Mi): one JSON line with both
medians, the ratios and the per-chunk timeline (H2D, decode, apply, encode, D2H), profiles/wire_gpu/rate_pipeline.json.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ENTRY = 34


def cas_stream(n, instances, id_first, seed=0xCA5):
    from copycat_amd import abi

    rng = np.random.default_rng(seed)
    e = np.zeros((n, ENTRY), np.uint8)
    e[:, 0:2] = (1, 30)
    e[:, 2:10] = (id_first + rng.integers(0, instances, n, dtype=np.uint64)).astype(">u8").view(np.uint8).reshape(n, 8)
    e[:, 10:12] = (1, abi.CC_OP_VALUE_CAS)
    for at in (12, 23):
        e[:, at:at + 3] = (2, abi.CC_WIRE_ID_LONG >> 8, abi.CC_WIRE_ID_LONG & 255)
        e[:, at + 3:at + 11] = rng.integers(0, 1 << 20, n, dtype=np.uint64).astype(">u8").view(np.uint8).reshape(n, 8)
    return e.reshape(-1), np.arange(n + 1, dtype=np.uint64) * ENTRY


SENTRY, SKEY = 53, 16


def put_stream(n, instances, id_first, keys, seed=0x57A):
    """n MAP_PUT entries (String key, Long value, ttl) under the default codec -> (bytes, offsets, the keys' bytes)"""
    from copycat_amd import abi

    rng = np.random.default_rng(seed)
    k = np.arange(keys, dtype=np.uint64)
    table = np.zeros((keys, SKEY), np.uint8)
    table[:, :4] = np.frombuffer(b"key-", np.uint8)
    for d in range(12):
        table[:, 4 + d] = 48 + (k // np.uint64(10 ** (11 - d))) % np.uint64(10)
    e = np.zeros((n, SENTRY), np.uint8)
    e[:, 0:2] = (1, 30)
    e[:, 2:10] = (id_first + rng.integers(0, instances, n, dtype=np.uint64)).astype(">u8").view(np.uint8).reshape(n, 8)
    e[:, 10:12] = (1, abi.CC_OP_MAP_PUT)
    e[:, 12:18] = (2, abi.CC_WIRE_ID_STRING >> 8, abi.CC_WIRE_ID_STRING & 255, 1, 0, SKEY)
    e[:, 18:34] = table[rng.integers(0, keys, n)]
    e[:, 34:37] = (2, abi.CC_WIRE_ID_LONG >> 8, abi.CC_WIRE_ID_LONG & 255)
    e[:, 37:45] = rng.integers(0, 1 << 20, n, dtype=np.uint64).astype(">u8").view(np.uint8).reshape(n, 8)
    return e.reshape(-1), np.arange(n + 1, dtype=np.uint64) * SENTRY, table


def same_columns(db, iid, bh, iidh):
    import torch

    ok = True
    for name in ("inst", "op", "flags", "key", "a", "b", "aux"):
        t = db.cols[name]
        got = t.view({8: torch.int64, 4: torch.int32, 1: torch.uint8}[t.element_size()]).cpu().numpy()
        ok = ok and np.array_equal(got.view(getattr(bh, name).dtype), getattr(bh, name))
    return ok and np.array_equal(iid.view(torch.int64).cpu().numpy().view(np.uint64), iidh)


def timed(E, D, buf, offs):
    import torch

    torch.cuda.synchronize()
    t = time.perf_counter()
    _, _, _, stats = D.decode_to_device(buf=buf, offsets=offs)
    return (time.perf_counter() - t) * 1e3, E.wire_timeline(), stats


def strings_leg(args):
    import torch

    from copycat_amd import abi
    from copycat_amd.engine import Engine
    from copycat_amd.wire import Interner, WireDecoder

    n, R, K = args.rows, args.instances, args.keys
    E = Engine(R, R, max(n, R), device=0)
    E.resource_create_range(0, R, abi.CC_RES_VALUE)  # (the decode resolves instance ids, whatever their resource)
    E.instance_open_range(0, R, 0, 1000, 7)
    if args.strings:
        buf, offs, table = put_stream(n, R, 1000, K)
    else:
        buf, offs = cas_stream(n, R, 1000)
        table = put_stream(1, 1, 0, K)[2]
    att, oth = WireDecoder(E, Interner(1)), WireDecoder(E, Interner(1))
    t = time.perf_counter()
    for row in table:
        b = row.tobytes()
        att.interner.intern(b)
        oth.interner.intern(b)
    intern_s = time.perf_counter() - t
    t = time.perf_counter()
    bh, iidh, kindh = oth.decode(buf=buf, offsets=offs)  # (registers every key's String.hashCode on the engine)
    host_s = time.perf_counter() - t
    att.attach_dictionary()
    db, iid, kind, st0 = att.decode_to_device(buf=buf, offsets=offs)
    ok = same_columns(db, iid, bh, iidh) and not kind.any()
    del db, iid
    db, iid, kind, st1 = oth.decode_to_device(buf=buf, offsets=offs)
    ok = ok and same_columns(db, iid, bh, iidh) and not kind.any()
    del db, iid, bh, iidh, kindh
    runs = {"attached": [], "unattached": []}
    for k in range(args.warmup + args.steps):
        for name, D in (("unattached", oth), ("attached", att)):
            r = timed(E, D, buf, offs)
            if k >= args.warmup:
                runs[name].append(r)
    med = statistics.median
    info = att.dictionary_info()
    out = {"workload": ("MapCommands.Put entries, a 16-byte String key, a Long value, a ttl" if args.strings
                        else "c2-shaped CompareAndSet entries, all plain"),
           "rows": n, "instances": R, "keys": K, "entry_bytes": SENTRY if args.strings else ENTRY,
           "parity_with_cc_wire_decode": bool(ok), "host_cc_wire_decode_s": round(host_s, 3),
           "host_cc_wire_decode_rows_per_s_one_thread": n / host_s, "intern_s": round(intern_s, 3),
           "dictionary": info, "table_bytes": info["cells"] * 32, "steps": args.steps, "gpu": torch.cuda.get_device_name(0)}
    for name, rs in runs.items():
        out[name] = {"call_ms": round(med(r[0] for r in rs), 3), "call_ms_min": round(min(r[0] for r in rs), 3),
                     "call_ms_max": round(max(r[0] for r in rs), 3), "h2d_ms": round(med(r[1][0] for r in rs), 3),
                     "kernel_ms": round(med(r[1][1] for r in rs), 4),
                     "kernel_ms_all": [round(r[1][1], 4) for r in rs],
                     "escape_round_trip_ms": round(med(r[1][2] for r in rs), 3),
                     "host_rows": rs[-1][2]["host_rows"], "device_rows": rs[-1][2]["device_rows"]}
    a, u = out["attached"], out["unattached"]
    out["attached_over_unattached_call"] = round(a["call_ms"] / u["call_ms"], 4)
    out["attached_kernel_within_its_h2d"] = bool(a["kernel_ms"] <= a["h2d_ms"])
    spread = max(u["kernel_ms_all"]) - min(u["kernel_ms_all"])
    out["unattached_kernel_spread_ms"] = round(spread, 4)
    out["kernel_median_difference_ms"] = round(abs(a["kernel_ms"] - u["kernel_ms"]), 4)
    if args.strings:
        ok = ok and a["host_rows"] == 0 and a["call_ms"] < u["call_ms"]
        if K <= 1024:  # the kernel's own bar, with the table in L2: the H2D of its input
            ok = ok and out["attached_kernel_within_its_h2d"]
    else:
        out["plain_kernel_within_spread"] = bool(out["kernel_median_difference_ms"] <= spread)
        ok = ok and out["plain_kernel_within_spread"]
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
    return 0 if ok else 1


def pipeline_leg(args):
    import ctypes as C

    import torch

    from copycat_amd import abi
    from copycat_amd.batch import Batch, _aligned_bytes, pack, pack_bound, results_bound, unpack_results
    from copycat_amd.engine import Engine, host_register
    from copycat_amd.wire import Interner, WireDecoder

    n, R = args.rows, args.instances
    buf, offs = cas_stream(n, R, 1000)
    engines = []
    for _ in range(2):
        E = Engine(R, R, max(n, R), device=0)
        E.resource_create_range(0, R, abi.CC_RES_VALUE)
        E.instance_open_range(0, R, 0, 1000, 7)
        engines.append((E, WireDecoder(E, Interner(1))))
    (Es, Ds), (Ep, Dp) = engines
    status, value = np.zeros(n, np.uint8), np.zeros(n, np.uint64)
    index = np.zeros(n, np.uint64)
    res, aux = _aligned_bytes(results_bound(n)), _aligned_bytes(pack_bound(n, columns=("index",)))
    for a in (buf, offs, status, value, index, res, aux):
        host_register(a)
    r = abi.cc_results(status.ctypes.data, value.ctypes.data)
    applied, ctl = C.c_uint64(), abi.cc_wire_control()
    calls = 0

    def next_index():
        nonlocal calls
        index[:] = np.arange(1 + calls * n, 1 + (calls + 1) * n, dtype=np.uint64)
        calls += 1
        b = Batch(0)
        b.index = index
        b.op = index  # (only its length is read)
        return pack(b, columns=("index",), out=aux)

    def serial():
        torch.cuda.synchronize()
        t = time.perf_counter()
        rc = Es.L.cc_apply_wire_host(Es.h, C.byref(Ds.codec), Ds.interner.h, buf.ctypes.data, buf.size, offs.ctypes.data, n,
                                     index.ctypes.data, None, C.byref(r), None, C.byref(applied), C.byref(ctl))
        dt = (time.perf_counter() - t) * 1e3
        assert rc == 0 and applied.value == n, (rc, applied.value)
        return dt

    def piped(blob, chunk_rows):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = Ep.apply_wire_host_packed(Dp, None, buf=buf, offsets=offs, aux=blob, chunk_rows=chunk_rows, events=False,
                                        out=res, timeline=True)
        dt = (time.perf_counter() - t) * 1e3
        assert out[3] == n and out[4] is None, out[3:]
        return dt, out[0], Ep.wire_packed_timeline()

    settings = (("default", 0), (f"chunk_rows_{args.chunk_rows}", args.chunk_rows))
    runs = {"serial": []}
    ok = True
    for k in range(args.warmup + args.steps):
        for name, chunk_rows in settings:
            blob = next_index()
            ts = serial()
            tp, rblob, tl = piped(blob, chunk_rows)
            s2, v2 = unpack_results(rblob)
            ok = ok and np.array_equal(s2, status) and np.array_equal(v2, value)
            if k >= args.warmup:
                runs["serial"].append(ts)
                runs.setdefault(name, []).append((tp, tl, int(rblob.nbytes)))
    ok = ok and Es.applied_index() == Ep.applied_index() == calls * n
    ok = ok and all(np.array_equal(x, y) for x, y in zip(Es.value_state(), Ep.value_state()))
    med = statistics.median
    out = {"workload": "c2-shaped CompareAndSet entries, all plain, decoded and applied", "rows": n, "instances": R,
           "entry_bytes": ENTRY, "results_and_state_equal": bool(ok), "steps": args.steps,
           "serial_call_ms": round(med(runs["serial"]), 3), "serial_call_ms_all": [round(x, 3) for x in runs["serial"]],
           "serial_result_bytes": 9 * n, "gpu": torch.cuda.get_device_name(0)}
    for name, _ in settings:
        rs = runs[name]
        tl = rs[-1][1]
        out[name] = {"call_ms": round(med(x[0] for x in rs), 3), "call_ms_all": [round(x[0], 3) for x in rs],
                     "over_serial": round(med(x[0] for x in rs) / med(runs["serial"]), 4), "chunks": int(len(tl)),
                     "result_blob_bytes": rs[-1][2], "h2d_ms_sum": round(float(tl[:, 0].sum()), 3),
                     "call_over_h2d_sum": round(med(x[0] for x in rs) / max(float(tl[:, 0].sum()), 1e-9), 3),
                     "timeline_ms_h2d_decode_apply_encode_d2h": [[round(float(x), 3) for x in row] for row in tl]}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--strings", action="store_true")
    ap.add_argument("--plain-ab", action="store_true")
    ap.add_argument("--pipeline", action="store_true")
    ap.add_argument("--chunk-rows", type=int, default=2 << 20)
    ap.add_argument("--keys", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=1 << 24)
    ap.add_argument("--instances", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    name = ("rate_strings.json" if args.strings else "rate_plain_ab.json" if args.plain_ab
            else "rate_pipeline.json" if args.pipeline else "rate.json")
    args.out = args.out or os.path.join(os.path.dirname(HERE), "profiles", "wire_gpu", name)
    sys.path.insert(0, os.path.dirname(HERE))
    if args.strings or args.plain_ab:
        return strings_leg(args)
    if args.pipeline:
        return pipeline_leg(args)
    import torch

    from copycat_amd import abi
    from copycat_amd.engine import Engine
    from copycat_amd.wire import Interner, WireDecoder

    n, R = args.rows, args.instances
    E = Engine(R, R, max(n, R), device=0)
    E.resource_create_range(0, R, abi.CC_RES_VALUE)
    E.instance_open_range(0, R, 0, 1000, 7)
    buf, offs = cas_stream(n, R, 1000)
    D = WireDecoder(E, Interner(1))

    host_s = []
    for k in range(2):  # the host decoder, one thread (twice: the first call also faults its output pages in)
        t = time.perf_counter()
        bh, iidh, kindh = D.decode(buf=buf, offsets=offs)
        host_s.append(time.perf_counter() - t)
    db, iid, kind, stats = D.decode_to_device(buf=buf, offsets=offs)
    ok = stats == {"rows": n, "device_rows": n, "host_rows": 0} and not kind.any()
    for name in ("inst", "op", "flags", "key", "a", "b", "aux"):
        t = db.cols[name]
        got = t.view({8: torch.int64, 4: torch.int32, 1: torch.uint8}[t.element_size()]).cpu().numpy()
        ok = ok and np.array_equal(got.view(getattr(bh, name).dtype), getattr(bh, name))
    ok = ok and np.array_equal(iid.view(torch.int64).cpu().numpy().view(np.uint64), iidh)
    del db, iid

    total, stage = [], []
    for k in range(args.warmup + args.steps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        D.decode_to_device(buf=buf, offsets=offs)
        dt = (time.perf_counter() - t) * 1e3
        if k >= args.warmup:
            total.append(dt)
            stage.append(E.wire_timeline())
    med = statistics.median
    h2d, kern, esc = (med(s[i] for s in stage) for i in range(3))
    kbytes = n * (ENTRY + 8 + 38)
    out = {"workload": "c2-shaped CompareAndSet entries, all plain", "rows": n, "instances": R, "entry_bytes": ENTRY,
           "parity_with_cc_wire_decode": bool(ok),
           "host_cc_wire_decode_rows_per_s_one_thread": n / min(host_s), "host_cc_wire_decode_s": round(min(host_s), 3),
           "device_call_ms_total": round(med(total), 3), "device_call_ms_min": round(min(total), 3),
           "device_call_ms_max": round(max(total), 3), "device_call_rows_per_s": n / (med(total) / 1e3),
           "h2d_ms": round(h2d, 3), "h2d_bytes": int(n * ENTRY + 8 * (n + 1)),
           "h2d_gb_per_s": round((n * ENTRY + 8 * (n + 1)) / (h2d * 1e-3) / 1e9, 2),
           "kernel_ms": round(kern, 3), "kernel_algorithmic_bytes": int(kbytes),
           "kernel_gb_per_s": round(kbytes / (kern * 1e-3) / 1e9, 1), "kernel_rows_per_s": n / (kern * 1e-3),
           "escape_round_trip_ms": round(esc, 3), "kernel_longer_than_its_h2d": bool(kern > h2d),
           "steps": args.steps, "gpu": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
