#!/usr/bin/env python3
"""Event rate of a message-bus stream: MessageBusState register / unregister fan-outs (k_apply_coord + k_topic_fanout),
to be read beside scripts/topic_rate.py's topic line at L = M, which goes through the same expansion kernel.

`--buses` buses of M members each (instances 0 .. M - 1 of a bus join before step 0, with 5 addresses among them, and
never leave).  A step's rows pick a bus at random: 98 % are the bus's next register / unregister row — pair p of a bus is
register then unregister of topic 1 + (p // M) % 8 by member p % M, so a bus holds at most one registration and up to 8
emptied topics — 1 % are a join and 1 % a leave of one of two more instances, taken in turn, so a bus has M to M + 2
members.  Every register and every unregister that finds its registration publishes to every member; a join returns its
Map rows.  Rows per step: enough for 100M events (--rows overrides).  Every step's rows are uploaded first; a step is
one cc_apply_batch on the resident columns with a device event stream, plus the final sync, host wall clock.  Step 0 is
gated and not timed: on a sample of buses every status, value, event per target and result row per joiner against the
Python restatement (tests/bus_model.py), and every row of the batch written.  Then 2 warm-up steps (the second one
under cc_profile, for the per-kernel times) and 5 timed steps.

Prints one JSON line: events/s and rows/s (median step, with the fastest and the slowest) and the per-kernel times.

    python scripts/bus_rate.py --members 8 [--buses 4096] [--rows N] [--steps 5] [--warmup 2] [--no-gate]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TOPICS, ADDRS = 8, 5


def bus_rows(step, n, buses, M, seq, index0):
    """seq[b] = register / unregister rows bus b has had (carried from step to step)"""
    from copycat_amd import abi
    from copycat_amd.batch import Batch

    rng = np.random.default_rng(0xB05 + step)
    b = Batch(n)
    b.index[:] = np.arange(index0, index0 + n, dtype=np.uint64)
    g = rng.integers(0, buses, n, dtype=np.int64)
    u = rng.random(n)
    pair = u < 0.98
    # rank of each pair row among its bus's pair rows of this step
    idx = np.nonzero(pair)[0]
    order = idx[np.argsort(g[idx], kind="stable")]
    gs = g[order]
    first = np.r_[0, np.nonzero(np.diff(gs))[0] + 1] if len(gs) else np.zeros(0, np.int64)
    rank = np.arange(len(gs)) - np.repeat(first, np.diff(np.r_[first, len(gs)]))
    j = np.zeros(n, np.int64)
    j[order] = seq[gs] + rank
    np.add.at(seq, g[idx], 1)
    p = j // 2
    rot = M + (np.arange(n, dtype=np.int64) + step * n) % 2  # instances M, M + 1 come and go
    b.op[:] = np.where(pair, np.where(j % 2 == 0, abi.CC_OP_BUS_REGISTER, abi.CC_OP_BUS_UNREGISTER),
                       np.where(u < 0.99, abi.CC_OP_BUS_JOIN, abi.CC_OP_BUS_LEAVE))
    b.inst[:] = np.where(pair, p % M, rot) * buses + g  # instance k of bus r sits in slot k * buses + r
    b.a[:] = np.where(pair, 1 + (p // M) % TOPICS, np.where(u < 0.99, 600 + rot, 0)).astype(np.uint64)
    b.flags[:] = np.where(b.op == abi.CC_OP_BUS_LEAVE, 0, abi.cc_flags(abi.CC_TAG_HANDLE)).astype(np.uint8)
    return b


def gate(b, status, value, ev, buses, M):
    from copycat_amd import abi
    from tests.bus_model import BusWorld

    K = M + 2
    sample = np.arange(0, buses, max(1, buses // 16))
    W = BusWorld()
    for r in sample.tolist():
        W.create(r)
        for k in range(K):
            W.open(k * buses + r, r, 1000 + k * buses + r, 7 + k)
            if k < M:
                W.buses[r].join(1000 + k * buses + r, 1 + k * buses + r, 500 + k % ADDRS)
    sel = np.nonzero(np.isin(b.inst % buses, sample))[0]
    sub = b.slice(0, len(sel))
    for name in ("index", "inst", "op", "flags", "a"):
        getattr(sub, name)[:] = getattr(b, name)[sel]
    res, mev, mrows = W.apply(sub)
    ok = all((int(status[sel[i]]), int(value[sel[i]])) == sv for i, sv in res.items()) and len(res) == len(sel)
    back = {int(r): i for i, r in enumerate(sel.tolist())}  # batch row -> row of the sampled sub-stream
    m = np.isin(ev["target"] % buses, sample)
    fan = m & np.isin(ev["code"], (abi.CC_EV_BUS_REGISTER, abi.CC_EV_BUS_UNREGISTER))
    rows = m & (ev["src"] == abi.CC_EVSRC_RESULT)
    ok &= bool((fan | rows)[m].all())
    got, want = {}, {}
    for p, t, c, pl in zip(ev["pos"][fan].tolist(), ev["target"][fan].tolist(), ev["code"][fan].tolist(), ev["payload"][fan].tolist()):
        got.setdefault(t, []).append((back[p], c, pl))
    for i, t, c, _, pl in mev:
        want.setdefault(t, []).append((i, c, pl))
    ok &= got == want
    grow = {}
    for p, t, c, pl in zip(ev["pos"][rows].tolist(), ev["target"][rows].tolist(), ev["code"][rows].tolist(), ev["payload"][rows].tolist()):
        grow.setdefault(back[p], []).append((c, pl))
    ok &= grow == {i: rr for i, rr in mrows.items() if rr}
    return bool(ok)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--members", type=int, default=8)
    ap.add_argument("--buses", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-gate", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(HERE))
    import torch

    from copycat_amd import abi
    from copycat_amd.batch import Batch
    from copycat_amd.engine import RESULT_SENTINEL, DeviceBatch, DeviceEvents, Engine

    M, R = args.members, args.buses
    n = args.rows or int(100e6 / (0.98 * M)) + 1
    K = M + 2
    sub = min(1 << 22, -(-n // 16384) * 16384)
    bound = M + 2  # events a fan-out row can publish (a join's rows, at most 2 x 9, are 1 % of the stream)
    dev = torch.device("cuda:0")
    E = Engine(R, R * K, max(n, R * K), device=dev.index, flags=abi.CC_CFG_TIMERS_DEFERRED, sub_batch=sub,
               max_events=sub * bound + 1024, coord_cap=max(64, 1 << (M + 2 + TOPICS + 1).bit_length()))
    E.resource_create_range(0, R, abi.CC_RES_BUS)
    for k in range(K):  # instance k of bus r sits in slot k * R + r
        E.instance_open_range(k * R, R, 0, 1000 + k * R, 7 + k)
    s0 = Batch(R * M)  # before step 0: every bus's instances 0 .. M - 1 join
    s0.index[:] = np.arange(1, R * M + 1, dtype=np.uint64)
    s0.inst[:] = np.arange(R * M)
    s0.op[:] = abi.CC_OP_BUS_JOIN
    s0.flags[:] = abi.cc_flags(abi.CC_TAG_HANDLE)
    s0.a[:] = 500 + (np.arange(R * M) // R) % ADDRS
    E.apply_host_events(s0, capacity=1024)
    index0 = R * M + 1
    total = args.warmup + args.steps + 1
    seq = np.zeros(R, np.int64)
    dbs, host0 = [], None
    for k in range(total):
        b = bus_rows(k, n, R, M, seq, index0)
        index0 += n
        dbs.append(DeviceBatch.upload(b, device=dev))
        if k == 0:
            host0 = b
    status = torch.full((n,), RESULT_SENTINEL, dtype=torch.uint8, device=dev)
    value = torch.zeros((n,), dtype=torch.int64, device=dev)
    evs = DeviceEvents(n * bound + 1024, device=dev)
    ok, ms, counts, prof = None, [], [], {}
    for k in range(total):
        profiled = k == args.warmup
        if profiled:
            E.profile(True)
        torch.cuda.synchronize()
        t = time.perf_counter()
        E.apply_events(dbs[k], status, value, evs)
        E.sync()
        dt = (time.perf_counter() - t) * 1e3
        cnt = int(evs.count.item())
        if profiled:
            prof = E.profile_read()
            E.profile(False)
        if not args.no_gate and k == 0:
            ok = gate(host0, status.cpu().numpy(), value.cpu().numpy().view(np.uint64), evs.host(), R, M)
        if k > args.warmup:
            ms.append(dt)
            counts.append(cnt)
    written = bool((status != RESULT_SENTINEL).all().item())
    med = statistics.median(ms)
    mev = statistics.median(counts)
    out = {"workload": "bus_register_unregister_fanout", "members": M, "resources": R, "rows": n, "steps": args.steps,
           "events_per_step": mev, "events_per_s": mev / (med / 1e3), "rows_per_s": n / (med / 1e3),
           "ms_per_step": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "gate": ok,
           "all_rows_written": written, "gpu": torch.cuda.get_device_name(0)}
    for name, (t_ms, launches) in prof.items():
        if launches:
            out[name + "_ms_per_step"] = round(t_ms, 3)
    print(json.dumps(out))
    return 0 if ok is not False and written else 1


if __name__ == "__main__":
    sys.exit(main())
