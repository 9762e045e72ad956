#!/usr/bin/env python3
"""Event rate of a pub/sub stream: TopicState.publish fan-out (k_apply_coord + k_topic_fanout), and, with --group, the
membership-group join / leave fan-out (emitted serially by the walking lane) as the yardstick.

Topic mode: `--topics` topics with L listeners each (instances 0 .. L - 1 of a topic listen before step 0 and never
leave); a step's rows pick a topic at random and are 98 % publish (by a publisher instance that never listens), 1 %
listen and 1 % unlisten by one of two more instances, taken in turn, so a list holds L to L + 2 listeners.  Rows per step: enough for 100M events, or 10M
rows at L = 1 (--rows overrides).  Every step's rows are uploaded first; a step is one cc_apply_batch on the resident
columns with a device event stream, plus the final sync, host wall clock.  Step 0 is gated and not timed: every result
row void, the event count of every publish row against a vectorised count of the listeners at that row, and on a
sample of topics every event per target against the Python restatement (tests/topic_model.py).  Then 2 warm-up steps
(the second one under cc_profile, for k_topic_fanout's time) and 5 timed steps.

Group mode (--group): `--topics` groups of L members; rows pick a group at random and alternate leave / join of one
rotating member of it, each telling the L - 1 others (JOIN / LEAVE) and, for a join, returning the L MEMBER rows.  The
count of event rows written is checked against that formula.  It needs nothing this commit adds, so the same script
measures an older build: --root DIR imports the package from another checkout.

Prints one JSON line: events/s and rows/s (median step, with the fastest and the slowest), and in topic mode
k_topic_fanout's time per step and its bytes per event (24 written + 4 of the listener log + 24 per record read).

    python scripts/topic_rate.py --listeners 8 [--group] [--topics 4096] [--rows N] [--steps 5] [--warmup 2] [--no-gate]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def topic_rows(step, n, topics, L, index0):
    from copycat_amd import abi
    from copycat_amd.batch import Batch

    rng = np.random.default_rng(0x70B1C + step)
    b = Batch(n)
    b.index[:] = np.arange(index0, index0 + n, dtype=np.uint64)
    t = rng.integers(0, topics, n, dtype=np.int64)
    u = rng.random(n)
    pub = u < 0.98
    rot = L + 1 + (np.arange(n, dtype=np.int64) + step * n) % 2  # instances L + 1, L + 2 come and go
    b.op[:] = np.where(pub, abi.CC_OP_TOPIC_PUBLISH, np.where(u < 0.99, abi.CC_OP_TOPIC_LISTEN, abi.CC_OP_TOPIC_UNLISTEN))
    b.inst[:] = np.where(pub, L, rot) * topics + t  # instance k of topic t sits in slot k * topics + t (L publishes)
    b.flags[:] = abi.cc_flags(abi.CC_TAG_LONG)
    b.a[:] = b.index
    return b


def group_rows(n, groups, L, seq, index0, rng):
    """seq[g] = rows group g has had: row j of a group is leave (j even) / join (j odd) of member (j // 2) % L."""
    from copycat_amd import abi
    from copycat_amd.batch import Batch

    b = Batch(n)
    b.index[:] = np.arange(index0, index0 + n, dtype=np.uint64)
    g = rng.integers(0, groups, n, dtype=np.int64)
    order = np.argsort(g, kind="stable")
    gs = g[order]
    first = np.r_[0, np.nonzero(np.diff(gs))[0] + 1]
    rank = np.arange(n) - np.repeat(first, np.diff(np.r_[first, n]))
    j = np.empty(n, np.int64)
    j[order] = seq[gs] + rank
    np.add.at(seq, g, 1)
    b.op[:] = np.where(j % 2 == 0, abi.CC_OP_GROUP_LEAVE, abi.CC_OP_GROUP_JOIN)
    b.inst[:] = ((j // 2) % L) * groups + g
    events = int(np.where(j % 2 == 0, L - 1, 2 * L - 1).sum())
    return b, events


def listeners_at_rows(b, topics, L):
    """Listeners of each row's topic just before the row (step 0: instances 0 .. L - 1 listen at the start)."""
    from copycat_amd import abi

    n = len(b)
    t, k = b.inst.astype(np.int64) % topics, b.inst.astype(np.int64) // topics
    chg = np.nonzero(b.op != abi.CC_OP_TOPIC_PUBLISH)[0]
    o = chg[np.lexsort((chg, b.inst[chg]))]  # by (instance, row)
    want = (b.op[o] == abi.CC_OP_TOPIC_LISTEN).astype(np.int64)
    same = np.r_[False, b.inst[o][1:] == b.inst[o][:-1]]
    prev = np.where(same, np.r_[0, want[:-1]], (k[o] < L).astype(np.int64))  # the instance's state before the row
    delta = np.zeros(n, np.int64)
    delta[o] = want - prev
    order = np.lexsort((np.arange(n), t))
    ts = t[order]
    cs = np.cumsum(delta[order])
    first = np.r_[0, np.nonzero(np.diff(ts))[0] + 1]
    base = np.repeat(np.r_[0, cs[first[1:] - 1]], np.diff(np.r_[first, n]))
    before = np.empty(n, np.int64)
    before[order] = L + cs - delta[order] - base
    return before


def gate_topics(b, status, value, ev, topics, L):
    from copycat_amd import abi
    from tests.topic_model import TopicWorld, per_target

    K = L + 3
    ok = bool((status == 0).all() and (value == 0).all())
    want = np.where(b.op == abi.CC_OP_TOPIC_PUBLISH, listeners_at_rows(b, topics, L), 0)
    ok &= bool(np.array_equal(np.bincount(ev["pos"], minlength=len(b)), want))
    ok &= bool((ev["code"] == abi.CC_EV_MESSAGE).all() and (ev["src"] == abi.CC_EVSRC_COMMIT).all())
    sample = np.arange(0, topics, max(1, topics // 16))
    W = TopicWorld()
    for r in sample.tolist():
        W.create(r)
        for k in range(K):
            W.open(k * topics + r, r, 1000 + k * topics + r, 7 + k)
            if k < L:
                W.topics[r].listen(1000 + k * topics + r, 0)
    sel = np.nonzero(np.isin(b.inst % topics, sample))[0]
    sub = b.slice(0, len(b))
    for name in ("index", "inst", "op", "flags", "a"):
        getattr(sub, name)[:len(sel)] = getattr(b, name)[sel]
    _, mev = W.apply(sub, 0, len(sel))
    m = np.isin(ev["target"] % topics, sample)
    back = {int(r): i for i, r in enumerate(sel.tolist())}  # batch row -> row of the sampled sub-stream
    got = per_target([back[int(p)] for p in ev["pos"][m]], ev["target"][m], ev["tag"][m], ev["payload"][m])
    ok &= got == per_target(*(zip(*mev) if mev else ([], [], [], [])))
    return ok


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--listeners", type=int, default=8)
    ap.add_argument("--topics", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--group", action="store_true", help="the group join / leave fan-out instead")
    ap.add_argument("--root", default=os.path.dirname(HERE), help="checkout to import copycat_amd from")
    ap.add_argument("--no-gate", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch

    from copycat_amd import abi
    from copycat_amd.engine import RESULT_SENTINEL, DeviceBatch, DeviceEvents, Engine

    L, R = args.listeners, args.topics
    per_row = (3 * L - 2) / 2 if args.group else 0.98 * L
    n = args.rows or (10_000_000 if L == 1 and not args.group else int(100e6 / per_row) + 1)
    K = L + 1 if args.group else L + 3
    sub = min(1 << 22, -(-n // 16384) * 16384)
    bound = 2 * L if args.group else L + 2  # events a row can publish
    dev = torch.device("cuda:0")
    E = Engine(R, R * K, max(n, R * K), device=dev.index, flags=abi.CC_CFG_TIMERS_DEFERRED, sub_batch=sub,
               max_events=sub * bound + 1024, coord_cap=max(64, 1 << (L + 2).bit_length()))
    E.resource_create_range(0, R, abi.CC_RES_GROUP if args.group else abi.CC_RES_TOPIC)
    from copycat_amd.batch import Batch

    for k in range(K):  # instance k of resource r sits in slot k * R + r
        E.instance_open_range(k * R, R, 0, 1000 + k * R, 7 + k)
    # before step 0: every topic's instances 0 .. L - 1 listen / every group's members 0 .. L - 1 join
    s0 = Batch(R * L)
    s0.index[:] = np.arange(1, R * L + 1, dtype=np.uint64)
    s0.inst[:] = np.arange(R * L)  # instances 0 .. L - 1 of every resource
    s0.op[:] = abi.CC_OP_GROUP_JOIN if args.group else abi.CC_OP_TOPIC_LISTEN
    E.apply_host_events(s0, capacity=R * L * (2 * L) + 1024)
    index0 = R * L + 1
    total = args.warmup + args.steps + 1
    rng = np.random.default_rng(0x6709)
    seq = np.zeros(R, np.int64)
    dbs, want_ev, host0 = [], [], None
    for k in range(total):
        if args.group:
            b, nev = group_rows(n, R, L, seq, index0, rng)
        else:
            b, nev = topic_rows(k, n, R, L, index0), None
        index0 += n
        dbs.append(DeviceBatch.upload(b, device=dev))
        want_ev.append(nev)
        if k == 0:
            host0 = b
    status = torch.full((n,), RESULT_SENTINEL, dtype=torch.uint8, device=dev)
    value = torch.zeros((n,), dtype=torch.int64, device=dev)
    evs = DeviceEvents(n * bound + 1024, device=dev)
    ok, ms, counts, prof = None, [], [], {}
    for k in range(total):
        profiled = k == args.warmup and hasattr(E, "profile")
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
        if not args.no_gate and args.group:  # every step: the event rows written against the formula
            ok = ok is not False and cnt == want_ev[k]
        elif not args.no_gate and k == 0:
            ok = gate_topics(host0, status.cpu().numpy(), value.cpu().numpy().view(np.uint64), evs.host(), R, L)
        if k > args.warmup:
            ms.append(dt)
            counts.append(cnt)
    written = bool((status != RESULT_SENTINEL).all().item())
    med = statistics.median(ms)
    mev = statistics.median(counts)
    out = {"workload": "group_join_leave_fanout" if args.group else "topic_publish_fanout", "listeners": L,
           "resources": R, "rows": n, "steps": args.steps, "events_per_step": mev,
           "events_per_s": mev / (med / 1e3), "rows_per_s": n / (med / 1e3), "ms_per_step": round(med, 3),
           "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "gate": ok, "all_rows_written": written,
           "gpu": torch.cuda.get_device_name(0)}
    for name in ("k_apply_coord", "k_events", "k_topic_fanout"):
        if name in prof and prof[name][1]:
            out[name + "_ms_per_step"] = round(prof[name][0], 3)
    if prof.get("k_topic_fanout", (0, 0))[1]:
        recs = 0.98 * n
        byts = 28.0 * mev + 24.0 * recs
        out["fanout_bytes_per_event"] = round(byts / mev, 2)
        out["fanout_gb_per_s"] = round(byts / (prof["k_topic_fanout"][0] * 1e-3) / 1e9, 1)
    print(json.dumps(out))
    return 0 if ok is not False and written else 1


if __name__ == "__main__":
    sys.exit(main())
