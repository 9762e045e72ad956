#!/usr/bin/env python3
"""Rate of a DistributedSet stream that carries whole-set rows (size / isEmpty / clear / Delete).

The config-3 stream (workload.map_zipf_rows: Zipf 0.99 put / get / remove over 1M (collection, key) pairs) over 4,096
sets, its rows rewritten to set ops (put -> add, get -> contains, remove -> remove), with 0.1 % of the rows turned into
SET_SIZE / SET_ISEMPTY and 0.01 % into SET_CLEAR / Delete.  Every step's rows are uploaded first; a step is one
cc_apply_batch on the resident columns plus the final sync, host wall clock.  Step 0 is gated against the CPU oracle
(every status and value, 64 sets' elements, the applied index) and not timed; the steps after it are.  Prints one JSON
line: rows/s (median step, with the fastest and the slowest), the engine's barrier-row counter over the timed steps
(rows that ended a segment for a host round trip and a table scan: 0 when every whole-set row ran in the stream) and
whether the gate held.

    python scripts/wide_rows_rate.py [--rows 10000000] [--steps 3] [--sets 4096] [--no-gate]
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
from copycat_amd.engine import RESULT_SENTINEL, DeviceBatch, Engine  # noqa: E402
from copycat_amd.workload import map_zipf_rows  # noqa: E402

P_QUERY, P_CLEAR = 0.001, 0.0001


def set_rows(step, n, sets):
    """Rows [step * n, (step + 1) * n) of the stream."""
    b = map_zipf_rows(step * n, n, maps=sets)
    op = b.op.copy()
    for m, s in ((abi.CC_OP_MAP_PUT, abi.CC_OP_SET_ADD), (abi.CC_OP_MAP_GET, abi.CC_OP_SET_CONTAINS),
                 (abi.CC_OP_MAP_REMOVE, abi.CC_OP_SET_REMOVE)):
        b.op[op == m] = s
    rng = np.random.default_rng(0x51DE + step)
    x = rng.random(n)
    q, c = x < P_QUERY, (x >= P_QUERY) & (x < P_QUERY + P_CLEAR)
    b.op[q] = rng.choice(np.array([abi.CC_OP_SET_SIZE, abi.CC_OP_SET_ISEMPTY], np.uint8), int(q.sum()))
    b.op[c] = rng.choice(np.array([abi.CC_OP_SET_CLEAR, abi.CC_OP_DELETE], np.uint8), int(c.sum()))
    return b, int(q.sum()), int(c.sum())


def gate(E, b, status, value, sets):
    from oracle.oracle_py import Oracle

    O = Oracle(sets, sets)
    for r in range(sets):
        O.resource_create(r, abi.CC_RES_SET)
        O.instance_open(r, r, 1000 + r, 7)
    s2, v2 = O.apply(b)
    ok = bool(np.array_equal(status.cpu().numpy(), s2))
    ok &= bool(np.array_equal(value.cpu().numpy().view(np.uint64), v2))
    for r in range(0, sets, max(1, sets // 64)):
        ok &= all(np.array_equal(x, y) for x, y in zip(E.map_entries(r), O.map_entries(r)))
    return ok and E.applied_index() == O.applied_index()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=3, help="timed steps after the gated step 0")
    ap.add_argument("--sets", type=int, default=4096)
    ap.add_argument("--no-gate", action="store_true")
    args = ap.parse_args()
    n, sets = args.rows, args.sets
    dev = torch.device("cuda:0")
    E = Engine(sets, sets, n, device=dev.index, map_capacity=1 << 20)
    E.resource_create_range(0, sets, abi.CC_RES_SET)
    E.instance_open_range(0, sets, 0, 1000, 7)
    host, dbs, nq, nc = [], [], 0, 0
    for k in range(args.steps + 1):
        b, q, c = set_rows(k, n, sets)
        dbs.append(DeviceBatch.upload(b, device=dev))
        host.append(b if k == 0 else None)
        if k:
            nq, nc = nq + q, nc + c
    status = torch.full((n,), RESULT_SENTINEL, dtype=torch.uint8, device=dev)
    value = torch.zeros((n,), dtype=torch.int64, device=dev)
    E.apply(dbs[0], status, value)
    E.sync()
    ok = None if args.no_gate else gate(E, host[0], status, value, sets)
    c0 = E.counters()
    ms = []
    for k in range(1, args.steps + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        E.apply(dbs[k], status, value)
        E.sync()
        ms.append((time.perf_counter() - t) * 1e3)
    c1 = E.counters()
    written = bool((status != RESULT_SENTINEL).all().item())
    med = statistics.median(ms)
    print(json.dumps({"workload": "sets_zipf_wide_rows", "rows": n, "sets": sets, "steps": args.steps,
                      "size_isempty_rows": nq, "clear_delete_rows": nc, "rows_per_s": n / (med / 1e3),
                      "ms_per_step": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
                      "barrier_rows": c1[0] - c0[0], "sub_batches": c1[2] - c0[2], "parity_step0": ok,
                      "all_rows_written": written, "gpu": torch.cuda.get_device_name(0)}))
    return 0 if ok is not False and written else 1


if __name__ == "__main__":
    sys.exit(main())
