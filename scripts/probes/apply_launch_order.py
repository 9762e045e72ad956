#!/usr/bin/env python3
"""Does a build of the engine enqueue the same kernels in the same order as another build?

cc_apply_batch's host orchestration (copycat_amd/csrc/apply_batch.hip) decides which kernels run, in which order and
with which grids.  This driver applies small seeded batches on six engines, each with a small explicit sub_batch so
that every case spans at least three sub-batches:

  value     value-only engine (value_path.hip)
  maps      maps outside TTL mode: hot keys, in-stream size / isEmpty / containsValue / clear rows
  ttl       maps in TTL mode, with barrier rows (containsValue / clear)
  coord     coordination with an event stream and group schedule rows whose timers fire inside the batch
  halves    more than kBarCap (65,536) barrier rows, with events: the batch is applied as two halves
  span      an index column whose range passes 2^32: sub-batches are cut by k_span_cut

and prints, per case, Engine.counters(), the launch counts of Engine.profile_read() and a checksum of the results.

  run                      the driver (CC_ENGINE_SO picks the build; run it under `rocprofv3 --kernel-trace
                           --output-format csv -d DIR -o NAME -- python3 scripts/probes/apply_launch_order.py run`,
                           with CC_NO_SIDE_REPLAY=1 for one stream: then the dispatch order is the launch order.
                           That switch is read by diagnostics builds only: build both libraries with
                           copycat_amd.build.build_variant(path, ["CC_DIAG"], tag).  With the side stream on, the
                           replay kernels' place among the engine stream's is a matter of timing: compare counts)
  reduce TRACE.csv OUT     the trace in dispatch order: a table "id = kernel grid workgroup", then the launches as
                           ids, a repeating block written once as Nx(...); the last line holds the number of
                           launches and the SHA-256 of the uncollapsed "kernel grid workgroup" lines
  counts TRACE.csv OUT     the trace as one "launches kernel" line per kernel
  diff A B                 exit 1 and print the first difference if the two listings differ
"""
import csv
import hashlib
import json
import sys
import zlib
from collections import Counter

import numpy as np

N, SUB = 60_000, 16384  # sub_batch is rounded up to the partition tile: 4 sub-batches


def _short(name):
    return name.split("(")[0].replace("void ", "").replace("cc::", "")


def _rows(trace):
    rows = list(csv.DictReader(open(trace)))
    dims = lambda r, p: "x".join(r[k] for k in sorted(r) if k.startswith(p))  # noqa: E731
    # not the engine's launches: torch's fills of the result tensors, and the copy / fill kernels the HIP runtime uses
    # for a memcpy or memset when it does not take the DMA engine (its choice: it differs between two runs of one build)
    rows = [r for r in rows if "at::native" not in r["Kernel_Name"] and "__amd_rocclr_" not in r["Kernel_Name"]]
    # enqueue order where the trace has it (two short kernels of one stream can carry start times out of order)
    key = "Dispatch_Id" if rows and "Dispatch_Id" in rows[0] else "Start_Timestamp"
    rows.sort(key=lambda r: int(r[key]))
    return [(_short(r["Kernel_Name"]), dims(r, "Grid_Size"), dims(r, "Workgroup_Size")) for r in rows]


def _collapse(items, max_period=256):
    """Greedy: at each place the repeating block (up to max_period items) that covers most is written once."""
    out, i = [], 0
    while i < len(items):
        period, reps = 1, 1
        for p in range(1, max_period + 1):
            if i + 2 * p > len(items):
                break
            r = 1
            while items[i + r * p:i + (r + 1) * p] == items[i:i + p]:
                r += 1
            if r >= 2 and r * p > period * reps:
                period, reps = p, r
        out.append(items[i] if reps == 1 else f"{reps}x({' '.join(items[i:i + period])})")
        i += period * reps
    return out


def write_listing(lines, out):
    ids = {}
    for x in lines:
        ids.setdefault(x, f"k{len(ids)}")
    seq = _collapse(_collapse([ids[x] for x in lines]))  # (twice: repeats of blocks that hold repeats)
    with open(out, "w") as f:
        f.write("# kernels: id = name grid workgroup\n")
        for x, k in ids.items():
            f.write(f"{k} = {x}\n")
        f.write("# launches in order; Nx(...) is the group N times\n")
        row = ""
        for tok in seq:  # (as many as fit 118 columns per line)
            if row and len(row) + 1 + len(tok) > 118:
                f.write(row + "\n")
                row = ""
            row = f"{row} {tok}" if row else tok
        f.write(row + "\n")
        f.write(f"# {len(lines)} launches, sha256 {hashlib.sha256(chr(10).join(lines).encode()).hexdigest()}\n")


def reduce_trace(trace, out):
    write_listing([f"{name} {grid} {wg}" for name, grid, wg in _rows(trace)], out)


def count_trace(trace, out):
    c = Counter(name for name, _, _ in _rows(trace))
    with open(out, "w") as f:
        for name in sorted(c):
            f.write(f"{c[name]} {name}\n")


def diff(a, b):
    la, lb = open(a).read().splitlines(), open(b).read().splitlines()
    for i, (x, y) in enumerate(zip(la, lb)):
        if x != y:
            print(f"line {i + 1} differs:\n  {a}: {x}\n  {b}: {y}")
            return 1
    if len(la) != len(lb):
        print(f"{a} has {len(la)} lines, {b} has {len(lb)}")
        return 1
    print(f"identical: {len(la)} lines")
    return 0


# ---- the driver ----

def _report(name, E, results):
    crc = 0
    for r in results:
        for col in r:
            crc = zlib.crc32(np.ascontiguousarray(col).tobytes(), crc)
    launches = {k: int(v[1]) for k, v in E.profile_read().items() if v[1]}
    print(json.dumps({"case": name, "counters": E.counters(), "launches": launches, "results_crc32": crc}), flush=True)


def _map_engine(abi, maps, max_inst, n, cap, sub_batch, flags):
    from copycat_amd.engine import Engine

    E = Engine(maps, max_inst, n, map_capacity=cap, sub_batch=sub_batch, flags=flags)
    E.resource_create_range(0, maps, abi.CC_RES_MAP)
    E.instance_open_range(0, maps, 0, 1000, 7)
    E.handle_strings({h: f"key-{h}" for h in range(8192)})  # the Strings behind the streams' HANDLE keys
    E.profile(True)
    return E


def _no_nulls(abi, b):
    f = b.flags
    ta, tb = f & 7, (f >> 3) & 7
    f[ta == abi.CC_TAG_NULL] |= np.uint8(abi.CC_TAG_LONG)
    f[tb == abi.CC_TAG_NULL] |= np.uint8(abi.CC_TAG_LONG << 3)


def _wide(abi, b, rows, ops, rng):
    b.op[rows] = rng.choice(np.array(ops, np.uint8), size=len(rows))
    cv = rows[b.op[rows] == abi.CC_OP_MAP_CONTAINSVALUE]
    b.a[cv] = rng.integers(0, 3, len(cv)).astype(np.uint64)
    b.flags[cv] = (b.flags[cv] & np.uint8(0xF8)) | np.uint8(abi.CC_TAG_LONG)
    b.aux[rows] = 0


def case_value(abi):
    from copycat_amd.engine import Engine
    from copycat_amd.workload import value_random_stream

    R = 1024
    E = Engine(R, R, N, sub_batch=SUB)
    E.resource_create_range(0, R, abi.CC_RES_VALUE)
    E.instance_open_range(0, R, 0, 1, 9)
    E.profile(True)
    b = value_random_stream(N, R, R, seed=101, hot=4, p_hot=0.2)
    _report("value", E, [E.apply_host(b)])


def case_maps(abi):
    from copycat_amd.workload import map_random_stream

    maps = 16
    b = map_random_stream(N, maps, maps, keys=64, seed=102, hot=2, p_hot=0.3)
    _no_nulls(abi, b)
    rng = np.random.default_rng(102)
    _wide(abi, b, rng.choice(N, 900, replace=False),
          [abi.CC_OP_MAP_SIZE, abi.CC_OP_MAP_ISEMPTY, abi.CC_OP_MAP_CONTAINSVALUE, abi.CC_OP_MAP_CLEAR], rng)
    E = _map_engine(abi, maps, maps, N, 65536, SUB, abi.CC_CFG_TIMERS_DEFERRED)
    _report("maps", E, [E.apply_host(b.slice(0, N // 2)), E.apply_host(b.slice(N // 2, N))])


def case_ttl(abi):
    from copycat_amd.workload import map_random_stream

    maps = 16
    b = map_random_stream(N, maps, maps, keys=64, seed=103)
    _no_nulls(abi, b)
    rng = np.random.default_rng(103)
    b.time[:] = np.arange(N, dtype=np.uint64) // np.uint64(8) + np.uint64(1000)
    arm = rng.random(N) < 0.4
    b.aux[:] = np.where(arm, rng.integers(1, 300, N), 0).astype(np.int64).view(np.uint64)
    _wide(abi, b, rng.choice(N, 120, replace=False),
          [abi.CC_OP_MAP_SIZE, abi.CC_OP_MAP_CONTAINSVALUE, abi.CC_OP_MAP_CLEAR], rng)
    E = _map_engine(abi, maps, maps, N, 65536, SUB, abi.CC_CFG_TIMERS_DEFERRED)
    _report("ttl", E, [E.apply_host(b.slice(0, N // 3)), E.apply_host(b.slice(N // 3, N))])


def _coord_engine(abi, types, K, n, flags, map_capacity=0):
    from copycat_amd.engine import Engine

    R = len(types)
    max_inst = R * K + 8
    E = Engine(R, max_inst, n, flags=flags, sub_batch=SUB, max_events=1 << 21, map_capacity=map_capacity)
    for r, t in enumerate(types):
        E.resource_create(r, int(t))
        for k in range(K):
            E.instance_open(r * K + k, r, 1000 + r * K + k, 7 + k)
    E.profile(True)
    return E, max_inst


def case_coord(abi):
    from copycat_amd.workload import coord_random_stream

    L, El, G, V = abi.CC_RES_LOCK, abi.CC_RES_ELECTION, abi.CC_RES_GROUP, abi.CC_RES_VALUE
    types = np.array([L, El, G, V, G, G] * 8, np.uint8)
    K = 5
    E, max_inst = _coord_engine(abi, types, K, N, abi.CC_CFG_TIMERS_DEFERRED | abi.CC_CFG_VALUE_EVENTS)
    b = coord_random_stream(N, types, K, max_inst, seed=104)
    rng = np.random.default_rng(104)
    res_of = np.where(b.inst < max_inst, b.inst // K, 0)
    grp = np.nonzero((types[np.minimum(res_of, len(types) - 1)] == G) & (b.inst < len(types) * K))[0]
    rows = rng.choice(grp, size=60, replace=False)
    b.op[rows] = abi.CC_OP_GROUP_SCHEDULE
    b.key[rows] = (1000 + res_of[rows] * K + rng.integers(0, K, len(rows))).astype(np.uint64)
    b.flags[rows] = abi.cc_flags(abi.CC_TAG_HANDLE, 0, 0)
    b.a[rows] = rng.integers(0, 1 << 20, len(rows)).astype(np.uint64)
    b.aux[rows] = rng.integers(1, 400, len(rows)).astype(np.int64).view(np.uint64)  # delays the batch's clock passes
    s, v, ev = E.apply_host_events(b, capacity=8 * N)
    assert (ev["src"] == abi.CC_EVSRC_TIMER).any(), "no group timer fired inside the batch"
    _report("coord", E, [(s, v), tuple(ev[k] for k in ("pos", "target", "code", "src", "tag", "payload"))])


def case_halves(abi):
    from copycat_amd.batch import Batch
    from copycat_amd.workload import coord_random_stream

    L = abi.CC_RES_LOCK
    # nm > kBarCap whole-map rows on maps that store nulls, in one run across the batch's middle (no sub-batch between
    # two of them: the listing stays short); 256 locks: every queue stays well within coord_cap
    locks, K, maps, n, nm = 256, 4, 2, 150_000, 80_000  # (a tenth of them puts: 72,000 barrier rows)
    types = np.array([L] * locks + [abi.CC_RES_MAP] * maps, np.uint8)
    E, max_inst = _coord_engine(abi, types, K, n, abi.CC_CFG_TIMERS_DEFERRED, map_capacity=4096)
    rng = np.random.default_rng(105)
    lk = coord_random_stream(n - nm, np.full(locks, L, np.uint8), K, max_inst, seed=105, p_delete=0.0)
    rows = np.arange((n - nm) // 2, (n - nm) // 2 + nm)
    at = np.ones(n, bool)
    at[rows] = False
    cols = {}
    for name, _ in abi.BATCH_COLUMNS:
        src = getattr(lk, name)
        cols[name] = np.zeros(n, src.dtype)
        cols[name][at] = src
    cols["index"] = np.arange(1, n + 1, dtype=np.uint64)
    cols["time"] = np.maximum.accumulate(cols["time"])  # (a map row takes the clock of the lock row before it)
    cols["op"][rows] = abi.CC_OP_MAP_CONTAINSVALUE
    cols["op"][rows[: nm // 10]] = abi.CC_OP_MAP_PUT
    cols["inst"][rows] = (locks + rng.integers(0, maps, nm)) * K + rng.integers(0, K, nm)
    cols["key"][rows] = rng.integers(0, 64, nm).astype(np.uint64)
    cols["a"][rows] = rng.integers(0, 4, nm).astype(np.uint64)
    nul = rng.random(nm) < 0.05
    cols["flags"][rows] = np.where(nul, abi.cc_flags(abi.CC_TAG_NULL, 0, 0), abi.cc_flags(abi.CC_TAG_LONG, 0, 0))
    cols["aux"][rows] = 0
    s, v, ev = E.apply_host_events(Batch.from_columns(**cols), capacity=4 * n)
    _report("halves", E, [(s, v), tuple(ev[k] for k in ("pos", "target", "code", "src", "tag", "payload"))])


def case_span(abi):
    from copycat_amd.workload import map_random_stream

    maps, n = 6, 2 * N
    b = map_random_stream(n, maps, maps, keys=40, seed=106)
    rng = np.random.default_rng(106)
    _wide(abi, b, rng.choice(n, 900, replace=False),
          [abi.CC_OP_MAP_SIZE, abi.CC_OP_MAP_ISEMPTY, abi.CC_OP_MAP_CONTAINSVALUE], rng)
    for at in sorted(rng.choice(np.arange(1, n), 7, replace=False)):
        b.index[at:] += np.uint64(1 << 33)
    E = _map_engine(abi, maps, maps, n, 4096, 2 * SUB, abi.CC_CFG_TIMERS_DEFERRED)
    _report("span", E, [E.apply_host(b)])


def run():
    import os

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from copycat_amd import abi

    for case in (case_value, case_maps, case_ttl, case_coord, case_halves, case_span):
        case(abi)


if __name__ == "__main__":
    cmd = sys.argv[1] if len(sys.argv) > 1 else "run"
    if cmd == "run":
        run()
    elif cmd == "reduce":
        reduce_trace(sys.argv[2], sys.argv[3])
    elif cmd == "counts":
        count_trace(sys.argv[2], sys.argv[3])
    elif cmd == "diff":
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
