"""What a large-valued workload pays for the 4-byte result word (value_path.hip): the c2 client-model stream with every
value offset by --offset (default 2^40), applied through the Engine API and event-timed.

Every resource is first set to the offset and the client model starts from there, so every CAS expects a value past
the record's 32 bits (an escaped record, read from the batch columns) and every get returns one past the result word's
24 bits (an escaped result: 8 more bytes written by the apply and gathered by the unpermute).  --offset 0 is the bench's
own stream.  Prints one JSON line: ms per step (event-timed, each step and the mean) and the per-kernel split.

  python scripts/probes/res32_escape_cliff.py [--commits N] [--steps 5] [--warmup 1] [--offset 1099511627776]
(CC_ENGINE_SO selects another build of the engine, e.g. the parent's, for the comparison.)"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from copycat_amd import abi  # noqa: E402
from copycat_amd.batch import Batch  # noqa: E402
from copycat_amd.engine import DeviceBatch, Engine  # noqa: E402
from copycat_amd.workload import SEED_C2, AtomicLongClients  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commits", type=int, default=100_000_000)
    ap.add_argument("--resources", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--offset", type=int, default=1 << 40)
    args = ap.parse_args()
    n, R = args.commits, args.resources
    dev = torch.device("cuda", 0)
    cols = ("index", "inst", "op", "flags", "a", "b")
    E = Engine(R, R, n, device=0)
    E.resource_create_range(0, R, abi.CC_RES_VALUE)
    E.instance_open_range(0, R, 0, 1, 1)
    clients = AtomicLongClients(resources=R, seed=SEED_C2)
    status = torch.full((n,), 0xFF, dtype=torch.uint8, device=dev)
    value = torch.full((n,), -1, dtype=torch.int64, device=dev)
    if args.offset:  # every resource holds the offset before the first client row
        pre = Batch.from_columns(index=np.arange(1, R + 1, dtype=np.uint64), time=np.zeros(R, np.uint64),
                                 inst=np.arange(R, dtype=np.uint32), op=np.full(R, abi.CC_OP_VALUE_SET, np.uint8),
                                 flags=np.full(R, abi.CC_TAG_LONG, np.uint8), a=np.full(R, args.offset, np.uint64),
                                 b=np.zeros(R, np.uint64))
        E.apply(DeviceBatch.upload(pre, device=dev), status[:R], value[:R])
        E.sync()
        clients.tag[:] = abi.CC_TAG_LONG
        clients.val[:] = args.offset
        clients.next_global = R + 1
    host = Batch(n)
    streams = []
    for _ in range(args.warmup + args.steps):
        clients.next(n, out=host)
        streams.append(DeviceBatch.upload(host, device=dev, columns=cols))
    del host
    stream = torch.cuda.Stream(dev)  # a stream of the probe's own: the events below are recorded on the one the engine runs on
    stream.wait_stream(torch.cuda.current_stream(dev))
    for k in range(args.warmup):
        E.apply(streams[k], status, value, stream=stream)
    torch.cuda.synchronize(dev)
    E.profile(True)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    ev[0].record(stream)
    for k in range(args.steps):
        E.apply(streams[args.warmup + k], status, value, stream=stream)
        ev[k + 1].record(stream)
    torch.cuda.synchronize(dev)
    E.sync()
    prof = E.profile_read()
    ms = [ev[k].elapsed_time(ev[k + 1]) for k in range(args.steps)]
    st, va = status.cpu().numpy(), value.cpu().numpy()
    op = streams[-1].cols["op"].cpu().numpy()
    ret = op == abi.CC_OP_VALUE_GET
    out = {"commits": n, "resources": R, "offset": args.offset, "steps": args.steps,
           "ms_per_step": round(float(np.mean(ms)), 4), "ms_steps": [round(x, 4) for x in ms],
           "per_kernel_ms_per_step": {k: round(t / args.steps, 4) for k, (t, nl) in prof.items() if nl},
           "unwritten": int(np.count_nonzero(st == 0xFF)),
           "gets": int(ret.sum()), "gets_past_24_bits": int(np.count_nonzero(np.abs(va[ret]) >= (1 << 23))),
           "cas_success_share": round(float(np.mean(va[op == abi.CC_OP_VALUE_CAS] == 1)), 4),
           "engine": os.environ.get("CC_ENGINE_SO", "in-tree")}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
