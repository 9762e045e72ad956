"""Multi-GPU routing of the commit-apply path (host side): one engine per GPU, resources sharded by id.

SURVEY §8(e): resources are independent state machines multiplexed in one log (ResourceManager.java:37-39),
so a committed batch splits by resource owner with no cross-shard order dependence; only the order of
commits WITHIN a resource matters, and a stable split keeps it.  The only exchanges are:
  * the applied-index watermark (global applied = min over ranks), and
  * the session-expiry result (OR of per-rank bitmaps),
both tiny and all-gathered over RCCL (torch.distributed "nccl" on ROCm) once per batch.
"""
import ctypes as C
import os

import numpy as np

from . import abi
from .batch import Batch

NO_OWNER = -1


def owner_of(resource_slot, world):
    """Resource -> rank (round-robin by global resource slot)."""
    return resource_slot % world


def inst_owner_table(inst_res, world):
    """inst_res[inst] = global resource slot (or -1 for a closed instance) -> owning rank per instance."""
    inst_res = np.asarray(inst_res, dtype=np.int64)
    own = np.where(inst_res >= 0, inst_res % world, 0)  # unknown instances: rank 0 reports UNKNOWN_SESSION
    return own.astype(np.int32)


def _threads(threads):
    if threads:
        return int(threads)
    n = os.cpu_count() or 1
    return max(1, min(n, int(os.environ.get("OMP_NUM_THREADS", n))))


def _rank_table(inst_owner, world):
    t = np.ascontiguousarray(inst_owner)
    if world > 256:
        raise ValueError("world must be <= 256")
    if t.dtype != np.uint8:
        if len(t) and (t.min() < 0 or t.max() >= world):
            raise ValueError("inst_owner names a rank outside [0, world)")
        t = t.astype(np.uint8)
    return t


def split_counts(b: Batch, inst_owner, world, threads=0):
    """Rows per rank of a stable split (cc_split_batch with no outputs)."""
    from .engine import _check, _np, lib

    tab = _rank_table(inst_owner, world)
    counts = np.zeros(world, np.uint64)
    cols = abi.cc_batch(**{name: _np(getattr(b, name)) for name in Batch.__slots__})
    _check(lib().cc_split_batch(C.byref(cols), len(b), _np(tab), len(tab), world, _threads(threads), None, None,
                                _np(counts), None))
    return counts


def split_batch(b: Batch, inst_owner, world, threads=0, rows=True):
    """Stable split of one global log's batch into per-rank batches (native, multi-threaded: cc_split_batch).

    Returns [(rows, Batch)] indexed by rank; rows[r] are the rank's rows of `b` in log order (None if rows=False:
    merge_by_owner does not need them).  Rows whose instance slot is beyond the owner table go to rank 0."""
    from .engine import _check, _np, lib

    tab = _rank_table(inst_owner, world)
    counts = split_counts(b, tab, world, threads)
    parts = []
    outs = (abi.cc_batch_out * world)()
    rowp = (C.c_void_p * world)()
    for r in range(world):
        sub = Batch(int(counts[r]))
        ridx = np.empty(int(counts[r]), np.uint64) if rows else None
        for name in Batch.__slots__:
            setattr(outs[r], name, _np(getattr(sub, name)))
        rowp[r] = _np(ridx) if rows else None
        parts.append((ridx, sub))
    cap = counts.copy()
    cols = abi.cc_batch(**{name: _np(getattr(b, name)) for name in Batch.__slots__})
    _check(lib().cc_split_batch(C.byref(cols), len(b), _np(tab), len(tab), world, _threads(threads), outs, _np(cap),
                                _np(counts), rowp if rows else None))
    return parts


def merge_by_owner(inst, inst_owner, world, parts, threads=0):
    """parts[r] = (status, value) of rank r, in its split order -> (status[n], value[n]) in log order
    (cc_merge_results: the split's owner walk backwards, no row ids needed)."""
    from .engine import _check, _np, lib

    tab = _rank_table(inst_owner, world)
    inst = np.ascontiguousarray(inst, np.uint32)
    n = len(inst)
    status = np.empty(n, np.uint8)
    value = np.empty(n, np.uint64)
    pr = (abi.cc_results * world)()
    keep = []
    for r, (s, v) in enumerate(parts):
        s, v = np.ascontiguousarray(s, np.uint8), np.ascontiguousarray(v, np.uint64)
        keep.append((s, v))
        pr[r].status, pr[r].value = _np(s), _np(v)
    out = abi.cc_results(_np(status), _np(value))
    _check(lib().cc_merge_results(_np(inst), n, _np(tab), len(tab), world, _threads(threads), pr, C.byref(out)))
    return status, value


# ---- the same split and merge for columns that are already in HBM (cc_split_batch_device, split_gpu.hip) ------------
def _owner_tensor(own_dev, world, device):
    """The owner table as a uint8 device tensor (a host table is validated and converted as _rank_table does)."""
    import torch

    if isinstance(own_dev, torch.Tensor):
        if own_dev.dtype != torch.uint8 or not own_dev.is_cuda or not own_dev.is_contiguous():
            raise ValueError("own_dev must be a contiguous uint8 device tensor")
        if not 1 <= world <= 256:
            raise ValueError("world must be in [1, 256]")
        return own_dev
    return torch.from_numpy(_rank_table(own_dev, world)).to(device)


def _split_workspace(n, world, device):
    import torch

    from .engine import _check, lib

    need = C.c_uint64()
    _check(lib().cc_split_device_bound(n, world, C.byref(need)))
    return torch.empty(need.value, dtype=torch.uint8, device=device)


def _stream_on(stream, device):
    import torch

    return stream if stream is not None else torch.cuda.current_stream(device)


def split_counts_device(db, own_dev, world, stream=None):
    """Rows per rank of a stable split of device columns (cc_split_batch_device with no outputs)."""
    from .engine import _check, _dptr, _np, _stream_ptr, lib

    inst = db.cols["inst"]
    tab = _owner_tensor(own_dev, world, inst.device)
    st = _stream_on(stream, inst.device)
    work = _split_workspace(db.n, world, inst.device)
    counts = np.zeros(world, np.uint64)
    cols = db.struct()
    _check(lib().cc_split_batch_device(C.byref(cols), db.n, _dptr(tab) if tab.numel() else None, tab.numel(), world,
                                       None, None, _np(counts), None, _dptr(work), work.numel(), _stream_ptr(st)))
    return counts


def split_batch_device(db, own_dev, world, rows=False, stream=None):
    """Stable split of a DeviceBatch into per-rank DeviceBatches, all in HBM (cc_split_batch_device).

    Returns [(rows, DeviceBatch)] indexed by rank; rows[r] (a uint64 device tensor, None if rows=False) are the rank's
    rows of `db` in log order: they map a rank's event `pos` back to log rows.  A column `db` lacks, the parts lack.
    The outputs are complete on return (the stream is synchronised)."""
    import torch

    from .engine import DeviceBatch, _check, _dptr, _np, _stream_ptr, lib

    inst = db.cols["inst"]
    dev = inst.device
    tab = _owner_tensor(own_dev, world, dev)
    st = _stream_on(stream, dev)
    counts = split_counts_device(db, tab, world, stream=st)
    work = _split_workspace(db.n, world, dev)
    outs = (abi.cc_batch_out * world)()
    rowp = (C.c_void_p * world)()
    parts = []
    with torch.cuda.stream(st):
        for r in range(world):
            c = int(counts[r])
            cols = {name: torch.empty(c, dtype=db.cols[name].dtype, device=dev)
                    for name, _ in abi.BATCH_COLUMNS if db.cols.get(name) is not None}
            for name, t in cols.items():
                setattr(outs[r], name, t.data_ptr() if c else None)
            ridx = torch.empty(c, dtype=torch.uint64, device=dev) if rows else None
            rowp[r] = ridx.data_ptr() if rows and c else None
            parts.append((ridx, DeviceBatch(cols, c)))
    cap = counts.copy()
    cols = db.struct()
    _check(lib().cc_split_batch_device(C.byref(cols), db.n, _dptr(tab) if tab.numel() else None, tab.numel(), world, outs,
                                       _np(cap), _np(counts), rowp if rows else None, _dptr(work), work.numel(),
                                       _stream_ptr(st)))
    st.synchronize()
    return parts


def merge_by_owner_device(inst, own_dev, world, parts, stream=None):
    """parts[r] = (status, value) device tensors of rank r, in its split order -> (status[n], value[n]) device tensors
    in log order (cc_merge_results_device; `inst` is the uint32 device column the split used).  The outputs are
    complete on return (the stream is synchronised)."""
    import torch

    from .engine import _check, _dptr, _stream_ptr, lib

    dev = inst.device
    tab = _owner_tensor(own_dev, world, dev)
    st = _stream_on(stream, dev)
    n = inst.numel()
    work = _split_workspace(n, world, dev)
    with torch.cuda.stream(st):
        status = torch.empty(n, dtype=torch.uint8, device=dev)
        value = torch.empty(n, dtype=torch.uint64, device=dev)
    pr = (abi.cc_results * world)()
    for r, (s, v) in enumerate(parts):
        if s.dtype != torch.uint8 or v.element_size() != 8 or not (s.is_contiguous() and v.is_contiguous()):
            raise ValueError("parts must be (uint8 status, 64-bit value) contiguous device tensors")
        pr[r].status = s.data_ptr() if s.numel() else None
        pr[r].value = v.data_ptr() if v.numel() else None
    out = abi.cc_results(status.data_ptr() if n else None, value.data_ptr() if n else None)
    _check(lib().cc_merge_results_device(_dptr(inst) if n else None, n, _dptr(tab) if tab.numel() else None, tab.numel(),
                                         world, pr, C.byref(out), _dptr(work), work.numel(), _stream_ptr(st)))
    st.synchronize()
    return status, value


# ---- the per-rank event streams back into log order (cc_merge_events, evmerge.cpp / evmerge_gpu.hip) ----------------
_EVENT_NP = {"u4": np.uint32, "u1": np.uint8, "u8": np.uint64}


def merge_events(parts, rows, n, threads=0):
    """parts[r] = rank r's events as numpy columns (pos, target, code, src, tag, payload: DeviceEvents.host()), pos a
    row of the rank's share; rows[r] = the rank's log rows (split_batch's row ids) -> the one log-ordered stream as
    the same dict, pos = the log row (cc_merge_events).  Streams of session closes or advance_time are refused."""
    from .engine import _check, _np, lib

    world = len(parts)
    pr = (abi.cc_events * world)()
    rowp = (C.c_void_p * world)()
    row_counts = np.zeros(world, np.uint64)
    keep = []
    total = 0
    for r, (p, rw) in enumerate(zip(parts, rows)):
        cols = [np.ascontiguousarray(p[name], _EVENT_NP[dt]) for name, dt in abi.EVENT_COLUMNS]
        cnt = np.array([len(cols[0])], np.uint64)
        rw = np.ascontiguousarray(rw if rw is not None else [], np.uint64)
        keep.append((cols, cnt, rw))
        for (name, _), c in zip(abi.EVENT_COLUMNS, cols):
            setattr(pr[r], name, _np(c) if len(c) else None)
        pr[r].capacity, pr[r].count = len(cols[0]), _np(cnt)
        rowp[r] = _np(rw) if len(rw) else None
        row_counts[r] = len(rw)
        total += len(cols[0])
    out = {name: np.empty(total, _EVENT_NP[dt]) for name, dt in abi.EVENT_COLUMNS}
    ocnt = np.zeros(1, np.uint64)
    o = abi.cc_events(*[_np(out[name]) if total else None for name, _ in abi.EVENT_COLUMNS], total, _np(ocnt))
    tot = C.c_uint64()
    _check(lib().cc_merge_events(pr, rowp, _np(row_counts), n, world, _threads(threads), C.byref(o), C.byref(tot)))
    out["count"] = int(tot.value)
    return out


def _events_workspace(n, world, device):
    import torch

    from .engine import _check, lib

    need = C.c_uint64()
    _check(lib().cc_merge_events_device_bound(n, world, C.byref(need)))
    return torch.empty(need.value, dtype=torch.uint8, device=device)


def merge_events_device(parts, rows, n, capacity=None, stream=None):
    """parts[r] = rank r's DeviceEvents after apply_events on its share; rows[r] = the rank's log rows (the uint64
    device tensors of split_batch_device(..., rows=True)) -> a DeviceEvents holding the one log-ordered stream, pos =
    the log row (cc_merge_events_device), which Engine.events_to_host_packed accepts.  capacity: the output's rows
    (default: the sum of the parts' capacities).  The output is complete on return (the stream is synchronised)."""
    import torch

    from .engine import DeviceEvents, _check, _np, _stream_ptr, lib

    world = len(parts)
    dev = parts[0].count.device
    st = _stream_on(stream, dev)
    work = _events_workspace(n, world, dev)
    pr = (abi.cc_events * world)()
    rowp = (C.c_void_p * world)()
    row_counts = np.zeros(world, np.uint64)
    for r, (p, rw) in enumerate(zip(parts, rows)):
        pr[r] = p.struct()
        if rw is not None and (rw.dtype != torch.uint64 or not rw.is_contiguous()):
            raise ValueError("rows must be contiguous uint64 device tensors")
        c = rw.numel() if rw is not None else 0
        rowp[r] = rw.data_ptr() if c else None
        row_counts[r] = c
    cap = int(capacity) if capacity is not None else sum(int(p.capacity) for p in parts)
    with torch.cuda.stream(st):
        out = DeviceEvents(max(cap, 1), device=dev)
    out.capacity = cap
    o = out.struct()
    tot = C.c_uint64()
    _check(lib().cc_merge_events_device(pr, rowp, _np(row_counts), n, world, C.byref(o), C.byref(tot), work.data_ptr(),
                                        work.numel(), _stream_ptr(st)))
    st.synchronize()
    return out


def merge_results(n, parts):
    """parts: [(rows, status, value)] -> (status[n], value[n]) in log order."""
    status = np.zeros(n, np.uint8)
    value = np.zeros(n, np.uint64)
    for rows, s, v in parts:
        status[rows] = s
        value[rows] = v
    return status, value


def global_watermark(local_applied):
    """All ranks have applied every entry up to min(local watermarks) (a rank with no work reports the batch end)."""
    return int(min(local_applied))


def allgather_watermark(local, device=None, group=None):
    """RCCL/gloo all-gather of one u64 watermark per rank -> list of ints."""
    import torch
    import torch.distributed as dist

    world = dist.get_world_size(group)
    t = torch.tensor([int(local)], dtype=torch.int64, device=device)
    out = torch.zeros(world, dtype=torch.int64, device=device)
    dist.all_gather_into_tensor(out, t, group=group)
    return out.cpu().tolist()


def allgather_expired(bitmap, device=None, group=None):
    """OR-merge of per-rank expired-session bitmaps (u64 words) over all ranks."""
    import torch
    import torch.distributed as dist

    world = dist.get_world_size(group)
    t = torch.as_tensor(np.ascontiguousarray(bitmap).view(np.int64), device=device)
    out = torch.zeros(world * t.numel(), dtype=torch.int64, device=device)
    dist.all_gather_into_tensor(out, t, group=group)
    words = out.view(world, -1).cpu().numpy().view(np.uint64)
    return np.bitwise_or.reduce(words, axis=0)


def expired_sessions(bitmap, sessions):
    """Session ids whose bit is set in an expired-session bitmap (u64 words, LSB first), ascending -- the order
    cc_sessions_expire closes them in."""
    words = np.ascontiguousarray(bitmap, np.uint64)
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:sessions]
    return np.nonzero(bits)[0].tolist()
