"""An event stream to its client sessions (cc_route_events, csrc/route.cpp / route_gpu.hip).

An event row names its receiver as an instance slot; the host publishes to the client session that owns the instance
(ManagedResourceSession.publish).  route_events groups a stream by owning session, stably, and returns a directory of
the sessions that received something, so the host publishes one contiguous run per session instead of one row at a
time."""
import ctypes as C

import numpy as np

from . import abi
from .shard import _EVENT_NP, _stream_on, _threads


def _table(a, dtype):
    return None if a is None else np.ascontiguousarray(a, dtype)


def route_events(ev, session_of_inst, n_sessions, id_of_inst=None, threads=0):
    """ev: numpy columns (pos, target, code, src, tag, payload: DeviceEvents.host(), shard.merge_events) -> (routed
    columns as the same dict plus "count", instance ids per routed row or None, (session, start)): session[k] is the k-th
    session ordinal that received rows, start[k]:start[k + 1] its rows of the routed stream (cc_route_events)."""
    from .engine import _check, _np, lib

    cols = [np.ascontiguousarray(ev[name], _EVENT_NP[dt]) for name, dt in abi.EVENT_COLUMNS]
    n = len(cols[0])
    tab, ids = _table(session_of_inst, np.uint32), _table(id_of_inst, np.uint64)
    if ids is not None and len(ids) != len(tab):
        raise ValueError("id_of_inst and session_of_inst must have one entry per instance slot")
    out = {name: np.empty(n, _EVENT_NP[dt]) for name, dt in abi.EVENT_COLUMNS}
    inst = np.empty(n, np.uint64) if ids is not None else None
    cap = min(n, int(n_sessions))
    session, start = np.empty(cap, np.uint32), np.empty(cap + 1, np.uint32)
    cnt, ocnt = np.zeros(1, np.uint64), np.zeros(1, np.uint64)
    i = abi.cc_events(*[_np(c) if n else None for c in cols], n, None)
    o = abi.cc_events(*[_np(out[name]) if n else None for name, _ in abi.EVENT_COLUMNS], n, _np(ocnt))
    d = abi.cc_route_dir(_np(session) if cap else None, _np(start), cap, _np(cnt))
    active = C.c_uint64()
    _check(lib().cc_route_events(C.byref(i), n, _np(tab) if len(tab) else None, _np(ids) if ids is not None else None,
                                 len(tab), int(n_sessions), _threads(threads), C.byref(o),
                                 _np(inst) if inst is not None else None, C.byref(d), C.byref(active)))
    k = int(active.value)
    if n == 0:
        start[0] = 0
    out["count"] = n
    return out, inst, (session[:k], start[:k + 1])


def route_events_device(ev, session_of_inst, n_sessions, id_of_inst=None, n_events=None, stream=None):
    """ev: a DeviceEvents (after apply_events, or shard.merge_events_device); session_of_inst / id_of_inst: uint32 /
    uint64 tables, numpy or device tensors -> (a DeviceEvents holding the routed stream, a uint64 device tensor of
    instance ids per routed row or None, (session, start) uint32 device tensors) (cc_route_events_device).  n_events
    defaults to the stream's count, read from the device.  The outputs are complete on return."""
    import torch

    from .engine import DeviceEvents, _check, _dptr, _stream_ptr, lib

    dev = ev.count.device
    st = _stream_on(stream, dev)
    n = int(ev.count.item()) if n_events is None else int(n_events)
    if n > ev.capacity:
        raise ValueError("the stream holds more events than its capacity (the apply overflowed)")

    def table(a, np_dt, t_dt):
        if a is None or isinstance(a, torch.Tensor):
            if a is not None and (a.dtype != t_dt or not a.is_contiguous() or a.device != dev):
                raise ValueError(f"a device table must be a contiguous {t_dt} tensor on the stream's device")
            return a
        return torch.from_numpy(np.ascontiguousarray(a, np_dt).view(np.int32 if np_dt == np.uint32 else np.int64)).to(dev).view(t_dt)

    tab, ids = table(session_of_inst, np.uint32, torch.uint32), table(id_of_inst, np.uint64, torch.uint64)
    if ids is not None and ids.numel() != tab.numel():
        raise ValueError("id_of_inst and session_of_inst must have one entry per instance slot")
    need = C.c_uint64()
    _check(lib().cc_route_events_device_bound(n, int(n_sessions), C.byref(need)))
    cap = min(n, int(n_sessions))
    with torch.cuda.stream(st):
        work = torch.empty(max(need.value, 16), dtype=torch.uint8, device=dev)
        out = DeviceEvents(max(n, 1), device=dev)
        inst = torch.empty(max(n, 1), dtype=torch.uint64, device=dev) if ids is not None else None
        session = torch.empty(max(cap, 1), dtype=torch.uint32, device=dev)
        start = torch.zeros(cap + 1, dtype=torch.uint32, device=dev)
        cnt = torch.zeros(1, dtype=torch.uint64, device=dev)
    out.capacity = n
    i, o = ev.struct(), out.struct()
    d = abi.cc_route_dir(session.data_ptr(), start.data_ptr(), cap, cnt.data_ptr())
    active = C.c_uint64()
    _check(lib().cc_route_events_device(C.byref(i), n, _dptr(tab) if tab.numel() else None, _dptr(ids), tab.numel(),
                                        int(n_sessions), C.byref(o), _dptr(inst), C.byref(d), C.byref(active),
                                        _dptr(work), work.numel(), _stream_ptr(st)))
    st.synchronize()
    k = int(active.value)
    return out, (inst[:n] if inst is not None else None), (session[:k], start[:k + 1])
