"""ctypes binding of libcopycat_apply.so — the host mirror of the reference's state-machine interface.

`Engine` plays the role of the Copycat `StateMachine` the reference's ResourceManager implements
(manager/src/main/java/io/atomix/manager/ResourceManager.java:35-264): resources and instance sessions are
registered (getResource/createResource/deleteResource), then committed entries are applied — here a whole
batch per call instead of one `operateResource` per entry (:56-72).  Per-commit exceptions come back as
status codes (abi.CC_ST_*), never as a failed call.

The HIP library is the only compute path: if it is missing or fails to load, importing this module raises.
Torch is used only as the device allocator / stream provider (it is imported first so that the engine and
torch share one HIP runtime instance).
"""
import ctypes as C
import os

import numpy as np
import torch  # noqa: F401  (shared HIP runtime; device memory and streams)

from . import abi
from .batch import Batch

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("CC_ENGINE_SO") or os.path.join(_HERE, "libcopycat_apply.so")  # override: diagnostics builds
_LIB = None


# Result prefill of the test / bench paths: status 0xFF has result tag nibble 15, which no commit can return
# (tags 0..4), so a row the kernels never wrote is told apart from a legal NULL result (status 0, value 0).
RESULT_SENTINEL = 0xFF


class EngineError(RuntimeError):
    def __init__(self, rc, msg):
        super().__init__(f"cc error {rc}: {msg}")
        self.rc = rc


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(SO_PATH):
            raise ImportError(f"{SO_PATH} is missing: build it with `python -m copycat_amd.build` (hipcc, gfx950)")
        L = C.CDLL(SO_PATH)
        P, i32, u32, u64 = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64
        sig = {
            "cc_abi_version": (i32, []),
            "cc_last_error": (C.c_char_p, []),
            "cc_engine_create": (i32, [P, P]),
            "cc_engine_destroy": (i32, [P]),
            "cc_sync": (i32, [P]),
            "cc_engine_stream": (P, [P]),
            "cc_resource_create": (i32, [P, u32, u32]),
            "cc_resource_create_range": (i32, [P, u32, u32, u32]),
            "cc_resource_delete": (i32, [P, u32]),
            "cc_instance_open": (i32, [P, u32, u32, u64, u64]),
            "cc_instance_open_range": (i32, [P, u32, u32, u32, u64, u64]),
            "cc_apply_batch": (i32, [P, P, u64, P, P, P]),
            "cc_apply_batch_host": (i32, [P, P, u64, P]),
            "cc_apply_batch_host_events": (i32, [P, P, u64, P, P]),
            "cc_sessions_close_host": (i32, [P, P, u64, P, P]),
            "cc_sessions_expire_host": (i32, [P, P, u64, P, P]),
            "cc_advance_time_events_host": (i32, [P, u64, P]),
            "cc_retained_bitmap_host": (i32, [P, u64, u64, P, P]),
            "cc_device_alloc": (i32, [i32, u64, P]),
            "cc_device_free": (i32, [P]),
            "cc_memcpy": (i32, [P, P, u64, i32, P]),
            "cc_memset": (i32, [P, i32, u64, P]),
            "cc_applied_index": (i32, [P, P]),
            "cc_engine_counters": (i32, [P, P, u32]),
            "cc_applied_index_async": (i32, [P, P, P]),
            "cc_read_value_state": (i32, [P, u32, u32, P, P, P]),
            "cc_read_value_retained": (i32, [P, u32, u32, P]),
            "cc_read_map_entries": (i32, [P, u32, u64, P, P, P, P, P, P]),
            "cc_read_map_table": (i32, [P, u64, P, P, P, P, P, P, P]),
            "cc_read_lock_state": (i32, [P, u32, P, P, P, u64, P, P, P]),
            "cc_read_election_state": (i32, [P, u32, P, P, u64, P, P, P]),
            "cc_read_group_members": (i32, [P, u32, u64, P, P]),
            "cc_read_topic_listeners": (i32, [P, u32, u64, P, P, P]),
            "cc_read_bus_members": (i32, [P, u32, u64, P, P, P, P, P]),
            "cc_read_bus_registrations": (i32, [P, u32, u64, P, P, P, P]),
            "cc_read_retained": (i32, [P, u32, u64, P, P]),
            "cc_retained_bitmap": (i32, [P, u64, u64, P, P]),
            "cc_advance_time": (i32, [P, u64]),
            "cc_advance_time_events": (i32, [P, u64, P]),
            "cc_snapshot_size": (i32, [P, P]),
            "cc_snapshot_save": (i32, [P, P, u64]),
            "cc_snapshot_restore": (i32, [P, P, u64]),
            "cc_quorum_commit": (i32, [P, u32, u64, P, P, P, P]),
            "cc_expire_sweep": (i32, [P, u64, u64, u64, P, P, P]),
            "cc_profile_enable": (i32, [P, i32]),
            "cc_profile_reset": (i32, [P]),
            "cc_profile_read": (i32, [P, i32, P, P, P]),
            "cc_sessions_close": (i32, [P, P, u64, P, P, P]),
            "cc_sessions_expire": (i32, [P, P, u64, P, P, P]),
            "cc_get_resource": (i32, [P, u64, u32, u64, u64, P, P, P]),
            "cc_create_resource": (i32, [P, u64, u32, u64, u64, P, P, P]),
            "cc_resource_exists": (i32, [P, u64, P]),
            "cc_delete_resource": (i32, [P, u64, P]),
            "cc_instance_slot": (i32, [P, u64, P]),
            "cc_resource_slot": (i32, [P, u64, P]),
            "cc_debug_phases": (i32, [P, i32, P]),
            "cc_wire_codec_default": (None, [P]),
            "cc_wire_interner_create": (i32, [u64, P]),
            "cc_wire_interner_destroy": (i32, [P]),
            "cc_wire_intern": (i32, [P, P, u64, P]),
            "cc_wire_lookup": (i32, [P, u64, P, u64, P]),
            "cc_wire_string_hash": (i32, [P, u64, P]),
            "cc_handle_hashes": (i32, [P, P, P, u64]),
            "cc_wire_decode": (i32, [P, P, P, P, u64, P, u64, P, P]),
            "cc_wire_decode_to_device": (i32, [P, P, P, P, u64, P, u64, P, P, P, u64, P, P, P, P]),
            "cc_wire_timeline": (i32, [P, P]),
            "cc_wire_dict_attach": (i32, [P, P]),
            "cc_wire_dict_detach": (i32, [P]),
            "cc_wire_dict_get_info": (i32, [P, P]),
            "cc_apply_wire_host": (i32, [P, P, P, P, u64, P, u64, P, P, P, P, P, P]),
            "cc_split_batch": (i32, [P, u64, P, u32, u32, u32, P, P, P, P]),
            "cc_apply_batch_host_prefix": (i32, [P, P, u64, P, P, P]),
            "cc_apply_batch_prefix": (i32, [P, P, u64, P, P, P, P]),
            "cc_merge_results": (i32, [P, u64, P, u32, u32, u32, P, P]),
            "cc_split_device_bound": (i32, [u64, u32, P]),
            "cc_split_batch_device": (i32, [P, u64, P, u32, u32, P, P, P, P, P, u64, P]),
            "cc_merge_results_device": (i32, [P, u64, P, u32, u32, P, P, P, u64, P]),
            "cc_split_device_timing": (i32, [i32, P]),
            "cc_merge_events": (i32, [P, P, P, u64, u32, u32, P, P]),
            "cc_merge_events_device_bound": (i32, [u64, u32, P]),
            "cc_merge_events_device": (i32, [P, P, P, u64, u32, P, P, P, u64, P]),
            "cc_merge_events_device_timing": (i32, [i32, P]),
            "cc_route_events": (i32, [P, u64, P, P, u32, u32, u32, P, P, P, P]),
            "cc_route_events_device_bound": (i32, [u64, u32, P]),
            "cc_route_events_device": (i32, [P, u64, P, P, u32, u32, P, P, P, P, P, u64, P]),
            "cc_route_events_device_timing": (i32, [i32, P]),
            "cc_pack_bound": (i32, [u64, u32, P]),
            "cc_pack_batch": (i32, [P, u64, P, u64, u32, P]),
            "cc_pack_check": (i32, [P, u64, P, P]),
            "cc_unpack_batch": (i32, [P, u64, P, u32]),
            "cc_unpack_to_device": (i32, [P, P, u64, P, P]),
            "cc_apply_batch_host_packed": (i32, [P, P, u64, P, P, P, P]),
            "cc_packed_timeline": (i32, [P, u64, P, P]),
            "cc_host_register": (i32, [P, u64]),
            "cc_host_unregister": (i32, [P]),
            "cc_respack_bound": (i32, [u64, P]),
            "cc_respack_pack": (i32, [P, u64, P, u64, u32, P]),
            "cc_respack_check": (i32, [P, u64, P]),
            "cc_respack_unpack": (i32, [P, u64, P, u32]),
            "cc_respack_from_device": (i32, [P, P, u64, P, u64, P, P]),
            "cc_apply_batch_host_packed_results": (i32, [P, P, u64, P, u64, P, P, P, P]),
            "cc_packed_results_timeline": (i32, [P, u64, P, P]),
            "cc_evpack_bound": (i32, [u64, P]),
            "cc_evpack_pack": (i32, [P, u64, P, u64, u32, P]),
            "cc_evpack_check": (i32, [P, u64, P]),
            "cc_evpack_unpack": (i32, [P, u64, P, u32]),
            "cc_evpack_from_device": (i32, [P, P, P, u64, P, P, P]),
            "cc_apply_batch_host_packed_events": (i32, [P, P, u64, P, u64, P, P, u64, u64, P, P, P, P]),
            "cc_packed_events_timeline": (i32, [P, u64, P, P]),
            "cc_apply_wire_host_packed": (i32, [P, P, P, P, P, u64, P, P, u64, u64, P, P, P, P, P, P]),
            "cc_wire_packed_timeline": (i32, [P, u64, P, P]),
        }
        sig.update(abi.PACK_DEVICE_PROTOTYPES)
        sig.update(abi.SNAPSHOT_GROW_PROTOTYPES)
        # the value-only apply's group / segment arithmetic (host calls; a library picked through CC_ENGINE_SO for an
        # A/B against an earlier commit may predate them)
        value_group = {
            "cc_value_group_knob": (i32, [C.c_char_p, P]),
            "cc_value_group_plan": (i32, [u64, u64, u64, u64, P]),
            "cc_value_group_segment": (i32, [u64, u64, u64, u64, P]),
        }
        sig.update(value_group)
        for name, (res, args) in sig.items():
            if name in value_group and os.environ.get("CC_ENGINE_SO") and not hasattr(L, name):
                continue
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        if L.cc_abi_version() != abi.CC_ABI_VERSION:
            raise ImportError("libcopycat_apply.so ABI version mismatch")
        _LIB = L
    return _LIB


def _check(rc):
    if rc != abi.CC_OK:
        raise EngineError(rc, lib().cc_last_error().decode(errors="replace"))


def _np(a):
    return a.ctypes.data_as(C.c_void_p)


def _dptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream_ptr(stream):
    if stream is None:
        return None
    return C.c_void_p(stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream))


class DeviceBatch:
    """Batch columns resident in HBM (torch tensors on a HIP device)."""

    TORCH_DT = {"u8": torch.uint64, "u4": torch.uint32, "u1": torch.uint8}

    def __init__(self, cols, n):
        self.cols = cols
        self.n = n

    @classmethod
    def upload(cls, b: Batch, device="cuda", columns=None):
        cols = {}
        for name, dt in abi.BATCH_COLUMNS:
            if columns is not None and name not in columns:
                continue
            arr = getattr(b, name)
            cols[name] = torch.from_numpy(arr.view({"u8": np.int64, "u4": np.int32, "u1": np.uint8}[dt])).to(
                device, non_blocking=False).view(cls.TORCH_DT[dt])
        return cls(cols, len(b))

    def struct(self):
        s = abi.cc_batch()
        for name, _ in abi.BATCH_COLUMNS:
            t = self.cols.get(name)
            setattr(s, name, t.data_ptr() if t is not None else None)
        return s


class DeviceEvents:
    """An event stream in HBM (cc_events): columns of `capacity` rows + a device row counter."""

    def __init__(self, capacity, device="cuda"):
        self.capacity = capacity
        self.pos = torch.zeros(capacity, dtype=torch.int32, device=device)
        self.target = torch.zeros(capacity, dtype=torch.int32, device=device)
        self.code = torch.zeros(capacity, dtype=torch.uint8, device=device)
        self.src = torch.zeros(capacity, dtype=torch.uint8, device=device)
        self.tag = torch.zeros(capacity, dtype=torch.uint8, device=device)
        self.payload = torch.zeros(capacity, dtype=torch.int64, device=device)
        self.count = torch.zeros(1, dtype=torch.int64, device=device)

    def struct(self):
        return abi.cc_events(self.pos.data_ptr(), self.target.data_ptr(), self.code.data_ptr(), self.src.data_ptr(),
                             self.tag.data_ptr(), self.payload.data_ptr(), self.capacity, self.count.data_ptr())

    def host(self):
        m = min(int(self.count.item()), self.capacity)
        return {"pos": self.pos[:m].cpu().numpy().view(np.uint32), "target": self.target[:m].cpu().numpy().view(np.uint32),
                "code": self.code[:m].cpu().numpy(), "src": self.src[:m].cpu().numpy(), "tag": self.tag[:m].cpu().numpy(),
                "payload": self.payload[:m].cpu().numpy().view(np.uint64), "count": int(self.count.item())}


class Engine:
    def __init__(self, max_resources, max_instances, max_batch, device=0, flags=abi.CC_CFG_TIMERS_DEFERRED,
                 sub_batch=0, max_events=0, map_capacity=0, coord_cap=0):
        L = lib()
        cfg = abi.cc_config()
        cfg.coord_cap = coord_cap  # entries per coordination resource (0 = 64)
        cfg.max_resources = max_resources
        cfg.max_instances = max_instances
        cfg.max_batch = max_batch
        cfg.max_events = max_events
        cfg.map_capacity = map_capacity
        cfg.device = device
        cfg.flags = flags
        cfg.sub_batch = sub_batch
        h = C.c_void_p()
        _check(L.cc_engine_create(C.byref(cfg), C.byref(h)))
        self.h = h
        self.max_resources = max_resources
        self.max_instances = max_instances
        self.device = device
        self.L = L
        self._config = dict(max_resources=max_resources, max_instances=max_instances, max_batch=max_batch, device=device,
                            flags=flags, sub_batch=sub_batch, max_events=max_events, map_capacity=map_capacity,
                            coord_cap=coord_cap)

    def close(self):
        if self.h:
            self.L.cc_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- registry (ResourceManager control commands, host side) --------------------------------------
    def resource_create(self, slot, rtype):
        _check(self.L.cc_resource_create(self.h, slot, rtype))

    def resource_create_range(self, first, count, rtype):
        _check(self.L.cc_resource_create_range(self.h, first, count, rtype))

    def resource_delete(self, slot):
        _check(self.L.cc_resource_delete(self.h, slot))

    def instance_open(self, inst, res, instance_id, client):
        _check(self.L.cc_instance_open(self.h, inst, res, instance_id, client))

    def instance_open_range(self, first, count, res_first, id_first, client):
        _check(self.L.cc_instance_open_range(self.h, first, count, res_first, id_first, client))

    # ---- ResourceManager control commands (ResourceManager.java:77-235; manager.hip) ------------------------
    def _ctl(self, fn, key, rtype, client, index):
        iid, islot, st = C.c_uint64(), C.c_uint32(), C.c_uint8()
        _check(fn(self.h, key, rtype, client, index, C.byref(iid), C.byref(islot), C.byref(st)))
        return st.value, iid.value, islot.value

    def get_resource(self, key, rtype, client, index):
        """GetResource commit -> (status byte, instance id, instance slot)."""
        return self._ctl(self.L.cc_get_resource, key, rtype, client, index)

    def create_resource(self, key, rtype, client, index):
        """CreateResource commit -> (status byte, instance id, instance slot)."""
        return self._ctl(self.L.cc_create_resource, key, rtype, client, index)

    def resource_exists(self, key):
        out = C.c_uint8()
        _check(self.L.cc_resource_exists(self.h, key, C.byref(out)))
        return bool(out.value)

    def delete_resource(self, resource_id):
        """DeleteResource commit (by resource id) -> status byte."""
        st = C.c_uint8()
        _check(self.L.cc_delete_resource(self.h, resource_id, C.byref(st)))
        return st.value

    def instance_slot(self, instance_id):
        out = C.c_int64()
        _check(self.L.cc_instance_slot(self.h, instance_id, C.byref(out)))
        return out.value

    def resource_slot(self, resource_id):
        out = C.c_int64()
        _check(self.L.cc_resource_slot(self.h, resource_id, C.byref(out)))
        return out.value

    # ---- session close / expire fan-out (ResourceManager.java:237-264) -----------------------------------
    def sessions_close(self, clients, capacity=1 << 16, device="cuda"):
        """Close client sessions in order; returns (instances closed, events dict as DeviceEvents.host())."""
        arr = np.ascontiguousarray(np.asarray(clients, dtype=np.uint64).reshape(-1))
        evs = DeviceEvents(capacity, device=device)
        ev = evs.struct()
        closed = C.c_uint64()
        _check(self.L.cc_sessions_close(self.h, _np(arr) if len(arr) else None, len(arr), C.byref(ev), None,
                                        C.byref(closed)))
        return closed.value, evs.host()

    def sessions_expire(self, bitmap, sessions, capacity=1 << 16, device="cuda", events=None):
        """Close every client session whose bit is set in `bitmap` (a device u64 tensor, cc_expire_sweep's output),
        in ascending id order; returns (instances closed, events).  With `events` (a DeviceEvents the caller keeps)
        the close events stay in HBM and the second value is that DeviceEvents (no host copy)."""
        evs = events if events is not None else DeviceEvents(capacity, device=device)
        ev = evs.struct()
        closed = C.c_uint64()
        _check(self.L.cc_sessions_expire(self.h, _dptr(bitmap), sessions, C.byref(ev), None, C.byref(closed)))
        return closed.value, (evs if events is not None else evs.host())

    def handle_strings(self, strings):
        """Register the java.lang.String behind each HANDLE key ({handle: str}): its String.hashCode places the key in
        MapState's java.util.HashMap (containsValue order, treeifyBin resizes; cc_handle_hashes)."""
        from .batch import java_string_hash

        items = sorted(strings.items())
        if not items:
            return
        hk = np.array([h for h, _ in items], np.uint64)
        hv = np.array([java_string_hash(x) for _, x in items], np.int32)
        _check(self.L.cc_handle_hashes(self.h, _np(hk), _np(hv), len(items)))

    # ---- the hot path ----------------------------------------------------------------------------------
    def apply(self, db: DeviceBatch, status, value, stream=None):
        """Apply device-resident columns; `status` (uint8) / `value` (uint64) are device tensors of n rows."""
        s = db.struct()
        r = abi.cc_results(status.data_ptr(), value.data_ptr())
        _check(self.L.cc_apply_batch(self.h, C.byref(s), db.n, C.byref(r), None, _stream_ptr(stream)))

    def apply_events(self, db: DeviceBatch, status, value, events: "DeviceEvents", stream=None):
        """apply() with an event stream (device tensors, see DeviceEvents)."""
        s = db.struct()
        r = abi.cc_results(status.data_ptr(), value.data_ptr())
        ev = events.struct()
        _check(self.L.cc_apply_batch(self.h, C.byref(s), db.n, C.byref(r), C.byref(ev), _stream_ptr(stream)))

    def apply_host_events(self, b: Batch, capacity=None, device="cuda"):
        """Host batch -> (status, value, events) through the device path with an event stream; events is a dict of
        numpy columns (pos, target, code, src, tag, payload) in stream order (log row, then publish order)."""
        n = len(b)
        db = DeviceBatch.upload(b, device=device)
        status = torch.zeros(n, dtype=torch.uint8, device=device)
        value = torch.zeros(n, dtype=torch.int64, device=device)
        status.fill_(RESULT_SENTINEL)  # a row no kernel writes stays 0xFF: never a legal status (see RESULT_SENTINEL)
        value.fill_(-0x5A5A5A5A5A5A5A5B)
        evs = DeviceEvents(capacity if capacity is not None else max(4 * n, 1024), device=device)
        self.apply_events(db, status, value, evs)
        self.sync()
        return status.cpu().numpy(), value.cpu().numpy().view(np.uint64), evs.host()

    def apply_wire_host(self, decoder, index, time=None, entries=None, buf=None, offsets=None, capacity=None):
        """cc_apply_wire_host: the log segment itself (entries, or buf + offsets; `decoder` a WireDecoder on this engine)
        decoded on the GPU and applied up to the first manager entry -> (status, value, events, applied, control);
        control is None or the manager entry at row `applied` as a dict (row, kind, key, a, b): the host runs it and
        calls again from row applied + 1."""
        buf, offsets = decoder._segment(entries, buf, offsets)
        n = len(offsets) - 1
        index = np.ascontiguousarray(index, np.uint64)
        time = None if time is None else np.ascontiguousarray(time, np.uint64)
        assert len(index) == n and (time is None or len(time) == n)
        status = np.full(n, RESULT_SENTINEL, np.uint8)
        value = np.zeros(n, np.uint64)
        cap = capacity if capacity is not None else max(4 * n, 1024)
        ev = {"pos": np.zeros(cap, np.uint32), "target": np.zeros(cap, np.uint32), "code": np.zeros(cap, np.uint8),
              "src": np.zeros(cap, np.uint8), "tag": np.zeros(cap, np.uint8), "payload": np.zeros(cap, np.uint64)}
        count = C.c_uint64(0)
        hev = abi.cc_events(*(ev[k].ctypes.data for k in ("pos", "target", "code", "src", "tag", "payload")), cap,
                            C.cast(C.byref(count), C.c_void_p))
        r = abi.cc_results(status.ctypes.data, value.ctypes.data)
        applied = C.c_uint64(0)
        ctl = abi.cc_wire_control()
        _check(self.L.cc_apply_wire_host(self.h, C.byref(decoder.codec), decoder.interner.h, _np(buf), buf.size,
                                         _np(offsets), n, _np(index), _np(time) if time is not None else None,
                                         C.byref(r), C.byref(hev), C.byref(applied), C.byref(ctl)))
        m = applied.value
        control = None
        if m < n:
            control = {k: int(getattr(ctl, k)) for k in ("row", "kind", "key", "a", "b")}
        return status[:m], value[:m], {k: v[:count.value] for k, v in ev.items()}, m, control

    def apply_wire_host_packed(self, decoder, index, time=None, entries=None, buf=None, offsets=None, capacity=None,
                               chunk_rows=0, timeline=False, events=True, out=None, ev_out=None, aux=None):
        """cc_apply_wire_host_packed: apply_wire_host through the chunk pipeline -> (result_blob, event_blob, ev_count,
        rows_done, ctl).  index / time travel as a packed blob (batch.pack); batch.unpack_results(result_blob) and
        batch.unpack_events(event_blob) give the rows and events (pos = segment rows) of the chunks applied.  ctl is
        None, or the manager entry at row rows_done as a dict (row, kind, key, a, b): the host runs it and calls again
        from row rows_done + 1.  A call that stops at a chunk on a capacity returns normally with rows_done < n and
        ctl None; a decode failure raises EngineError with .bad_row, .rows_done and the two blobs attached.
        events=False: no event stream (event_blob is None).  `out` / `ev_out`: 16-byte-aligned uint8 buffers of at
        least batch.results_bound(n) / batch.events_bound(capacity) bytes (e.g. page-locked with host_register).
        `aux`: the packed index / time blob itself (index and time are then ignored), e.g. packed once and page-locked."""
        from .batch import Batch, pack

        buf, offsets = decoder._segment(entries, buf, offsets, check=False)
        n = len(offsets) - 1
        if aux is None:
            b = Batch(n)
            b.index[:] = np.ascontiguousarray(index, np.uint64)
            if time is not None:
                b.time[:] = np.ascontiguousarray(time, np.uint64)
            aux = pack(b, columns=("index",) if time is None else ("index", "time"))
        seg = abi.cc_wire_segment(buf.ctypes.data, buf.size, offsets.ctypes.data, n, aux.ctypes.data, aux.nbytes)
        return self._wire_packed(decoder, seg, n, capacity, chunk_rows, timeline, events, out, ev_out, (buf, offsets, aux))

    def _wire_packed(self, decoder, seg, n, capacity, chunk_rows, timeline, events, out, ev_out, keep):
        from .batch import _aligned_bytes, events_bound, results_bound

        cap = capacity if capacity is not None else max(4 * n, 1024)
        res = out if out is not None else _aligned_bytes(results_bound(n))
        evb = None
        if events:
            evb = ev_out if ev_out is not None else _aligned_bytes(events_bound(cap))
        opts = abi.cc_packed_opts(chunk_rows=chunk_rows, flags=abi.CC_PACKED_TIMELINE if timeline else 0)
        done, size, ev_size, ev_count, bad = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        ctl = abi.cc_wire_control()
        rc = self.L.cc_apply_wire_host_packed(self.h, C.byref(decoder.codec), decoder.interner.h, C.byref(seg),
                                              res.ctypes.data, res.nbytes, C.byref(size),
                                              evb.ctypes.data if events else None, cap, evb.nbytes if events else 0,
                                              C.byref(ev_size), C.byref(ev_count), C.byref(opts), C.byref(done),
                                              C.byref(ctl), C.byref(bad))
        blobs_ok = size.value <= res.nbytes and (not events or ev_size.value <= evb.nbytes)
        rblob = res[:size.value] if blobs_ok else None
        eblob = evb[:ev_size.value] if events and blobs_ok else None
        if rc != abi.CC_OK and not (rc == abi.CC_ERR_CAPACITY and done.value < n and blobs_ok):
            err = EngineError(rc, lib().cc_last_error().decode(errors="replace"))
            err.bad_row, err.rows_done, err.result_blob, err.event_blob = bad.value, done.value, rblob, eblob
            err.ev_count = ev_count.value
            raise err
        control = None
        if rc == abi.CC_OK and done.value < n:
            control = {k: int(getattr(ctl, k)) for k in ("row", "kind", "key", "a", "b")}
        return rblob, eblob, ev_count.value, done.value, control

    def wire_packed_timeline(self):
        """Per chunk of the last apply_wire_host_packed(timeline=True): (H2D, decode, apply, encode, D2H) ms."""
        n = C.c_uint64()
        _check(self.L.cc_wire_packed_timeline(self.h, 0, C.byref(n), None))
        ms = np.zeros((max(n.value, 1), 5), np.float32)
        _check(self.L.cc_wire_packed_timeline(self.h, n.value, C.byref(n), _np(ms)))
        return ms[:n.value]

    def wire_timeline(self):
        """cc_wire_timeline: (H2D, kernel, escape round trip) milliseconds of the last decode on the device."""
        ms = (C.c_float * 3)()
        _check(self.L.cc_wire_timeline(self.h, ms))
        return tuple(float(x) for x in ms)

    def apply_host(self, b: Batch):
        """PCIe-inclusive path: host columns in, host results out (H2D + apply + D2H + sync)."""
        n = len(b)
        status = np.full(n, RESULT_SENTINEL, np.uint8)  # cc_apply_batch_host prefills too; a row never written stays 0xFF
        value = np.zeros(n, np.uint64)
        s = abi.cc_batch()
        for name, _ in abi.BATCH_COLUMNS:
            setattr(s, name, getattr(b, name).ctypes.data)
        r = abi.cc_results(status.ctypes.data, value.ctypes.data)
        _check(self.L.cc_apply_batch_host(self.h, C.byref(s), n, C.byref(r)))
        return status, value

    def apply_host_prefix(self, b: Batch, capacity=None):
        """cc_apply_batch_host_prefix: rows applied up to the first commit a full coordination collection cannot hold.
        Returns (applied, status, value, events): `applied` = rows applied (len(b) on success; the engine state is the
        one after exactly those rows), events as apply_host_events returns them (numpy columns)."""
        n = len(b)
        status = np.full(n, RESULT_SENTINEL, np.uint8)
        value = np.zeros(n, np.uint64)
        s = abi.cc_batch()
        for name, _ in abi.BATCH_COLUMNS:
            setattr(s, name, getattr(b, name).ctypes.data)
        r = abi.cc_results(status.ctypes.data, value.ctypes.data)
        cap = capacity if capacity is not None else max(4 * n, 1024)
        cols = {"pos": np.zeros(cap, np.uint32), "target": np.zeros(cap, np.uint32), "code": np.zeros(cap, np.uint8),
                "src": np.zeros(cap, np.uint8), "tag": np.zeros(cap, np.uint8), "payload": np.zeros(cap, np.uint64)}
        count = np.zeros(1, np.uint64)
        ev = abi.cc_events(*(cols[k].ctypes.data for k in ("pos", "target", "code", "src", "tag", "payload")), cap,
                           count.ctypes.data)
        applied = C.c_uint64()
        rc = self.L.cc_apply_batch_host_prefix(self.h, C.byref(s), n, C.byref(r), C.byref(ev), C.byref(applied))
        if rc not in (abi.CC_OK, abi.CC_ERR_CAPACITY) or (rc == abi.CC_ERR_CAPACITY and applied.value >= n):
            _check(rc)
        m = int(min(count[0], cap))
        return applied.value, status, value, {k: v[:m] for k, v in cols.items()}

    def apply_prefix(self, db: DeviceBatch, status, value, events: "DeviceEvents" = None, stream=None):
        """cc_apply_batch_prefix: apply() / apply_events() with the stop-before-row contract of apply_host_prefix on
        device-resident columns.  Returns the rows applied: db.n on success, fewer when the next row meets a full
        coordination collection, map table region or event stream (the engine state, `status` / `value` rows and
        `events` are then exactly those after the applied rows; the rows from there on keep what the tensors held).
        Synchronous.  Any other failure raises."""
        s = db.struct()
        r = abi.cc_results(status.data_ptr(), value.data_ptr())
        ev = events.struct() if events is not None else None
        applied = C.c_uint64()
        rc = self.L.cc_apply_batch_prefix(self.h, C.byref(s), db.n, C.byref(r), C.byref(ev) if ev is not None else None,
                                          _stream_ptr(stream), C.byref(applied))
        if rc not in (abi.CC_OK, abi.CC_ERR_CAPACITY) or (rc == abi.CC_ERR_CAPACITY and applied.value >= db.n):
            _check(rc)
        return applied.value

    def apply_host_packed(self, blob, n, capacity=None, chunk_rows=0, events=True, out=None, timeline=False):
        """cc_apply_batch_host_packed: a packed blob (batch.pack) of n rows in, host results and events out, pipelined in
        chunks of `chunk_rows` rows (0 = 16 Mi).  Returns (status, value, events, rows_done): what apply_host_events
        returns plus the rows of the chunks fully applied (n on success).  A call that stops at a chunk on a capacity
        returns normally with rows_done < n (events["count"] then includes the failing chunk's events); any other
        failure raises.  events=False: no event stream (as apply_host; the third value is None).  `out`: (status,
        value) numpy arrays to write into (e.g. page-locked with host_register)."""
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        status, value = out if out is not None else (np.full(n, RESULT_SENTINEL, np.uint8), np.zeros(n, np.uint64))
        r = abi.cc_results(status.ctypes.data, value.ctypes.data)
        opts = abi.cc_packed_opts(chunk_rows=chunk_rows, flags=abi.CC_PACKED_TIMELINE if timeline else 0)
        done = C.c_uint64()
        ev, cols, count = None, None, np.zeros(1, np.uint64)
        if events:
            cap = capacity if capacity is not None else max(4 * n, 1024)
            cols = {"pos": np.zeros(cap, np.uint32), "target": np.zeros(cap, np.uint32), "code": np.zeros(cap, np.uint8),
                    "src": np.zeros(cap, np.uint8), "tag": np.zeros(cap, np.uint8), "payload": np.zeros(cap, np.uint64)}
            ev = abi.cc_events(*(cols[k].ctypes.data for k in ("pos", "target", "code", "src", "tag", "payload")), cap,
                               count.ctypes.data)
        rc = self.L.cc_apply_batch_host_packed(self.h, blob.ctypes.data, blob.nbytes, C.byref(r),
                                               C.byref(ev) if ev is not None else None, C.byref(opts), C.byref(done))
        if rc != abi.CC_OK and not (rc == abi.CC_ERR_CAPACITY and done.value < n):
            _check(rc)
        evs = None
        if events:
            m = int(min(count[0], cap))
            evs = {k: v[:m] for k, v in cols.items()}
            evs["count"] = int(count[0])
        return status, value, evs, done.value

    def packed_timeline(self):
        """Per chunk of the last apply_host_packed(timeline=True): (H2D, decode, apply, D2H) milliseconds."""
        n = C.c_uint64()
        _check(self.L.cc_packed_timeline(self.h, 0, C.byref(n), None))
        ms = np.zeros((max(n.value, 1), 4), np.float32)
        _check(self.L.cc_packed_timeline(self.h, n.value, C.byref(n), _np(ms)))
        return ms[:n.value]

    def results_to_host_packed(self, status, value, stream=None, out=None):
        """cc_respack_from_device: device result tensors (status uint8, value 64-bit, n rows each, 16-byte aligned) ->
        a packed result blob in host memory (batch.unpack_results decodes it), byte for byte batch.pack_results of the
        same rows.  Synchronous.  `out`: a 16-byte-aligned uint8 buffer of at least batch.results_bound(n) bytes."""
        from .batch import _aligned_bytes, results_bound

        n = status.numel()
        blob = out if out is not None else _aligned_bytes(results_bound(n))
        r = abi.cc_results(status.data_ptr(), value.data_ptr())
        size = C.c_uint64()
        _check(self.L.cc_respack_from_device(self.h, C.byref(r), n, blob.ctypes.data, blob.nbytes, C.byref(size),
                                             _stream_ptr(stream)))
        return blob[:size.value]

    def apply_host_packed_results(self, blob, n, capacity=None, chunk_rows=0, events=True, out=None, timeline=False):
        """cc_apply_batch_host_packed_results: apply_host_packed with the results as a packed result blob.  Returns
        (result_blob, events, rows_done); batch.unpack_results(result_blob) gives the (status, value) rows of the chunks
        whose results the wide call copies out (results_info(result_blob)["n"] of them).  `out`: a 16-byte-aligned uint8
        buffer of at least batch.results_bound(n) bytes to write the blob into (e.g. page-locked with host_register)."""
        from .batch import _aligned_bytes, results_bound

        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        res = out if out is not None else _aligned_bytes(results_bound(n))
        opts = abi.cc_packed_opts(chunk_rows=chunk_rows, flags=abi.CC_PACKED_TIMELINE if timeline else 0)
        done, size = C.c_uint64(), C.c_uint64()
        ev, cols, count = None, None, np.zeros(1, np.uint64)
        if events:
            cap = capacity if capacity is not None else max(4 * n, 1024)
            cols = {"pos": np.zeros(cap, np.uint32), "target": np.zeros(cap, np.uint32), "code": np.zeros(cap, np.uint8),
                    "src": np.zeros(cap, np.uint8), "tag": np.zeros(cap, np.uint8), "payload": np.zeros(cap, np.uint64)}
            ev = abi.cc_events(*(cols[k].ctypes.data for k in ("pos", "target", "code", "src", "tag", "payload")), cap,
                               count.ctypes.data)
        rc = self.L.cc_apply_batch_host_packed_results(self.h, blob.ctypes.data, blob.nbytes, res.ctypes.data, res.nbytes,
                                                       C.byref(size), C.byref(ev) if ev is not None else None,
                                                       C.byref(opts), C.byref(done))
        if rc != abi.CC_OK and not (rc == abi.CC_ERR_CAPACITY and done.value < n and size.value <= res.nbytes):
            _check(rc)
        evs = None
        if events:
            m = int(min(count[0], cap))
            evs = {k: v[:m] for k, v in cols.items()}
            evs["count"] = int(count[0])
        return res[:size.value], evs, done.value

    def packed_results_timeline(self):
        """Per chunk of the last apply_host_packed_results(timeline=True): (H2D, decode, apply, encode, D2H) ms."""
        n = C.c_uint64()
        _check(self.L.cc_packed_results_timeline(self.h, 0, C.byref(n), None))
        ms = np.zeros((max(n.value, 1), 5), np.float32)
        _check(self.L.cc_packed_results_timeline(self.h, n.value, C.byref(n), _np(ms)))
        return ms[:n.value]

    def events_to_host_packed(self, events, stream=None, out=None):
        """cc_evpack_from_device: a device event stream (DeviceEvents) -> (event_blob, count): a packed event blob in
        host memory (batch.unpack_events decodes it), byte for byte batch.pack_events of the first min(count, capacity)
        events, and the device count.  Synchronous.  count > capacity raises EngineError (CC_ERR_CAPACITY) carrying the
        blob of the first `capacity` events as .blob and the count as .count.  `out`: a 16-byte-aligned uint8 buffer of
        at least batch.events_bound(events.capacity) bytes."""
        from .batch import _aligned_bytes, events_bound

        blob = out if out is not None else _aligned_bytes(events_bound(events.capacity))
        s = events.struct()
        size, count = C.c_uint64(), C.c_uint64()
        rc = self.L.cc_evpack_from_device(self.h, C.byref(s), blob.ctypes.data, blob.nbytes, C.byref(size), C.byref(count),
                                          _stream_ptr(stream))
        if rc == abi.CC_ERR_CAPACITY and size.value <= blob.nbytes and count.value > events.capacity:
            err = EngineError(rc, lib().cc_last_error().decode(errors="replace"))
            err.blob, err.count = blob[:size.value], count.value
            raise err
        _check(rc)
        return blob[:size.value], count.value

    def apply_host_packed_events(self, blob, n, capacity=None, chunk_rows=0, out=None, ev_out=None, timeline=False):
        """cc_apply_batch_host_packed_events: apply_host_packed_results with the events as a packed event blob of at most
        `capacity` events.  Returns (result_blob, event_blob, ev_count, rows_done): batch.unpack_events(event_blob) gives
        the events of the chunks fully applied (pos = batch rows); ev_count is what the wide call leaves in its event
        count.  `out` / `ev_out`: 16-byte-aligned uint8 buffers of at least batch.results_bound(n) /
        batch.events_bound(capacity) bytes (e.g. page-locked with host_register)."""
        from .batch import _aligned_bytes, events_bound, results_bound

        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        cap = capacity if capacity is not None else max(4 * n, 1024)
        res = out if out is not None else _aligned_bytes(results_bound(n))
        evb = ev_out if ev_out is not None else _aligned_bytes(events_bound(cap))
        opts = abi.cc_packed_opts(chunk_rows=chunk_rows, flags=abi.CC_PACKED_TIMELINE if timeline else 0)
        done, size, ev_size, ev_count = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        rc = self.L.cc_apply_batch_host_packed_events(self.h, blob.ctypes.data, blob.nbytes, res.ctypes.data, res.nbytes,
                                                      C.byref(size), evb.ctypes.data, cap, evb.nbytes, C.byref(ev_size),
                                                      C.byref(ev_count), C.byref(opts), C.byref(done))
        if rc != abi.CC_OK and not (rc == abi.CC_ERR_CAPACITY and done.value < n and size.value <= res.nbytes
                                    and ev_size.value <= evb.nbytes):
            _check(rc)
        return res[:size.value], evb[:ev_size.value], ev_count.value, done.value

    def packed_events_timeline(self):
        """Per chunk of the last apply_host_packed_events(timeline=True): (H2D, decode, apply, result encode, result D2H,
        event encode, event D2H) milliseconds; the event blob is encoded and sent once per call, so the last two figures
        are the call's in every row."""
        n = C.c_uint64()
        _check(self.L.cc_packed_events_timeline(self.h, 0, C.byref(n), None))
        ms = np.zeros((max(n.value, 1), 7), np.float32)
        _check(self.L.cc_packed_events_timeline(self.h, n.value, C.byref(n), _np(ms)))
        return ms[:n.value]

    def unpack_to_device(self, blob, cols, stream=None):
        """cc_unpack_to_device: decode a packed host blob into device column tensors ({name: tensor}, n rows each)."""
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        s = abi.cc_batch_out()
        for name, _ in abi.BATCH_COLUMNS:
            t = cols.get(name)
            setattr(s, name, t.data_ptr() if t is not None else None)
        _check(self.L.cc_unpack_to_device(self.h, blob.ctypes.data, blob.nbytes, C.byref(s), _stream_ptr(stream)))

    def batch_to_host_packed(self, db, stream=None, out=None):
        """cc_pack_from_device: device batch columns (a DeviceBatch; an absent column is left out of the blob) -> a packed
        batch blob in host memory, byte for byte batch.pack of the same columns: what apply_host_packed* and
        unpack_to_device take.  Synchronous.  `out`: a 16-byte-aligned uint8 buffer of at least batch.pack_bound bytes
        for the present columns."""
        from .batch import _aligned_bytes

        s = db.struct()
        present = sum(1 << k for k, (name, _) in enumerate(abi.BATCH_COLUMNS) if db.cols.get(name) is not None)
        blob = out
        if blob is None:
            bound = C.c_uint64()
            _check(self.L.cc_pack_bound(db.n, present, C.byref(bound)))
            blob = _aligned_bytes(bound.value)
        size = C.c_uint64()
        _check(self.L.cc_pack_from_device(self.h, C.byref(s), db.n, blob.ctypes.data, blob.nbytes, C.byref(size),
                                          _stream_ptr(stream)))
        return blob[:size.value]

    def results_to_device(self, blob, status, value, stream=None):
        """cc_respack_to_device: a packed result blob in host memory -> the device tensors status (uint8) and value
        (64-bit), results_info(blob)["n"] rows each, 16-byte aligned; byte for byte batch.unpack_results.  Stream-ordered
        and not waited for: sync before `blob` or this engine is used again."""
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        r = abi.cc_results(status.data_ptr(), value.data_ptr())
        _check(self.L.cc_respack_to_device(self.h, blob.ctypes.data, blob.nbytes, C.byref(r), _stream_ptr(stream)))

    def events_to_device(self, blob, events, stream=None):
        """cc_evpack_to_device: a packed event blob in host memory -> the device event stream `events` (DeviceEvents of
        capacity >= the blob's events), its device count word included; byte for byte batch.unpack_events.  `events` is
        then what merge_events_device and events_to_host_packed take.  Stream-ordered and not waited for: sync before
        `blob` or this engine is used again."""
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        s = events.struct()
        _check(self.L.cc_evpack_to_device(self.h, blob.ctypes.data, blob.nbytes, C.byref(s), _stream_ptr(stream)))

    def sync(self):
        _check(self.L.cc_sync(self.h))

    def stream(self):
        return self.L.cc_engine_stream(self.h)

    def counters(self):
        """(barrier rows applied, containsValue rows answered in the stream, sub-batches, map events) since creation,
        and the big HashMap models held now (maps past capacity 64 with a tree bin)."""
        out = np.zeros(5, np.uint64)
        _check(self.L.cc_engine_counters(self.h, out.ctypes.data, 5))
        return tuple(int(x) for x in out)

    def applied_index(self):
        out = C.c_uint64()
        _check(self.L.cc_applied_index(self.h, C.byref(out)))
        return out.value

    def applied_index_async(self, out, stream=None):
        """Write the applied watermark into the device tensor `out` (one int64), stream-ordered, no host sync."""
        _check(self.L.cc_applied_index_async(self.h, C.c_void_p(out.data_ptr()), _stream_ptr(stream)))

    # ---- per-kernel HIP-event timing ------------------------------------------------------------------
    def profile(self, on=True):
        _check(self.L.cc_profile_enable(self.h, 1 if on else 0))
        _check(self.L.cc_profile_reset(self.h))

    def profile_read(self):
        """{kernel name: (total device ms, launches)} since the last profile() call (synchronizes)."""
        out = {}
        for k in range(abi.CC_PROFILE_KERNELS):
            ms, n, name = C.c_double(), C.c_uint64(), C.c_char_p()
            _check(self.L.cc_profile_read(self.h, k, C.byref(ms), C.byref(n), C.byref(name)))
            out[name.value.decode()] = (ms.value, n.value)
        return out

    def value_state(self, first=0, count=None):
        count = self.max_resources - first if count is None else count
        tag, val, cur = np.zeros(count, np.uint8), np.zeros(count, np.uint64), np.zeros(count, np.uint8)
        _check(self.L.cc_read_value_state(self.h, first, count, _np(tag), _np(val), _np(cur)))
        return tag, val, cur

    def value_retained(self, first=0, count=None):
        """Per value slot, the log index of the commit AtomicValueState still retains (0 = none)."""
        count = self.max_resources - first if count is None else count
        idx = np.zeros(count, np.uint64)
        _check(self.L.cc_read_value_retained(self.h, first, count, _np(idx)))
        return idx

    def advance_time(self, now):
        _check(self.L.cc_advance_time(self.h, now))

    def advance_time_events(self, now, capacity=1024, device="cuda"):
        """advance_time publishing the events of group timers that come due (see cc_advance_time_events)."""
        evs = DeviceEvents(capacity, device=device)
        ev = evs.struct()
        _check(self.L.cc_advance_time_events(self.h, now, C.byref(ev)))
        return evs.host()

    def snapshot(self) -> bytes:
        """The engine's whole state (device arrays + host registry mirrors) as bytes (cc_snapshot_save)."""
        n = C.c_uint64()
        _check(self.L.cc_snapshot_size(self.h, C.byref(n)))
        buf = np.zeros(n.value, np.uint8)
        _check(self.L.cc_snapshot_save(self.h, _np(buf), n.value))
        return buf.tobytes()

    def restore(self, snap: bytes, grow=False):
        """Load a snapshot into this engine: one of the same max_resources / max_instances / map_capacity / coord_cap
        (cc_snapshot_restore), or with grow=True one whose map_capacity and coord_cap are no larger than this engine's
        (cc_snapshot_restore_grow)."""
        buf = np.frombuffer(snap, np.uint8).copy()
        fn = self.L.cc_snapshot_restore_grow if grow else self.L.cc_snapshot_restore
        _check(fn(self.h, _np(buf), len(buf)))

    @staticmethod
    def snapshot_info(snap: bytes) -> dict:
        """What a snapshot was taken from (cc_snapshot_info: the header only, no engine and no device)."""
        buf = np.frombuffer(snap, np.uint8).copy()
        info = abi.cc_snapshot_info_t()
        _check(lib().cc_snapshot_info(_np(buf), len(buf), C.byref(info)))
        return {name: getattr(info, name) for name, _ in abi.cc_snapshot_info_t._fields_}

    def grown(self, coord_cap=None, map_capacity=None):
        """A new engine of this engine's configuration with a larger coord_cap and / or map_capacity, holding this
        engine's state (snapshot, then restore with grow=True).  This engine stays as it is; close it when done."""
        cfg = dict(self._config)
        if coord_cap is not None:
            cfg["coord_cap"] = coord_cap
        if map_capacity is not None:
            cfg["map_capacity"] = map_capacity
        snap = self.snapshot()
        e = Engine(**cfg)
        try:
            e.restore(snap, grow=True)
        except Exception:
            e.close()
            raise
        return e

    def lock_state(self, slot, cap=1024):
        """(holder instance slot or -1, holder index, holder cleaned, [(waiter instance slot, index)])"""
        h, hi, hc, n = C.c_int64(), C.c_uint64(), C.c_uint8(), C.c_uint64()
        qi, qx = np.zeros(cap, np.uint32), np.zeros(cap, np.uint64)
        _check(self.L.cc_read_lock_state(self.h, slot, C.byref(h), C.byref(hi), C.byref(hc), cap, C.byref(n), _np(qi),
                                         _np(qx)))
        m = min(n.value, cap)
        return h.value, hi.value, hc.value, list(zip(qi[:m].tolist(), qx[:m].tolist()))

    def election_state(self, slot, cap=1024):
        """(leader instance slot or -1, leader index, [(listener instance slot, index)])"""
        ld, li, n = C.c_int64(), C.c_uint64(), C.c_uint64()
        qi, qx = np.zeros(cap, np.uint32), np.zeros(cap, np.uint64)
        _check(self.L.cc_read_election_state(self.h, slot, C.byref(ld), C.byref(li), cap, C.byref(n), _np(qi), _np(qx)))
        m = min(n.value, cap)
        return ld.value, li.value, list(zip(qi[:m].tolist(), qx[:m].tolist()))

    def group_members(self, slot, cap=4096):
        ids, n = np.zeros(cap, np.uint64), C.c_uint64()
        _check(self.L.cc_read_group_members(self.h, slot, cap, C.byref(n), _np(ids)))
        return ids[:min(n.value, cap)].tolist()

    def topic_listeners(self, slot, cap=4096):
        """[(listener instance id, its Listen commit index)], ascending by id (cc_read_topic_listeners)"""
        ids, idx, n = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64), C.c_uint64()
        _check(self.L.cc_read_topic_listeners(self.h, slot, cap, C.byref(n), _np(ids), _np(idx)))
        m = min(n.value, cap)
        return list(zip(ids[:m].tolist(), idx[:m].tolist()))

    def read_bus_members(self, slot, cap=4096):
        """[(member instance id, address handle, Join commit index, cleaned)], ascending by id (cc_read_bus_members)"""
        ids, addr, idx = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64), np.zeros(cap, np.uint64)
        cl, n = np.zeros(cap, np.uint8), C.c_uint64()
        _check(self.L.cc_read_bus_members(self.h, slot, cap, C.byref(n), _np(ids), _np(addr), _np(idx), _np(cl)))
        m = min(n.value, cap)
        return list(zip(ids[:m].tolist(), addr[:m].tolist(), idx[:m].tolist(), cl[:m].astype(bool).tolist()))

    def read_bus_registrations(self, slot, cap=4096):
        """[(topic handle, registrant instance id, Register commit index)], ascending by (topic, id); a topic whose
        registration map is empty is one row (topic, 0, 0) (cc_read_bus_registrations)"""
        tp, ids, idx, n = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64), np.zeros(cap, np.uint64), C.c_uint64()
        _check(self.L.cc_read_bus_registrations(self.h, slot, cap, C.byref(n), _np(tp), _np(ids), _np(idx)))
        m = min(n.value, cap)
        return list(zip(tp[:m].tolist(), ids[:m].tolist(), idx[:m].tolist()))

    def retained(self, slot):
        """Ascending log indices of every commit the slot's state machine still holds without having clean()ed it
        (cc_read_retained) — the layout of the oracle's retained()."""
        n = C.c_uint64()
        _check(self.L.cc_read_retained(self.h, slot, 0, C.byref(n), None))
        out = np.zeros(max(n.value, 1), np.uint64)
        _check(self.L.cc_read_retained(self.h, slot, n.value, C.byref(n), _np(out)))
        return out[:n.value].tolist()

    def retained_bitmap(self, first, count, out=None, device="cuda"):
        """cc_retained_bitmap: (device u64 bitmap over log indices [first, first + count), retained count)."""
        words = (count + 63) // 64
        bm = out if out is not None else torch.empty(max(words, 1), dtype=torch.int64, device=device)
        n = C.c_uint64()
        _check(self.L.cc_retained_bitmap(self.h, first, count, _dptr(bm), C.byref(n)))
        return bm, n.value

    def map_entries(self, slot):
        """MapState entries of one map slot sorted by (key tag, key): (key_tag, key, value_tag, value, commit_index)
        — the same layout as the oracle's map_entries."""
        n = C.c_uint64()
        _check(self.L.cc_read_map_entries(self.h, slot, 0, C.byref(n), None, None, None, None, None))
        m = n.value
        kt, k, vt, v, ci = (np.zeros(m, np.uint8), np.zeros(m, np.uint64), np.zeros(m, np.uint8),
                            np.zeros(m, np.uint64), np.zeros(m, np.uint64))
        _check(self.L.cc_read_map_entries(self.h, slot, m, C.byref(n), _np(kt), _np(k), _np(vt), _np(v), _np(ci)))
        return kt, k, vt, v, ci

    def map_table(self):
        """Every map / set slot's entries in one table pass, sorted by (slot, key tag, key):
        (slot, key_tag, key, value_tag, value, commit_index)."""
        n = C.c_uint64()
        _check(self.L.cc_read_map_table(self.h, 0, C.byref(n), None, None, None, None, None, None))
        m = n.value
        sl, kt, k, vt, v, ci = (np.zeros(m, np.uint32), np.zeros(m, np.uint8), np.zeros(m, np.uint64),
                                np.zeros(m, np.uint8), np.zeros(m, np.uint64), np.zeros(m, np.uint64))
        _check(self.L.cc_read_map_table(self.h, m, C.byref(n), _np(sl), _np(kt), _np(k), _np(vt), _np(v), _np(ci)))
        return sl, kt, k, vt, v, ci


def host_register(arr):
    """Page-lock a numpy array's memory (cc_host_register) so asynchronous copies from / into it overlap."""
    _check(lib().cc_host_register(C.c_void_p(arr.ctypes.data), arr.nbytes))


def host_unregister(arr):
    _check(lib().cc_host_unregister(C.c_void_p(arr.ctypes.data)))


def quorum_commit(match, term_start, commit_in, commit_out, stream=None):
    """match: (replicas, groups) uint64 device tensor; others (groups,) uint64 device tensors."""
    replicas, groups = match.shape
    _check(lib().cc_quorum_commit(_dptr(match), replicas, groups, _dptr(term_start), _dptr(commit_in), _dptr(commit_out),
                                  _stream_ptr(stream)))


def expire_sweep(last, now, timeout, bitmap, count, stream=None):
    _check(lib().cc_expire_sweep(_dptr(last), last.numel(), now, timeout, _dptr(bitmap), _dptr(count),
                                 _stream_ptr(stream)))
