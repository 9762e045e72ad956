"""Catalyst wire format -> engine columns (host side of cc_wire_decode, include/copycat_apply.h).

A committed Atomix resource entry is InstanceCommand / InstanceQuery {writeLong(instance id); writeObject(op)}
(manager/src/main/java/io/atomix/resource/InstanceOperation.java:60-69); WireDecoder turns a run of such entries
(plus manager GetResource / CreateResource / DeleteResource / ResourceExists entries) into a Batch the engine
applies, resolving instance ids through the engine's session registry and interning Strings to HANDLE values."""
import ctypes as C

import numpy as np

from . import abi
from .batch import Batch
from .engine import _check, _np, lib

KIND_OP, KIND_GET, KIND_CREATE, KIND_DELETE, KIND_EXISTS = 0, 35, 36, 37, 38


def default_codec():
    c = abi.cc_wire_codec()
    lib().cc_wire_codec_default(C.byref(c))
    return c


class Interner:
    """String <-> CC_TAG_HANDLE handle (cc_wire_interner): equal bytes, equal handle."""

    def __init__(self, first_handle=1):
        self.h = C.c_void_p()
        _check(lib().cc_wire_interner_create(first_handle, C.byref(self.h)))

    def __del__(self):
        try:
            lib().cc_wire_interner_destroy(self.h)
        except Exception:
            pass

    def intern(self, s):
        b = s.encode() if isinstance(s, str) else bytes(s)
        out = C.c_uint64()
        buf = (C.c_uint8 * max(len(b), 1)).from_buffer_copy(b or b"\0")
        _check(lib().cc_wire_intern(self.h, buf, len(b), C.byref(out)))
        return out.value

    def lookup(self, handle):
        n = C.c_uint64()
        _check(lib().cc_wire_lookup(self.h, handle, None, 0, C.byref(n)))
        buf = (C.c_uint8 * max(n.value, 1))()
        _check(lib().cc_wire_lookup(self.h, handle, buf, n.value, C.byref(n)))
        return bytes(buf[:n.value]).decode()


class WireDecoder:
    """Decodes log entries (one bytes object each, or a buffer + offsets) into a Batch and per-row kinds."""

    def __init__(self, engine=None, interner=None, codec=None):
        self.engine = engine
        self.interner = interner or Interner()
        self.codec = codec or default_codec()

    @staticmethod
    def _segment(entries, buf, offsets, check=True):
        if entries is not None:
            offsets = np.zeros(len(entries) + 1, np.uint64)
            offsets[1:] = np.cumsum([len(e) for e in entries])
            buf = np.frombuffer(b"".join(entries) or b"\0", np.uint8)
        buf = np.ascontiguousarray(buf, np.uint8)  # (a contiguous uint8 view, an odd address included, stays as it is)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        if check and len(offsets) > 1 and int(offsets[-1]) > buf.size:
            raise ValueError(f"offsets end at {int(offsets[-1])} past the {buf.size}-byte buffer")
        return buf, offsets

    def decode_to_device(self, entries=None, buf=None, offsets=None, device="cuda", stream=None, ctl_cap=None,
                         check_offsets=True):
        """cc_wire_decode_to_device: the same decode with the plain entries parsed on the GPU and the columns left in
        device memory -> (DeviceBatch, iid tensor, kind, stats).  kind (numpy, as decode's) is rebuilt from the control
        list; stats is a dict (rows, device_rows, host_rows).  The DeviceBatch's index / time columns are zero: they
        are the log entries' own."""
        import torch

        from .engine import DeviceBatch, _stream_ptr

        assert self.engine is not None, "decode_to_device needs an engine"
        buf, offsets = self._segment(entries, buf, offsets, check_offsets)
        n = len(offsets) - 1
        cols = {}
        for name, dt in abi.BATCH_COLUMNS:
            cols[name] = torch.zeros(max(n, 1), dtype={"u8": torch.int64, "u4": torch.int32, "u1": torch.uint8}[dt],
                                     device=device).view(DeviceBatch.TORCH_DT[dt])[:n]
        iid = torch.zeros(max(n, 1), dtype=torch.int64, device=device).view(torch.uint64)[:n]
        out = abi.cc_batch_out()
        for name in ("inst", "op", "flags", "key", "a", "b", "aux"):
            setattr(out, name, cols[name].data_ptr())
        cap = n if ctl_cap is None else ctl_cap
        ctl = (abi.cc_wire_control * max(cap, 1))()
        nctl = C.c_uint64(0)
        stats = abi.cc_wire_stats()
        bad = C.c_uint64(~0 & 0xFFFFFFFFFFFFFFFF)
        torch.cuda.synchronize()  # (the zero fills above run on torch's stream)
        rc = lib().cc_wire_decode_to_device(self.engine.h, C.byref(self.codec), self.interner.h, _np(buf), buf.size,
                                            _np(offsets), n, C.byref(out), iid.data_ptr(), ctl, cap, C.byref(nctl),
                                            C.byref(stats), _stream_ptr(stream), C.byref(bad))
        self.bad_row, self.ctl_count = bad.value, nctl.value
        self.last_device = (DeviceBatch(cols, n), iid)  # (what a failed call decoded, for inspection)
        _check(rc)
        kind = np.zeros(n, np.uint8)
        for k in range(nctl.value):
            kind[ctl[k].row] = ctl[k].kind
        return DeviceBatch(cols, n), iid, kind, {k: int(getattr(stats, k)) for k in ("rows", "device_rows", "host_rows")}

    def attach_dictionary(self):
        """cc_wire_dict_attach: upload this decoder's interner to the engine as the device String dictionary; from
        then on decode_to_device / Engine.apply_wire_host with this decoder resolve its known Strings on the GPU."""
        assert self.engine is not None, "attach_dictionary needs an engine"
        _check(lib().cc_wire_dict_attach(self.engine.h, self.interner.h))

    def detach_dictionary(self):
        """cc_wire_dict_detach: free the engine's dictionary (whichever decoder attached it)."""
        assert self.engine is not None, "detach_dictionary needs an engine"
        _check(lib().cc_wire_dict_detach(self.engine.h))

    def dictionary_info(self):
        """cc_wire_dict_get_info -> dict (strings, long_strings, pool_bytes, cells, full_uploads, last_sync_strings,
        last_str_rows)"""
        assert self.engine is not None, "dictionary_info needs an engine"
        info = abi.cc_wire_dict_info()
        _check(lib().cc_wire_dict_get_info(self.engine.h, C.byref(info)))
        return {name: int(getattr(info, name)) for name, _ in abi.cc_wire_dict_info._fields_}

    def decode(self, entries=None, buf=None, offsets=None):
        buf, offsets = self._segment(entries, buf, offsets)
        n = len(offsets) - 1
        b = Batch(n)
        iid = np.zeros(n, np.uint64)
        kind = np.zeros(n, np.uint8)
        out = abi.cc_wire_out(inst=_np(b.inst), iid=_np(iid), op=_np(b.op), flags=_np(b.flags), key=_np(b.key),
                              a=_np(b.a), b=_np(b.b), aux=_np(b.aux), kind=_np(kind))
        bad = C.c_uint64(~0 & 0xFFFFFFFFFFFFFFFF)
        eh = self.engine.h if self.engine is not None else None
        _check(lib().cc_wire_decode(eh, C.byref(self.codec), self.interner.h, _np(buf), buf.size, _np(offsets), n,
                                    C.byref(out), C.byref(bad)))
        return b, iid, kind
