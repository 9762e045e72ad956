"""Host-side column encoder: committed commits -> the SoA columns of `cc_batch`.

This is the host half of the drop-in boundary.  In the reference each committed entry is an
InstanceCommand/InstanceQuery {long instance; op} (InstanceOperation.java:59-69) whose inner op carries
its operands (e.g. MapCommands.TtlCommand key/value/ttl, MapCommands.java:215-250).  The encoder turns a
run of such entries into fixed-width columns (one row per entry, log order) that the engine applies in
one call.  Values are canonical tagged values (tag, payload) — see include/copycat_apply.h.
"""
import numpy as np

from . import abi


class Batch:
    """A batch of committed entries as numpy columns (host memory)."""

    __slots__ = tuple(name for name, _ in abi.BATCH_COLUMNS)

    def __init__(self, n):
        for name, dt in abi.BATCH_COLUMNS:
            setattr(self, name, np.zeros(n, dtype=np.dtype(dt)))

    def __len__(self):
        return len(self.op)

    @classmethod
    def from_columns(cls, **cols):
        n = len(cols["op"])
        b = cls(0)
        for name, dt in abi.BATCH_COLUMNS:
            if name in cols and cols[name] is not None:
                arr = np.ascontiguousarray(cols[name], dtype=np.dtype(dt))
                if len(arr) != n:
                    raise ValueError(f"column {name} has {len(arr)} rows, expected {n}")
            else:
                arr = np.zeros(n, dtype=np.dtype(dt))
            setattr(b, name, arr)
        return b

    def slice(self, lo, hi):
        b = Batch(0)
        for name, _ in abi.BATCH_COLUMNS:
            setattr(b, name, getattr(self, name)[lo:hi].copy())  # a copy: callers reuse the source buffer
        return b

    def columns(self):
        return {name: getattr(self, name) for name, _ in abi.BATCH_COLUMNS}


def _pack_lib():
    from .engine import lib  # (the packed-batch calls live in the engine library; no device is touched)

    return lib()


def _pack_fail(rc):
    from .engine import EngineError

    raise EngineError(rc, _pack_lib().cc_last_error().decode(errors="replace"))


def _aligned_bytes(n, align=64):
    buf = np.zeros(n + align, np.uint8)
    off = (-buf.ctypes.data) % align
    return buf[off:off + n]


def pack_bound(n, columns=None):
    """cc_pack_bound: the worst-case size of a blob of n rows with all nine columns, or with those named in `columns`."""
    import ctypes as C

    present = sum(1 << c for c, (name, _) in enumerate(abi.BATCH_COLUMNS) if columns is None or name in columns)
    bound = C.c_uint64()
    rc = _pack_lib().cc_pack_bound(n, present, C.byref(bound))
    if rc:
        _pack_fail(rc)
    return bound.value


def pack(b, columns=None, threads=0, out=None):
    """cc_pack_batch: the batch's columns (all nine, or those named in `columns`; the others are absent, the NULL
    column pointers of cc_batch) as one packed blob, a 16-byte-aligned uint8 array.  `out`: a 16-byte-aligned uint8
    buffer to pack into (e.g. page-locked once and reused); the result is then a view of it.  Give it pack_bound()
    bytes: into a smaller buffer the encoder first sizes the blob (it never writes into a buffer it refuses), one more
    pass over the columns."""
    import ctypes as C

    L = _pack_lib()
    n = len(b)
    s = abi.cc_batch()
    present = 0
    keep = []  # (the contiguous columns, alive across the call)
    for c, (name, dt) in enumerate(abi.BATCH_COLUMNS):
        if columns is None or name in columns:
            arr = np.ascontiguousarray(getattr(b, name), dtype=np.dtype(dt))
            keep.append(arr)
            setattr(s, name, arr.ctypes.data)
            present |= 1 << c
    blob = out
    if blob is None:
        blob = _aligned_bytes(pack_bound(n, columns))
    size = C.c_uint64()
    rc = L.cc_pack_batch(C.byref(s), n, blob.ctypes.data, blob.nbytes, threads, C.byref(size))
    if rc:
        _pack_fail(rc)
    return blob[:size.value]


def pack_check(blob):
    """cc_pack_check: (n, present mask) of a well-formed blob; raises EngineError (CC_ERR_INVALID) otherwise."""
    import ctypes as C

    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    n, present = C.c_uint64(), C.c_uint32()
    rc = _pack_lib().cc_pack_check(blob.ctypes.data, blob.nbytes, C.byref(n), C.byref(present))
    if rc:
        _pack_fail(rc)
    return n.value, present.value


def unpack(blob, threads=0):
    """cc_unpack_batch: the host decoder.  Absent columns come back as zeros (see pack_check for the mask)."""
    import ctypes as C

    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    n, present = pack_check(blob)
    b = Batch(n)
    s = abi.cc_batch_out()
    for c, (name, _) in enumerate(abi.BATCH_COLUMNS):
        if (present >> c) & 1:
            setattr(s, name, getattr(b, name).ctypes.data)
    rc = _pack_lib().cc_unpack_batch(blob.ctypes.data, blob.nbytes, C.byref(s), threads)
    if rc:
        _pack_fail(rc)
    return b


def pack_info(blob):
    """The directory of a packed blob: {"n", "blocks", "bytes", "present", "bytes_per_row", "columns": {name:
    {"rows": {(mode, width): rows}, "bytes_per_row": packed bytes per row, "blocks": [(mode, width, base), ...]}}}."""
    import ctypes as C

    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    n, present = pack_check(blob)
    hd = abi.cc_pack_header.from_buffer_copy(blob[:C.sizeof(abi.cc_pack_header)].tobytes())
    lo = C.sizeof(abi.cc_pack_header)
    dir_ = (abi.cc_pack_block * hd.blocks).from_buffer_copy(blob[lo:lo + hd.blocks * C.sizeof(abi.cc_pack_block)].tobytes())
    cols = {}
    for c, (name, _) in enumerate(abi.BATCH_COLUMNS):
        if not (present >> c) & 1:
            continue
        rows, blocks, size = {}, [], 0
        for blk in dir_:
            e = blk.col[c]
            rows[(e.mode, e.width)] = rows.get((e.mode, e.width), 0) + blk.rows
            blocks.append((e.mode, e.width, e.base))
            size += blk.rows * e.width
        cols[name] = {"rows": rows, "blocks": blocks, "bytes_per_row": size / n if n else 0.0}
    return {"n": n, "blocks": hd.blocks, "bytes": hd.bytes, "present": present,
            "bytes_per_row": hd.bytes / n if n else 0.0, "columns": cols}


def results_bound(n):
    """cc_respack_bound: the worst-case size of a packed result blob of n rows."""
    import ctypes as C

    bound = C.c_uint64()
    rc = _pack_lib().cc_respack_bound(n, C.byref(bound))
    if rc:
        _pack_fail(rc)
    return bound.value


def pack_results(status, value, threads=0, out=None):
    """cc_respack_pack, the host reference encoder: result rows (status uint8, value uint64) as one packed result blob,
    a 16-byte-aligned uint8 array.  `out`: a 16-byte-aligned uint8 buffer to pack into; the result is a view of it."""
    import ctypes as C

    status = np.ascontiguousarray(status, dtype=np.uint8)
    value = np.ascontiguousarray(value)
    value = value.view(np.uint64) if value.dtype == np.int64 else np.ascontiguousarray(value, dtype=np.uint64)
    if len(status) != len(value):
        raise ValueError(f"status has {len(status)} rows, value {len(value)}")
    n = len(status)
    blob = out if out is not None else _aligned_bytes(results_bound(n))
    r = abi.cc_results(status.ctypes.data, value.ctypes.data)
    size = C.c_uint64()
    rc = _pack_lib().cc_respack_pack(C.byref(r), n, blob.ctypes.data, blob.nbytes, threads, C.byref(size))
    if rc:
        _pack_fail(rc)
    return blob[:size.value]


def results_check(blob):
    """cc_respack_check: the rows of a well-formed result blob; raises EngineError (CC_ERR_INVALID) otherwise."""
    import ctypes as C

    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    n = C.c_uint64()
    rc = _pack_lib().cc_respack_check(blob.ctypes.data, blob.nbytes, C.byref(n))
    if rc:
        _pack_fail(rc)
    return n.value


def unpack_results(blob, threads=0):
    """cc_respack_unpack, the host decoder: (status, value) numpy columns of a packed result blob."""
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    n = results_check(blob)
    status, value = np.zeros(n, np.uint8), np.zeros(n, np.uint64)
    r = abi.cc_results(status.ctypes.data, value.ctypes.data)
    import ctypes as C

    rc = _pack_lib().cc_respack_unpack(blob.ctypes.data, blob.nbytes, C.byref(r), threads)
    if rc:
        _pack_fail(rc)
    return status, value


def results_info(blob):
    """The directory of a packed result blob, as pack_info: {"n", "blocks", "bytes", "bytes_per_row", "columns":
    {"status" / "value": {"rows": {(mode, width): rows}, "bytes_per_row", "blocks": [(mode, width, base), ...]}}}."""
    import ctypes as C

    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    n = results_check(blob)
    hd = abi.cc_pack_header.from_buffer_copy(blob[:C.sizeof(abi.cc_pack_header)].tobytes())
    lo = C.sizeof(abi.cc_pack_header)
    dir_ = (abi.cc_respack_block * hd.blocks).from_buffer_copy(
        blob[lo:lo + hd.blocks * C.sizeof(abi.cc_respack_block)].tobytes())
    cols = {}
    for c, name in enumerate(abi.RESULT_COLUMNS):
        rows, blocks, size = {}, [], 0
        for blk in dir_:
            e = blk.col[c]
            rows[(e.mode, e.width)] = rows.get((e.mode, e.width), 0) + blk.rows
            blocks.append((e.mode, e.width, e.base))
            size += blk.rows * e.width
        cols[name] = {"rows": rows, "blocks": blocks, "bytes_per_row": size / n if n else 0.0}
    return {"n": n, "blocks": hd.blocks, "bytes": hd.bytes, "bytes_per_row": hd.bytes / n if n else 0.0, "columns": cols}


def events_bound(n):
    """cc_evpack_bound: the worst-case size of a packed event blob of n events."""
    import ctypes as C

    bound = C.c_uint64()
    rc = _pack_lib().cc_evpack_bound(n, C.byref(bound))
    if rc:
        _pack_fail(rc)
    return bound.value


def pack_events(events, threads=0, out=None):
    """cc_evpack_pack, the host reference encoder: event columns ({"pos", "target", "code", "src", "tag", "payload"}, as
    apply_host_events returns them) as one packed event blob, a 16-byte-aligned uint8 array.  `out`: a 16-byte-aligned
    uint8 buffer to pack into; the result is a view of it."""
    import ctypes as C

    cols = []
    for name, dt in abi.EVENT_COLUMNS:
        a = np.ascontiguousarray(events[name])
        a = a.view(np.dtype(dt)) if a.dtype.kind == "i" and a.dtype.itemsize == np.dtype(dt).itemsize else a
        cols.append(np.ascontiguousarray(a, dtype=np.dtype(dt)))
    n = len(cols[0])
    if any(len(c) != n for c in cols):
        raise ValueError("event columns differ in length")
    blob = out if out is not None else _aligned_bytes(events_bound(n))
    ev = abi.cc_events(*(c.ctypes.data for c in cols), n, None)
    size = C.c_uint64()
    rc = _pack_lib().cc_evpack_pack(C.byref(ev), n, blob.ctypes.data, blob.nbytes, threads, C.byref(size))
    if rc:
        _pack_fail(rc)
    return blob[:size.value]


def events_check(blob):
    """cc_evpack_check: the events of a well-formed event blob; raises EngineError (CC_ERR_INVALID) otherwise."""
    import ctypes as C

    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    n = C.c_uint64()
    rc = _pack_lib().cc_evpack_check(blob.ctypes.data, blob.nbytes, C.byref(n))
    if rc:
        _pack_fail(rc)
    return n.value


def unpack_events(blob, threads=0):
    """cc_evpack_unpack, the host decoder: the six numpy columns of a packed event blob, as a dict."""
    import ctypes as C

    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    n = events_check(blob)
    cols = {name: np.zeros(n, np.dtype(dt)) for name, dt in abi.EVENT_COLUMNS}
    count = np.zeros(1, np.uint64)
    ev = abi.cc_events(*(cols[name].ctypes.data for name, _ in abi.EVENT_COLUMNS), n, count.ctypes.data)
    rc = _pack_lib().cc_evpack_unpack(blob.ctypes.data, blob.nbytes, C.byref(ev), threads)
    if rc:
        _pack_fail(rc)
    return cols


def events_info(blob):
    """The directory of a packed event blob, as pack_info: {"n", "blocks", "bytes", "bytes_per_row", "columns": {name:
    {"rows": {(mode, width): rows}, "bytes_per_row", "blocks": [(mode, width, base, entries), ...]}}}; `entries` is a
    CC_PK_BY_POS table's entry count (0 in mode CC_PK_FOR)."""
    import ctypes as C

    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    n = events_check(blob)
    hd = abi.cc_pack_header.from_buffer_copy(blob[:C.sizeof(abi.cc_pack_header)].tobytes())
    lo = C.sizeof(abi.cc_pack_header)
    dir_ = (abi.cc_evpack_block * hd.blocks).from_buffer_copy(
        blob[lo:lo + hd.blocks * C.sizeof(abi.cc_evpack_block)].tobytes())
    cols = {}
    for c, (name, _) in enumerate(abi.EVENT_COLUMNS):
        rows, blocks, size = {}, [], 0
        for blk in dir_:
            e = blk.col[c]
            rows[(e.mode, e.width)] = rows.get((e.mode, e.width), 0) + blk.rows
            blocks.append((e.mode, e.width, e.base, e.reserved16))
            size += (e.reserved16 if e.mode == abi.CC_PK_BY_POS else blk.rows) * e.width
        cols[name] = {"rows": rows, "blocks": blocks, "bytes_per_row": size / n if n else 0.0}
    return {"n": n, "blocks": hd.blocks, "bytes": hd.bytes, "bytes_per_row": hd.bytes / n if n else 0.0, "columns": cols}


def tagged(v):
    """Python value -> canonical (tag, payload).  None -> NULL; bool -> BOOL; int -> LONG.

    Use `Int(x)` for java.lang.Integer and `Handle(h)` for interned objects (strings, callbacks)."""
    if v is None:
        return abi.CC_TAG_NULL, 0
    if isinstance(v, Int):
        return abi.CC_TAG_INT, v.v & 0xFFFFFFFFFFFFFFFF
    if isinstance(v, Handle):
        return abi.CC_TAG_HANDLE, v.h
    if isinstance(v, bool):
        return abi.CC_TAG_BOOL, int(v)
    if isinstance(v, int):
        return abi.CC_TAG_LONG, v & 0xFFFFFFFFFFFFFFFF
    raise TypeError(f"no canonical encoding for {type(v)}")


def untagged(tag, payload):
    """Inverse of `tagged` (LONG payloads become signed Python ints)."""
    payload = int(payload)
    if tag == abi.CC_TAG_NULL:
        return None
    if tag == abi.CC_TAG_LONG:
        return payload - (1 << 64) if payload >> 63 else payload
    if tag == abi.CC_TAG_INT:
        p = payload & 0xFFFFFFFF
        return Int(p - (1 << 32) if p >> 31 else p)
    if tag == abi.CC_TAG_BOOL:
        return bool(payload)
    if tag == abi.CC_TAG_HANDLE:
        return Handle(payload)
    if tag == abi.CC_TAG_SET:
        return ("set", payload)
    if tag == abi.CC_TAG_MAP:  # MessageBusState.join: the topic count; the rows are in the event stream
        return ("map", payload)
    raise ValueError(f"unknown tag {tag}")


class Int:
    """A java.lang.Integer value (Long(1) != Integer(1))."""

    __slots__ = ("v",)

    def __init__(self, v):
        self.v = int(v)

    def __eq__(self, o):
        return isinstance(o, Int) and o.v == self.v

    def __hash__(self):
        return hash(("Int", self.v))

    def __repr__(self):
        return f"Int({self.v})"


class Handle:
    """A host-interned object (String, serialized Runnable, ...): equality is handle equality."""

    __slots__ = ("h",)

    def __init__(self, h):
        self.h = int(h)

    def __eq__(self, o):
        return isinstance(o, Handle) and o.h == self.h

    def __hash__(self):
        return hash(("Handle", self.h))

    def __repr__(self):
        return f"Handle({self.h})"


def java_string_hash(s):
    """java.lang.String.hashCode: s[0]*31^(n-1) + ... + s[n-1] over the UTF-16 code units, as a Java int."""
    b = s.encode("utf-16-le")
    h = 0
    for i in range(0, len(b), 2):
        h = (31 * h + (b[i] | (b[i + 1] << 8))) & 0xFFFFFFFF
    return h - (1 << 32) if h >> 31 else h


class Interner:
    """Interns host objects (e.g. Java Strings) to HANDLE ids so `equals` is id equality."""

    def __init__(self):
        self._ids = {}
        self._objs = []

    def __call__(self, obj):
        if obj not in self._ids:
            self._ids[obj] = len(self._objs) + 1
            self._objs.append(obj)
        return Handle(self._ids[obj])

    def lookup(self, h):
        return self._objs[h.h - 1]


class Encoder:
    """Appends committed entries one at a time (for tests / small host-side batches)."""

    def __init__(self):
        self.rows = []

    def add(self, inst, op, index=0, time=0, key=None, a=None, b=None, aux=0):
        ta, pa = tagged(a)
        tb, pb = tagged(b)
        if key is None:
            kt, kp = 0, 0
        else:
            t, kp = tagged(key)
            if t == abi.CC_TAG_NULL:
                raise ValueError("map keys are never null (MapCommands.java:77)")
            kt = abi.KTAG_OF_TAG[t]
        self.rows.append((index, time, inst, op, abi.cc_flags(ta, tb, kt), kp, pa, pb, aux & 0xFFFFFFFFFFFFFFFF))
        return len(self.rows) - 1

    def batch(self):
        n = len(self.rows)
        b = Batch(n)
        for i, r in enumerate(self.rows):
            (b.index[i], b.time[i], b.inst[i], b.op[i], b.flags[i], b.key[i], b.a[i], b.b[i], b.aux[i]) = r
        return b
