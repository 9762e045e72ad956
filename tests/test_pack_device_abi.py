"""cc_pack_from_device / cc_respack_to_device / cc_evpack_to_device (copycat_amd/csrc/host_path.hip, pack_enc.hip,
unpack_res.hip) on CPU.

The symbols are exported, abi.py's prototypes are the header's, and every argument check comes before the first HIP
call: the cases here are answered on a machine without a GPU.  The engine and the device columns are plain integers
that are never dereferenced (each call fails its check first, or has nothing to launch)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from copycat_amd import abi
from copycat_amd.batch import (Batch, _aligned_bytes, events_bound, pack, pack_bound, pack_events, pack_results)
from copycat_amd.engine import lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "copycat_apply.h")
NAMES = ("cc_pack_from_device", "cc_respack_to_device", "cc_evpack_to_device")
A = 0x10000  # a 16-byte aligned "device address"; also the never-dereferenced engine
ENGINE = C.c_void_p(A * 99)


def test_symbols_are_exported():
    """Fails without the feature: the three symbols do not exist."""
    L = C.CDLL(lib()._name)
    for name in NAMES:
        assert hasattr(L, name), name


def _ctype_of(param):
    if "*" in param:
        return C.c_void_p
    kind = param.replace("const", "").split()[0]
    return {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int": C.c_int}[kind]


def test_prototypes_match_the_header():
    text = open(HEADER).read()
    assert set(abi.PACK_DEVICE_PROTOTYPES) == set(NAMES)
    for name in NAMES:
        m = re.search(r"^(\w+)\s+" + name + r"\(([^;]*)\);", text, re.M)
        assert m, f"{name} is not declared in the header"
        res, args = abi.PACK_DEVICE_PROTOTYPES[name]
        assert m.group(1) == "int" and res is C.c_int
        want = [_ctype_of(p.strip()) for p in m.group(2).replace("\n", " ").split(",")]
        assert args == want, name
        f = getattr(lib(), name)  # engine.lib() binds what abi.py says
        assert f.restype is C.c_int and list(f.argtypes) == want
    assert abi.CC_ABI_VERSION == 6 and lib().cc_abi_version() == 6  # symbols are only added


def _cols(**change):
    s = abi.cc_batch(**{name: A * (k + 1) for k, (name, _) in enumerate(abi.BATCH_COLUMNS)})
    for k, v in change.items():
        setattr(s, k, v)
    return s


def test_null_engine_is_refused_before_any_hip_call():
    L = lib()
    blob = _aligned_bytes(pack_bound(100))
    size = C.c_uint64()
    s = _cols()
    assert L.cc_pack_from_device(None, C.byref(s), 100, blob.ctypes.data, blob.nbytes, C.byref(size), None) == abi.CC_ERR_INVALID
    assert L.cc_last_error()
    res = pack_results(np.zeros(10, np.uint8), np.arange(10, dtype=np.uint64))
    r = abi.cc_results(A, A * 2)
    assert L.cc_respack_to_device(None, res.ctypes.data, res.nbytes, C.byref(r), None) == abi.CC_ERR_INVALID
    ev = {"pos": np.arange(10, dtype=np.uint32), "target": np.zeros(10, np.uint32), "code": np.zeros(10, np.uint8),
          "src": np.zeros(10, np.uint8), "tag": np.zeros(10, np.uint8), "payload": np.arange(10, dtype=np.uint64)}
    evb = pack_events(ev)
    e = abi.cc_events(A, A * 2, A * 3, A * 4, A * 5, A * 6, 10, A * 7)
    assert L.cc_evpack_to_device(None, evb.ctypes.data, evb.nbytes, C.byref(e), None) == abi.CC_ERR_INVALID


def test_pack_from_device_refusals_leave_the_blob_untouched():
    L = lib()
    n = 1000
    bound = pack_bound(n)
    blob = _aligned_bytes(bound + 16)
    blob[:] = 0xCD
    size = C.c_uint64(7)

    def call(s, ptr, cap, sz=size):
        return L.cc_pack_from_device(ENGINE, C.byref(s) if s is not None else None, n, ptr, cap,
                                     C.byref(sz) if sz is not None else None, None)

    assert call(None, blob.ctypes.data, bound) == abi.CC_ERR_INVALID
    assert call(_cols(), blob.ctypes.data, bound, sz=None) == abi.CC_ERR_INVALID
    assert call(_cols(), None, bound) == abi.CC_ERR_INVALID
    assert call(_cols(), blob.ctypes.data + 8, bound) == abi.CC_ERR_INVALID  # a misaligned blob
    for name, off in (("key", 8), ("inst", 4), ("op", 1), ("b", 8)):  # a misaligned device column
        assert call(_cols(**{name: A + off}), blob.ctypes.data, bound) == abi.CC_ERR_INVALID, name
    assert size.value == 7
    assert call(_cols(), blob.ctypes.data, bound - 1) == abi.CC_ERR_CAPACITY and size.value == bound
    # the bound follows the present mask: without key, aux and time it is smaller, and is refused one byte short too
    few = _cols(key=None, aux=None, time=None)
    small = pack_bound(n, columns=("index", "inst", "op", "flags", "a", "b"))
    assert small < bound
    assert call(few, blob.ctypes.data, small - 1) == abi.CC_ERR_CAPACITY and size.value == small
    assert (blob == 0xCD).all()


def test_zero_rows_is_the_host_encoder_s_header_only_blob():
    """n == 0 launches nothing and touches neither the engine nor a column: the blob cc_pack_batch writes for no rows"""
    L = lib()
    for columns in (None, ("index", "inst", "op", "flags", "a", "b"), ("inst",)):
        want = pack(Batch(0), columns=columns)
        s = _cols(**{name: None for name, _ in abi.BATCH_COLUMNS if columns is not None and name not in columns})
        blob = _aligned_bytes(128)
        blob[:] = 0xCD
        size = C.c_uint64()
        assert L.cc_pack_from_device(ENGINE, C.byref(s), 0, blob.ctypes.data, blob.nbytes, C.byref(size), None) == abi.CC_OK
        assert size.value == len(want) == 64 and np.array_equal(blob[:64], want) and (blob[64:] == 0xCD).all()


def test_decoders_refuse_on_the_host():
    L = lib()
    st, va = np.arange(100, dtype=np.uint8), np.arange(100, dtype=np.uint64) * 3
    res = pack_results(st, va)
    r = abi.cc_results(A, A * 2)
    assert L.cc_respack_to_device(ENGINE, res.ctypes.data, res.nbytes, None, None) == abi.CC_ERR_INVALID
    bad = res.copy()
    bad[0] ^= 1  # the magic
    assert L.cc_respack_to_device(ENGINE, bad.ctypes.data, bad.nbytes, C.byref(r), None) == abi.CC_ERR_INVALID
    assert b"result blob" in L.cc_last_error()
    assert L.cc_respack_to_device(ENGINE, res.ctypes.data, res.nbytes - 1, C.byref(r), None) == abi.CC_ERR_INVALID
    for status, value in ((A + 1, A * 2), (A, A * 2 + 8), (None, A * 2), (A, None)):  # misaligned or missing outputs
        rr = abi.cc_results(status, value)
        assert L.cc_respack_to_device(ENGINE, res.ctypes.data, res.nbytes, C.byref(rr), None) == abi.CC_ERR_INVALID
    empty = pack_results(st[:0], va[:0])  # a header-only blob: nothing to write, no device needed
    assert L.cc_respack_to_device(ENGINE, empty.ctypes.data, empty.nbytes, C.byref(abi.cc_results(None, None)), None) == abi.CC_OK

    ev = {"pos": np.arange(100, dtype=np.uint32), "target": np.zeros(100, np.uint32), "code": np.zeros(100, np.uint8),
          "src": np.zeros(100, np.uint8), "tag": np.zeros(100, np.uint8), "payload": np.arange(100, dtype=np.uint64) * 5}
    evb = pack_events(ev)
    assert len(evb) <= events_bound(100)

    def events(capacity=100, **change):
        e = abi.cc_events(A, A * 2, A * 3, A * 4, A * 5, A * 6, capacity, A * 7)
        for k, v in change.items():
            setattr(e, k, v)
        return e

    def call(blob, e, nbytes=None):
        return L.cc_evpack_to_device(ENGINE, blob.ctypes.data, blob.nbytes if nbytes is None else nbytes, C.byref(e), None)

    assert call(evb, events(count=None)) == abi.CC_ERR_INVALID
    bad = evb.copy()
    bad[4] ^= 2  # the version
    assert call(bad, events()) == abi.CC_ERR_INVALID and b"event blob" in L.cc_last_error()
    assert call(evb, events(), nbytes=evb.nbytes - 16) == abi.CC_ERR_INVALID
    assert call(evb, events(capacity=99)) == abi.CC_ERR_CAPACITY
    r = pack_results(st, va)  # a result blob is no event blob, and the other way round
    assert call(r, events()) == abi.CC_ERR_INVALID
    assert L.cc_respack_to_device(ENGINE, evb.ctypes.data, evb.nbytes, C.byref(abi.cc_results(A, A * 2)), None) == abi.CC_ERR_INVALID


@pytest.mark.parametrize("name", NAMES)
def test_calls_are_documented_in_the_section_of_their_format(name):
    text = open(HEADER).read()
    section = {"cc_pack_from_device": "packed host batches", "cc_respack_to_device": "packed result blobs",
               "cc_evpack_to_device": "packed event blobs"}[name]
    heads = [(m.start(), m.group(1)) for m in re.finditer(r"/\* ---- ([^(\n]*?) \(", text)]
    at = text.index(name + "(")
    assert max(h for h in heads if h[0] < at)[1] == section
