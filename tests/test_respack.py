"""Packed result blobs on the CPU (copycat_amd/csrc/respack.cpp): the reference encoder, the validator and the decoder.

Bar: exact.  A decoded blob equals the result columns byte for byte; the blob is the same for every thread count; the
directory carries the width the encoder rule demands and the blob's size follows from the widths; the validator refuses
every malformed blob and the decoder then writes nothing."""
import ctypes as C

import numpy as np
import pytest

from copycat_amd import abi
from copycat_amd.batch import _aligned_bytes, pack_results, results_bound, results_check, results_info, unpack_results
from copycat_amd.engine import EngineError, lib
from tests import respack_cases as rc
from tests.pack_cases import B

HEADER, ENTRY = rc.HEADER, rc.ENTRY


def _aligned_copy(blob):
    out = _aligned_bytes(len(blob))
    out[:] = blob
    return out


def test_struct_sizes():
    assert C.sizeof(abi.cc_respack_block) == ENTRY == 48
    assert C.sizeof(abi.cc_pack_header) == HEADER == 64
    assert abi.cc_respack_block.col.offset == 16 and C.sizeof(abi.cc_pack_col) == 16
    assert abi.CC_RESPACK_MAGIC == int.from_bytes(b"CCPR", "little")


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 4095, 4096, 4097, 12293])
def test_round_trip_and_thread_independence(n):
    status, value = rc.random_results(n, seed=n + 1)
    blobs = [pack_results(status, value, threads=t) for t in (1, 3, 0)]
    assert all(np.array_equal(blobs[0], b) for b in blobs[1:]), "the blob depends on the thread count"
    blob = blobs[0]
    assert blob.ctypes.data % 16 == 0 and len(blob) <= results_bound(n)
    assert results_check(blob) == n
    for t in (1, 3, 0):
        s, v = unpack_results(blob, threads=t)
        assert s.tobytes() == status.tobytes() and v.tobytes() == value.tobytes()
    info = results_info(blob)
    assert info["n"] == n and info["blocks"] == (n + B - 1) // B and info["bytes"] == len(blob)
    if n == 0:
        assert len(blob) == HEADER


def test_width_selection_and_blob_size():
    status, value, expect = rc.width_rows()
    cases = rc.width_cases()
    blob = pack_results(status, value)
    info = results_info(blob)
    seen = {"status": set(), "value": set()}
    for k, ((sw, sbase), (vw, vbase)) in enumerate(expect):
        name = cases[k][0]
        assert info["columns"]["status"]["blocks"][k] == (rc.FOR, sw, sbase), name
        assert info["columns"]["value"]["blocks"][k] == (rc.FOR, vw, vbase), name
        seen["status"].add(sw), seen["value"].add(vw)
    assert seen == {"status": {0, 1}, "value": {0, 1, 2, 4, 8}}  # every (column, width) the format allows
    assert len(blob) == rc.blob_bytes([(len(c[1]), c[3][0], c[4][0]) for c in cases])
    s, v = unpack_results(blob)
    assert s.tobytes() == status.tobytes() and v.tobytes() == value.tobytes()


# ---- refusals -------------------------------------------------------------------------------------------------------------
def _put(blob, at, value, size):
    blob[at:at + size] = np.frombuffer(int(value).to_bytes(size, "little"), np.uint8)


def _get(blob, at, size):
    return int.from_bytes(blob[at:at + size].tobytes(), "little")


E0, E1 = HEADER, HEADER + ENTRY  # the two directory entries of the blob below
MUTATIONS = [
    ("magic", lambda b: _put(b, 0, abi.CC_PACK_MAGIC, 4), "bad magic"),
    ("version", lambda b: _put(b, 4, 2, 4), "version"),
    ("present", lambda b: _put(b, 32, 1, 4), "present"),
    ("n", lambda b: _put(b, 8, _get(b, 8, 8) + 1, 8), "rows"),
    ("blocks", lambda b: _put(b, 16, 3, 8), "block count"),
    ("bytes", lambda b: _put(b, 24, len(b) + 16, 8), "larger than the buffer"),
    ("block_rows", lambda b: _put(b, E0, B - 1, 4), "rows"),
    ("misaligned_offset", lambda b: _put(b, E0 + 36, _get(b, E0 + 36, 4) + 8, 4), "not 16-byte aligned"),
    ("area_outside", lambda b: _put(b, E1 + 8, _get(b, 24, 8), 8), "outside the blob"),
    ("columns_overlap", lambda b: _put(b, E0 + 36, 0, 4), "overlap"),
    ("value_width_3", lambda b: _put(b, E0 + 33, 3, 1), "width is not"),
    ("status_width_2", lambda b: _put(b, E0 + 17, 2, 1), "native width"),
    ("mode_rel_a", lambda b: _put(b, E0 + 32, abi.CC_PK_REL_A, 1), "mode"),
]


@pytest.fixture(scope="module")
def good_blob():
    n = B + 100  # two blocks; status raw and value 2 bytes wide in both, so both columns have rows to overlap
    status = (np.arange(n) % 3 * 0x10).astype(np.uint8)
    value = (np.arange(n, dtype=np.uint64) * np.uint64(7)) % np.uint64(50000) + np.uint64(1 << 33)
    blob = pack_results(status, value)
    info = results_info(blob)
    assert set(info["columns"]["status"]["rows"]) == {(rc.FOR, 1)} and set(info["columns"]["value"]["rows"]) == {(rc.FOR, 2)}
    return n, blob


def _refused(blob, what):
    L = lib()
    with pytest.raises(EngineError) as e:
        results_check(blob)
    assert e.value.rc == abi.CC_ERR_INVALID
    assert "result blob" in str(e.value) and what in str(e.value), str(e.value)
    # the decoder refuses the same blob and touches no output
    status, value = np.full(2 * B, 0xEE, np.uint8), np.full(2 * B, 0xEEEE, np.uint64)
    r = abi.cc_results(status.ctypes.data, value.ctypes.data)
    assert L.cc_respack_unpack(blob.ctypes.data, blob.nbytes, C.byref(r), 1) == abi.CC_ERR_INVALID
    assert (status == 0xEE).all() and (value == 0xEEEE).all()


@pytest.mark.parametrize("name,mutate,what", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_validator_refuses(good_blob, name, mutate, what):
    n, blob = good_blob
    bad = _aligned_copy(blob)
    mutate(bad)
    _refused(bad, what)
    assert results_check(blob) == n  # (the fixture itself is intact)


def test_validator_refuses_truncation_null_and_misaligned(good_blob):
    n, blob = good_blob
    _refused(_aligned_copy(blob)[:len(blob) - 16], "larger than the buffer")
    _refused(_aligned_copy(blob)[:48], "shorter than its header")
    shifted = _aligned_bytes(len(blob) + 16)[8:8 + len(blob)]
    shifted[:] = blob
    _refused(shifted, "not 16-byte aligned")
    L = lib()
    assert L.cc_respack_check(None, 64, None) == abi.CC_ERR_INVALID
    assert "result blob" in L.cc_last_error().decode()


def test_short_cap_returns_the_size_and_writes_nothing():
    L = lib()
    n = 3 * B + 17
    status, value = rc.random_results(n, seed=5)
    blob = pack_results(status, value)
    r = abi.cc_results(status.ctypes.data, value.ctypes.data)
    for cap in (0, HEADER, HEADER + 4 * ENTRY, len(blob) - 16, len(blob) - 1):
        buf = _aligned_bytes(len(blob))
        buf[:] = 0xEE
        size = C.c_uint64()
        assert L.cc_respack_pack(C.byref(r), n, buf.ctypes.data, cap, 2, C.byref(size)) == abi.CC_ERR_CAPACITY
        assert size.value == len(blob)
        assert (buf == 0xEE).all(), f"cap {cap}: the encoder wrote into a buffer it refused"
    buf = _aligned_bytes(len(blob))  # the exact size is enough
    size = C.c_uint64()
    assert L.cc_respack_pack(C.byref(r), n, buf.ctypes.data, len(blob), 2, C.byref(size)) == abi.CC_OK
    assert np.array_equal(buf, blob)
    bound = C.c_uint64()
    assert L.cc_respack_bound(n, C.byref(bound)) == abi.CC_OK and bound.value >= len(blob)
    assert L.cc_respack_bound(n, None) == abi.CC_ERR_INVALID


def test_c2_step_results_pack_to_3_25_bytes_per_row():
    """The oracle's results for the third 4M-row AtomicLongClients step (65,536 resources, default seed): at most
    3.25 B per row, header and directory (48 B per block) included, against 9 B wide."""
    from copycat_amd.workload import AtomicLongClients
    from oracle.oracle_py import Oracle

    R, n = 65536, 4 << 20
    O = Oracle(R, R)
    for r in range(R):
        O.resource_create(r, abi.CC_RES_VALUE)
        O.instance_open(r, r, 1 + r, 1)
    clients = AtomicLongClients(resources=R)
    for _ in range(3):
        status, value = O.apply(clients.next(n))
    blob = pack_results(status, value)
    info = results_info(blob)
    print({k: (v["rows"], v["bytes_per_row"]) for k, v in info["columns"].items()}, info["bytes_per_row"])
    s, v = unpack_results(blob)
    assert s.tobytes() == status.tobytes() and v.tobytes() == value.tobytes()
    assert len(blob) / n <= 3.25
