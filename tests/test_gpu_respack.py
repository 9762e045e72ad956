"""Packed result blobs on the MI355X: the encoder kernels (respack.hip) against the host reference encoder, and
cc_apply_batch_host_packed_results (packed batch in, packed results out) against cc_apply_batch_host_packed on a twin
engine.

Bar: bit-exact.  The kernels' blob equals cc_respack_pack's byte for byte; the pipelined call's blob decodes to the wide
call's result rows byte for byte, with the same events (in order), rows_done, applied index and state readbacks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from copycat_amd import abi
from copycat_amd.batch import (Batch, _aligned_bytes, pack, pack_results, results_bound, results_check, results_info,
                               unpack_results)
from tests import pack_cases as pc
from tests import respack_cases as rc
from tests.test_gpu_pack import (COORD_K, COORD_TYPES, EV_KEYS, _coord_engine, _coord_stream, _map_engine, _map_stream,
                                 _state, _value_engine, _value_stream)

pytestmark = pytest.mark.gpu

B = pc.B
CHUNK = 2 * B        # chunk_rows of the pipelined calls
N = 2 * CHUNK + 3616  # 20,000 rows: three chunks, the last one ragged (3,616 = 4,096 - 480 rows)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _place_pass():
    """kPackPlacePass: the blocks one pass of an encoder's placement scan (k_respack_place, k_evpack_place) holds."""
    txt = open(os.path.join(ROOT, "copycat_amd", "csrc", "engine_internal.h")).read()
    return int(re.search(r"kPackPlacePass\s*=\s*(\d+)", txt).group(1))


@pytest.fixture(scope="module")
def small_engine():
    from copycat_amd.engine import Engine

    E = Engine(16, 16, 4096)
    yield E
    E.close()


def _encode_cases():
    out = [(f"random/{n}", *rc.random_results(n, seed=n)) for n in (1, 15, 16, 17, B - 1, B, B + 1, 3 * B + 5)]
    status, value, _ = rc.width_rows()
    out.append(("widths", status, value))
    # raw values (width 8) with mixed status: a full block, and a tail block of 3 rows or of 1,003 (an odd length)
    for n in (B + 3, B + 1003):
        value = np.resize(np.array([0, rc.M64, 1 << 63, 5], np.uint64), n)
        out.append((f"raw/{n}", (np.arange(n) % 3 * 0x10).astype(np.uint8), value))
    # one block more than a pass of the placement scan: constant blocks (no data) but a few, spread over both passes
    blocks = _place_pass() + 1
    status, value = np.full(blocks * B, 0x10, np.uint8), np.full(blocks * B, 3, np.uint64)
    for k, span in ((0, 200), (7, 70000), (blocks - 2, 1 << 40), (blocks - 1, 9)):
        value[k * B:(k + 1) * B] = pc.spread(1 << 20, span, B, k)
        status[k * B + 5] = 0x23
    out.append((f"place_pass_plus_one/{blocks}", status, value))
    return out


def test_encoder_kernels_match_host_encoder(small_engine):
    """Fails without the feature: cc_respack_from_device does not exist."""
    import torch

    for name, status, value in _encode_cases():
        want = pack_results(status, value)
        d_status = torch.from_numpy(status).cuda()
        d_value = torch.from_numpy(value.view(np.int64)).cuda()
        assert d_status.data_ptr() % 16 == 0 and d_value.data_ptr() % 16 == 0
        out = _aligned_bytes(results_bound(len(status)) + 64)
        out[:] = 0xCD
        got = small_engine.results_to_host_packed(d_status, d_value, out=out[:len(out) - 64])
        assert len(got) == len(want), f"{name}: {len(got)} bytes, the host encoder writes {len(want)}"
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, f"{name}: the blob differs from the host encoder's first at byte {bad[0]}"
        assert (out[len(got):] == 0xCD).all(), f"{name}: bytes after the blob were written"
        assert results_check(got) == len(status)
        # the device columns are read only
        assert np.array_equal(d_status.cpu().numpy(), status) and np.array_equal(d_value.cpu().numpy().view(np.uint64), value)


def test_results_to_host_packed_arguments(small_engine):
    import torch

    L = small_engine.L
    n = B + 9
    d_status = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
    d_value = torch.zeros(n + 2, dtype=torch.int64, device="cuda")
    blob = _aligned_bytes(results_bound(n))
    size = C.c_uint64()

    def call(status, value, rows, buf, cap):
        r = abi.cc_results(status.data_ptr(), value.data_ptr())
        return L.cc_respack_from_device(small_engine.h, C.byref(r), rows, buf, cap, C.byref(size), None)

    assert call(d_status, d_value, n, blob.ctypes.data, results_bound(n) - 1) == abi.CC_ERR_CAPACITY
    assert size.value == results_bound(n)
    assert call(d_status, d_value, n, None, results_bound(n)) == abi.CC_ERR_INVALID
    assert call(d_status, d_value, n, blob.ctypes.data + 8, results_bound(n) - 8) == abi.CC_ERR_INVALID
    assert call(d_status[1:], d_value, n, blob.ctypes.data, blob.nbytes) == abi.CC_ERR_INVALID  # misaligned columns
    assert call(d_status, d_value[1:], n, blob.ctypes.data, blob.nbytes) == abi.CC_ERR_INVALID
    assert call(d_status, d_value, 0, blob.ctypes.data, blob.nbytes) == abi.CC_OK and size.value == 64
    assert results_check(blob[:64]) == 0 and np.array_equal(blob[:64], pack_results(np.zeros(0, np.uint8), np.zeros(0, np.uint64)))


# ---- packed results = wide results, on twin engines ---------------------------------------------------------------------
def _same(wide, packed, n):
    """apply_host_packed's (status, value, events, rows_done) against apply_host_packed_results' (blob, events,
    rows_done): the decoded blob is the wide call's copied-out rows, byte for byte."""
    s1, v1, ev1, done1 = wide
    blob, ev2, done2 = packed
    assert done1 == done2 == n
    assert results_check(blob) == n
    s2, v2 = unpack_results(blob)
    assert s1.tobytes() == s2.tobytes() and v1.tobytes() == v2.tobytes()
    assert np.array_equal(blob, pack_results(s1, v1)), "a complete call's blob is the host encoder's"
    assert ev1["count"] == ev2["count"]
    for k in EV_KEYS:  # every event, in order
        assert np.array_equal(ev1[k], ev2[k]), k


def _twin(make, stream, kind, columns=pc.ALL):
    b = stream(2 * N)
    wide, packed = make(), make()
    for lo, hi in ((0, N), (N, 2 * N)):  # the second batch: the stagings survive reuse
        blob = pack(b.slice(lo, hi), columns=columns)
        r1 = wide.apply_host_packed(blob, N, capacity=8 * N, chunk_rows=CHUNK)
        r2 = packed.apply_host_packed_results(blob, N, capacity=8 * N, chunk_rows=CHUNK)
        _same(r1, r2, N)
        assert _state(wide, kind, int(b.index[-1])) == _state(packed, kind, int(b.index[-1]))
    return r2


def test_packed_results_value_engine():
    blob, _, _ = _twin(_value_engine, _value_stream, "value", columns=pc.VALUE_COLS)
    assert results_info(blob)["blocks"] == 5


def test_packed_results_map_engine_whole_map_rows_and_nulls():
    blob, _, _ = _twin(_map_engine, lambda n: _map_stream(n, 502, ttl=False), "map")
    s, _ = unpack_results(blob)
    assert (abi.status_tag(s) == abi.CC_TAG_NULL).any()  # stored nulls and absent keys: NULL-tagged rows, value bytes kept


def test_packed_results_coordination_engine_with_events():
    _, ev, _ = _twin(_coord_engine, _coord_stream, "coord")
    assert len(ev["pos"]) > 1000 and len(set(ev["code"].tolist())) >= 4  # locks, elections, joins, leaves ... published


def test_event_stream_too_small_for_the_third_chunk():
    from oracle.oracle_py import Oracle
    from tests.test_gpu_coord import _check_state

    b = _coord_stream(N)
    ref, wide, E = _coord_engine(), _coord_engine(), _coord_engine()
    s0, v0, ev0 = ref.apply_host_events(b, capacity=8 * N)
    c2, c3 = int((ev0["pos"] < 2 * CHUNK).sum()), len(ev0["pos"])
    assert c3 > c2 > 0
    cap = c2 + (c3 - c2) // 2  # room for two chunks' events, not for the third's
    blob_in = pack(b)
    _, _, evw, donew = wide.apply_host_packed(blob_in, N, capacity=cap, chunk_rows=CHUNK)
    blob, ev, done = E.apply_host_packed_results(blob_in, N, capacity=cap, chunk_rows=CHUNK)
    assert done == donew == 2 * CHUNK and ev["count"] == evw["count"]
    assert results_check(blob) == done == results_info(blob)["n"]  # the rolled-back chunk is not in the blob
    s, v = unpack_results(blob)
    assert s.tobytes() == s0[:done].tobytes() and v.tobytes() == v0[:done].tobytes()
    for k in EV_KEYS:
        assert np.array_equal(ev[k][:c2], ev0[k][:c2]) and np.array_equal(ev[k], evw[k]), k
    assert _state(E, "coord", N) == _state(wide, "coord", N)
    # the host drains its stream and resumes at rows_done
    rest = pack(b.slice(done, N))
    blob2, ev2, done2 = E.apply_host_packed_results(rest, N - done, capacity=8 * N, chunk_rows=CHUNK)
    assert done2 == N - done
    s, v = unpack_results(blob2)
    assert s.tobytes() == s0[done:].tobytes() and v.tobytes() == v0[done:].tobytes()
    assert _state(E, "coord", N) == _state(ref, "coord", N)
    R = len(COORD_TYPES)
    O = Oracle(R, R * COORD_K + 8, abi.CC_CFG_TIMERS_DEFERRED)
    for r, t in enumerate(COORD_TYPES):
        O.resource_create(r, int(t))
        for k in range(COORD_K):
            O.instance_open(r * COORD_K + k, r, 1000 + r * COORD_K + k, 7 + k)
    O.apply(b)
    _check_state(E, O, COORD_TYPES)


def test_arguments():
    from copycat_amd.engine import EngineError

    b = _value_stream(N)
    E, twin = _value_engine(), _value_engine()
    before = _state(E, "value", N)
    blob = pack(b, columns=pc.VALUE_COLS)
    res = _aligned_bytes(results_bound(N))
    L, size, done = E.L, C.c_uint64(), C.c_uint64()

    def call(res_ptr, res_cap, blob_=blob):
        return L.cc_apply_batch_host_packed_results(E.h, blob_.ctypes.data, blob_.nbytes, res_ptr, res_cap, C.byref(size),
                                                    None, None, C.byref(done))

    assert call(res.ctypes.data, results_bound(N) - 1) == abi.CC_ERR_CAPACITY and size.value == results_bound(N)
    assert call(None, res.nbytes) == abi.CC_ERR_INVALID
    assert call(res.ctypes.data + 8, res.nbytes - 8) == abi.CC_ERR_INVALID
    opts = abi.cc_packed_opts(chunk_rows=CHUNK, flags=2)  # an unknown flag
    assert L.cc_apply_batch_host_packed_results(E.h, blob.ctypes.data, blob.nbytes, res.ctypes.data, res.nbytes,
                                                C.byref(size), None, C.byref(opts), C.byref(done)) == abi.CC_ERR_INVALID
    # a corrupted input blob never reaches the engine
    for at, bit in ((0, 1), (9, 0x40), (64 + 1, 0x80), (64 + 160 + 16 * 7, 2)):  # magic, n, a block's rows, a's mode
        bad = blob.copy()
        bad[at] ^= bit
        with pytest.raises(EngineError) as e:
            E.apply_host_packed_results(bad, N, chunk_rows=CHUNK)
        assert e.value.rc == abi.CC_ERR_INVALID
    assert E.applied_index() == 0 and _state(E, "value", N) == before
    # n == 0: a valid header-only blob and a zero event count
    rblob, ev, done0 = E.apply_host_packed_results(pack(Batch(0)), 0, chunk_rows=CHUNK)
    assert (len(rblob), results_check(rblob), done0, ev["count"]) == (64, 0, 0, 0) and E.applied_index() == 0
    # and the engine is as good as new
    r1 = twin.apply_host_packed(blob, N, chunk_rows=CHUNK)
    _same(r1, E.apply_host_packed_results(blob, N, chunk_rows=CHUNK), N)
    assert _state(E, "value", N) == _state(twin, "value", N)


def test_registered_blobs_and_timeline():
    from copycat_amd.engine import host_register, host_unregister

    b = _value_stream(N)
    blob = pack(b, columns=pc.VALUE_COLS)
    res = _aligned_bytes(results_bound(N))
    for arr in (blob, res):
        host_register(arr)
    try:
        E, twin = _value_engine(), _value_engine()
        packed = E.apply_host_packed_results(blob, N, chunk_rows=CHUNK, out=res, timeline=True)
        assert packed[0].ctypes.data == res.ctypes.data
        _same(twin.apply_host_packed(blob, N, chunk_rows=CHUNK), packed, N)
        assert _state(E, "value", N) == _state(twin, "value", N)
        ms = E.packed_results_timeline()
        assert ms.shape == (3, 5) and (ms >= 0).all()
    finally:
        for arr in (blob, res):
            host_unregister(arr)
