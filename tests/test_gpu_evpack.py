"""Packed event blobs on the MI355X: the encoder kernels (evpack.hip) against the host reference encoder, and
cc_apply_batch_host_packed_events (packed batch in, packed results and packed events out) against
cc_apply_batch_host_packed_results with a wide host event stream on a twin engine.

Bar: bit-exact.  The kernels' blob equals cc_evpack_pack's byte for byte (and so the blob the format's rules demand,
tests/evpack_cases.py); the pipelined call's event blob decodes to the wide call's event rows byte for byte whatever the
chunking, with the same result blob, rows_done, event count, applied index and state readbacks."""
import ctypes as C

import numpy as np
import pytest

from copycat_amd import abi
from copycat_amd.batch import (Batch, _aligned_bytes, events_bound, events_check, events_info, pack, pack_events,
                               results_bound, unpack_events, unpack_results)
from tests import evpack_cases as ec
from tests import pack_cases as pc
from tests.test_gpu_pack import COORD_K, COORD_TYPES, EV_KEYS, _coord_engine, _coord_stream, _state
from tests.test_gpu_respack import _place_pass

pytestmark = pytest.mark.gpu

B = pc.B
CHUNK = 2 * B         # chunk_rows of the overflow test (test_gpu_respack.py's)
N = 2 * CHUNK + 3616  # 20,000 rows: three chunks, the last one ragged
NT = 3 * B + 1        # 12,289 rows in 4,096-row chunks: chunk boundaries fall inside event blocks
PLACE_PASS = _place_pass()  # blocks one pass of k_evpack_place holds (one per lane)


@pytest.fixture(scope="module")
def small_engine():
    from copycat_amd.engine import Engine

    E = Engine(16, 16, 4096)
    yield E
    E.close()


def _device_events(ev, capacity=None, count=None):
    """The numpy event columns in a DeviceEvents of `capacity` rows whose device count reads `count`."""
    import torch

    from copycat_amd.engine import DeviceEvents

    n = len(ev["pos"])
    d = DeviceEvents(max(n if capacity is None else capacity, 1))
    d.capacity = n if capacity is None else capacity
    m = min(n, d.capacity)
    views = {"pos": np.int32, "target": np.int32, "code": np.uint8, "src": np.uint8, "tag": np.uint8, "payload": np.int64}
    for k, dt in views.items():
        getattr(d, k)[:m] = torch.from_numpy(ev[k][:m].view(dt)).cuda()
    d.count[0] = n if count is None else count
    return d


def _encode_cases():
    out = [(f"random/{n}", ec.random_events(n, seed=n)) for n in (1, 15, 16, 17, B - 1, B, B + 1)]
    out += [(f"cases/{i}", ev) for i, ev in enumerate(ec.all_case_blocks())]  # every width and BY_POS case
    # one event more than a pass of the placement scan: constant blocks (no data) but a few, spread over both passes
    n = PLACE_PASS * B + 1
    ev = ec.events(np.full(n, 3, np.uint32), payload=11)
    for k, part in ((0, ec.fanout(64, 64, seed=1)), (7, ec.random_events(B, seed=7)), (PLACE_PASS - 1, ec.fanout(512, 8, seed=2))):
        for name in ec.NAMES:
            ev[name][k * B:(k + 1) * B] = part[name]
    ev["payload"][-1] = 12  # (the tail block of one event)
    out.append((f"place_pass_plus_one/{n}", ev))
    return out


def test_encoder_kernels_match_host_encoder(small_engine):
    """Fails without the feature: cc_evpack_from_device does not exist."""
    for name, ev in _encode_cases():
        n = len(ev["pos"])
        want = pack_events(ev)
        if n <= 8 * B:
            assert np.array_equal(want, ec.encode(ev)), name
        d = _device_events(ev)
        assert all(getattr(d, k).data_ptr() % 16 == 0 for k in ec.NAMES)
        out = _aligned_bytes(events_bound(n) + 64)
        out[:] = 0xCD
        got, count = small_engine.events_to_host_packed(d, out=out[:len(out) - 64])
        assert count == n
        assert len(got) == len(want), f"{name}: {len(got)} bytes, the host encoder writes {len(want)}"
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, f"{name}: the blob differs from the host encoder's first at byte {bad[0]}"
        assert (out[len(got):] == 0xCD).all(), f"{name}: bytes after the blob were written"
        assert events_check(got) == n
        assert ec.same(d.host(), ev), f"{name}: the device columns are read only"


def test_count_above_capacity_and_count_zero(small_engine):
    from copycat_amd.engine import EngineError

    ev = ec.random_events(B + 100, seed=3)
    cap = B + 5
    d = _device_events(ev, capacity=cap, count=B + 100)  # the producer counted 95 events it had no room for
    with pytest.raises(EngineError) as e:
        small_engine.events_to_host_packed(d)
    assert e.value.rc == abi.CC_ERR_CAPACITY and e.value.count == B + 100
    assert np.array_equal(e.value.blob, pack_events(ec.take(ev, 0, cap)))
    d = _device_events(ev, count=0)
    blob, count = small_engine.events_to_host_packed(d)
    assert count == 0 and len(blob) == 64 and events_check(blob) == 0
    assert np.array_equal(blob, pack_events(ec.take(ev, 0, 0)))


def test_events_to_host_packed_arguments(small_engine):
    L = small_engine.L
    ev = ec.random_events(B + 9, seed=4)
    d = _device_events(ev)
    bound = events_bound(d.capacity)
    blob = _aligned_bytes(bound)
    size, count = C.c_uint64(), C.c_uint64()

    def call(s, buf, cap):
        return L.cc_evpack_from_device(small_engine.h, C.byref(s), buf, cap, C.byref(size), C.byref(count), None)

    assert call(d.struct(), blob.ctypes.data, bound - 1) == abi.CC_ERR_CAPACITY and size.value == bound
    assert call(d.struct(), None, bound) == abi.CC_ERR_INVALID
    assert call(d.struct(), blob.ctypes.data + 8, bound) == abi.CC_ERR_INVALID
    for k in ("pos", "code", "payload"):  # a misaligned or missing column
        s = d.struct()
        setattr(s, k, getattr(s, k) + 4)
        assert call(s, blob.ctypes.data, bound) == abi.CC_ERR_INVALID
        setattr(s, k, None)
        assert call(s, blob.ctypes.data, bound) == abi.CC_ERR_INVALID
    s = d.struct()
    s.count = None
    assert call(s, blob.ctypes.data, bound) == abi.CC_ERR_INVALID
    assert call(d.struct(), blob.ctypes.data, bound) == abi.CC_OK and count.value == B + 9
    assert np.array_equal(blob[:size.value], pack_events(ev))


def test_from_device_after_sessions_close():
    """Close events carry pos 0xFFFFFFFF on every row and payloads that are no function of it: every block is FOR."""
    from copycat_amd.engine import DeviceEvents

    E = _coord_engine()
    E.apply_host_events(_coord_stream(4000), capacity=1 << 16)
    evs = DeviceEvents(1 << 14)
    s = evs.struct()
    clients = np.array([7, 8, 9], np.uint64)
    closed = C.c_uint64()
    assert E.L.cc_sessions_close(E.h, clients.ctypes.data, len(clients), C.byref(s), None, C.byref(closed)) == abi.CC_OK
    blob, count = E.events_to_host_packed(evs)
    wide = evs.host()
    assert count == wide["count"] > 0 and closed.value > 0
    assert (wide["pos"] == 0xFFFFFFFF).all()
    assert np.array_equal(blob, pack_events(wide)) and ec.same(unpack_events(blob), wide)
    info = events_info(blob)
    assert all(b[0] == abi.CC_PK_FOR for b in info["columns"]["payload"]["blocks"])
    assert info["columns"]["pos"]["blocks"][0] == (abi.CC_PK_FOR, 0, 0xFFFFFFFF, 0)
    E.close()


# ---- packed events = wide events, on twin engines -----------------------------------------------------------------------
TOPIC_K = 72  # instance k of topic t sits in slot 3 k + t: k < 70 may listen, 70 comes and goes, 71 publishes


def _topic_engine():
    """Three topics of 0, 1 and 70 listeners."""
    from copycat_amd.engine import Engine

    E = Engine(3, 3 * TOPIC_K, 1 << 16, flags=abi.CC_CFG_TIMERS_DEFERRED, max_events=1 << 20, coord_cap=128)
    E.resource_create_range(0, 3, abi.CC_RES_TOPIC)
    for k in range(TOPIC_K):
        E.instance_open_range(3 * k, 3, 0, 1000 + 3 * k, 7 + k)
    slots = [1] + [3 * k + 2 for k in range(70)]
    s0 = Batch(len(slots))
    s0.index[:] = np.arange(1, len(slots) + 1, dtype=np.uint64)
    s0.inst[:] = slots
    s0.op[:] = abi.CC_OP_TOPIC_LISTEN
    E.apply_host_events(s0, capacity=1024)
    return E


def _topic_stream(n):
    rng = np.random.default_rng(0x70B1C)
    b = Batch(n)
    b.index[:] = np.arange(100, 100 + n, dtype=np.uint64)
    t = rng.integers(0, 3, n, dtype=np.int64)
    u = rng.random(n)
    pub = u < 0.96
    b.op[:] = np.where(pub, abi.CC_OP_TOPIC_PUBLISH, np.where(u < 0.98, abi.CC_OP_TOPIC_LISTEN, abi.CC_OP_TOPIC_UNLISTEN))
    b.inst[:] = np.where(pub, 71, 70) * 3 + t
    b.flags[:] = abi.cc_flags(abi.CC_TAG_LONG)
    b.a[:] = rng.integers(0, 1 << 62, n, dtype=np.uint64)  # a message per publish
    return b


def _topic_state(E, last_index):
    return {"applied": E.applied_index(), "listeners": [E.topic_listeners(r) for r in range(3)],
            "retained": [E.retained(r) for r in range(3)]}


VALUE_R, VALUE_K = 64, 3


def _value_listener_engine():
    """64 AtomicValues with three instances each, value events on."""
    from copycat_amd.engine import Engine

    flags = abi.CC_CFG_TIMERS_DEFERRED | abi.CC_CFG_VALUE_EVENTS | abi.CC_CFG_VALUE_RETAINED
    E = Engine(VALUE_R, VALUE_R * VALUE_K + 8, 1 << 16, flags=flags, max_events=1 << 20)
    E.resource_create_range(0, VALUE_R, abi.CC_RES_VALUE)
    for k in range(VALUE_K):
        E.instance_open_range(k * VALUE_R, VALUE_R, 0, 1000 + k * VALUE_R, 7 + k)
    return E


def _value_listener_stream(n):
    """Every instance listens, then sets (published to the value's listeners), CAS on small values and re-listens."""
    ni = VALUE_R * VALUE_K
    rng = np.random.default_rng(4201)
    op = rng.choice(np.array([abi.CC_OP_VALUE_SET, abi.CC_OP_VALUE_CAS, abi.CC_OP_VALUE_LISTEN], np.uint8), n, p=[0.6, 0.3, 0.1])
    inst = rng.integers(0, ni, n).astype(np.uint32)
    op[:ni], inst[:ni] = abi.CC_OP_VALUE_LISTEN, np.arange(ni)
    lng = abi.CC_TAG_LONG
    flags = np.where(op == abi.CC_OP_VALUE_SET, abi.cc_flags(lng), np.where(op == abi.CC_OP_VALUE_CAS, abi.cc_flags(lng, lng), 0))
    a = np.where(op == abi.CC_OP_VALUE_LISTEN, 0, rng.integers(0, 4, n))
    bb = np.where(op == abi.CC_OP_VALUE_CAS, rng.integers(0, 4, n), 0)
    return Batch.from_columns(index=np.arange(1, n + 1, dtype=np.uint64), time=np.uint64(2) + np.arange(n, dtype=np.uint64) // np.uint64(8),
                              inst=inst, op=op, flags=flags.astype(np.uint8), a=a.astype(np.uint64), b=bb.astype(np.uint64))


def _value_listener_state(E, last_index):
    return {"applied": E.applied_index(), "values": [x.tobytes() for x in E.value_state(0, VALUE_R)],
            "retained": [E.retained(r) for r in range(0, VALUE_R, 7)]}


def _same(wide, packed, n):
    """apply_host_packed_results' (result blob, events, rows_done) with a wide event stream against
    apply_host_packed_events' (result blob, event blob, ev_count, rows_done)."""
    res1, ev1, done1 = wide
    res2, evb, ev_count, done2 = packed
    assert done1 == done2 == n
    assert np.array_equal(res1, res2), "the result blobs differ"
    assert ev_count == ev1["count"]
    assert events_check(evb) == len(ev1["pos"])
    assert ec.same(unpack_events(evb), ev1), "the decoded events are not the wide call's"
    assert np.array_equal(evb, pack_events(ev1)), "a complete call's event blob is the host encoder's"


def _twin(make, stream, state, n, chunk, cap):
    b = stream(2 * n)
    wide, packed = make(), make()
    for lo, hi in ((0, n), (n, 2 * n)):  # the second batch: the device columns and the staging survive reuse
        blob = pack(b.slice(lo, hi))
        r1 = wide.apply_host_packed_results(blob, n, capacity=cap, chunk_rows=chunk)
        r2 = packed.apply_host_packed_events(blob, n, capacity=cap, chunk_rows=chunk)
        _same(r1, r2, n)
        assert state(wide, int(b.index[-1])) == state(packed, int(b.index[-1]))
    wide.close(), packed.close()
    return r1[1], r2[1]


def test_packed_events_coordination_engine():
    """Fails without the feature: cc_apply_batch_host_packed_events does not exist."""
    ev, _ = _twin(_coord_engine, _coord_stream, lambda E, i: _state(E, "coord", i), N, CHUNK, 8 * N)
    assert len(ev["pos"]) > 1000 and len(set(ev["code"].tolist())) >= 4  # locks, elections, joins, leaves ... published


def test_packed_events_topic_engine():
    ev, evb = _twin(_topic_engine, _topic_stream, _topic_state, NT, B, 80 * NT)
    assert len(ev["pos"]) >= 3 * B  # three event blocks and more
    per_row = np.bincount(ev["pos"], minlength=NT)
    assert {0, 1, 70} <= set(per_row.tolist())  # publishes to topics of 0, 1 and 70 listeners
    first = np.searchsorted(ev["pos"], [B, 2 * B, 3 * B])  # the first event of chunks 1, 2, 3
    assert all(f % B for f in first.tolist()), "a chunk boundary fell on an event block's"
    info = events_info(evb)
    assert (abi.CC_PK_BY_POS, 8) in info["columns"]["payload"]["rows"]  # a fan-out's messages go as a table by pos
    print(info["bytes_per_row"], {k: v["rows"] for k, v in info["columns"].items()})


def test_packed_events_value_engine_with_listeners():
    # (an odd event capacity: the engine-owned device columns stay 16-byte aligned behind each other)
    ev, _ = _twin(_value_listener_engine, _value_listener_stream, _value_listener_state, NT, B, 8 * NT + 1)
    assert len(ev["pos"]) > NT


def test_chunking_does_not_change_the_blob():
    b = _topic_stream(NT)
    blob = pack(b)
    wide = _topic_engine()
    _, ev, done = wide.apply_host_packed_results(blob, NT, capacity=80 * NT, chunk_rows=B)
    assert done == NT
    want = pack_events(ev)
    for chunk in (B, 2 * B, 0):
        E = _topic_engine()
        _, evb, ev_count, done = E.apply_host_packed_events(blob, NT, capacity=80 * NT, chunk_rows=chunk)
        assert done == NT and ev_count == ev["count"]
        assert np.array_equal(evb, want), f"chunk_rows {chunk}: the event blob differs from pack_events of the wide columns"
        assert _topic_state(E, 0) == _topic_state(wide, 0)
        E.close()
    wide.close()


def test_event_capacity_too_small_for_the_third_chunk():
    from oracle.oracle_py import Oracle
    from tests.test_gpu_coord import _check_state

    b = _coord_stream(N)
    ref, wide, E = _coord_engine(), _coord_engine(), _coord_engine()
    s0, v0, ev0 = ref.apply_host_events(b, capacity=8 * N)
    c2, c3 = int((ev0["pos"] < 2 * CHUNK).sum()), len(ev0["pos"])
    assert c3 > c2 > 0
    cap = c2 + (c3 - c2) // 2  # room for two chunks' events, not for the third's
    blob_in = pack(b)
    resw, evw, donew = wide.apply_host_packed_results(blob_in, N, capacity=cap, chunk_rows=CHUNK)
    res, evb, ev_count, done = E.apply_host_packed_events(blob_in, N, capacity=cap, chunk_rows=CHUNK)
    assert done == donew == 2 * CHUNK and ev_count == evw["count"] > cap
    assert np.array_equal(res, resw)
    assert events_check(evb) == c2  # exactly the first two chunks' events: the rolled-back chunk's are not in the blob
    assert ec.same(unpack_events(evb), ec.take(ev0, 0, c2)) and ec.same(unpack_events(evb), ec.take(evw, 0, c2))
    assert np.array_equal(evb, pack_events(ec.take(ev0, 0, c2)))
    assert _state(E, "coord", N) == _state(wide, "coord", N)
    # the host drains its stream and resumes at rows_done
    rest = pack(b.slice(done, N))
    res2, evb2, ev_count2, done2 = E.apply_host_packed_events(rest, N - done, capacity=8 * N, chunk_rows=CHUNK)
    assert done2 == N - done and ev_count2 == c3 - c2
    s, v = unpack_results(res2)
    assert s.tobytes() == s0[done:].tobytes() and v.tobytes() == v0[done:].tobytes()
    ev2 = unpack_events(evb2)
    assert np.array_equal(ev2["pos"] + np.uint32(done), ev0["pos"][c2:])  # (pos counts from the resumed batch's row 0)
    for k in EV_KEYS[1:]:
        assert np.array_equal(ev2[k], ev0[k][c2:]), k
    assert _state(E, "coord", N) == _state(ref, "coord", N)
    R = len(COORD_TYPES)
    O = Oracle(R, R * COORD_K + 8, abi.CC_CFG_TIMERS_DEFERRED)
    for r, t in enumerate(COORD_TYPES):
        O.resource_create(r, int(t))
        for k in range(COORD_K):
            O.instance_open(r * COORD_K + k, r, 1000 + r * COORD_K + k, 7 + k)
    O.apply(b)
    _check_state(E, O, COORD_TYPES)
    for x in (ref, wide, E):
        x.close()


def test_arguments():
    from copycat_amd.engine import EngineError

    b = _topic_stream(NT)
    E, twin = _topic_engine(), _topic_engine()
    before = _topic_state(E, 0)
    blob = pack(b)
    cap = 80 * NT
    res, evb = _aligned_bytes(results_bound(NT)), _aligned_bytes(events_bound(cap))
    L = E.L
    size, ev_size, ev_count, done = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()

    def call(res_ptr, res_cap, ev_ptr, ev_cap_bytes, blob_=blob, opts=None, sizes=(size, ev_size, ev_count)):
        p = [C.byref(x) if x is not None else None for x in sizes]
        return L.cc_apply_batch_host_packed_events(E.h, blob_.ctypes.data, blob_.nbytes, res_ptr, res_cap, p[0], ev_ptr, cap,
                                                   ev_cap_bytes, p[1], p[2], opts, C.byref(done))

    good = (res.ctypes.data, res.nbytes, evb.ctypes.data, evb.nbytes)
    assert call(good[0], results_bound(NT) - 1, good[2], good[3]) == abi.CC_ERR_CAPACITY and size.value == results_bound(NT)
    assert call(good[0], good[1], good[2], events_bound(cap) - 1) == abi.CC_ERR_CAPACITY and ev_size.value == events_bound(cap)
    assert call(None, good[1], good[2], good[3]) == abi.CC_ERR_INVALID
    assert call(good[0], good[1], None, good[3]) == abi.CC_ERR_INVALID
    assert call(good[0] + 8, good[1] - 8, good[2], good[3]) == abi.CC_ERR_INVALID
    assert call(good[0], good[1], good[2] + 8, good[3] - 8) == abi.CC_ERR_INVALID
    assert call(*good, sizes=(size, None, ev_count)) == abi.CC_ERR_INVALID
    assert call(*good, sizes=(size, ev_size, None)) == abi.CC_ERR_INVALID
    opts = abi.cc_packed_opts(chunk_rows=B, flags=2)  # an unknown flag
    assert call(*good, opts=C.byref(opts)) == abi.CC_ERR_INVALID
    # a corrupted input blob never reaches the engine
    for at, bit in ((0, 1), (9, 0x40), (64 + 1, 0x80)):  # magic, n, a block's rows
        bad = blob.copy()
        bad[at] ^= bit
        with pytest.raises(EngineError) as e:
            E.apply_host_packed_events(bad, NT, capacity=cap, chunk_rows=B)
        assert e.value.rc == abi.CC_ERR_INVALID
    assert _topic_state(E, 0) == before
    # n == 0: valid header-only blobs and a zero event count
    rblob, eblob, cnt, done0 = E.apply_host_packed_events(pack(Batch(0)), 0, capacity=cap, chunk_rows=B)
    assert (len(rblob), len(eblob), events_check(eblob), cnt, done0) == (64, 64, 0, 0, 0)
    # and the engine is as good as new
    r1 = twin.apply_host_packed_results(blob, NT, capacity=cap, chunk_rows=B)
    _same(r1, E.apply_host_packed_events(blob, NT, capacity=cap, chunk_rows=B), NT)
    assert _topic_state(E, 0) == _topic_state(twin, 0)
    E.close(), twin.close()


def test_registered_blobs_and_timeline():
    from copycat_amd.engine import host_register, host_unregister

    b = _topic_stream(NT)
    blob = pack(b)
    cap = 80 * NT
    res, evb = _aligned_bytes(results_bound(NT)), _aligned_bytes(events_bound(cap))
    for arr in (blob, res, evb):
        host_register(arr)
    try:
        E, twin = _topic_engine(), _topic_engine()
        packed = E.apply_host_packed_events(blob, NT, capacity=cap, chunk_rows=B, out=res, ev_out=evb, timeline=True)
        assert packed[0].ctypes.data == res.ctypes.data and packed[1].ctypes.data == evb.ctypes.data
        _same(twin.apply_host_packed_results(blob, NT, capacity=cap, chunk_rows=B), packed, NT)
        assert _topic_state(E, 0) == _topic_state(twin, 0)
        ms = E.packed_events_timeline()
        print(ms)
        assert ms.shape == (4, 7) and (ms > 0).all()  # seven positive stage times per completed chunk
        E.close(), twin.close()
    finally:
        for arr in (blob, res, evb):
            host_unregister(arr)
