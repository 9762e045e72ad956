"""Packed host batches on the MI355X: k_unpack against the host decoder, and cc_apply_batch_host_packed (the pipelined
packed apply) against the wide apply on a twin engine.

Bar: bit-exact.  The kernel's columns equal cc_unpack_batch's byte for byte with the rows around them untouched; the
packed apply's statuses, values, events (in order), applied index and state readbacks equal those of one wide call."""
import ctypes as C

import numpy as np
import pytest

from copycat_amd import abi
from copycat_amd.batch import Batch, pack, unpack
from tests import pack_cases as pc

pytestmark = pytest.mark.gpu

N = 5 * pc.B + 123  # six chunks of 4096 rows: both piece buffers and both result sets are used again
GUARD = 64
ESZ = {"u8": 8, "u4": 4, "u1": 1}
L, E_, G, V = abi.CC_RES_LOCK, abi.CC_RES_ELECTION, abi.CC_RES_GROUP, abi.CC_RES_VALUE
EV_KEYS = ("pos", "target", "code", "src", "tag", "payload")


# ---- 6. the kernel against the host decoder ----------------------------------------------------------------------------
def _decode_cases():
    out = [(f"width/{name}", b, pc.ALL) for name, b, _ in pc.width_cases()]
    for n in (1, pc.B - 1, pc.B, pc.B + 1, 3 * pc.B + 1):
        out += [(f"{name}/{n}", b, cols) for name, b, cols in pc.streams(n) if name in ("random", "map", "random_value_cols")]
    return out


@pytest.fixture(scope="module")
def small_engine():
    from copycat_amd.engine import Engine

    E = Engine(16, 16, 4096)
    yield E
    E.close()


def test_unpack_kernel_matches_host_decoder(small_engine):
    import torch

    for name, b, columns in _decode_cases():
        blob = pack(b, columns=columns)
        ref = unpack(blob)
        n = len(b)
        bufs, cols = {}, {}
        for col, dt in abi.BATCH_COLUMNS:
            if col not in columns:
                continue
            esz = ESZ[dt]
            bufs[col] = torch.full(((n + 2 * GUARD) * esz,), 0xCD, dtype=torch.uint8, device="cuda")
            cols[col] = bufs[col][GUARD * esz:(GUARD + n) * esz]  # 64 sentinel rows before and after; 16-byte aligned
            assert cols[col].data_ptr() % 16 == 0
        small_engine.unpack_to_device(blob, cols)
        torch.cuda.synchronize()
        for col, dt in abi.BATCH_COLUMNS:
            if col not in columns:
                continue
            esz = ESZ[dt]
            got = bufs[col].cpu().numpy()
            assert (got[:GUARD * esz] == 0xCD).all(), f"{name}: rows before {col} were written"
            assert (got[(GUARD + n) * esz:] == 0xCD).all(), f"{name}: rows after {col} were written"
            want = getattr(ref, col).view(np.uint8)
            bad = np.nonzero(got[GUARD * esz:(GUARD + n) * esz] != want)[0]
            assert len(bad) == 0, f"{name}: column {col} differs from the host decoder first at row {bad[0] // esz}"


def test_unpack_to_device_refuses_bad_arguments(small_engine):
    import torch

    from copycat_amd.engine import EngineError

    b = pc.random_batch(100, 1)
    blob = pack(b)
    cols = {col: torch.zeros(100 * ESZ[dt] + 16, dtype=torch.uint8, device="cuda") for col, dt in abi.BATCH_COLUMNS}
    bad = blob.copy()
    bad[0] ^= 1
    for args in ((bad, cols), (blob, {k: v for k, v in cols.items() if k != "key"}),
                 (blob, dict(cols, key=cols["key"][8:]))):  # malformed blob; a missing column; a misaligned column
        with pytest.raises(EngineError) as e:
            small_engine.unpack_to_device(*args)
        assert e.value.rc == abi.CC_ERR_INVALID
    torch.cuda.synchronize()
    assert all(not t.any() for t in cols.values())


# ---- 7. packed apply = wide apply, on twin engines ---------------------------------------------------------------------
def _value_engine(flags=abi.CC_CFG_TIMERS_DEFERRED | abi.CC_CFG_VALUE_RETAINED):
    from copycat_amd.engine import Engine

    E = Engine(300, 308, 1 << 16, flags=flags)
    E.resource_create_range(0, 300, abi.CC_RES_VALUE)
    E.instance_open_range(0, 300, 0, 1000, 7)
    return E


def _value_stream(n):
    from copycat_amd.workload import value_random_stream

    return value_random_stream(n, 300, 308, seed=21, hot=4, p_hot=0.3)


MAPS = 4


def _map_engine(flags=abi.CC_CFG_TIMERS_DEFERRED):
    from copycat_amd.engine import Engine

    E = Engine(MAPS, MAPS + 8, 1 << 16, map_capacity=65536, flags=flags)
    E.resource_create_range(0, MAPS, abi.CC_RES_MAP)
    E.instance_open_range(0, MAPS, 0, 1000, 7)
    from tests.handles import register_key_strings

    register_key_strings(E)  # String keys: java.util.HashMap places them by String.hashCode
    return E


def _map_stream(n, seed, ttl):
    """map_random_stream (every key op, stored nulls) with clear, size, isEmpty and containsValue rows mixed in (the
    stream of tests/test_gpu_map.py::test_map_clear_in_stream_parity).  With `ttl` the log time advances and a share
    of the stores arm timers (the stream of test_map_ttl_parity: values non-null and no clears, since in TTL mode the
    engine refuses a containsValue whose answer hangs on an iteration order it cannot bound)."""
    from copycat_amd.workload import map_random_stream

    b = map_random_stream(n, MAPS, MAPS + 8, keys=16, seed=seed)
    rng = np.random.default_rng(seed)
    wide = np.array([abi.CC_OP_MAP_SIZE, abi.CC_OP_MAP_ISEMPTY, abi.CC_OP_MAP_CONTAINSVALUE], np.uint8)
    if ttl:
        f = b.flags
        f[(f & 7) == abi.CC_TAG_NULL] |= np.uint8(abi.CC_TAG_LONG)
        f[((f >> 3) & 7) == abi.CC_TAG_NULL] |= np.uint8(abi.CC_TAG_LONG << 3)
        b.time[:] = np.arange(n, dtype=np.uint64) // np.uint64(8) + np.uint64(1000)
        arm = rng.random(n) < 0.4
        b.aux[:] = np.where(arm, rng.integers(1, 300, n), rng.choice([0, -5], n)).astype(np.int64).view(np.uint64)
        q = np.nonzero(rng.random(n) < 0.002)[0]
    else:
        rows = np.nonzero(rng.random(n) < 0.05)[0]
        b.op[rows] = abi.CC_OP_MAP_CLEAR
        q = np.nonzero(rng.random(n) < 0.01)[0]
        q = q[b.op[q] != abi.CC_OP_MAP_CLEAR]
    b.op[q] = rng.choice(wide, len(q))
    cv = q[b.op[q] == abi.CC_OP_MAP_CONTAINSVALUE]
    b.a[cv] = rng.integers(0, 3, len(cv)).astype(np.uint64)
    b.flags[cv] = (b.flags[cv] & np.uint8(0xF8)) | np.uint8(abi.CC_TAG_LONG)
    assert len(cv) > 10
    return b


COORD_TYPES = np.array([L, E_, G, V] * 4, np.uint8)
COORD_K = 6


def _coord_engine(flags=abi.CC_CFG_TIMERS_DEFERRED | abi.CC_CFG_VALUE_EVENTS | abi.CC_CFG_VALUE_RETAINED):
    from copycat_amd.engine import Engine

    R = len(COORD_TYPES)
    E = Engine(R, R * COORD_K + 8, 1 << 16, flags=flags, max_events=1 << 20)
    for r, t in enumerate(COORD_TYPES):
        E.resource_create(r, int(t))
        for k in range(COORD_K):
            E.instance_open(r * COORD_K + k, r, 1000 + r * COORD_K + k, 7 + k)
    return E


def _coord_stream(n):
    from copycat_amd.workload import coord_random_stream

    K, max_inst = COORD_K, len(COORD_TYPES) * COORD_K + 8
    b = coord_random_stream(n, COORD_TYPES, K, max_inst, seed=31)
    # MembershipGroup.schedule rows (batch barriers that arm timers), as tests/test_gpu_coord.py builds them
    rng = np.random.default_rng(31)
    res_of = np.where(b.inst < max_inst, b.inst // K, 0)
    grp = np.nonzero((COORD_TYPES[np.minimum(res_of, len(COORD_TYPES) - 1)] == G) & (b.inst < len(COORD_TYPES) * K))[0]
    rows = rng.choice(grp, size=n // 200, replace=False)
    b.op[rows] = abi.CC_OP_GROUP_SCHEDULE
    member = 1000 + res_of[rows] * K + rng.integers(0, K + 2, len(rows))  # some ids are not instances of this group
    b.key[rows] = member.astype(np.uint64)
    b.flags[rows] = abi.cc_flags(abi.CC_TAG_HANDLE, 0, 0)
    b.a[rows] = rng.integers(0, 1 << 20, len(rows)).astype(np.uint64)
    b.aux[rows] = rng.integers(-5, 400, len(rows)).astype(np.int64).view(np.uint64)
    assert (b.op == abi.CC_OP_LOCK_LOCK).any() and (b.op == abi.CC_OP_ELECT_LISTEN).any() and (b.op == abi.CC_OP_GROUP_JOIN).any()
    return b


def _state(E, kind, last_index):
    """Every readback the engine kind has, as comparable Python values."""
    out = {"applied": E.applied_index()}
    bm, cnt = E.retained_bitmap(1, last_index + 8)
    out["retained"] = (bm.cpu().numpy().tobytes(), cnt)
    if kind == "value":
        out["values"] = [x.tobytes() for x in E.value_state(0, 300)]
    elif kind == "map":
        out["table"] = [x.tobytes() for x in E.map_table()]
    else:
        for r, t in enumerate(COORD_TYPES):
            out[r] = (E.lock_state(r) if t == L else E.election_state(r) if t == E_ else E.group_members(r) if t == G
                      else tuple(int(x[0]) for x in E.value_state(r, 1)))
    return out


def _same_results(wide, packed, n):
    s1, v1, ev1 = wide
    s2, v2, ev2, done = packed
    assert done == n
    bad = np.nonzero((s1 != s2) | (v1 != v2))[0]
    assert len(bad) == 0, f"{len(bad)} rows differ, first {bad[:5]}: wide {s1[bad[:5]]},{v1[bad[:5]]} packed {s2[bad[:5]]},{v2[bad[:5]]}"
    assert ev1["count"] == ev2["count"]
    for k in EV_KEYS:  # every event, in order
        assert np.array_equal(ev1[k], ev2[k]), k


def _twin(make, stream, kind, columns=pc.ALL, **packed_kw):
    b = stream(2 * N)
    wide, packed = make(), make()
    for lo, hi in ((0, N), (N, 2 * N)):  # the second batch: the staging survives reuse
        part = b.slice(lo, hi)
        cap = 8 * N
        r1 = wide.apply_host_events(part, capacity=cap)
        r2 = packed.apply_host_packed(pack(part, columns=columns), N, capacity=cap, chunk_rows=pc.B, **packed_kw)
        _same_results(r1, r2, N)
        assert _state(wide, kind, int(b.index[-1])) == _state(packed, kind, int(b.index[-1]))
    return r1[2]


def test_packed_apply_value_engine():
    _twin(_value_engine, _value_stream, "value", columns=pc.VALUE_COLS)


def test_packed_apply_map_engine_whole_map_rows_and_nulls():
    _twin(_map_engine, lambda n: _map_stream(n, 502, ttl=False), "map")


@pytest.mark.parametrize("flags", [abi.CC_CFG_TIMERS_DEFERRED, 0], ids=["manager", "module"])
def test_packed_apply_ttl_map_engine(flags):
    _twin(lambda: _map_engine(flags), lambda n: _map_stream(n, 91, ttl=True), "map")


def test_packed_apply_coordination_engine_with_events():
    ev = _twin(_coord_engine, _coord_stream, "coord")
    assert len(ev["pos"]) > 1000 and len(set(ev["code"].tolist())) >= 4  # locks, elections, joins, leaves ... published


# ---- 8. failure and edge contract ---------------------------------------------------------------------------------------
def test_corrupted_blob_never_reaches_the_engine():
    from copycat_amd.engine import EngineError

    b = _value_stream(N)
    E, twin = _value_engine(), _value_engine()
    before = _state(E, "value", N)
    blob = pack(b, columns=pc.VALUE_COLS)
    for at, bit in ((0, 1), (9, 0x40), (64 + 1, 0x80), (64 + 160 + 16 * 7, 2)):  # magic, n, a block's rows, a's mode
        bad = blob.copy()
        bad[at] ^= bit
        with pytest.raises(EngineError) as e:
            E.apply_host_packed(bad, N, chunk_rows=pc.B)
        assert e.value.rc == abi.CC_ERR_INVALID
        assert _state(E, "value", N) == before
    _same_results(twin.apply_host_events(b), E.apply_host_packed(blob, N, chunk_rows=pc.B), N)
    assert _state(E, "value", N) == _state(twin, "value", N)


def test_event_stream_too_small_for_the_third_chunk():
    from copycat_amd.engine import RESULT_SENTINEL

    b = _coord_stream(N)
    ref, E, twin = _coord_engine(), _coord_engine(), _coord_engine()
    s0, v0, ev0 = ref.apply_host_events(b, capacity=8 * N)
    c2, c3 = int((ev0["pos"] < 2 * pc.B).sum()), int((ev0["pos"] < 3 * pc.B).sum())
    assert c3 > c2 > 0
    cap = c2 + (c3 - c2) // 2  # room for two chunks' events, not for the third's
    s, v, ev, done = E.apply_host_packed(pack(b), N, capacity=cap, chunk_rows=pc.B)
    assert done == 2 * pc.B
    # the events of the chunks applied plus the failing chunk's count as cc_apply_batch reports it: past the capacity
    # (that is the failure), at most what the chunk publishes (the engine does not count every event of a full stream)
    assert cap < ev["count"] <= c3
    assert np.array_equal(s[:done], s0[:done]) and np.array_equal(v[:done], v0[:done])
    for k in EV_KEYS:
        assert np.array_equal(ev[k][:c2], ev0[k][:c2]), k
    assert (s[done:] == RESULT_SENTINEL).all() and not v[done:].any()  # rows of the later chunks: as the caller had them
    twin.apply_host_events(b.slice(0, done), capacity=8 * N)  # a twin that applied exactly those rows
    assert _state(E, "coord", N) == _state(twin, "coord", N)
    # the host drains its stream and resumes at rows_done
    rest = b.slice(done, N)
    _same_results(twin.apply_host_events(rest, capacity=8 * N),
                  E.apply_host_packed(pack(rest), N - done, capacity=8 * N, chunk_rows=pc.B), N - done)
    assert _state(E, "coord", N) == _state(ref, "coord", N)


def test_zero_rows_and_one_chunk():
    E, twin = _value_engine(), _value_engine()
    s, v, ev, done = E.apply_host_packed(pack(Batch(0)), 0, chunk_rows=pc.B)
    assert (len(s), len(v), done, ev["count"]) == (0, 0, 0, 0)
    assert E.applied_index() == 0
    b = _value_stream(N)
    for chunk_rows in (1 << 30, 0):  # larger than n, and the default: one chunk
        part = b.slice(0, N)
        _same_results(twin.apply_host_events(part), E.apply_host_packed(pack(part), N, chunk_rows=chunk_rows), N)
    assert _state(E, "value", N) == _state(twin, "value", N)


# ---- 9. cc_host_register -------------------------------------------------------------------------------------------------
def test_registered_blob_and_results():
    from copycat_amd.engine import RESULT_SENTINEL, host_register, host_unregister, lib

    b = _value_stream(N)
    blob = pack(b, columns=pc.VALUE_COLS)
    status, value = np.full(N, RESULT_SENTINEL, np.uint8), np.zeros(N, np.uint64)
    for arr in (blob, status, value):
        host_register(arr)
    try:
        E, twin = _value_engine(), _value_engine()
        packed = E.apply_host_packed(blob, N, chunk_rows=pc.B, out=(status, value), timeline=True)
        assert packed[0] is status and packed[1] is value
        _same_results(twin.apply_host_events(b), packed, N)
        assert _state(E, "value", N) == _state(twin, "value", N)
        ms = E.packed_timeline()
        assert ms.shape == (6, 4) and (ms >= 0).all()
    finally:
        for arr in (blob, status, value):
            host_unregister(arr)
    L_ = lib()
    assert L_.cc_host_register(None, 16) == abi.CC_ERR_INVALID
    assert L_.cc_host_register(C.c_void_p(blob.ctypes.data), 0) == abi.CC_ERR_INVALID
    assert L_.cc_host_unregister(None) == abi.CC_ERR_INVALID
