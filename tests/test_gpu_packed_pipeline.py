"""The chunk pipeline behind cc_apply_batch_host_packed, cc_apply_batch_host_packed_results and
cc_apply_batch_host_packed_events on the MI355X: the paths where the three calls differ and that the twin tests of
test_gpu_pack.py, test_gpu_respack.py and test_gpu_evpack.py leave out.

  1. a chunk rolled back for a full event stream at chunk index 0, 1 and 3 (no copy-out to wait for; a header-only
     result blob; the second reuse of result set / staging 1);
  2. a chunk that fails a device-side check other than a capacity: it stays applied and its rows are delivered;
  3. a chunk rolled back for a full map table region on a call without an event stream.

Bar: bit-exact.  Every comparison is integer or byte equality against a reference engine that applied the same rows
through the wide entry points, or between the three calls.  All calls go through ctypes, so the return codes are the
library's."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from copycat_amd import abi
from copycat_amd.batch import (Batch, _aligned_bytes, events_bound, events_check, pack, results_bound, results_check,
                               unpack_events, unpack_results)
from tests import evpack_cases as ec
from tests import pack_cases as pc
from tests.test_gpu_pack import EV_KEYS, N, _coord_engine, _coord_stream, _state, _value_engine, _value_stream

pytestmark = pytest.mark.gpu

B = pc.B  # chunk_rows of every call here: N = 5 B + 123 rows are six chunks
KINDS = ("wide", "results", "events")


def _call(kind, E, blob, n, cap):
    """One of the three pipelined calls on a packed batch of n rows in chunks of B rows.  cap: the event capacity
    (None: no event stream, which the events call does not offer).  Returns rc, rows_done, the result rows (wide: the
    caller's n rows, prefilled as Engine.apply_host_packed prefills them; blob: the rows the result blob holds, and
    the blob as .res), the events kept (.ev, columns; the events call: its blob decoded, the blob as .evb) and the
    reported event count."""
    from copycat_amd.engine import RESULT_SENTINEL

    L = E.L
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    opts = abi.cc_packed_opts(chunk_rows=B, flags=0)
    done = C.c_uint64()
    out = SimpleNamespace(res=None, evb=None, ev=None, count=None)
    hev = None
    if kind != "events" and cap is not None:
        dt = {"pos": np.uint32, "target": np.uint32, "code": np.uint8, "src": np.uint8, "tag": np.uint8, "payload": np.uint64}
        cols = {k: np.zeros(cap, dt[k]) for k in EV_KEYS}
        count = np.zeros(1, np.uint64)
        ev = abi.cc_events(*(cols[k].ctypes.data for k in EV_KEYS), cap, count.ctypes.data)
        hev = C.byref(ev)
    if kind == "wide":
        out.status, out.value = np.full(n, RESULT_SENTINEL, np.uint8), np.zeros(n, np.uint64)
        r = abi.cc_results(out.status.ctypes.data, out.value.ctypes.data)
        out.rc = L.cc_apply_batch_host_packed(E.h, blob.ctypes.data, blob.nbytes, C.byref(r), hev, C.byref(opts), C.byref(done))
    else:
        res, size = _aligned_bytes(results_bound(n)), C.c_uint64()
        if kind == "results":
            out.rc = L.cc_apply_batch_host_packed_results(E.h, blob.ctypes.data, blob.nbytes, res.ctypes.data, res.nbytes,
                                                          C.byref(size), hev, C.byref(opts), C.byref(done))
        else:
            evb, ev_size, ev_count = _aligned_bytes(events_bound(cap)), C.c_uint64(), C.c_uint64()
            out.rc = L.cc_apply_batch_host_packed_events(E.h, blob.ctypes.data, blob.nbytes, res.ctypes.data, res.nbytes,
                                                         C.byref(size), evb.ctypes.data, cap, evb.nbytes, C.byref(ev_size),
                                                         C.byref(ev_count), C.byref(opts), C.byref(done))
            assert ev_size.value <= evb.nbytes
            out.evb, out.count = evb[:ev_size.value], ev_count.value
            out.ev = unpack_events(out.evb)
        assert size.value <= res.nbytes
        out.res = res[:size.value]
        out.status, out.value = unpack_results(out.res)
    if hev is not None:
        out.count = int(count[0])
        out.ev = {k: v[:min(out.count, cap)] for k, v in cols.items()}
    out.done = done.value
    return out


def _untouched(r, lo):
    """Rows [lo, n) of a wide call's results are as the caller had them."""
    from copycat_amd.engine import RESULT_SENTINEL

    return bool((r.status[lo:] == RESULT_SENTINEL).all()) and not r.value[lo:].any()


# ---- 1. rollback at chunk 0, 1 and 3 -------------------------------------------------------------------------------------
ROLLBACK_AT = (0, 1, 3)


@pytest.fixture(scope="module")
def coord_ref():
    """The coordination stream applied once through the wide device path, and twins that applied exactly k chunks."""
    b = _coord_stream(N)
    ref = _coord_engine()
    s0, v0, ev0 = ref.apply_host_events(b, capacity=8 * N)
    final = _state(ref, "coord", N)
    ref.close()
    cum = np.searchsorted(ev0["pos"], np.arange(0, N + B, B).clip(max=N))  # cum[k]: the events of chunks before k
    assert cum[-1] == len(ev0["pos"])
    after = {}
    for k in ROLLBACK_AT:
        twin = _coord_engine()
        if k:
            twin.apply_host_events(b.slice(0, k * B), capacity=8 * N)
        after[k] = _state(twin, "coord", N)
        twin.close()
    return SimpleNamespace(b=b, blob=pack(b), s=s0, v=v0, ev=ev0, cum=[int(c) for c in cum], final=final, after=after,
                           rest={k: pack(b.slice(k * B, N)) for k in ROLLBACK_AT})


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", ROLLBACK_AT)
def test_event_stream_too_small_for_chunk(coord_ref, k, kind):
    ref, cum = coord_ref, coord_ref.cum
    assert all(b - a >= 2 for a, b in zip(cum[:-1], cum[1:])), "a chunk publishes fewer than two events"
    ck, ck1 = cum[k], cum[k + 1]
    cap = ck + (ck1 - ck) // 2  # room for the chunks before k and half of chunk k's events
    assert ck < cap < ck1
    E = _coord_engine()
    r = _call(kind, E, ref.blob, N, cap)
    done = k * B
    assert r.rc == abi.CC_ERR_CAPACITY and r.done == done
    if kind == "wide":
        assert _untouched(r, done)
    else:
        assert results_check(r.res) == done == len(r.status)  # the rolled-back chunk is not in the blob
        assert k or len(r.res) == 64
    assert r.status[:done].tobytes() == ref.s[:done].tobytes() and r.value[:done].tobytes() == ref.v[:done].tobytes()
    if kind == "events":
        assert events_check(r.evb) == ck and ec.same(r.ev, ec.take(ref.ev, 0, ck))
    else:
        for key in EV_KEYS:
            assert np.array_equal(r.ev[key][:ck], ref.ev[key][:ck]), key
    assert cap < r.count <= ck1
    assert _state(E, "coord", N) == ref.after[k]
    # the host drains its stream and resumes at rows_done
    r2 = _call(kind, E, ref.rest[k], N - done, 8 * N)
    assert r2.rc == abi.CC_OK and r2.done == N - done == len(r2.status)
    assert r2.status.tobytes() == ref.s[done:].tobytes() and r2.value.tobytes() == ref.v[done:].tobytes()
    assert r2.count == cum[-1] - ck == len(r2.ev["pos"])
    assert np.array_equal(r2.ev["pos"] + np.uint32(done), ref.ev["pos"][ck:])  # (pos counts from the resumed batch's row 0)
    for key in EV_KEYS[1:]:
        assert np.array_equal(r2.ev[key], ref.ev[key][ck:]), key
    assert _state(E, "coord", N) == ref.final
    E.close()


# ---- 2. a failing chunk that stays applied -------------------------------------------------------------------------------
BAD_ROW = 2 * B + 17  # a row of the third chunk


def _unsupported_op():
    """An AtomicValue listen on an engine without CC_CFG_VALUE_EVENTS: an op the build does not run there."""
    b = _value_stream(N)
    b.op[BAD_ROW] = abi.CC_OP_VALUE_LISTEN
    return _value_engine, "value", b, pc.VALUE_COLS, abi.CC_ERR_UNSUPPORTED


def _decreasing_time():
    """A log time below the row before it on an engine that checks time order."""
    b = _coord_stream(N)
    assert b.time[BAD_ROW - 1] > 0
    b.time[BAD_ROW] = b.time[BAD_ROW - 1] - np.uint64(1)
    return _coord_engine, "coord", b, pc.ALL, abi.CC_ERR_INVALID


@pytest.mark.parametrize("case", [_unsupported_op, _decreasing_time], ids=["unsupported_op", "decreasing_time"])
def test_failing_chunk_that_stays_applied_is_delivered(case):
    make, state_kind, b, columns, want_rc = case()
    blob = pack(b, columns=columns)
    ref = make()
    s0, v0, ev0 = ref.apply_host_events(b.slice(0, 2 * B), capacity=8 * N)  # the chunks before the failing one
    ref.close()
    engines = {kind: make() for kind in KINDS}
    r = {kind: _call(kind, engines[kind], blob, N, 8 * N) for kind in KINDS}
    for kind in KINDS:
        assert r[kind].rc == want_rc and r[kind].done == 2 * B, kind
    # not a rollback: the three chunks' rows went out, the later chunks' rows did not
    w = r["wide"]
    assert _untouched(w, 3 * B) and not _untouched(SimpleNamespace(status=w.status[:3 * B], value=w.value[:3 * B]), 2 * B)
    for kind in ("results", "events"):
        assert results_check(r[kind].res) == 3 * B == len(r[kind].status)
        assert np.array_equal(r[kind].res, r["results"].res)
        assert r[kind].status.tobytes() == w.status[:3 * B].tobytes() and r[kind].value.tobytes() == w.value[:3 * B].tobytes()
    assert w.status[:2 * B].tobytes() == s0.tobytes() and w.value[:2 * B].tobytes() == v0.tobytes()
    # the failing chunk's events are counted by all three and kept by the host streams; the event blob holds the
    # events of the chunks fully applied
    assert r["wide"].count == r["results"].count == r["events"].count >= len(ev0["pos"])
    assert ec.same(r["wide"].ev, r["results"].ev)
    assert events_check(r["events"].evb) == len(ev0["pos"]) and ec.same(r["events"].ev, ev0)
    for key in EV_KEYS:
        assert np.array_equal(r["wide"].ev[key][:len(ev0["pos"])], ev0[key]), key
    states = [_state(E, state_kind, N) for E in engines.values()]
    assert states[0] == states[1] == states[2]
    for E in engines.values():
        E.close()


# ---- 3. map-region rollback without an event stream ----------------------------------------------------------------------
def _small_map_engine():
    """One map in two 2,048-entry table regions (map_capacity 1,024)."""
    from copycat_amd.engine import Engine

    E = Engine(1, 4, 1 << 14, map_capacity=1024, flags=abi.CC_CFG_TIMERS_DEFERRED)
    E.resource_create_range(0, 1, abi.CC_RES_MAP)
    E.instance_open_range(0, 1, 0, 1000, 7)
    return E


def _overflowing_map_stream():
    """Chunks 0 and 1 put and get 1,000 keys over and over; chunk 2 puts 4,096 keys nothing has used: with the 1,000
    that is a thousand more than the table's 4,096 entries; the chunks after it get the first keys."""
    rng = np.random.default_rng(77)
    old = np.arange(1000, dtype=np.uint64) * np.uint64(7919) + np.uint64(3)
    key = old[rng.integers(0, len(old), N)]
    op = rng.choice(np.array([abi.CC_OP_MAP_PUT, abi.CC_OP_MAP_GET], np.uint8), N, p=[0.7, 0.3])
    key[2 * B:3 * B] = np.arange(B, dtype=np.uint64) * np.uint64(104729) + np.uint64(1 << 40)
    op[2 * B:3 * B] = abi.CC_OP_MAP_PUT
    op[3 * B:] = abi.CC_OP_MAP_GET
    return Batch.from_columns(index=np.arange(1, N + 1, dtype=np.uint64), inst=np.zeros(N, np.uint32), op=op,
                              flags=np.full(N, abi.cc_flags(abi.CC_TAG_LONG, 0, 0), np.uint8), key=key,
                              a=key * np.uint64(3) + np.arange(N, dtype=np.uint64))


def test_map_region_full_in_the_third_chunk_without_an_event_stream():
    from copycat_amd.engine import EngineError

    b = _overflowing_map_stream()
    ref = _small_map_engine()  # the precondition: chunks 0 and 1 fit, chunk 2 does not
    ref.apply_host(b.slice(0, B))
    ref.apply_host(b.slice(B, 2 * B))
    with pytest.raises(EngineError) as e:
        ref.apply_host(b.slice(2 * B, 3 * B))
    assert e.value.rc == abi.CC_ERR_CAPACITY
    ref.close()
    twin = _small_map_engine()  # applied exactly the rows of chunks 0 and 1
    s0, v0 = twin.apply_host(b.slice(0, 2 * B))
    want = _state(twin, "map", N)
    twin.close()
    blob = pack(b)
    for kind in ("wide", "results"):
        E = _small_map_engine()
        r = _call(kind, E, blob, N, None)
        assert r.rc == abi.CC_ERR_CAPACITY and r.done == 2 * B, kind
        if kind == "wide":
            assert _untouched(r, 2 * B)
        else:
            assert results_check(r.res) == 2 * B == len(r.status)
        assert r.status[:2 * B].tobytes() == s0.tobytes() and r.value[:2 * B].tobytes() == v0.tobytes(), kind
        assert _state(E, "map", N) == want, kind
        E.close()
