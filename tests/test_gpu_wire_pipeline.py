"""cc_apply_wire_host_packed on the MI355X: a wire segment as a source of the chunk pipeline (host_path.hip WireSource,
wire_gpu.hip wire_chunk_decode, k_wire_offsets_check / k_wire_offsets_clamp), packed results and events out.

The yardstick is a twin engine driven by cc_apply_wire_host chunk by chunk over the same cuts (the existing, tested
path; never the code under test): `_twin` stops where the contract says a segment stops (a manager entry, a failing
chunk) and reports rows as segment rows.  Per case: the unpacked results and events, rows_done, ctl, return code, bad
row and error text, the interner's Strings, the engine's snapshot bytes (registered String.hashCodes included) and the
applied index are equal, and both blobs pass their checks.  B = 4096 rows is chunk_rows unless a case says otherwise.

A chunk that fails on a full event stream or map table region is rolled back by the pipeline but stays applied in
cc_apply_wire_host, so there the twin is driven over the chunks before it only."""
import ctypes as C
import re
from types import SimpleNamespace

import numpy as np
import pytest

from copycat_amd import abi
from copycat_amd.batch import Batch, _aligned_bytes, events_check, pack, results_check, unpack_events, unpack_results
from tests.test_gpu_wire_device import _decoders, _segment, _strings_of
from tests.test_gpu_wire_strings import _entry

pytestmark = pytest.mark.gpu

B = abi.CC_PACK_BLOCK_ROWS
EV_KEYS = ("pos", "target", "code", "src", "tag", "payload")
EV_DT = {"pos": np.uint32, "target": np.uint32, "code": np.uint8, "src": np.uint8, "tag": np.uint8, "payload": np.uint64}
VALUES, MAP_IID, TOPIC_IID, LOCK_IID = 200, 5000, 6000, 7000


def _engine():
    """200 values (instance ids 100..299), one map (5000), one topic and one lock with eight sessions each"""
    from copycat_amd.engine import Engine

    E = Engine(256, 256, 1 << 16, flags=abi.CC_CFG_VALUE_EVENTS | abi.CC_CFG_TIMERS_DEFERRED, max_events=1 << 16,
               map_capacity=4096)
    E.resource_create_range(0, VALUES, abi.CC_RES_VALUE)
    E.instance_open_range(0, VALUES, 0, 100, 1)
    E.resource_create(200, abi.CC_RES_MAP)
    E.instance_open(200, 200, MAP_IID, 1)
    E.resource_create(201, abi.CC_RES_TOPIC)
    E.resource_create(202, abi.CC_RES_LOCK)
    for k in range(8):
        E.instance_open(201 + k, 201, TOPIC_IID + k, 10 + k)
        E.instance_open(209 + k, 202, LOCK_IID + k, 20 + k)
    return E


def _cas(rng, n):
    """a plain CAS stream over the 200 values, eight listeners first"""
    out = [_entry(100 + int(i), abi.CC_OP_VALUE_LISTEN, []) for i in rng.integers(0, VALUES, min(8, n))]
    for _ in range(n - len(out)):
        a = ("NULL", 0) if rng.integers(0, 4) == 0 else ("LONG", int(rng.integers(0, 4)))
        out.append(_entry(100 + int(rng.integers(0, VALUES)), abi.CC_OP_VALUE_CAS, [a, ("LONG", int(rng.integers(0, 4)))]))
    return out


_STREAMS = {}


def _cas_stream(n):
    """(buf, offsets) of the first n entries of one CAS stream, built once"""
    if "cas" not in _STREAMS:
        _STREAMS["cas"] = _cas(np.random.default_rng(5), 3 * B + 5)
    return _STREAMS["cas"][:n]


def _set_str(iid, s):
    return _entry(iid, abi.CC_OP_VALUE_SET, [("STR", s)])


def _manager(kind, key, rtype="io.atomix.atomic.state.AtomicValueState"):
    """GetResource (35) / ResourceExists (38) under the default codec"""
    k = key.encode()
    e = bytes([2]) + kind.to_bytes(2, "big") + b"\x01" + len(k).to_bytes(2, "big") + k
    if kind != 38:
        e += len(rtype).to_bytes(4, "big") + rtype.encode()
    return e


def _cuts(n, chunk=B):
    return list(range(0, n, chunk)) + [n]


def _hev(cap):
    cols = {k: np.zeros(max(cap, 1), EV_DT[k]) for k in EV_KEYS}
    count = np.zeros(1, np.uint64)
    return cols, count, abi.cc_events(*(cols[k].ctypes.data for k in EV_KEYS), cap, count.ctypes.data)


def _text(E):
    return E.L.cc_last_error().decode(errors="replace")


def _twin(E, d, buf, offs, index, time, cuts, events=True, upto=None):
    """consecutive cc_apply_wire_host calls over the chunks [cuts[k], cuts[k + 1]) (the first `upto` of them), stopping as
    a segment stops; rows are reported as segment rows"""
    out = SimpleNamespace(rc=0, text="", bad_row=None, done=0, ctl=None, status=[], value=[], ev={k: [] for k in EV_KEYS})
    offs = np.ascontiguousarray(offs, np.uint64)
    for lo, hi in list(zip(cuts[:-1], cuts[1:]))[:upto]:
        m = hi - lo
        status, value = np.full(m, 0xEE, np.uint8), np.zeros(m, np.uint64)
        r = abi.cc_results(status.ctypes.data, value.ctypes.data)
        cols, count, hev = _hev(8 * m + 1024)
        applied, ctl = C.c_uint64(), abi.cc_wire_control()
        o, ix = offs[lo:hi + 1], index[lo:hi]
        tm = None if time is None else time[lo:hi]
        rc = E.L.cc_apply_wire_host(E.h, C.byref(d.codec), d.interner.h, buf.ctypes.data, buf.size, o.ctypes.data, m,
                                    ix.ctypes.data, tm.ctypes.data if tm is not None else None, C.byref(r),
                                    C.byref(hev) if events else None, C.byref(applied), C.byref(ctl))
        if rc:
            out.rc, text = rc, _text(E)
            mm = re.match(r"wire row (\d+): (.*)", text)
            if mm:  # (a chunk call numbers its own rows)
                out.bad_row = lo + int(mm.group(1))
                text = f"wire row {out.bad_row}: {mm.group(2)}"
            else:   # an offsets violation: the first row the scan of this chunk stops at
                bad = [i for i in range(m) if o[i + 1] < o[i] or o[i + 1] > buf.size]
                out.bad_row = lo + bad[0]
            out.text = text
            return out
        a = applied.value
        out.status.append(status[:a]), out.value.append(value[:a])
        if events:
            c = int(count[0])
            for k in EV_KEYS:
                out.ev[k].append(cols[k][:c] + np.uint32(lo) if k == "pos" else cols[k][:c])
        out.done = lo + a
        if a < m:
            out.ctl = {"row": lo + int(ctl.row), "kind": int(ctl.kind), "key": int(ctl.key), "a": int(ctl.a), "b": int(ctl.b)}
            return out
    return out


def _new(E, d, buf, offs, index, time=None, cap=None, chunk_rows=B, events=True, aux=None):
    """the call under test through the binding; an error is caught and kept"""
    from copycat_amd.engine import EngineError

    n = len(offs) - 1
    out = SimpleNamespace(rc=0, text="", bad_row=None, ctl=None)
    try:
        out.res, out.evb, out.ev_count, out.done, out.ctl = E.apply_wire_host_packed(
            d, index, time=time, buf=buf, offsets=offs, capacity=cap if cap is not None else 8 * n + 1024,
            chunk_rows=chunk_rows, events=events, aux=aux)
        if out.ctl is None and out.done < n:
            out.rc = abi.CC_ERR_CAPACITY
    except EngineError as x:
        out.rc, out.text, out.bad_row, out.done = x.rc, str(x).split(": ", 1)[1], x.bad_row, x.rows_done
        out.res, out.evb, out.ev_count = x.result_blob, x.event_blob, x.ev_count
    assert results_check(out.res) == out.done  # (cc_respack_check passes, and the blob holds the rows done)
    out.status, out.value = unpack_results(out.res)
    if events:
        out.ev = unpack_events(out.evb)  # (cc_evpack_check first)
        assert events_check(out.evb) == len(out.ev["pos"]) <= out.ev_count
    return out


def _same(new, twin, events=True):
    assert (new.rc, new.done, new.ctl) == (twin.rc, twin.done, twin.ctl), ((new.rc, new.text, new.done, new.ctl),
                                                                            (twin.rc, twin.text, twin.done, twin.ctl))
    if twin.rc:
        assert new.text == twin.text and new.bad_row == twin.bad_row, (new.text, new.bad_row, twin.text, twin.bad_row)
    ts = np.concatenate(twin.status) if twin.status else np.zeros(0, np.uint8)
    tv = np.concatenate(twin.value) if twin.value else np.zeros(0, np.uint64)
    bad = np.nonzero((new.status != ts) | (new.value != tv))[0]
    assert bad.size == 0, (bad[:8], new.status[bad[:8]], ts[bad[:8]], new.value[bad[:8]], tv[bad[:8]])
    if events:
        for k in EV_KEYS:
            want = np.concatenate(twin.ev[k]) if twin.ev[k] else np.zeros(0, EV_DT[k])
            assert np.array_equal(np.asarray(new.ev[k]).astype(np.uint64), want.astype(np.uint64)), k


def _same_state(En, dn, Et, dt):
    assert _strings_of(dn) == _strings_of(dt)
    assert En.applied_index() == Et.applied_index()
    assert En.snapshot() == Et.snapshot()


def _pair(attach=False, strings=()):
    En, Et = _engine(), _engine()
    dn, dt = _decoders(En, strings)[0], _decoders(Et, strings)[0]
    if attach:
        dn.attach_dictionary()
        dt.attach_dictionary()
    return En, dn, Et, dt


def _run(entries, attach=False, strings=(), time=False, events=True, cap=None, base=1):
    """one segment through both paths in chunks of B rows; everything compared -> (new, twin, engines and decoders)"""
    buf, offs = _segment(entries)
    n = len(entries)
    index = np.arange(base, base + n, dtype=np.uint64)
    tm = np.arange(n, dtype=np.uint64) // np.uint64(7) + np.uint64(50) if time else None
    En, dn, Et, dt = _pair(attach, strings)
    assert En.snapshot() == Et.snapshot()  # (two engines built alike: the comparisons below mean something)
    new = _new(En, dn, buf, offs, index, tm, cap=cap, events=events)
    twin = _twin(Et, dt, buf, offs, index, tm, _cuts(n), events=events)
    _same(new, twin, events)
    _same_state(En, dn, Et, dt)
    return new, twin, (En, dn, Et, dt), (buf, offs, index, tm)


def _close(*engines):
    for E in engines:
        E.close()


# ---- 1. sizes, with and without time, three chunkings ------------------------------------------------------------------
@pytest.mark.parametrize("time", [False, True], ids=["notime", "time"])
@pytest.mark.parametrize("n", [1, B - 1, B, B + 1, 3 * B + 5])
def test_sizes_and_chunkings(n, time):
    new, twin, (En, dn, Et, dt), (buf, offs, index, tm) = _run(_cas_stream(n), time=time)
    assert new.rc == 0 and new.done == n and new.ctl is None
    assert n < 8 or new.ev_count > 0
    for chunk in (2 * B, n):  # the blobs' bytes do not depend on the chunking
        E2 = _engine()
        d2 = _decoders(E2)[0]
        other = _new(E2, d2, buf, offs, index, tm, chunk_rows=chunk)
        assert other.rc == 0 and other.done == n
        assert other.res.tobytes() == new.res.tobytes() and other.evb.tobytes() == new.evb.tobytes()
        assert E2.snapshot() == En.snapshot()
        E2.close()
    _close(En, Et)


# ---- 2. escapes at the seams ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attach", [False, True], ids=["unattached", "attached"])
def test_string_entries_at_the_seams(attach):
    n = 2 * B + 100
    entries = list(_cas_stream(n))
    for k, row in enumerate((B - 1, B, n - 1)):
        entries[row] = _set_str(100 + k, f"seam-{k}")
    new, twin, (En, dn, Et, dt), _ = _run(entries, attach=attach)
    assert new.rc == 0 and new.done == n
    assert _strings_of(dn) == ["seam-0", "seam-1", "seam-2"]
    _close(En, Et)


# ---- 3. a String first seen in chunk k, used again in chunk k + 1 --------------------------------------------------------------
def test_string_of_chunk_k_resolves_on_the_device_in_chunk_k_plus_1():
    n = 2 * B
    entries = list(_cas_stream(n))
    entries[10] = _set_str(100, "fresh")
    again = list(range(B + 5, B + 25))
    for row in again:
        entries[row] = _set_str(100 + row % 7, "fresh")
    new, twin, (En, dn, Et, dt), _ = _run(entries, attach=True)
    assert new.rc == 0 and new.done == n and _strings_of(dn) == ["fresh"]
    # the handles are the twin's (the results carry them: _same compared every row), and the last chunk's String rows
    # were all resolved by the kernel
    assert dn.dictionary_info()["last_str_rows"] == len(again) == dt.dictionary_info()["last_str_rows"]
    assert dn.dictionary_info()["strings"] == 1
    _close(En, Et)


# ---- 4. a String key whose hash is not registered yet --------------------------------------------------------------------------
def test_unregistered_string_key_is_registered_as_on_the_twin():
    n = B + 50
    entries = list(_cas_stream(n))
    keys = {7: "alpha", B - 1: "beta", B + 3: "alpha", B + 9: "gamma"}
    for row, key in keys.items():
        entries[row] = _entry(MAP_IID, abi.CC_OP_MAP_PUT, [("STR", key), ("LONG", row), ("RAW8", 0)])
    for attach in (False, True):
        new, twin, (En, dn, Et, dt), (buf, offs, index, _) = _run(entries, attach=attach, strings=("alpha", "beta", "gamma"))
        assert new.rc == 0 and new.done == n
        # registered now (the snapshots, which hold the registered hashes, were equal): the same segment again decodes
        # those rows on the device when the dictionary is attached
        index2 = index + np.uint64(n)
        new2 = _new(En, dn, buf, offs, index2)
        twin2 = _twin(Et, dt, buf, offs, index2, None, _cuts(n))
        _same(new2, twin2)
        _same_state(En, dn, Et, dt)
        if attach:
            assert dn.dictionary_info()["last_str_rows"] == 2  # chunk 1's two String-keyed rows
        _close(En, Et)


# ---- 5. manager entries ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [0, B - 1, 2 * B], ids=["row0", "chunk_last", "chunk2_first"])
def test_manager_entry_stops_and_the_segment_resumes(r):
    n = 2 * B + 50
    entries = list(_cas_stream(n))
    entries[r] = _manager(35, "made-by-the-log")
    later = min(r + 20, n - 1)
    if later > r:
        entries[later] = _set_str(101, "after-the-stop")
    buf, offs = _segment(entries)
    index = np.arange(1 << 20, (1 << 20) + n, dtype=np.uint64)  # (GetResource names its instance by the commit index)
    En, dn, Et, dt = _pair()
    new = _new(En, dn, buf, offs, index)
    twin = _twin(Et, dt, buf, offs, index, None, _cuts(n))
    _same(new, twin)
    assert new.rc == 0 and new.done == r and new.ctl["row"] == r and new.ctl["kind"] == 35
    assert _strings_of(dn) == ["made-by-the-log"]  # no String of a later row is interned
    _same_state(En, dn, Et, dt)
    # the host runs the manager command, then the rest of the segment
    for E, ctl in ((En, new.ctl), (Et, twin.ctl)):
        st, iid, _ = E.get_resource(ctl["key"], ctl["a"], 7, int(index[r]))
        assert abi.status_code(st) == abi.CC_ST_OK
    rest = n - r - 1
    new2 = _new(En, dn, buf, offs[r + 1:], index[r + 1:])
    twin2 = _twin(Et, dt, buf, offs[r + 1:], index[r + 1:], None, _cuts(rest))
    _same(new2, twin2)
    assert new2.rc == 0 and new2.done == rest
    _same_state(En, dn, Et, dt)
    _close(En, Et)


# ---- 6. a malformed entry in chunk 2 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["truncated", "unknown_inner_id"])
def test_malformed_entry_in_chunk_2(how):
    n = 3 * B + 5
    row = 2 * B + 17
    entries = list(_cas_stream(n))
    entries[2 * B + 3] = _set_str(100, "before-the-bad-row")  # (interned on both paths before the row fails)
    entries[row] = entries[row][:-1] if how == "truncated" else _entry(100, 200, [("LONG", 1)])
    new, twin, (En, dn, Et, dt), _ = _run(entries)
    assert new.rc == abi.CC_ERR_INVALID and new.bad_row == row and new.text.startswith(f"wire row {row}: ")
    assert new.done == 2 * B and len(new.status) == 2 * B  # chunks 0-1 applied and in the blobs, chunk 2 not applied
    assert En.applied_index() == 2 * B
    _close(En, Et)


# ---- 7. offsets violations -------------------------------------------------------------------------------------------------------------
def _violate(offs, buf, how, at):
    """`at` = the offset rewritten (the end of row at - 1)"""
    offs = offs.copy()
    if how == "decreasing":
        offs[at] = offs[at - 1] - np.uint64(1) if at % B else offs[at - B] - np.uint64(1)  # (a chunk end: below its start)
    elif how == "past_buf_len":
        offs[at] = np.uint64(buf.size + 7)
    else:  # inside the buffer, but past the end of the chunk of row at - 1 (the device's check is the stricter one)
        offs[at] = offs[(at + B - 1) // B * B] + np.uint64(3)
    return offs


@pytest.mark.parametrize("how,where", [("decreasing", "inside"), ("past_buf_len", "inside"), ("past_chunk_end", "inside"),
                                       ("decreasing", "chunk_end"), ("past_buf_len", "chunk_end")])
def test_offsets_violations(how, where):
    n = 3 * B + 5
    buf, good = _segment(_cas_stream(n))
    at = B + 1234 if where == "inside" else 2 * B
    offs = _violate(good, buf, how, at)
    index = np.arange(1, n + 1, dtype=np.uint64)
    En, dn, Et, dt = _pair()
    new = _new(En, dn, buf, offs, index)
    twin = _twin(Et, dt, buf, offs, index, None, _cuts(n))
    _same(new, twin)
    assert new.rc == abi.CC_ERR_INVALID and new.bad_row == at - 1 and new.done == B
    if how == "past_chunk_end":  # the row itself is in bounds: it fails in the host decoder, as on the twin
        assert new.text.startswith(f"wire row {at - 1}: ")
    else:
        assert new.text == ("wire decode: offsets decrease" if how == "decreasing" else "wire decode: entry ends past the buffer")
    _same_state(En, dn, Et, dt)
    _close(En, Et)


def test_offsets_violation_after_a_manager_entry_in_the_same_chunk_is_not_reached():
    n = 2 * B
    entries = list(_cas_stream(n))
    entries[B + 10] = _manager(38, "exists?")
    buf, good = _segment(entries)
    offs = _violate(good, buf, "past_buf_len", B + 500)
    index = np.arange(1, n + 1, dtype=np.uint64)
    En, dn, Et, dt = _pair()
    new = _new(En, dn, buf, offs, index)
    twin = _twin(Et, dt, buf, offs, index, None, _cuts(n))
    _same(new, twin)
    assert new.rc == 0 and new.done == B + 10 and new.ctl["kind"] == 38
    _same_state(En, dn, Et, dt)
    _close(En, Et)


# ---- 8. events ---------------------------------------------------------------------------------------------------------------------------
def _topic_and_lock_stream(n):
    """topic listens / unlistens / publishes and lock / unlock rows.  The lock is modelled here (a holder and a FIFO of
    waiters): a session asks for it only while it neither holds nor waits for it, and only the holder unlocks, so the
    queue never grows past the eight sessions"""
    rng = np.random.default_rng(9)
    out = [_entry(TOPIC_IID + k, abi.CC_OP_TOPIC_LISTEN, []) for k in range(5)]
    holder, waiters = None, []
    while len(out) < n:
        x = int(rng.integers(0, 10))
        k = int(rng.integers(0, 8))
        if x < 4:
            out.append(_entry(TOPIC_IID + k, abi.CC_OP_TOPIC_PUBLISH, [("LONG", len(out))]))
        elif x < 9:
            if holder is not None and (x < 7 or k == holder or k in waiters):
                out.append(_entry(LOCK_IID + holder, abi.CC_OP_LOCK_UNLOCK, []))
                holder = waiters.pop(0) if waiters else None
            else:
                out.append(_entry(LOCK_IID + k, abi.CC_OP_LOCK_LOCK, [("RAW8", -1)]))
                if holder is None:
                    holder = k
                else:
                    waiters.append(k)
        else:
            out.append(_entry(TOPIC_IID + k, abi.CC_OP_TOPIC_LISTEN if rng.integers(0, 2) else abi.CC_OP_TOPIC_UNLISTEN, []))
    return out


def _readbacks(E):
    """the read-back calls of the engine of _engine(), as tests/test_gpu_packed_pipeline.py compares a rolled-back call
    (a restored checkpoint is the same state, not the same snapshot bytes)"""
    return {"applied": E.applied_index(), "values": [x.tobytes() for x in E.value_state(0, VALUES)],
            "lock": E.lock_state(202), "topic": E.topic_listeners(201)}


def test_topic_and_lock_events_span_chunks_and_a_full_event_stream_rolls_chunk_2_back():
    n = 3 * B + 5
    entries = _topic_and_lock_stream(n)
    new, twin, (En, dn, Et, dt), (buf, offs, index, _) = _run(entries)
    assert new.rc == 0 and new.done == n
    pos = np.asarray(new.ev["pos"])
    per_chunk = [int(((pos >= lo) & (pos < hi)).sum()) for lo, hi in zip(_cuts(n)[:-1], _cuts(n)[1:])]
    assert all(c > 100 for c in per_chunk[:3]), per_chunk
    codes = set(np.asarray(new.ev["code"]).tolist())
    assert len(codes) >= 2, codes  # topic messages and lock grants
    _close(En, Et)
    # capacity: chunks 0 and 1 fit, chunk 2 does not -> rolled back: the state is the one after 2 B rows
    cap = per_chunk[0] + per_chunk[1] + per_chunk[2] // 2
    En, dn, Et, dt = _pair()
    new = _new(En, dn, buf, offs, index, cap=cap)
    twin = _twin(Et, dt, buf, offs, index, None, _cuts(n), upto=2)
    assert new.rc == abi.CC_ERR_CAPACITY and new.done == 2 * B
    assert new.ev_count > cap  # (the failing chunk's events are counted, as the packed events call counts them)
    new.rc = 0
    _same(new, twin)
    assert _strings_of(dn) == _strings_of(dt)
    got, want = _readbacks(En), _readbacks(Et)
    assert str(got) == str(want)
    _close(En, Et)


def test_map_table_region_full_in_chunk_1_is_rolled_back():
    from copycat_amd.engine import Engine

    def small():  # one map in two 2,048-entry table regions (map_capacity 1,024)
        E = Engine(1, 4, 1 << 14, map_capacity=1024, flags=abi.CC_CFG_TIMERS_DEFERRED)
        E.resource_create_range(0, 1, abi.CC_RES_MAP)
        E.instance_open_range(0, 1, 0, 1000, 7)
        return E

    n = 2 * B + 9
    rng = np.random.default_rng(77)
    old = [int(k) * 7919 + 3 for k in range(1000)]
    entries = []
    for i in range(n):
        key = old[int(rng.integers(0, 1000))] if i < B or i >= 2 * B else (i - B) * 104729 + (1 << 40)
        entries.append(_entry(1000, abi.CC_OP_MAP_PUT, [("LONG", key), ("LONG", i), ("RAW8", 0)]))
    buf, offs = _segment(entries)
    index = np.arange(1, n + 1, dtype=np.uint64)
    En, Et = small(), small()
    dn, dt = _decoders(En)[0], _decoders(Et)[0]
    for events in (False, True):
        new = _new(En, dn, buf, offs, index if not events else index + np.uint64(n), events=events)
        twin = _twin(Et, dt, buf, offs, index if not events else index + np.uint64(n), None, _cuts(n), events=events, upto=1)
        assert new.rc == abi.CC_ERR_CAPACITY and new.done == B
        new.rc = 0
        _same(new, twin, events)
        # the read-back calls, as tests/test_gpu_packed_pipeline.py compares a chunk rolled back for a full region
        assert En.applied_index() == Et.applied_index()
        assert [x.tobytes() for x in En.map_table()] == [x.tobytes() for x in Et.map_table()]
    _close(En, Et)


# ---- 9. argument checks ----------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    from copycat_amd.batch import results_bound

    n = B + 7
    buf, offs = _segment(_cas_stream(n))
    index = np.arange(1, n + 1, dtype=np.uint64)
    E = _engine()
    d = _decoders(E)[0]
    before = E.snapshot()

    def aux_of(rows, columns):
        b = Batch(rows)
        b.index[:] = np.arange(1, rows + 1, dtype=np.uint64)
        return pack(b, columns=columns)

    for aux, why in ((aux_of(n - 1, ("index",)), "row count"), (aux_of(n, ("index", "time", "key")), "other than index / time"),
                     (aux_of(n, ("time",)), "lacks the index")):
        r = _new_raw(E, d, buf, offs, aux)
        assert r.rc == abi.CC_ERR_INVALID and why in r.text, (why, r.text)
    good = aux_of(n, ("index", "time"))
    shifted = _aligned_bytes(good.nbytes + 16)[8:8 + good.nbytes]
    shifted[:] = good
    assert _new_raw(E, d, buf, offs, shifted).rc == abi.CC_ERR_INVALID        # a misaligned aux blob
    assert _new_raw(E, d, buf, offs, good, res_shift=8).rc == abi.CC_ERR_INVALID  # a misaligned result blob
    r = _new_raw(E, d, buf, offs, good, res_cap=results_bound(n) - 1)
    assert r.rc == abi.CC_ERR_CAPACITY and r.size == results_bound(n)
    assert E.snapshot() == before and _strings_of(d) == []  # nothing was applied or interned
    # n == 0: header-only blobs, nothing launched
    res, evb, ev_count, done, ctl = E.apply_wire_host_packed(d, index[:0], buf=buf, offsets=offs[:1])
    assert (ev_count, done, ctl) == (0, 0, None)
    assert len(unpack_results(res)[0]) == 0 and len(unpack_events(evb)["pos"]) == 0
    assert res.nbytes == 64 and evb.nbytes == 64
    assert E.snapshot() == before
    assert _new_raw(E, d, buf, offs, good).rc == 0  # (the same arguments, well-formed, apply)
    E.close()


def _new_raw(E, d, buf, offs, aux, res_cap=None, res_shift=0):
    from copycat_amd.batch import events_bound, results_bound

    n = len(offs) - 1
    res = _aligned_bytes(results_bound(n) + 16)[res_shift:]
    evb = _aligned_bytes(events_bound(8 * n))
    seg = abi.cc_wire_segment(buf.ctypes.data, buf.size, offs.ctypes.data, n, aux.ctypes.data, aux.nbytes)
    size, ev_size, ev_count, done, bad = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    ctl = abi.cc_wire_control()
    rc = E.L.cc_apply_wire_host_packed(E.h, C.byref(d.codec), d.interner.h, C.byref(seg), res.ctypes.data,
                                       res_cap if res_cap is not None else results_bound(n), C.byref(size),
                                       evb.ctypes.data, 8 * n, evb.nbytes, C.byref(ev_size), C.byref(ev_count), None,
                                       C.byref(done), C.byref(ctl), C.byref(bad))
    return SimpleNamespace(rc=rc, text=_text(E) if rc else "", size=size.value, done=done.value)


# ---- 10. the refactor's witness: the packed-blob source after a wire call -----------------------------------------------------
def test_packed_events_call_after_a_wire_call_still_matches_its_twin():
    from copycat_amd.batch import events_bound, results_bound

    n = 2 * B + 77
    En, dn, Et, dt = _pair()
    buf, offs = _segment(_cas_stream(n))
    index = np.arange(1, n + 1, dtype=np.uint64)
    _same(_new(En, dn, buf, offs, index), _twin(Et, dt, buf, offs, index, None, _cuts(n)))
    # the same rows as host columns, packed: through cc_apply_batch_host_packed_events on the engine that just ran the
    # wire call, and through the wide host call in chunks on its twin
    bh, _, _ = _decoders(Et)[1].decode(buf=buf, offsets=offs)
    bh.index[:] = index + np.uint64(n)
    res, evb, ev_count, done = En.apply_host_packed_events(pack(bh), n, capacity=8 * n, chunk_rows=B)
    assert done == n
    status, value = unpack_results(res)
    ev = unpack_events(evb)
    ts, tv, tev = [], [], {k: [] for k in EV_KEYS}
    for lo, hi in zip(_cuts(n)[:-1], _cuts(n)[1:]):
        s, v, e = Et.apply_host_events(bh.slice(lo, hi), capacity=8 * B)
        ts.append(s), tv.append(v)
        for k in EV_KEYS:
            tev[k].append(np.asarray(e[k]).astype(np.uint64) + (lo if k == "pos" else 0))
    assert np.array_equal(status, np.concatenate(ts)) and np.array_equal(value, np.concatenate(tv))
    for k in EV_KEYS:
        assert np.array_equal(np.asarray(ev[k]).astype(np.uint64), np.concatenate(tev[k])), k
    assert ev_count == len(ev["pos"]) > 0
    assert En.snapshot() == Et.snapshot()
    _close(En, Et)
