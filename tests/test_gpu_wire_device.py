"""cc_wire_decode_to_device / cc_apply_wire_host (copycat_amd/csrc/wire_gpu.hip): the Catalyst log decoded on the GPU.

Every test compares against WireDecoder.decode (cc_wire_decode) on the same engine with a fresh interner: the device
columns, instance ids, kinds, interned Strings, and on failure the return code, message and bad row must be the host
decoder's.  T is CC_WIRE_TILE_ROWS, the entries one workgroup takes."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from copycat_amd import abi
from copycat_amd.batch import Batch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
T = abi.CC_WIRE_TILE_ROWS
COLS = ("inst", "op", "flags", "key", "a", "b", "aux")
U64 = 0xFFFFFFFFFFFFFFFF


def _engine(max_resources=256, max_instances=64, **kw):
    from copycat_amd.engine import Engine

    return Engine(max_resources, max_instances, 1 << 16, **kw)


def _kat_engine(max_resources=256, max_instances=64):
    return _engine(max_resources, max_instances, map_capacity=4096,
                   flags=abi.CC_CFG_VALUE_EVENTS | abi.CC_CFG_TIMERS_DEFERRED, max_events=1 << 16)


def _decoders(E, strings=(), codec=None):
    from copycat_amd.wire import Interner, WireDecoder

    ds = WireDecoder(E, Interner(1), codec), WireDecoder(E, Interner(1), codec)
    for d in ds:
        for s in strings:
            d.interner.intern(s)
    return ds


def _segment(entries, lead=3):
    """entries -> (buf, offsets) with offsets[0] = lead, the buffer at an odd address"""
    blob = b"".join(entries)
    raw = np.zeros(lead + len(blob) + 2, np.uint8)
    start = 1 - raw.ctypes.data % 2
    buf = raw[start:start + lead + len(blob)]
    assert buf.ctypes.data % 2 == 1
    buf[:lead] = 0xEE
    buf[lead:] = np.frombuffer(blob, np.uint8)
    offsets = np.full(len(entries) + 1, lead, np.uint64)
    offsets[1:] += np.cumsum([len(e) for e in entries], dtype=np.uint64)
    return buf, offsets


def _host_cols(db, iid):
    import torch

    out = {name: db.cols[name].view({8: torch.int64, 4: torch.int32, 1: torch.uint8}[db.cols[name].element_size()])
           .cpu().numpy().view(getattr(Batch(0), name).dtype) for name in COLS}
    out["iid"] = iid.view(torch.int64).cpu().numpy().view(np.uint64)
    return out


def _strings_of(d):
    from copycat_amd.engine import EngineError

    out = []
    while True:
        try:
            out.append(d.interner.lookup(len(out) + 1))
        except EngineError:
            return out


def _parity(E, buf, offsets, strings=(), codec=None):
    """decode on both paths; every column, iid, kind and the interners are equal -> (host batch, kind, stats)"""
    dh, dd = _decoders(E, strings, codec)
    bh, iidh, kindh = dh.decode(buf=buf, offsets=offsets)
    db, iidd, kindd, stats = dd.decode_to_device(buf=buf, offsets=offsets)
    got = _host_cols(db, iidd)
    for name in COLS:
        want = getattr(bh, name)
        bad = np.nonzero(got[name] != want)[0]
        assert bad.size == 0, (name, bad[:8], got[name][bad[:8]], want[bad[:8]])
    assert np.array_equal(got["iid"], iidh) and np.array_equal(kindd, kindh)
    assert _strings_of(dd) == _strings_of(dh)
    n = len(offsets) - 1
    assert stats["rows"] == n and stats["device_rows"] + stats["host_rows"] == n
    return bh, kindh, stats


@pytest.fixture(scope="module")
def eng():
    """an engine with 20 open instances: ids above 2^40 and ids congruent modulo the device table's size (128 cells)"""
    E = _engine()
    E.resource_create(0, abi.CC_RES_VALUE)
    ids = [5, 5 + 128, 5 + 256, 5 + 128 * 1024, (1 << 41) + 5, (1 << 41) + 133, (1 << 62) + 1, 77, 78, 79] + \
          [1000 + 7 * k for k in range(10)]
    for slot, iid in enumerate(ids):
        E.instance_open(slot, 0, iid, 1)
    E.known_ids = ids
    E.unknown_ids = [6, 6 + 128, (1 << 41) + 6, (1 << 50), 1, 2, 3, 4, 80, 81] + [1001 + 7 * k for k in range(10)]
    yield E
    E.close()


# ---- 1. fixture parity ---------------------------------------------------------------------------------------------
def test_fixture_parity(eng):
    with open(os.path.join(GOLD, "wire_fixture.json")) as f:
        meta = json.load(f)
    blob = np.fromfile(os.path.join(GOLD, "wire_fixture.bin"), np.uint8)
    offs = np.array(meta["offsets"], np.uint64)
    assert len(offs) - 1 == 63
    _, kind, stats = _parity(eng, blob, offs, strings=meta["strings"])
    handle = lambda f: (f & 7) == 4 or ((f >> 3) & 7) == 4 or (f >> 6) == 3  # noqa: E731
    want = sum(1 for r in meta["rows"] if r["kind"] != 0 or handle(r["flags"]))
    assert stats["host_rows"] == want and 0 < want < 63
    assert [int(k) for k in kind] == [r["kind"] for r in meta["rows"]]


# ---- 2. seeded random ops -------------------------------------------------------------------------------------------
STRINGS = [f"s{i}" for i in range(20)]
_RANDOM = {}


def _random_ops(eng):
    """the generator of test_wire.test_random_round_trip over the engine's known and unknown instance ids, once"""
    if not _RANDOM:
        from tests.golden.make_wire import OP, instance_op
        from tests.test_wire import _carried

        rng = np.random.default_rng(5)
        pool = eng.known_ids + eng.unknown_ids

        def val(nullable=True):
            k = rng.integers(0, 5 if nullable else 4)
            if k == 0:
                return ("LONG", int(rng.integers(-(1 << 62), 1 << 62)))
            if k == 1:
                return ("INT", int(rng.integers(-(1 << 31), 1 << 31)))
            if k == 2:
                return ("BOOL", bool(rng.integers(0, 2)))
            if k == 3:
                return ("STR", STRINGS[rng.integers(0, len(STRINGS))])
            return None

        entries, has_str = [], []
        names = sorted(OP)
        for _ in range(3 * T + 17):
            op = names[rng.integers(0, len(names))]
            grp = op.startswith("GROUP_S") or op.startswith("GROUP_E")
            kw = dict(key=val(False), a=val(), b=val(), aux=int(rng.integers(-100, 1000)),
                      member=int(rng.integers(0, 1 << 40)) if grp else None)
            e, _ = instance_op(pool[rng.integers(0, len(pool))], op, STRINGS, **kw)
            entries.append(e)
            carried = _carried(op) - ({"key"} if grp else set())
            has_str.append(any(kw[f] is not None and kw[f][0] == "STR" for f in carried if f != "aux"))
        _RANDOM["entries"], _RANDOM["has_str"] = entries, np.array(has_str)
    return _RANDOM["entries"], _RANDOM["has_str"]


@pytest.mark.parametrize("n", [1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17])
def test_random_ops(eng, n):
    entries, has_str = _random_ops(eng)
    buf, offs = _segment(entries[:n])
    bh, kind, stats = _parity(eng, buf, offs, strings=STRINGS)
    assert stats["host_rows"] == int(has_str[:n].sum())
    known = np.isin(bh.inst, np.arange(len(eng.known_ids)))
    assert ((bh.inst == eng.max_instances) | known).all()
    if n > 1000:
        assert known.sum() > n // 4 and (~known).sum() > n // 4


# ---- 3. an all-plain CAS stream, decoded and applied ----------------------------------------------------------------
def test_cas_stream_applies_as_the_host_decoded_batch():
    from tests.golden.make_wire import instance_op

    n, inst = 3 * T + 17, 1000
    rng = np.random.default_rng(11)
    entries = [instance_op(100 + int(i), "VALUE_LISTEN", [])[0] for i in rng.integers(0, inst, 8)]
    for _ in range(n - len(entries)):
        a = None if rng.integers(0, 4) == 0 else ("LONG", int(rng.integers(0, 4)))
        entries.append(instance_op(100 + int(rng.integers(0, inst)), "VALUE_CAS", [], a=a,
                                   b=("LONG", int(rng.integers(0, 4))))[0])
    buf, offs = _segment(entries)
    index = np.arange(1, n + 1, dtype=np.uint64)
    engines = []
    for _ in range(2):
        E = _kat_engine(1024, 1024)
        E.resource_create_range(0, inst, abi.CC_RES_VALUE)
        E.instance_open_range(0, inst, 0, 100, 1)
        engines.append(E)
    Ew, Eh = engines
    _, _, stats = _parity(Ew, buf, offs)
    assert stats["host_rows"] == 0 and stats["device_rows"] == n
    dh, dd = _decoders(Eh)[0], _decoders(Ew)[0]
    bh, _, _ = dh.decode(buf=buf, offsets=offs)
    bh.index[:] = index
    s0, v0, ev0 = Eh.apply_host_events(bh)
    s1, v1, ev1, applied, control = Ew.apply_wire_host(dd, index, time=np.zeros(n, np.uint64), buf=buf, offsets=offs)
    assert applied == n and control is None
    assert np.array_equal(s1, s0) and np.array_equal(v1, v0)
    assert len(ev0["pos"]) > 0
    for k in ("pos", "target", "code", "src", "tag", "payload"):
        assert np.array_equal(np.asarray(ev1[k]).astype(np.uint64), np.asarray(ev0[k]).astype(np.uint64)), k
    for E in engines:
        E.close()


# ---- 4. malformed entries -------------------------------------------------------------------------------------------
def _raw(d, buf, offs, device):
    """the C call itself -> (rc, message, bad_row, columns or None)"""
    from copycat_amd.engine import _np, lib

    n = len(offs) - 1
    bad = C.c_uint64(U64)
    if not device:
        b, iid, kind = Batch(n), np.zeros(n, np.uint64), np.zeros(n, np.uint8)
        out = abi.cc_wire_out(inst=_np(b.inst), iid=_np(iid), op=_np(b.op), flags=_np(b.flags), key=_np(b.key),
                              a=_np(b.a), b=_np(b.b), aux=_np(b.aux), kind=_np(kind))
        rc = lib().cc_wire_decode(d.engine.h, C.byref(d.codec), d.interner.h, _np(buf), buf.size, _np(offs), n,
                                  C.byref(out), C.byref(bad))
        cols = {name: getattr(b, name) for name in COLS}
        cols["iid"] = iid
    else:
        from copycat_amd.engine import EngineError

        try:
            d.decode_to_device(buf=buf, offsets=offs, check_offsets=False)  # (the C call's own check is under test)
            rc = 0
        except EngineError as e:
            rc = e.rc
        bad = C.c_uint64(d.bad_row)
        cols = _host_cols(*d.last_device)
    return rc, lib().cc_last_error().decode(errors="replace") if rc else "", bad.value, cols


def _same_failure(E, buf, offs, strings_before):
    dh, dd = _decoders(E)
    rc0, msg0, bad0, c0 = _raw(dh, buf, offs, False)
    rc1, msg1, bad1, c1 = _raw(dd, buf, offs, True)
    assert rc0 == abi.CC_ERR_INVALID and (rc1, msg1, bad1) == (rc0, msg0, bad0), (rc0, msg0, bad0, rc1, msg1, bad1)
    for name in c0:
        assert np.array_equal(c1[name][:bad0], c0[name][:bad0]), name
    assert _strings_of(dd) == _strings_of(dh) == strings_before
    return msg0, bad0


MUTATIONS = [
    (lambda e: e[:-1], "truncated"),
    (lambda e: e + b"\x00", "trailing"),
    (lambda e: e[:10] + bytes([1, 49]) + e[12:], "no resource operation"),
    (lambda e: b"\x01\x2a" + e[2:], "not an InstanceCommand"),
]


@pytest.mark.parametrize("mutate,why", MUTATIONS, ids=[w.split()[0] for _, w in MUTATIONS])
def test_malformed_entry_fails_as_the_host_decoder(eng, mutate, why):
    from tests.golden.make_wire import instance_op

    good = instance_op(5, "MAP_PUT", [], key=("LONG", 1), a=("LONG", 2), aux=5)[0]
    early = instance_op(5, "VALUE_SET", ["early"], a=("STR", "early"))[0]
    late = instance_op(5, "VALUE_SET", ["late"], a=("STR", "late"))[0]
    entries = [good] * (T + 12)
    entries[T + 2] = early
    entries[T + 5] = mutate(good)
    entries[T + 7] = late            # a String after the failing row: never interned
    entries[T + 9] = good[:-3]       # another malformed row after it: never reported
    buf, offs = _segment(entries)
    msg, bad = _same_failure(eng, buf, offs, ["early"])
    assert bad == T + 5 and f"wire row {T + 5}" in msg and why in msg


@pytest.mark.parametrize("first", ["offsets", "entry"])
def test_offsets_violation_against_a_malformed_entry(eng, first):
    from tests.golden.make_wire import instance_op

    good = instance_op(5, "MAP_PUT", [], key=("LONG", 1), a=("LONG", 2), aux=5)[0]
    entries = [good] * (T + 40)
    entries[3] = instance_op(5, "VALUE_SET", ["early"], a=("STR", "early"))[0]
    lo, hi = T + 10, T + 30
    entries[lo if first == "entry" else hi] = good[:-1]
    buf, offs = _segment(entries)
    at = hi if first == "entry" else lo  # row `at` runs backwards: offsets[at + 1] < offsets[at]
    offs = np.concatenate([offs[:at + 1], offs[at:at + 1] - 1, offs[at + 1:]])
    msg, bad = _same_failure(eng, buf, offs, ["early"])
    assert bad == lo and (("offsets decrease" in msg) if first == "offsets" else ("truncated" in msg))
    # an entry that ends past the buffer
    buf, offs = _segment([good] * (T + 3))
    msg, bad = _same_failure(eng, buf[:-1], offs, [])
    assert bad == T + 2 and "past the buffer" in msg


# ---- 5. long entries --------------------------------------------------------------------------------------------------
def test_long_entries_stream_through_the_window(eng):
    from tests.golden.make_wire import instance_op

    good = instance_op(77, "MAP_PUT", [], key=("INT", -4), a=("LONG", 2), aux=5)[0]
    big = "x" * 65535
    entries = [instance_op(78, "VALUE_CAS", [], a=("LONG", i), b=("BOOL", i & 1))[0] if i & 1 else good
               for i in range(T)]
    entries[T // 2 + 3] = instance_op(79, "VALUE_SET", [big], a=("STR", big))[0]
    assert len(entries[T // 2 + 3]) > 65535
    buf, offs = _segment(entries)
    _, _, stats = _parity(eng, buf, offs)
    assert stats["host_rows"] == 1
    # every other entry carries a 200-byte String: the tile's span is beyond any LDS window
    strs = [chr(ord("a") + k) * 200 for k in range(5)]
    entries = [instance_op(5, "MAP_PUT", strs, key=("LONG", i), a=("STR", strs[i % 5]), aux=1)[0] if i & 1 else
               instance_op(5 + 128, "MAP_GET", [], key=("LONG", i))[0] for i in range(T + 9)]
    buf, offs = _segment(entries)
    assert int(offs[T] - offs[0]) > 160 * 1024
    _, _, stats = _parity(eng, buf, offs)
    assert stats["host_rows"] == (T + 9) // 2


# ---- 6. codec -----------------------------------------------------------------------------------------------------------
def _ident(type_id, width, be):
    return bytes([width]) + (type_id & ((1 << (8 * width)) - 1)).to_bytes(width, "big" if be else "little")


def _entry(iid, op, fields, be, ids, width):
    """an InstanceCommand under a codec: fields = [("LONG" | "INT" | "BOOL" | "NULL" | "RAW8", value)]"""
    o = "big" if be else "little"
    e = _ident(30, width, be) + iid.to_bytes(8, o) + _ident(op, width, be)
    for t, v in fields:
        if t == "NULL":
            e += b"\x00"
        elif t == "LONG":
            e += _ident(ids["long"], width, be) + (v & U64).to_bytes(8, o)
        elif t == "INT":
            e += _ident(ids["int"], width, be) + (v & 0xFFFFFFFF).to_bytes(4, o)
        elif t == "BOOL":
            e += _ident(ids["bool"], width, be) + bytes([v])
        else:
            e += (v & U64).to_bytes(8, o)
    return e


@pytest.mark.parametrize("be", [0, 1], ids=["little-endian", "big-endian"])
def test_codec_parameters(eng, be):
    from copycat_amd.wire import default_codec

    c = default_codec()
    c.big_endian = be
    c.id_long, c.id_int, c.id_bool = 7, 9, 11
    ids = {"long": 7, "int": 9, "bool": 11}
    entries = []
    for width in (1, 2, 3, 4):  # identifier widths 1 to 4 for the same ids
        for iid in (5, (1 << 41) + 5, 6):
            entries += [
                _entry(iid, abi.CC_OP_VALUE_CAS, [("LONG", -(1 << 63)), ("LONG", (1 << 63) - 1)], be, ids, width),
                _entry(iid, abi.CC_OP_VALUE_CAS, [("INT", -1), ("BOOL", 2)], be, ids, width),
                _entry(iid, abi.CC_OP_VALUE_SET, [("BOOL", 0)], be, ids, width),
                _entry(iid, abi.CC_OP_MAP_REPLACEIFPRESENT, [("INT", -(1 << 31)), ("NULL", 0), ("RAW8", -7),
                                                             ("LONG", -3)], be, ids, width),
                _entry(iid, abi.CC_OP_MMAP_SIZE, [("NULL", 0)], be, ids, width),
                _entry(iid, abi.CC_OP_GROUP_SCHEDULE, [("RAW8", 1 << 40), ("RAW8", 250), ("BOOL", 1)], be, ids, width),
            ]
    buf, offs = _segment(entries)
    bh, _, stats = _parity(eng, buf, offs, codec=c)
    assert stats["host_rows"] == 0
    assert int(bh.a[0]) == 1 << 63 and int(bh.b[0]) == (1 << 63) - 1
    assert int(bh.a[1]) == U64 and int(bh.b[1]) == 1 and int(bh.flags[1]) == abi.cc_flags(abi.CC_TAG_INT, abi.CC_TAG_BOOL, 0)
    assert int(bh.key[3]) == U64 - (1 << 31) + 1 and int(bh.aux[3]) == U64 - 6
    # the default codec reads none of these as plain rows it could decode: the same failure on both paths
    _same_failure(eng, buf, offs, [])


# ---- 7. registry changes ------------------------------------------------------------------------------------------------
def test_registry_changes_reach_the_device_table():
    from tests.golden.make_wire import instance_op

    E = _engine()
    E.resource_create(0, abi.CC_RES_VALUE)
    E.resource_create(1, abi.CC_RES_VALUE)
    entries = [instance_op(i, "VALUE_GET", [])[0] for i in (900, 901, 902)]
    buf, offs = _segment(entries)

    def insts():
        bh, _, _ = _parity(E, buf, offs)
        return bh.inst.tolist()

    M = E.max_instances
    assert insts() == [M, M, M]
    E.instance_open(3, 0, 900, 11)
    E.instance_open(4, 1, 901, 12)
    assert insts() == [3, 4, M]
    E.sessions_close([11])            # the client's session closes: its instance goes
    assert insts() == [M, 4, M]
    E.resource_delete(1)              # the resource goes, and its instances with it
    assert insts() == [M, M, M]
    E.resource_create(1, abi.CC_RES_VALUE)
    E.instance_open(5, 1, 902, 13)
    assert insts() == [M, M, 5]
    snap = E.snapshot()
    E.instance_open(6, 0, 900, 14)
    E.sessions_close([13])
    assert insts() == [6, M, M]
    E.restore(snap)
    assert insts() == [M, M, 5]
    E.close()


# ---- 8. control rows ------------------------------------------------------------------------------------------------------
def test_control_row_stops_the_apply_and_the_stream_resumes():
    from tests.golden.make_wire import instance_op, manager_op

    n = T + 40
    base = 10
    index = np.arange(base, base + n, dtype=np.uint64)
    new_iid = base + T + 1  # the instance GetResource creates is named by its commit index
    strings = ["r0", "r1"]
    entries = []
    for i in range(n):
        if i == T + 1:
            entries.append(manager_op(35, strings, key="r1", rtype="VALUE")[0])
        elif i < T + 1:
            entries.append(instance_op(1, "VALUE_SET" if i % 3 else "VALUE_GET", [], a=("LONG", i))[0])
        else:
            entries.append(instance_op(new_iid, "VALUE_GETANDSET", [], a=("LONG", i))[0])
    buf, offs = _segment(entries)
    Ew, Eh = _kat_engine(), _kat_engine()
    dw, dh = _decoders(Ew)[0], _decoders(Eh)[0]
    for E, d in ((Ew, dw), (Eh, dh)):
        st, iid, _ = E.get_resource(d.interner.intern("r0"), abi.CC_RES_VALUE, 7, 1)
        assert abi.status_code(st) == abi.CC_ST_OK and iid == 1
    # the host-decoded reference: decode and apply up to the control row, run it, go on
    bh, _, kind = dh.decode(buf=buf, offsets=offs)
    bh.index[:] = index
    r = int(np.nonzero(kind)[0][0])
    assert r == T + 1 and int(kind[r]) == 35
    s0, v0, _ = Eh.apply_host_events(bh.slice(0, r))
    st, iid, _ = Eh.get_resource(int(bh.key[r]), int(bh.a[r]), 7, int(index[r]))
    assert abi.status_code(st) == abi.CC_ST_OK and iid == new_iid
    bh2, _, _ = dh.decode(buf=buf, offsets=offs[r + 1:])
    bh2.index[:] = index[r + 1:]
    s2, v2, _ = Eh.apply_host_events(bh2)
    # the wire path
    s1, v1, _, applied, ctl = Ew.apply_wire_host(dw, index, buf=buf, offsets=offs)
    assert applied == T + 1
    assert ctl == {"row": T + 1, "kind": 35, "key": int(bh.key[r]), "a": abi.CC_RES_VALUE, "b": 0}
    assert dw.interner.lookup(ctl["key"]) == "r1"
    assert np.array_equal(s1, s0) and np.array_equal(v1, v0)
    st, iid, islot = Ew.get_resource(ctl["key"], ctl["a"], 7, int(index[applied]))
    assert abi.status_code(st) == abi.CC_ST_OK and iid == new_iid
    s3, v3, _, applied2, ctl2 = Ew.apply_wire_host(dw, index[applied + 1:], buf=buf, offsets=offs[applied + 1:])
    assert applied2 == n - T - 2 and ctl2 is None
    assert np.array_equal(s3, s2) and np.array_equal(v3, v2)
    assert (np.array([abi.status_code(int(x)) for x in s3]) == abi.CC_ST_OK).all()  # the new instance resolved
    assert int(v3[-1]) == n - 2  # getAndSet returns the value the row before it set
    # more control rows than the caller's list holds
    from copycat_amd.engine import EngineError

    two = [entries[0], manager_op(38, strings, key="r0")[0], entries[1], manager_op(37, strings, resource=9)[0]]
    d = _decoders(Ew)[0]
    with pytest.raises(EngineError) as ei:
        d.decode_to_device(entries=two, ctl_cap=1)
    assert ei.value.rc == abi.CC_ERR_CAPACITY and d.ctl_count == 2
    _, _, kind, _ = d.decode_to_device(entries=two, ctl_cap=2)
    assert kind.tolist() == [0, 38, 0, 37]
    Ew.close()
    Eh.close()


# ---- 9. the reference-pinned KATs through the device decoder ------------------------------------------------------------------
from tests.test_gpu_wire import KATS, WireBackend  # noqa: E402


class DeviceWireBackend(WireBackend):
    """WireBackend whose decoder is decode_to_device, its columns downloaded"""

    def __init__(self, kat):
        super().__init__(kat)
        from copycat_amd.wire import WireDecoder

        class DeviceDecoder(WireDecoder):
            def decode(self, entries=None, buf=None, offsets=None):
                db, iid, kind, stats = self.decode_to_device(entries=entries, buf=buf, offsets=offsets)
                cols = _host_cols(db, iid)
                b = Batch(db.n)
                for name in COLS:
                    getattr(b, name)[:] = cols[name]
                return b, cols["iid"], kind

        self.D = DeviceDecoder(self.E, self.D.interner)


@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_kat_through_device_decoder(kat):
    from tests.kat_runner import KatRun

    B = DeviceWireBackend(kat)
    KatRun(kat, B).run()
