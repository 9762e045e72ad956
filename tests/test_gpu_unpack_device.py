"""cc_respack_to_device / cc_evpack_to_device on the MI355X: the decoder kernels (unpack_res.hip) against the host
decoders cc_respack_unpack / cc_evpack_unpack.

Bar: bit-exact.  Every decoded column equals the host decoder's byte for byte with the rows around it untouched, the
device count word reads n, and a blob the validator refuses (or an event stream too small) leaves the sentinel-filled
outputs as they were: nothing was launched.  Blobs come from the host encoders and, for the table sizes no encoder
takes (1 entry, 4,096 entries), from a block written by hand that the validator accepts."""
import numpy as np
import pytest

from copycat_amd import abi
from copycat_amd.batch import (events_check, pack_events, pack_results, results_check, unpack_events, unpack_results)
from tests import evpack_cases as ec
from tests import respack_cases as rc

pytestmark = pytest.mark.gpu

B = rc.B
FOR, BY_POS = ec.FOR, ec.BY_POS
GUARD = 64  # sentinel rows before and after every output column (a multiple of 16: the columns stay 16-byte aligned)
FILL = 0xCD
COUNT_FILL = 0x7777
SIZES = (1, 15, 16, 17, 255, 256, 257, B - 1, B, B + 1, 2 * B + 33, 256 * B + 1)
ESZ = {"pos": 4, "target": 4, "code": 1, "src": 1, "tag": 1, "payload": 8}
NPDT = {"pos": np.uint32, "target": np.uint32, "code": np.uint8, "src": np.uint8, "tag": np.uint8, "payload": np.uint64}


@pytest.fixture(scope="module")
def small_engine():
    from copycat_amd.engine import Engine

    E = Engine(16, 16, 4096)
    yield E
    E.close()


class Guarded:
    """a device column of n rows of esz bytes between GUARD sentinel rows on each side"""

    def __init__(self, n, esz):
        import torch

        self.n, self.esz = n, esz
        self.buf = torch.full(((n + 2 * GUARD) * esz,), FILL, dtype=torch.uint8, device="cuda")
        self.rows = self.buf[GUARD * esz:(GUARD + n) * esz]
        assert self.rows.data_ptr() % 16 == 0 or n == 0

    def check(self, want, what):
        got = self.buf.cpu().numpy()
        lo, hi = GUARD * self.esz, (GUARD + self.n) * self.esz
        assert (got[:lo] == FILL).all(), f"{what}: rows before the column were written"
        assert (got[hi:] == FILL).all(), f"{what}: rows after the column were written"
        if want is None:
            assert (got[lo:hi] == FILL).all(), f"{what}: the column was written"
            return
        bad = np.nonzero(got[lo:hi] != np.ascontiguousarray(want).view(np.uint8))[0]
        assert len(bad) == 0, f"{what}: differs from the host decoder first at row {bad[0] // self.esz}"


# ---- results -------------------------------------------------------------------------------------------------------------
def _results_to_device(E, blob, n, stream=None):
    import torch

    s, v = Guarded(n, 1), Guarded(n, 8)
    torch.cuda.synchronize()
    E.results_to_device(blob, s.rows, v.rows, stream=stream)
    torch.cuda.synchronize()
    return s, v


def _decode_results(E, status, value, name, stream=None):
    blob = pack_results(status, value)
    ref_s, ref_v = unpack_results(blob)
    assert ref_s.tobytes() == status.tobytes() and ref_v.tobytes() == value.tobytes()
    s, v = _results_to_device(E, blob, len(status), stream)
    s.check(ref_s, f"{name}: status"), v.check(ref_v, f"{name}: value")


def test_result_width_cases(small_engine):
    """Fails without the feature: cc_respack_to_device does not exist."""
    for name, status, value, _, _ in rc.width_cases():
        _decode_results(small_engine, status, value, name)
    status, value, _ = rc.width_rows()  # ... and one per block of one blob
    _decode_results(small_engine, status, value, "width_rows")


@pytest.mark.parametrize("n", SIZES)
def test_random_results(small_engine, n):
    status, value = rc.random_results(n, seed=n)
    _decode_results(small_engine, status, value, f"random/{n}")


def test_prefilled_rows(small_engine):
    """rows no kernel wrote keep the callers' prefill (status 0xFF, value 0 or 0xA5 bytes) through the blob"""
    n = 3 * B + 100
    status, value = rc.random_results(n, seed=5)
    for lo, hi, fill in ((100, 300, 0), (B - 7, B + 9, 0xA5A5A5A5A5A5A5A5), (2 * B, 3 * B, 0xA5A5A5A5A5A5A5A5), (n - 3, n, 0)):
        status[lo:hi], value[lo:hi] = 0xFF, fill
    _decode_results(small_engine, status, value, "prefill")


def test_results_on_a_stream_of_the_caller_s(small_engine):
    import torch

    status, value = rc.random_results(5 * B + 3, seed=9)
    _decode_results(small_engine, status, value, "stream", stream=torch.cuda.Stream())


# ---- events --------------------------------------------------------------------------------------------------------------
def _events_to_device(E, blob, n, capacity=None, stream=None, rc_want=abi.CC_OK):
    import torch

    from copycat_amd.engine import EngineError

    cols = {k: Guarded(n, ESZ[k]) for k in ec.NAMES}
    count = torch.full((1,), COUNT_FILL, dtype=torch.int64, device="cuda")

    class Stream_:  # what Engine.events_to_device takes: struct()
        def struct(self):
            return abi.cc_events(*[cols[k].rows.data_ptr() for k in ec.NAMES], n if capacity is None else capacity,
                                 count.data_ptr())

    torch.cuda.synchronize()
    if rc_want == abi.CC_OK:
        E.events_to_device(blob, Stream_(), stream=stream)
    else:
        with pytest.raises(EngineError) as e:
            E.events_to_device(blob, Stream_(), stream=stream)
        assert e.value.rc == rc_want, e.value
    torch.cuda.synchronize()
    return cols, int(count.item())


def _decode_blob(E, blob, name, stream=None):
    """a blob the validator accepts: the device columns equal the host decoder's, the count word its n"""
    n = events_check(blob)
    ref = unpack_events(blob)
    cols, count = _events_to_device(E, blob, n, stream=stream)
    for k in ec.NAMES:
        cols[k].check(ref[k], f"{name}: {k}")
    assert count == n, f"{name}: the device count word"
    return ref


def _decode_events(E, ev, name, stream=None):
    ref = _decode_blob(E, pack_events(ev), name, stream)
    assert ec.same(ref, ev)


def test_event_case_blocks(small_engine):
    """Fails without the feature: cc_evpack_to_device does not exist."""
    for i, ev in enumerate(ec.all_case_blocks()):
        _decode_events(small_engine, ev, f"cases/{i}")
    for name, ev, _ in ec.width_cases():
        _decode_events(small_engine, ev, name)


def test_by_pos_cases_and_near_misses(small_engine):
    from copycat_amd.batch import events_info

    for name, ev, (mode, width, base, entries) in ec.by_pos_cases():  # tables, and blocks that just miss one and stay FOR
        blob = pack_events(ev)
        assert events_info(blob)["columns"]["payload"]["blocks"][0][:2] == (mode, width), name
        _decode_blob(small_engine, blob, name)
    # a fan-out in the tail block, behind full blocks of other shapes
    ev = ec.concat([ec.random_events(2 * B, seed=1), ec.fanout(37, 9, seed=2)])
    _decode_events(small_engine, ev, "fanout_tail")


def test_fanouts_closed_sessions_and_a_tail_of_one(small_engine):
    _decode_events(small_engine, ec.fanout(64, 64), "fanout")
    _decode_events(small_engine, ec.fanout(4096, 1, target_span=100), "fanout_1")       # E == rows: stays FOR
    _decode_events(small_engine, ec.fanout(2, 2048, first_row=0xFFFF0000), "fanout_2")   # two table entries
    _decode_events(small_engine, ec.fanout(300, 40, step=200), "fanout_3_blocks")        # pos width 2 in every block
    _decode_events(small_engine, ec.fanout(20, 100, step=5000), "fanout_pos_4")          # rows far apart: pos width 4 blocks
    _decode_events(small_engine, ec.fanout(1000, 4, step=2), "fanout_pos_2")             # tables under a 2-byte pos column
    _decode_events(small_engine, ec.closed_sessions(), "closed_sessions")
    _decode_events(small_engine, ec.closed_sessions(B + 1), "closed_sessions_tail_1")
    _decode_events(small_engine, ec.concat([ec.fanout(64, 64), ec.events(np.array([9000], np.uint32), payload=5)]), "tail_of_1")


@pytest.mark.parametrize("n", SIZES)
def test_random_events(small_engine, n):
    _decode_events(small_engine, ec.random_events(n, seed=n), f"random/{n}")


def _hand_block(m, pos_w, pos_off, table_w, table, base=1000, pos_base=77):
    """One block of m events written by hand: pos at width pos_w (offsets pos_off), target / code / src / tag constant,
    the payload a CC_PK_BY_POS table of len(table) entries of table_w bytes.  The validator decides whether it is a blob."""
    def narrow(v, w):
        raw = np.asarray(v, np.uint64).astype({1: "<u1", 2: "<u2", 4: "<u4", 8: "<u8"}[w]).tobytes() if w else b""
        return raw + bytes(ec.r16(len(raw)) - len(raw))

    area, cols = b"", b""
    for mode, w, base_, entries, raw in ((FOR, pos_w, pos_base, 0, narrow(pos_off, pos_w)), (FOR, 0, 9, 0, b""),
                                         (FOR, 0, 3, 0, b""), (FOR, 0, 1, 0, b""), (FOR, 0, 2, 0, b""),
                                         (BY_POS, table_w, base, len(table), narrow(table, table_w))):
        cols += bytes([mode, w]) + entries.to_bytes(2, "little") + len(area).to_bytes(4, "little") + base_.to_bytes(8, "little")
        area += raw
    at = ec.HEADER + ec.ENTRY
    entry = m.to_bytes(4, "little") + len(area).to_bytes(4, "little") + at.to_bytes(8, "little") + cols
    header = (abi.CC_EVPACK_MAGIC.to_bytes(4, "little") + (1).to_bytes(4, "little") + m.to_bytes(8, "little")
              + (1).to_bytes(8, "little") + (at + len(area)).to_bytes(8, "little") + (0x3F).to_bytes(4, "little")
              + B.to_bytes(4, "little") + bytes(24))
    from copycat_amd.batch import _aligned_bytes

    raw = header + entry + area
    blob = _aligned_bytes(len(raw))
    blob[:] = np.frombuffer(raw, np.uint8)
    return blob


def test_tables_of_1_and_4096_entries_and_every_pos_width(small_engine):
    """The table sizes at the validator's ends, which no encoder takes (a table is taken only when it is smaller than
    the rows): 1 entry under a pos column of width 0, 4,096 entries of 8 bytes (the 32 KiB image, full) under a pos
    column of width 2 whose offsets are in no order."""
    rng = np.random.default_rng(3)
    blob = _hand_block(B, 0, [], 1, [5])
    ref = _decode_blob(small_engine, blob, "table_of_1")
    assert (ref["payload"] == 1005).all() and (ref["pos"] == 77).all()
    blob = _hand_block(1003, 0, [], 8, [1 << 60], base=(-7) & ec.M64)  # (base + entry wraps modulo 2^64)
    assert (_decode_blob(small_engine, blob, "table_of_1_wide")["payload"] == (1 << 60) - 7).all()
    table = rng.integers(0, ec.M64, B, dtype=np.uint64, endpoint=True)
    for m in (B, B - 1, 1):
        off = rng.permutation(B)[:m]
        if m == B:
            off[-1] = B - 1  # (the last row looks up the table's last entry)
        ref = _decode_blob(small_engine, _hand_block(m, 2, off, 8, table), f"table_of_4096/{m}")
        assert np.array_equal(ref["payload"], np.uint64(1000) + table[off])
    for pos_w, entries in ((1, 256), (1, 7), (2, 4096), (2, 300)):  # pos widths 1 and 2 at every table width
        for table_w in (1, 2, 4, 8):
            t = rng.integers(0, (1 << (8 * table_w)) - 1, entries, dtype=np.uint64, endpoint=True)
            off = rng.integers(0, entries, 1003)
            off[0], off[-1] = entries - 1, 0
            ref = _decode_blob(small_engine, _hand_block(1003, pos_w, off, table_w, t), f"pos_{pos_w}/table_{table_w}x{entries}")
            assert np.array_equal(ref["payload"], np.uint64(1000) + t[off]) and np.array_equal(ref["pos"], (77 + off).astype(np.uint32))


def test_events_on_a_stream_of_the_caller_s(small_engine):
    import torch

    _decode_events(small_engine, ec.random_events(5 * B + 3, seed=9), "stream", stream=torch.cuda.Stream())


# ---- the count word and the capacity -------------------------------------------------------------------------------------
def test_capacity_one_short_and_a_header_only_blob(small_engine):
    ev = ec.random_events(B + 100, seed=3)
    n = B + 100
    blob = pack_events(ev)
    cols, count = _events_to_device(small_engine, blob, n, capacity=n - 1, rc_want=abi.CC_ERR_CAPACITY)
    for k in ec.NAMES:
        cols[k].check(None, f"capacity n - 1: {k}")
    assert count == COUNT_FILL
    cols, count = _events_to_device(small_engine, blob, n, capacity=n + 1000)  # a stream larger than the blob
    for k in ec.NAMES:
        cols[k].check(ev[k], f"capacity n + 1000: {k}")
    assert count == n
    empty = pack_events(ec.take(ev, 0, 0))
    assert len(empty) == 64
    cols, count = _events_to_device(small_engine, empty, 50)  # room for 50 events, none in the blob
    for k in ec.NAMES:
        cols[k].check(None, f"header only: {k}")
    assert count == 0
    s, v = _results_to_device(small_engine, pack_results(np.zeros(0, np.uint8), np.zeros(0, np.uint64)), 50)
    s.check(None, "header only: status"), v.check(None, "header only: value")


# ---- malformed blobs never reach the GPU ---------------------------------------------------------------------------------
H, RE, EE = 64, 48, 112  # header, a result entry, an event entry
COL = 16                 # the first cc_pack_col of an entry; {mode, width, reserved16 (2), offset (4), base (8)} each


def _corrupt(blob, at, value):
    bad = blob.copy()
    assert bad[at] != value
    bad[at] = value
    return bad


def _result_corruptions():
    """(blob, status, value, {what: (byte, value)}): one corrupted byte of each kind cc_respack_check names"""
    status, value = rc.random_results(2 * B + 9, seed=2)
    status[:] = np.arange(len(status)) % 5  # (both columns hold bytes in every block)
    value[:] = np.arange(len(value), dtype=np.uint64) * np.uint64(1000003)
    blob = pack_results(status, value)
    e1 = H + RE  # block 1's entry
    return blob, status, value, {
        "magic": (0, blob[0] ^ 1), "version": (4, 2), "n": (8, blob[8] ^ 1), "blocks": (16, 4), "total bytes": (24, blob[24] ^ 0x80),
        "present": (32, 1), "block_rows": (37, 0x20),
        "a block's rows": (e1, blob[e1] ^ 1), "a block's bytes": (e1 + 4, blob[e1 + 4] ^ 8), "a block's offset": (e1 + 8, blob[e1 + 8] ^ 4),
        "a block's offset into the directory": (H + 8, 0x20),
        "status mode": (e1 + COL, 1), "status width": (e1 + COL + 1, 2), "value mode": (e1 + 2 * COL, abi.CC_PK_BY_POS),
        "value width 3": (e1 + 2 * COL + 1, 3), "value offset misaligned": (e1 + 2 * COL + 4, blob[e1 + 2 * COL + 4] ^ 8),
        "value offset outside": (e1 + 2 * COL + 7, 0x40), "value rows over status rows": (e1 + 2 * COL + 5, 0),
    }


def test_malformed_result_blobs(small_engine):
    import torch

    from copycat_amd.engine import EngineError

    blob, status, value, cases = _result_corruptions()
    n = len(status)
    for name, (at, v) in cases.items():
        bad = _corrupt(blob, at, v)
        with pytest.raises(EngineError) as e:
            results_check(bad)
        assert e.value.rc == abi.CC_ERR_INVALID, name
        s, va = Guarded(n, 1), Guarded(n, 8)
        with pytest.raises(EngineError) as e:
            small_engine.results_to_device(bad, s.rows, va.rows)
        assert e.value.rc == abi.CC_ERR_INVALID and "result blob" in str(e.value), name
        torch.cuda.synchronize()
        s.check(None, name), va.check(None, name)
    _decode_results(small_engine, status, value, "and the engine is as good as new")


def _event_corruptions():
    """(blob, events, {what: (byte, value)}): one corrupted byte of each kind cc_evpack_check names"""
    ev = ec.concat([ec.random_events(B, seed=4), ec.fanout(64, 64, seed=3), ec.fanout(30, 10, seed=5)])
    ev["code"][:] = np.arange(len(ev["code"])) % 3  # (every byte column holds bytes)
    blob = pack_events(ev)
    e1 = H + EE  # block 1: the fan-out, payload BY_POS under a pos column one byte wide
    pay = e1 + COL + 5 * COL
    hd = abi.cc_evpack_block.from_buffer_copy(blob[e1:e1 + EE].tobytes())
    assert hd.col[5].mode == BY_POS and hd.col[0].width == 1 and hd.col[5].reserved16 == 64
    pos_area = hd.offset + hd.col[0].offset
    return blob, ev, {
        "magic": (0, blob[0] ^ 1), "version": (4, 2), "n": (8, blob[8] ^ 1), "blocks": (16, 9), "total bytes": (24, blob[24] ^ 0x80),
        "present": (32, 0x1F), "block_rows": (37, 0x20),
        "a block's rows": (e1, blob[e1] ^ 1), "a block's bytes": (e1 + 4, blob[e1 + 4] ^ 8), "a block's offset": (e1 + 8, blob[e1 + 8] ^ 4),
        "pos mode": (e1 + COL, BY_POS), "target mode": (e1 + 2 * COL, 7), "code width": (e1 + 3 * COL + 1, 2),
        "target width 3": (e1 + 2 * COL + 1, 3), "src offset misaligned": (e1 + 4 * COL + 4, blob[e1 + 4 * COL + 4] ^ 4),
        "payload offset outside": (pay + 7, 0x40), "payload mode": (pay, abi.CC_PK_REL_A),
        "table of no entry": (pay + 2, 0), "table of more than 4096": (pay + 3, 0x20), "table under a wide pos": (e1 + COL + 1, 4),
        "a pos offset outside its table": (pos_area + 100, 64),
    }


def test_malformed_event_blobs(small_engine):
    from copycat_amd.engine import EngineError

    blob, ev, cases = _event_corruptions()
    n = len(ev["pos"])
    for name, (at, v) in cases.items():
        bad = _corrupt(blob, at, v)
        with pytest.raises(EngineError):
            events_check(bad)
        cols, count = _events_to_device(small_engine, bad, n, rc_want=abi.CC_ERR_INVALID)
        for k in ec.NAMES:
            cols[k].check(None, f"{name}: {k}")
        assert count == COUNT_FILL, name
    _decode_events(small_engine, ev, "and the engine is as good as new")


# ---- round trips ---------------------------------------------------------------------------------------------------------
def test_round_trips_through_the_device_encoders(small_engine):
    """cc_respack_from_device -> cc_respack_to_device and cc_evpack_from_device -> cc_evpack_to_device -> ... again"""
    import torch

    from copycat_amd.engine import DeviceEvents

    n = 3 * B + 77
    status, value = rc.random_results(n, seed=6)
    s0 = torch.from_numpy(status).cuda()
    v0 = torch.from_numpy(value.view(np.int64)).cuda()
    blob = small_engine.results_to_host_packed(s0, v0)
    s1, v1 = torch.zeros_like(s0), torch.zeros_like(v0)
    small_engine.results_to_device(blob, s1, v1)
    torch.cuda.synchronize()
    assert torch.equal(s0, s1) and torch.equal(v0, v1)
    assert np.array_equal(small_engine.results_to_host_packed(s1, v1), blob)

    ev = ec.concat([ec.random_events(2 * B, seed=8), ec.fanout(64, 64, seed=9), ec.fanout(5, 7, seed=10)])
    m = len(ev["pos"])
    d = DeviceEvents(m + 50)  # a stream with room to spare: the count word says how many rows hold events
    small_engine.events_to_device(pack_events(ev), d)
    torch.cuda.synchronize()
    assert ec.same(d.host(), ev) and d.host()["count"] == m
    blob, count = small_engine.events_to_host_packed(d)  # the decoded stream is a cc_events the encoder takes as it stands
    assert count == m and np.array_equal(blob, pack_events(ev))
    d2 = DeviceEvents(m)
    small_engine.events_to_device(blob, d2)
    torch.cuda.synchronize()
    assert ec.same(d2.host(), ev)
