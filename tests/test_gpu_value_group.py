"""GPU parity of a value-only call applied by group (apply_batch.hip apply_group, value_group.h): one k_part_v4 launch
over the whole group, then one k_apply_value_v3 and one k_unpermute_v3 launch per segment of it, each on its slice of
the group's staging arrays.

Bar: bit-exact per-commit status / value, value_state and applied index against the CPU oracle (integer path, no
tolerance), and bit-exact results against a second engine created with CC_VALUE_GROUP_TILES=0, which partitions and
unpermutes per sub-batch as before.  Every call also checks the launch counts cc_profile reports, so a case cannot
pass by quietly taking the other path.

Geometry (value_path.hip): every engine here has sub_batch = 16384, so a segment is two 8192-commit tiles; 512
resources are two super-buckets (resource r is slot r & 255 of super-bucket r >> 8); a super-bucket's list within a
segment is its rows of that segment in log order, walked in 3072-record chunks (nch = ceil(records / 3072)), chunk c
in LDS buffer c & 1."""
import contextlib
import os

import numpy as np
import pytest

from copycat_amd import abi
from tests.test_gpu_value_apply import _batch, _escapes, _mixed_ops

pytestmark = pytest.mark.gpu

SUB, TILE, CHUNK, SLOTS, R = 16384, 8192, 3072, 256, 512
L, N = abi.CC_TAG_LONG, abi.CC_TAG_NULL
GET, SET, CAS, GAS, DEL = (abi.CC_OP_VALUE_GET, abi.CC_OP_VALUE_SET, abi.CC_OP_VALUE_CAS, abi.CC_OP_VALUE_GETANDSET,
                           abi.CC_OP_DELETE)
UNKNOWN = abi.CC_ST_UNKNOWN_SESSION | (N << 4)


@contextlib.contextmanager
def _knob(value):
    old = os.environ.pop("CC_VALUE_GROUP_TILES", None)
    if value is not None:
        os.environ["CC_VALUE_GROUP_TILES"] = value
    try:
        yield
    finally:
        os.environ.pop("CC_VALUE_GROUP_TILES", None)
        if old is not None:
            os.environ["CC_VALUE_GROUP_TILES"] = old


def _launches(n, group_segs):
    """(partition launches, apply launches = unpermute launches) of a call of n rows: one partition per group of
    group_segs segments at most; a rest of one segment or less goes the per-sub-batch way (0: everything does)."""
    part, left = 0, n
    while left > 0:
        take = min(left, group_segs * SUB) if group_segs and left > SUB else min(left, SUB)
        part, left = part + 1, left - take
    return part, -(-n // SUB)


class _Trio:
    """An engine that applies by group, one that applies per sub-batch, and the oracle, with the same registry."""

    def __init__(self, max_batch, knob=None, max_inst=R):
        from copycat_amd.engine import Engine
        from oracle.oracle_py import Oracle

        self.group_segs = 1 << 40 if knob is None else max(int(knob) // (SUB // TILE), 1)
        with _knob(knob):
            self.E = Engine(R, max_inst, max_batch, sub_batch=SUB, map_capacity=0)
        with _knob("0"):
            self.E0 = Engine(R, max_inst, max_batch, sub_batch=SUB, map_capacity=0)
        self.O = Oracle(R, max_inst)
        for e in (self.E, self.E0):
            e.resource_create_range(0, R, abi.CC_RES_VALUE)
            e.instance_open_range(0, R, 0, 1000, 7)
        for r in range(R):
            self.O.resource_create(r, abi.CC_RES_VALUE)
            self.O.instance_open(r, r, 1000 + r, 7)

    def check(self, got, got0, part):
        (gs, gv), (s0, v0) = got, got0
        os_, ov = self.O.apply(part)
        bad = np.nonzero((gs != os_) | (gv != ov))[0]
        assert len(bad) == 0, (f"{len(bad)} rows differ from the oracle; first {bad[:5]}: gpu {gs[bad[:5]]},{gv[bad[:5]]} "
                               f"oracle {os_[bad[:5]]},{ov[bad[:5]]}")
        assert np.array_equal(gs, s0) and np.array_equal(gv, v0), "by group and per sub-batch differ"
        for x, y, z in zip(self.E.value_state(0, R), self.O.value_state(0, R), self.E0.value_state(0, R)):
            assert np.array_equal(x, y) and np.array_equal(z, y)
        assert self.E.applied_index() == self.O.applied_index() == self.E0.applied_index()

    def apply(self, part):
        """One call on both engines through the host entry point, checked; returns the grouped engine's results."""
        n = len(part)
        out = []
        for e, segs in ((self.E, self.group_segs), (self.E0, 0)):
            e.profile(True)
            before = e.counters()[2]
            out.append(e.apply_host(part))
            pr = e.profile_read()
            want = _launches(n, segs)
            seen = (pr["k_part_tile"][1], pr["k_apply_value"][1], pr["k_unpermute"][1])
            assert seen == (want[0], want[1], want[1]), (n, segs, seen)
            assert e.counters()[2] - before == -(-n // SUB)  # (the sub-batch counter counts segments on both)
            e.profile(False)
        self.check(out[0], out[1], part)
        return out[0]


def _per_segment(b, n_seg):
    """records of each super-bucket in each segment, from the inst column: [segment][super-bucket]"""
    seg = np.arange(len(b)) // SUB
    ok = b.inst < R
    return [[int(np.sum(ok & (seg == k) & (b.inst >> 8 == s))) for s in range(2)] for k in range(n_seg)]


@pytest.mark.parametrize("n", [16384, 16385, 32768, 32769, 5 * 16384 + 4097])
def test_segment_edges(n):
    """Exactly one segment (the per-sub-batch launches, nothing staged by group), a second segment of one row, two
    whole segments, a third of one row, and six segments whose last is one partial tile of 4097 rows with odd n (the
    unpermute's straddling pair is the group's last row).  Mixed ops over both super-buckets in every segment."""
    rng = np.random.default_rng(n)
    b = _mixed_ops(rng, rng.integers(0, R, n).astype(np.uint32))
    n_seg = -(-n // SUB)
    assert n_seg == {16384: 1, 16385: 2, 32768: 2, 32769: 3, 86017: 6}[n]
    per = _per_segment(b, n_seg)
    assert all(sum(p) == min(SUB, n - k * SUB) for k, p in enumerate(per))
    assert all(p[0] > 0 and p[1] > 0 for p in per[:n // SUB])  # every whole segment feeds both super-buckets
    if n == 86017:
        assert n % 2 == 1 and n - 5 * SUB == 4097 < TILE
    _Trio(n).apply(b)


def test_chunk_counts_and_buffer_parity_per_segment():
    """Super-bucket 0's records per segment are 1, 3073, 0, 3072, 6144, 6145, 9217: nch = 1, 2, 0, 1, 2, 3, 4.  An odd
    nch (1, then 3: the last chunk's results leave LDS buffer 0) and an even one (2 before the 6145-record segment: they
    leave buffer 1) each precede a segment with records; the empty segment sits between two that have some.
    Super-bucket 1 takes the other rows of every segment (16383 .. 7167 records: nch 6 .. 3)."""
    counts = [1, 3073, 0, 3072, 6144, 6145, 9217]
    n = len(counts) * SUB
    rng = np.random.default_rng(42)
    inst = (SLOTS + rng.integers(0, SLOTS, n)).astype(np.uint32)
    for k, c in enumerate(counts):
        rows = k * SUB + rng.choice(SUB, c, replace=False)
        inst[rows] = rng.integers(0, SLOTS, c)
    b = _mixed_ops(rng, inst)
    per = _per_segment(b, len(counts))
    assert [p[0] for p in per] == counts and [p[1] for p in per] == [SUB - c for c in counts]
    nch = [-(-c // CHUNK) for c in counts]
    assert nch == [1, 2, 0, 1, 2, 3, 4]
    nxt = list(zip(nch, counts[1:]))
    assert any(a % 2 == 1 and c > 0 for a, c in nxt) and any(a and a % 2 == 0 and c > 0 for a, c in nxt)
    assert counts[2] == 0 and counts[1] > 0 and counts[3] > 0
    assert sorted(-(-(SUB - c) // CHUNK) for c in counts) == [3, 4, 4, 5, 5, 6, 6]
    _Trio(n).apply(b)


def _quiet(rng, n, keep_out):
    """Mixed ops over every slot but `keep_out`, values 0..3: background that leaves those slots alone."""
    free = np.setdiff1d(np.arange(R), np.asarray(keep_out))
    return _mixed_ops(rng, free[rng.integers(0, len(free), n)].astype(np.uint32))


def _plant(b, row, inst, op, flags, a=0, bb=0):
    b.inst[row], b.op[row], b.flags[row] = inst, op, flags
    b.a[row], b.b[row] = np.uint64(a % (1 << 64)), np.uint64(bb % (1 << 64))


def _plant_boundary_story(b, k, x, y, z, zget_off=TILE):
    """Slot x: set 41 in segment k, CAS 41 -> 42 in k+1 (succeeds), CAS 41 -> 43 in k+2 (stale: fails).  Slot y:
    getAndSet 51, 52, 53 in k, k+1, k+2.  Slot z: set 61 in k, delete in k+1, get in k+2.  Returns the rows (two
    stories one segment apart share no row)."""
    at = lambda seg, off: seg * SUB + off
    rows = {"set": at(k, SUB - 1), "cas_ok": at(k + 1, 0), "cas_stale": at(k + 2, 3),
            "gas": [at(k, 100), at(k + 1, TILE + 7), at(k + 2, 1)],
            "zset": at(k, 5), "zdel": at(k + 1, SUB - 2), "zget": at(k + 2, zget_off)}
    assert len({rows[q] for q in ("set", "cas_ok", "cas_stale", "zset", "zdel", "zget")} | set(rows["gas"])) == 9
    _plant(b, rows["set"], x, SET, L, 41)
    _plant(b, rows["cas_ok"], x, CAS, L | (L << 3), 41, 42)
    _plant(b, rows["cas_stale"], x, CAS, L | (L << 3), 41, 43)
    for q, row in enumerate(rows["gas"]):
        _plant(b, row, y, GAS, L, 51 + q)
    _plant(b, rows["zset"], z, SET, L, 61)
    _plant(b, rows["zdel"], z, DEL, 0)
    _plant(b, rows["zget"], z, GET, 0)
    return rows


def _story_rows(rows):
    return {rows[q] for q in ("set", "cas_ok", "cas_stale", "zset", "zdel", "zget")} | set(rows["gas"])


def _check_boundary_story(rows, gs, gv, first_gas):
    assert gv[rows["cas_ok"]] == 1 and gv[rows["cas_stale"]] == 0
    assert [int(gv[r]) for r in rows["gas"]] == [first_gas, 51, 52]
    assert gs[rows["zget"]] >> 4 == N and gv[rows["zget"]] == 0  # deleted in the segment before: NULL


def test_state_across_the_segment_boundary():
    """Walker state leaves one apply launch through val_meta / val_v and enters the next: a set, a CAS against it and a
    CAS against the stale value in three consecutive segments; a getAndSet chain across them; a delete read as NULL in
    the next segment.  Slots of both super-buckets, background ops everywhere else."""
    n = 4 * SUB
    rng = np.random.default_rng(3)
    slots = [17, 300, 255, 256, 511, 0]
    b = _quiet(rng, n, slots)
    r1 = _plant_boundary_story(b, 0, 17, 300, 255)
    r2 = _plant_boundary_story(b, 1, 256, 511, 0)
    assert not _story_rows(r1) & _story_rows(r2)
    assert {r // SUB for r in (r1["set"], r1["cas_ok"], r1["cas_stale"])} == {0, 1, 2}
    assert {r // SUB for r in r2["gas"]} == {1, 2, 3}
    gs, gv = _Trio(n).apply(b)
    _check_boundary_story(r1, gs, gv, 0)
    _check_boundary_story(r2, gs, gv, 0)


def test_escapes_in_later_segments():
    """Escaped operands (a set / getAndSet value of 2^45 and beyond, a CAS whose update - expected is 2^13 and beyond)
    and escaped results (a get of 2^23 and beyond) in both tiles of segments 1 and 3, on slots of both super-buckets
    that nothing else touches: the apply of a later segment finds the operands at its own first row + the record's
    tile, and the unpermute finds the payloads at the group position of the word that points to them."""
    n = 4 * SUB + 11
    rng = np.random.default_rng(8)
    mine = [5, 6, 7, 260, 261, 262]
    b = _quiet(rng, n, mine)
    big, mid = (1 << 45) + 12345, (1 << 23) + 5
    planted = []
    for seg in (1, 3):
        for tile in (0, 1):
            r0 = seg * SUB + tile * TILE + 1000 * (tile + 1)
            for q, s in enumerate((5, 260)):
                base = r0 + 40 * q
                _plant(b, base + 0, s, SET, L, -big - seg)              # escaped operand
                _plant(b, base + 1, s, GET, 0)                          # escaped result (past 2^55 in magnitude too)
                _plant(b, base + 2, s + 1, SET, L, mid + seg)           # fits the record
                _plant(b, base + 3, s + 1, GET, 0)                      # escaped result: past the word's 24 bits
                _plant(b, base + 4, s + 1, CAS, L | (L << 3), mid + seg, mid + seg + (1 << 13))  # escaped operand
                _plant(b, base + 5, s + 1, GAS, L, big + tile)          # escaped operand and result
                _plant(b, base + 6, s + 2, CAS, L | (L << 3), big, 1)   # escaped, fails
                planted += list(range(base, base + 7))
    esc = np.array([_escapes(int(b.op[i]), int(b.flags[i]), int(b.a[i]), int(b.b[i])) for i in range(n)])
    at = np.nonzero(esc)[0]
    assert set(at // TILE) == {2, 3, 6, 7} and set(at) <= set(planted)  # both tiles of segments 1 and 3, nowhere else
    gs, gv = _Trio(n).apply(b)
    wide = np.nonzero((gv.view(np.int64) >= 1 << 23) | (gv.view(np.int64) < -(1 << 23)))[0]
    assert set(wide // TILE) == {2, 3, 6, 7} and set(wide) <= set(planted)
    for seg in (1, 3):
        r0 = seg * SUB + 1000
        assert gv[r0 + 1].view(np.int64) == -big - seg and gv[r0 + 3] == mid + seg and gv[r0 + 4] == 1
        assert gv[r0 + 5] == mid + seg + (1 << 13) and gv[r0 + 6] == 0


def test_unknown_sessions_in_every_segment():
    """Rows of instances past max_instances and of instances never opened, a tenth of every segment and the whole of
    tile 3 (segment 1's second: its super-bucket runs are all empty) and of tile 4 but one row: UNKNOWN_SESSION, and
    the state as the oracle leaves it."""
    n, max_inst = 3 * SUB + 999, R + 64
    rng = np.random.default_rng(13)
    b = _mixed_ops(rng, rng.integers(0, R, n).astype(np.uint32))
    u = rng.random(n)
    b.inst[u < 0.05] = max_inst + rng.integers(0, 1000, int(np.sum(u < 0.05)))
    b.inst[(u >= 0.05) & (u < 0.1)] = R + rng.integers(0, 64, int(np.sum((u >= 0.05) & (u < 0.1))))
    b.inst[3 * TILE:4 * TILE] = max_inst + 1
    b.inst[4 * TILE:5 * TILE] = R + 3
    b.inst[4 * TILE + 77] = 9
    unk = b.inst >= R
    seg = np.arange(n) // SUB
    assert all(np.any(unk & (seg == k) & (b.inst >= max_inst)) and np.any(unk & (seg == k) & (b.inst < max_inst))
               for k in range(4))
    assert np.all(unk[3 * TILE:4 * TILE]) and np.sum(~unk[4 * TILE:5 * TILE]) == 1
    gs, gv = _Trio(n, max_inst=max_inst).apply(b)
    assert np.all(gs[unk] == UNKNOWN) and np.all(gv[unk] == 0) and not np.any(gs[~unk] == UNKNOWN)


def test_more_than_one_group():
    """CC_VALUE_GROUP_TILES=4: groups of two segments.  n = two groups, one segment and five rows: three partition
    launches (the last group is a segment and the five rows), six apply and six unpermute launches.  The set / CAS / stale-CAS, getAndSet
    and delete stories run across the first group boundary (segments 1, 2, 3) and the second (3, 4, 5)."""
    n = 5 * SUB + 5
    rng = np.random.default_rng(21)
    slots = [17, 300, 255, 256, 511, 0]
    b = _quiet(rng, n, slots)
    r1 = _plant_boundary_story(b, 1, 17, 300, 255)
    r2 = _plant_boundary_story(b, 3, 256, 511, 0, zget_off=4)  # (segment 5 has five rows: the story's last three)
    assert r2["cas_stale"] == 5 * SUB + 3 and r2["gas"][2] == 5 * SUB + 1 and r2["zget"] == n - 1
    assert not _story_rows(r1) & _story_rows(r2)
    assert _launches(n, 2) == (3, 6) and _launches(n, 0) == (6, 6)
    gs, gv = _Trio(n, knob="4").apply(b)
    _check_boundary_story(r1, gs, gv, 0)
    _check_boundary_story(r2, gs, gv, 0)


def test_staging_growth_and_reuse():
    """One engine: a call of one segment (nothing staged by group), of three and a row (the staging is allocated: four
    segments' worth of tiles less one), of six (grown), of two (reused, its dummy rows further out than the call needs)
    and of six again with other rows (reused whole)."""
    sizes = [SUB, 3 * SUB + 1, 6 * SUB, 2 * SUB, 6 * SUB]
    rng = np.random.default_rng(34)
    b = _mixed_ops(rng, rng.integers(0, R, sum(sizes)).astype(np.uint32))
    t = _Trio(max(sizes))
    lo = 0
    for k, n in enumerate(sizes):
        part = b.slice(lo, lo + n)
        assert _launches(n, t.group_segs) == (1, (1, 4, 6, 2, 6)[k])
        t.apply(part)
        lo += n


def test_two_calls_on_different_streams():
    """Device columns, two calls in turn on two streams of the caller's (the engine drains the stream it used last
    before it launches on another): three segments and a row, then two segments."""
    import torch

    from copycat_amd.engine import RESULT_SENTINEL, DeviceBatch

    n1, n2 = 3 * SUB + 1, 2 * SUB
    rng = np.random.default_rng(55)
    b = _mixed_ops(rng, rng.integers(0, R, n1 + n2).astype(np.uint32))
    t = _Trio(n1)
    parts = [b.slice(0, n1), b.slice(n1, n1 + n2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got = {id(t.E): [], id(t.E0): []}
    for e in (t.E, t.E0):
        outs = []
        for part, s in zip(parts, streams):
            db = DeviceBatch.upload(part, device="cuda:0")
            st = torch.full((len(part),), RESULT_SENTINEL, dtype=torch.uint8, device="cuda:0")
            va = torch.zeros(len(part), dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            e.apply(db, st, va, stream=s)
            outs.append((db, st, va))  # (alive until the engine is drained)
        e.sync()
        got[id(e)] = [(st.cpu().numpy(), va.cpu().numpy().view(np.uint64)) for _, st, va in outs]
    for k, part in enumerate(parts):
        os_, ov = t.O.apply(part)
        for e in (t.E, t.E0):
            gs, gv = got[id(e)][k]
            assert np.array_equal(gs, os_) and np.array_equal(gv, ov), (k, e is t.E)
    for x, y, z in zip(t.E.value_state(0, R), t.O.value_state(0, R), t.E0.value_state(0, R)):
        assert np.array_equal(x, y) and np.array_equal(z, y)
    assert t.E.applied_index() == t.O.applied_index() == t.E0.applied_index()
