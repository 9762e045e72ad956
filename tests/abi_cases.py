"""The batch input space of the C-ABI (include/copycat_apply.h, cc_batch): which columns each op reads, batches whose
other cells hold garbage, and the sweep over every op byte and flags byte.

`USED` is the one statement of "Columns an op does not use may hold anything": the header's cc_batch comment carries
the same table, tests/test_abi_dont_care.py checks it against the wire decoder's carried fields and shows that the
references keep the promise, and tests/test_gpu_dont_care.py / tests/test_gpu_op_matrix.py hold the engine to it.
Integers only; this module imports neither torch nor the engine."""
import numpy as np

from copycat_amd import abi
from copycat_amd.batch import Batch

OPERANDS = ("key", "a", "b", "aux")


def _op(name):
    return getattr(abi, "CC_OP_" + name)


# columns read | ops (the header's table, row for row); `a` implies tag a, `b` tag b, `key` the key tag
_TABLE = (
    ("a", "VALUE_SET VALUE_GETANDSET MAP_CONTAINSVALUE MMAP_CONTAINSVALUE MMAP_REMOVEVALUE QUEUE_CONTAINS QUEUE_ADD "
          "QUEUE_OFFER QUEUE_REMOVE TOPIC_PUBLISH BUS_JOIN BUS_REGISTER BUS_UNREGISTER"),
    ("a b", "VALUE_CAS"),
    ("key", "MAP_CONTAINSKEY MAP_GET MAP_REMOVE MMAP_CONTAINSKEY MMAP_GET MMAP_SIZE SET_CONTAINS SET_REMOVE"),
    ("key a", "MAP_GETORDEFAULT MAP_REMOVEIFPRESENT MMAP_CONTAINSENTRY MMAP_REMOVE GROUP_EXECUTE"),
    ("key a aux", "MAP_PUT MAP_PUTIFABSENT MAP_REPLACE MMAP_PUT GROUP_SCHEDULE"),
    ("key a b aux", "MAP_REPLACEIFPRESENT"),
    ("key aux", "SET_ADD"),
    ("aux", "LOCK_LOCK"),
)
USED_BY_NAME = {name: frozenset(cols.split()) for cols, names in _TABLE for name in names.split()}
# op byte -> the set of {key, a, b, aux} it reads; every other op byte reads nothing (index, time, inst and op are
# always read)
USED = {op: frozenset() for op in range(256)}
USED.update({_op(name): cols for name, cols in USED_BY_NAME.items()})

_USED_LUT = np.zeros((256, len(OPERANDS)), bool)
for _o, _cols in USED.items():
    for _c, _name in enumerate(OPERANDS):
        _USED_LUT[_o, _c] = _name in _cols


def used_mask(op):
    """{column: bool array} over the rows of an op column: does the row's op read the column"""
    op = np.asarray(op, np.uint8)
    return {name: _USED_LUT[op, c] for c, name in enumerate(OPERANDS)}


def copy_batch(b):
    return b.slice(0, len(b))


def scribble(b, seed):
    """A copy of b with every cell outside USED replaced by a random u64 and every unused tag field by random bits:
    tag a / tag b take 0..7 (the result-only tags 5..7 among them), the key tag 0..3 (HANDLE among them)."""
    rng = np.random.default_rng(seed)
    out = copy_batch(b)
    n = len(b)
    use = used_mask(b.op)
    for name in OPERANDS:
        col = getattr(out, name)
        free = ~use[name]
        col[free] = rng.integers(0, 1 << 64, n, dtype=np.uint64)[free]
    f = out.flags
    for name, shift, bits in (("a", 0, 7), ("b", 3, 7), ("key", 6, 3)):
        free = ~use[name]
        rnd = rng.integers(0, bits + 1, n).astype(np.uint8)
        f[free] = (f[free] & np.uint8(0xFF ^ (bits << shift))) | (rnd[free] << np.uint8(shift))
    return out


def changed_share(b, s):
    """the share of rows whose flags byte differs between a batch and its scribbled copy"""
    return float((b.flags != s.flags).mean()) if len(b) else 0.0


# ---- every op byte x flags byte --------------------------------------------------------------------------------------
TAGS_AB = (0, 1, 2, 3, 4)   # operand tags of the sweep: NULL, LONG, INT, BOOL, HANDLE
KTAGS = (0, 1, 2, 3)        # key tags: LONG, INT, BOOL, HANDLE (handles 0..3 are registered by tests/handles.py)
SWEEP_AUX = np.array([0, 0, 0, -1, -5, 1, 7, 40], np.int64).view(np.uint64)  # ttl / timeout / delay: none, forever, short


TTL_OPS = (abi.CC_OP_MAP_PUT, abi.CC_OP_MAP_PUTIFABSENT, abi.CC_OP_MAP_REPLACE, abi.CC_OP_MAP_REPLACEIFPRESENT,
           abi.CC_OP_MMAP_PUT, abi.CC_OP_SET_ADD)


def sweep_rows(resources, seed, ops=range(256), tags_a=TAGS_AB, tags_b=TAGS_AB, ktags=KTAGS, repeat=2, index0=1,
               skip=lambda res, op: False, handle_a=lambda res, op: False, ttl=False):
    """The (instance, op, flags) sweep.  resources: [(instance slots, instance ids)] per resource; every resource gets
    one row per (op, tag a, tag b, key tag) on one of its instances, the rows of all resources are permuted by a seeded
    rng and the whole permutation is repeated `repeat` times in one batch with a fresh draw of instances and operands,
    so that every op also meets populated state.  Used columns hold small values (key, a, b in 0..3, aux from SWEEP_AUX;
    the member of a group's schedule / execute is one of the group's instance ids or a foreign id), the unused ones are
    scribbled.  skip(res, op): rows left out; handle_a(res, op): rows whose operand a is forced to a HANDLE; ttl: may a
    store into the map table arm a timer (else the ttl of TTL_OPS is <= 0).  The log clock advances by one every 16
    rows."""
    rng = np.random.default_rng(seed)
    ops = np.array(list(ops), np.uint8)
    fl = np.array([abi.cc_flags(ta, tb, kt) for ta in tags_a for tb in tags_b for kt in ktags], np.uint8)
    res_col, op_col, fl_col = [], [], []
    for r in range(len(resources)):
        keep = np.array([not skip(r, int(o)) for o in ops], bool)
        o = np.repeat(ops[keep], len(fl))
        res_col.append(np.full(len(o), r, np.int64))
        op_col.append(o)
        fl_col.append(np.tile(fl, int(keep.sum())))
    res_col, op_col, fl_col = (np.concatenate(x) for x in (res_col, op_col, fl_col))
    m = len(op_col)
    parts = []
    for _ in range(repeat):
        p = rng.permutation(m)
        parts.append((res_col[p], op_col[p], fl_col[p]))
    res_col, op_col, fl_col = (np.concatenate([q[i] for q in parts]) for i in range(3))
    n = len(op_col)
    b = Batch(n)
    b.index[:] = np.arange(index0, index0 + n, dtype=np.uint64)
    b.time[:] = np.arange(n, dtype=np.uint64) // np.uint64(16) + np.uint64(1)
    b.op[:] = op_col
    b.flags[:] = fl_col
    pick = rng.integers(0, 1 << 30, n)
    member = rng.integers(0, 1 << 30, n)
    sched = np.isin(op_col, (abi.CC_OP_GROUP_SCHEDULE, abi.CC_OP_GROUP_EXECUTE))
    b.key[:] = rng.integers(0, 4, n).astype(np.uint64)
    for r, (slots, iids) in enumerate(resources):
        rows = res_col == r
        slots, iids = np.asarray(slots, np.uint32), np.asarray(iids, np.uint64)
        b.inst[rows] = slots[pick[rows] % len(slots)]
        mine = rows & sched
        ids = np.concatenate([iids, iids[:1] + np.uint64(77_777)])  # (one id that is no instance of the resource)
        b.key[mine] = ids[member[mine] % len(ids)]
        force = rows & np.array([handle_a(r, int(o)) for o in range(256)], bool)[op_col]
        b.flags[force] = (b.flags[force] & np.uint8(0xF8)) | np.uint8(abi.CC_TAG_HANDLE)
    b.a[:] = rng.integers(0, 4, n).astype(np.uint64)
    b.b[:] = rng.integers(0, 4, n).astype(np.uint64)
    b.aux[:] = SWEEP_AUX[rng.integers(0, len(SWEEP_AUX), n)]
    if not ttl:  # no stored entry arms a timer (ttl <= 0): the table stays out of TTL mode, where the engine refuses a
        arm = np.isin(op_col, TTL_OPS) & (b.aux.view(np.int64) > 0)  # containsValue over stored nulls (copycat_apply.h)
        b.aux[arm] = 0
    return scribble(b, seed + 1)


def peak_lengths(O, b, lengths, step=32):
    """Applies b to the oracle O in slices of `step` rows and reads lengths() (a list of collection lengths) after each:
    returns (statuses, values, events, aux rows, the largest length read + step), the last an upper bound of every
    collection's peak inside the batch.  Events and aux rows come back with their positions in b."""
    n = len(b)
    s, v = np.zeros(n, np.uint8), np.zeros(n, np.uint64)
    ev = {k: [] for k in ("pos", "target", "code", "src", "tag", "payload")}
    apos, amem = [], []
    peak = max(lengths(), default=0)
    for lo in range(0, n, step):
        hi = min(lo + step, n)
        s[lo:hi], v[lo:hi] = O.apply(b.slice(lo, hi))
        e = O.take_events()
        p, mbr = O.take_aux()
        for k in ev:
            ev[k].append(e[k] + np.uint32(lo) if k == "pos" else e[k])
        apos.append(p + np.uint32(lo))
        amem.append(mbr)
        peak = max(peak, max(lengths(), default=0))
    ev = {k: np.concatenate(x) if x else np.zeros(0, np.uint64) for k, x in ev.items()}
    return s, v, ev, (np.concatenate(apos), np.concatenate(amem)), peak + step


# ---- quorum and expiry inputs over the whole unsigned range (tests/test_gpu_quorum.py) -------------------------------
QUORUM_BASES = np.array([0, 1, (1 << 63) - 1, 1 << 63, (1 << 64) - 2, (1 << 64) - 1], np.uint64)


def quorum_edge_groups(groups, replicas, seed):
    """(match, term_start, commit_in): per group a base from QUORUM_BASES; match = base + 0..2 per replica, term_start
    and commit_in = base + 0..2, all wrapping at 2^64, so the quorum value n meets n == term_start (advances),
    n == commit_in (does not), n < term_start, heavy ties and both ends of the unsigned range."""
    rng = np.random.default_rng(seed)
    base = QUORUM_BASES[rng.integers(0, len(QUORUM_BASES), groups)]
    with np.errstate(over="ignore"):
        match = base[None, :] + rng.integers(0, 3, (replicas, groups)).astype(np.uint64)
        ts = base + rng.integers(0, 3, groups).astype(np.uint64)
        ci = base + rng.integers(0, 3, groups).astype(np.uint64)
    return np.ascontiguousarray(match), ts, ci


def quorum_numpy(match, ts, ci):
    """the rule restated in numpy: sort descending, take entry replicas / 2 (the quorum-th largest)"""
    n = np.sort(match, axis=0)[::-1][match.shape[0] // 2]
    return np.where((n >= ts) & (n > ci), n, ci)


EXPIRY_TIMEOUTS = (0, (1 << 63) - 1, 1 << 63, (1 << 64) - 1)


def expiry_edge_sessions(sessions, now, seed):
    """lastKeepAlive stamps around `now`: a little and a lot in the past, equal to now, in the future, with the top bit
    set, 0 and 2^64 - 1"""
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 7, sessions)
    with np.errstate(over="ignore"):
        last = np.select(
            [kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5],
            [np.uint64(now) - rng.integers(0, 20_000, sessions).astype(np.uint64),
             np.uint64(now) + rng.integers(0, 100, sessions).astype(np.uint64),
             np.uint64(1 << 63) + rng.integers(0, 1 << 62, sessions).astype(np.uint64),
             np.full(sessions, (1 << 64) - 1, np.uint64), np.zeros(sessions, np.uint64),
             np.uint64(now) - np.uint64(1 << 63) + rng.integers(0, 3, sessions).astype(np.uint64) - np.uint64(1)],
            rng.integers(0, 1 << 64, sessions, dtype=np.uint64))
    return np.ascontiguousarray(last, np.uint64)


# ---- the three engine configurations of tests/test_gpu_dont_care.py and their streams --------------------------------
SUB_BATCH = 16384


def merge_streams(parts, seed, time_from=None):
    """Rows of several streams interleaved at random places, each stream's own order kept; the index column restarts
    at 1.  time_from: the part whose clock the batch keeps (the other parts' rows take the clock of the row before
    them); None: the caller sets the time column."""
    rng = np.random.default_rng(seed)
    src = rng.permutation(np.concatenate([np.full(len(p), k) for k, p in enumerate(parts)]))
    n = len(src)
    b = Batch(n)
    for k, p in enumerate(parts):
        at = src == k
        for name, _ in abi.BATCH_COLUMNS:
            getattr(b, name)[at] = getattr(p, name)
        if time_from is not None and k != time_from:
            b.time[at] = 0
    b.index[:] = np.arange(1, n + 1, dtype=np.uint64)
    b.time[:] = np.maximum.accumulate(b.time) if time_from is not None else np.arange(n, dtype=np.uint64) // np.uint64(8)
    return b


# 1. value-only: k_part_v4 -> k_apply_value_v3 -> k_unpermute_v3, three segments of one group, a ragged last tile
VALUE = dict(n=2 * SUB_BATCH + 8192 + 37, resources=1000, seed=601, hot=4, p_hot=0.3)


def value_stream():
    from copycat_amd.workload import value_random_stream

    c = VALUE
    return value_random_stream(c["n"], c["resources"], c["resources"] + 8, seed=c["seed"], hot=c["hot"], p_hot=c["p_hot"])


# 2. values + maps + sets + multimaps in one table: resource r has the one instance slot r (id 1000 + r, client 7)
TABLE = dict(values=64, maps_small=16, maps_large=8, mixed=16, map_capacity=65536, seed=611,
             rows=dict(values=12_000, maps_small=20_000, maps_large=16_000, mixed=12_000))


def table_types():
    c = TABLE
    mixed = [abi.CC_RES_MULTIMAP, abi.CC_RES_MAP, abi.CC_RES_MULTIMAP, abi.CC_RES_SET] * (c["mixed"] // 4)
    return np.array([abi.CC_RES_VALUE] * c["values"] + [abi.CC_RES_MAP] * (c["maps_small"] + c["maps_large"]) + mixed,
                    np.uint8)


def table_stream(ttl):
    """60,000 rows: value_random_stream on the values, map_random_stream on maps of 64 keys and of 1,024 keys (hot keys,
    HANDLE keys, every key op), tests/test_gpu_multimap._stream over MultiMap + Map + Set, then in-stream containsValue
    rows and barrier rows.  Plain: stored nulls on the odd 64-key maps, clears and Deletes.  ttl: no stored null, a
    moving clock and armed timers, and size / isEmpty / containsValue barriers only (in TTL mode the engine refuses a
    containsValue whose answer hangs on an iteration order it cannot bound)."""
    from copycat_amd.workload import map_random_stream, value_random_stream
    from tests.test_gpu_map import _cv_rows, _no_null_values, _with_barriers, _with_ttl
    from tests.test_gpu_multimap import _stream as keyed_stream

    c, rows = TABLE, TABLE["rows"]
    types = table_types()
    R = len(types)
    max_inst = R + 8
    v0, s0, l0, m0 = 0, c["values"], c["values"] + c["maps_small"], c["values"] + c["maps_small"] + c["maps_large"]
    bv = value_random_stream(rows["values"], c["values"], max_inst, first_inst=v0, seed=c["seed"])
    bs = map_random_stream(rows["maps_small"], c["maps_small"], max_inst, keys=64, first_inst=s0, seed=c["seed"] + 1,
                           hot=2, p_hot=0.3)
    bl = map_random_stream(rows["maps_large"], c["maps_large"], max_inst, keys=1024, first_inst=l0, seed=c["seed"] + 2,
                           hot=2, p_hot=0.3)
    bk = keyed_stream(rows["mixed"], types[m0:], 16, c["seed"] + 3)
    bk.inst[:] = np.where(bk.inst < c["mixed"], bk.inst + m0, max_inst + 3)
    bk.aux[:] = 0
    b = merge_streams([bv, bs, bl, bk], c["seed"] + 4)
    if ttl:
        _no_null_values(b)
        _with_ttl(b, c["seed"] + 5)
        wide = np.array([abi.CC_OP_MAP_SIZE, abi.CC_OP_MAP_CONTAINSVALUE, abi.CC_OP_MAP_ISEMPTY], np.uint8)
        _cv_rows(b, 0.01, c["seed"] + 6)
        _with_barriers(b, 0.001, c["seed"] + 7, ops=wide)
    else:
        keep_null = (b.inst >= s0) & (b.inst < l0) & (b.inst % 2 == 1)
        f = b.flags.copy()
        _no_null_values(b)
        b.flags[keep_null] = f[keep_null]
        _cv_rows(b, 0.01, c["seed"] + 6, clear_rate=0.0005)
        _with_barriers(b, 0.001, c["seed"] + 7)
    return b


# 3. coordination: locks, elections, groups, values (K instances each), queues (one instance each), coord_cap 256
COORD = dict(n=40_000, K=5, legv=6, queues=4, queue_rows=6_000, schedules=100, seed=621, coord_cap=256, p_bus=0.15)


def coord_types(bus):
    from tests.coord_bus_cases import B, E_, G, L, T, V

    c = COORD
    types = [L, E_, G, V] * c["legv"] + [abi.CC_RES_QUEUE] * c["queues"] + ([B, T] if bus else [])
    K = [c["K"]] * (4 * c["legv"]) + [1] * c["queues"] + ([c["K"], c["K"]] if bus else [])
    return types, K


def coord_world(bus, **cfg):
    from tests.coord_bus_cases import DEFERRED, EVENTS, CoordBusWorld

    types, K = coord_types(bus)
    return CoordBusWorld(types, K, DEFERRED | EVENTS, coord_cap=COORD["coord_cap"], sub_batch=SUB_BATCH,
                         max_events=1 << 22, **cfg)


def coord_stream(w, bus):
    """coord_random_stream over the locks, elections, groups and values of w (with a bus: 15 % of the election, group
    and value rows overwritten by bus and topic traffic), 100 group rows turned into GROUP_SCHEDULE as
    tests/test_gpu_coord.py::test_group_schedule_timers does, queue rows from tests/test_gpu_queue._stream between
    them, and a drain of every queue at the end (its contents, in order)."""
    from tests.coord_bus_cases import G, coord_bus_stream, row_types
    from tests.test_gpu_queue import _stream as queue_stream

    c = COORD
    nq, nd = c["queue_rows"], c["queues"] * abi.CC_QUEUE_CAP
    nc = c["n"] - nq - nd
    b = coord_bus_stream(w, nc, c["seed"], c["p_bus"] if bus else 0.0)
    rng = np.random.default_rng(c["seed"] + 1)
    ty = row_types(w, b)
    grp = np.nonzero((ty == G) & np.isin(b.op, (abi.CC_OP_GROUP_JOIN, abi.CC_OP_GROUP_LEAVE, abi.CC_OP_GROUP_EXECUTE)))[0]
    rows = rng.choice(grp, size=c["schedules"], replace=False)
    res_of = {s: r for r in range(len(w.types)) for s in w.inst[r]}
    b.op[rows] = abi.CC_OP_GROUP_SCHEDULE
    for i in rows.tolist():
        slots = w.inst[res_of[int(b.inst[i])]]
        k = int(rng.integers(0, len(slots) + 2))  # some ids are not instances of this group
        b.key[i] = w.iid(slots[k]) if k < len(slots) else 50_000 + k
    b.flags[rows] = abi.cc_flags(abi.CC_TAG_HANDLE, 0, 0)
    b.a[rows] = rng.integers(0, 1 << 20, len(rows)).astype(np.uint64)
    b.aux[rows] = rng.integers(-5, 400, len(rows)).astype(np.int64).view(np.uint64)
    qslots = np.array([w.inst[r][0] for r, t in enumerate(w.types) if t == abi.CC_RES_QUEUE], np.uint32)
    bq = queue_stream(nq, c["queues"], w.max_inst, c["seed"] + 2)
    bq.inst[:] = np.where(bq.inst < c["queues"], qslots[np.minimum(bq.inst, c["queues"] - 1)], w.max_inst + 5)
    body = merge_streams([b, bq], c["seed"] + 3, time_from=0)
    drain = Batch(nd)
    drain.inst[:] = np.tile(qslots, abi.CC_QUEUE_CAP)
    drain.op[:] = abi.CC_OP_QUEUE_POLL
    drain.time[:] = body.time[-1]
    out = Batch.from_columns(**{name: np.concatenate([getattr(body, name), getattr(drain, name)])
                                for name, _ in abi.BATCH_COLUMNS})
    out.index[:] = np.arange(1, len(out) + 1, dtype=np.uint64)
    return out
