"""Worlds and streams for the coordination suite on engines that hold a MessageBus (tests/test_coord_bus_cases.py on the
CPU, tests/test_gpu_coord_bus.py on the GPU).

One bus in an engine moves every lock, election, group and value commit of that engine onto k_apply_coord<true>, so the
worlds here put the oracle (locks, elections, groups, values), tests/topic_model.py and tests/bus_model.py over one
engine with every flag, and the streams mix the oracle's generator (copycat_amd.workload.coord_random_stream, whose
lock client model keeps the waiter queues within K) with bus and topic rows.  The scenarios of the GPU file are defined
here, so that the CPU file can walk exactly the same streams through the references alone and assert that none of them
is trivial.  Integers only; this module imports neither torch nor the engine."""
import copy
import functools

import numpy as np

from copycat_amd import abi
from copycat_amd.batch import Batch

L, E_, G, V, T, B = (abi.CC_RES_LOCK, abi.CC_RES_ELECTION, abi.CC_RES_GROUP, abi.CC_RES_VALUE, abi.CC_RES_TOPIC,
                     abi.CC_RES_BUS)
ORACLE_TYPES = (L, E_, G, V)
JOIN, LEAVE, REG, UNREG, DELETE = (abi.CC_OP_BUS_JOIN, abi.CC_OP_BUS_LEAVE, abi.CC_OP_BUS_REGISTER,
                                   abi.CC_OP_BUS_UNREGISTER, abi.CC_OP_DELETE)
BUS_OPS = (JOIN, LEAVE, REG, UNREG)
TOPICS, ADDRS = 6, 5  # the topic and address handles that random bus rows draw from

DEFERRED, EVENTS, RETAINED = abi.CC_CFG_TIMERS_DEFERRED, abi.CC_CFG_VALUE_EVENTS, abi.CC_CFG_VALUE_RETAINED
FLAG_SETS = {"deferred": DEFERRED | EVENTS, "module": EVENTS}  # module: the timers fire before the commit (A8)


# ---- the bus and topic rows of a random stream ----------------------------------------------------------------------
class BusTopicRows:
    """Draws one random bus row or one random topic row into a batch, for tests/test_gpu_bus._mixed_stream and
    coord_bus_stream.  Bus rows are register / unregister heavy, with joins, leaves, a few Deletes and foreign ops.  A
    scratch copy of the bus model walks the bus rows as they are drawn and turns a join or register that would take a
    bus past cap - 2 entries into a leave, so a stream never fills a block.  Only buses and topics that exist in the
    world's models when the stream is drawn get rows."""

    def __init__(self, w, rng, cap=64):
        self.rng, self.cap = rng, cap
        self.binst = np.array([s for r, t in enumerate(w.types) if t == B and r in w.BW.buses for s in w.inst[r]], np.uint32)
        self.tinst = np.array([s for r, t in enumerate(w.types) if t == T and r in w.W.topics for s in w.inst[r]], np.uint32)
        self.scratch = copy.deepcopy(w.BW)
        self.H = abi.cc_flags(abi.CC_TAG_HANDLE)

    def bus(self, b, i, x):
        """row i of b becomes a bus row; x is the row's uniform draw in [0, 1)"""
        rng = self.rng
        s = int(self.binst[rng.integers(0, len(self.binst))])
        if x < 0.10:
            op, a = JOIN, 500 + int(rng.integers(0, ADDRS))
        elif x < 0.16:
            op, a = LEAVE, 0
        elif x < 0.55:
            op, a = REG, 1 + int(rng.integers(0, TOPICS))
        elif x < 0.97:
            op, a = UNREG, 1 + int(rng.integers(0, TOPICS))
        elif x < 0.98:
            op, a = DELETE, 0
        else:
            op, a = abi.CC_OP_TOPIC_PUBLISH, 0
        open_ = self.scratch.inst.get(s)  # (None: the instance's session closed; the row is an UNKNOWN_SESSION one)
        if open_ is not None:
            r, iid, _ = open_
            if op in (JOIN, REG) and self.scratch.buses[r].entries() >= self.cap - 2:
                op, a = LEAVE, 0
            self.scratch.buses[r].apply(op, iid, int(b.index[i]), a)
        b.inst[i], b.op[i], b.a[i] = s, op, a
        b.flags[i] = self.H if op in (JOIN, REG, UNREG) else 0

    def topic(self, b, i, x):
        """row i of b becomes a topic row (publish heavy; the message is the row number, a LONG)"""
        b.inst[i] = self.tinst[self.rng.integers(0, len(self.tinst))]
        b.op[i] = abi.CC_OP_TOPIC_PUBLISH if x < 0.6 else (abi.CC_OP_TOPIC_LISTEN if x < 0.85 else abi.CC_OP_TOPIC_UNLISTEN)
        b.flags[i], b.a[i] = abi.cc_flags(abi.CC_TAG_LONG), i


# ---- a world with flags ---------------------------------------------------------------------------------------------
class _NoEngine:
    """Stands where the engine would: every call does nothing (the CPU tests walk the references alone)."""

    def __getattr__(self, name):
        return lambda *a, **k: None


@functools.lru_cache(maxsize=None)
def _world_class():
    # tests/test_gpu_bus.py imports BusTopicRows from this module, so its World is looked up on first use
    from tests.test_gpu_bus import World
    from tests.test_gpu_close import _per_target
    from tests.test_gpu_coord import _check_state

    class _CoordBusWorld(World):
        """tests/test_gpu_bus.World with engine flags and the oracle's own state checks: types L / E / G / V live in the
        oracle, T in the topic model, B in the bus model, over one engine.

        Every resource has its K instances on the slots the world hands out in resource order (r * K + k with one K),
        instance k of every resource belongs to client 7 + k.
        absent: resource slots that are not created yet (create(r) creates one later).
        shadow: the oracle runs ResourceManager.close's loop over its own instances in java.util.HashMap order and an
          exception (a cleaned election leader) ends it early, so which instances a close reaches depends on every
          instance id in the table.  With shadow the bus and topic instances are open in the oracle too, on one more
          value resource that the world appends (no row of a stream addresses it as a value, close does nothing to it),
          and close() takes from the oracle which of them the loop reached."""

        def __init__(self, types, K, flags, shadow=False, absent=(), engine=True, **cfg):
            types = list(types)
            Ks = list(K) if isinstance(K, (list, tuple)) else [K] * len(types)
            self.flags, self.absent, self.engine = flags, set(absent), engine
            self.shadow = len(types) if shadow else None
            if shadow:
                types, Ks = types + [V], Ks + [0]
            self.own = [r for r, t in enumerate(types) if t in ORACLE_TYPES and r != self.shadow]
            cfg.setdefault("client", self._client)
            self._slot_k = {}
            s = 0
            for k_r in Ks:
                for k in range(k_r):
                    self._slot_k[s + k] = k
                s += k_r
            super().__init__(types, Ks, flags=flags, **cfg)
            if shadow:  # (the shadow resource is the last one created: its instances are opened after it)
                for r, t in enumerate(self.types):
                    if t in (T, B) and r not in self.absent:
                        self._open_shadows(r)

        def _open_shadows(self, r):
            for s in self.inst[r]:
                self.O.instance_open(s, self.shadow, self.iid(s), self.client(s))

        def _client(self, s):
            return 7 + self._slot_k[s]

        def fresh_engine(self):
            return super().fresh_engine() if self.engine else _NoEngine()

        def create(self, r):
            if r in self.absent:
                return
            super().create(r)

        def create_absent(self, r):
            self.absent.discard(r)
            self.create(r)
            if self.shadow is not None and self.types[r] in (T, B):
                self._open_shadows(r)

        def delete_bus(self, r):
            """cc_resource_delete of bus r on the engine and in the model; the slot can be created again"""
            assert self.types[r] == B and self.shadow is None
            self.E.resource_delete(r)
            self.BW.delete_resource(r)
            self.absent.add(r)

        def slots(self, want):
            return [s for r, t in enumerate(self.types) if t in want for s in self.inst[r]]

        # -- checks --
        def check_state(self, E=None):
            E = E or self.E
            types = self.types
            self.types = [None if r in self.absent else t for r, t in enumerate(types)]  # (no model for an absent slot)
            try:
                super().check_state(E)
                _check_state(E, self.O, self.types)  # locks, elections, groups, values and the applied index
            finally:
                self.types = types
            if self.flags & RETAINED:
                self.check_retained(E)

        def check_retained(self, E=None):
            E = E or self.E
            for r in self.own:
                got, want = E.retained(r), self.O.retained(r)
                assert got == want, (r, len(got), len(want), sorted(set(got) ^ set(want))[:8])

        def advance(self, now):
            """the clock moved past `now` on the engine and the oracle: the timer events, equal as multisets"""
            ev = self.E.advance_time_events(now, capacity=1 << 16)
            self.O.advance_time(now)
            oe = self.O.take_events()
            if self.engine:
                key = ("target", "code", "tag", "payload")
                assert sorted(zip(*(ev[k].tolist() for k in key))) == sorted(zip(*(oe[k].tolist() for k in key)))
                assert (ev["src"] == abi.CC_EVSRC_TIMER).all() and (ev["pos"] == 0xFFFFFFFF).all()
            return oe

        def close(self, clients, expire=False):
            """cc_sessions_close of `clients`, in order (expire: cc_sessions_expire of their bitmap, ascending), against
            the oracle and the two models together: the events per target (the oracle's targets and the models' are
            different instances) and the instances that left the table."""
            if expire and self.engine:
                import torch

                assert list(clients) == sorted(clients) and max(clients) < 64
                bm = torch.zeros(1, dtype=torch.int64, device="cuda")
                bm[0] = sum(1 << int(c) for c in clients)
                closed, ev = self.E.sessions_expire(bm, 64, capacity=1 << 18)
            else:
                closed, ev = self.E.sessions_close(clients, capacity=1 << 18) or (0, None)
            for c in clients:
                (self.O.session_expire if expire else self.O.session_close)(int(c))
            oe = self.O.take_events()
            want = _per_target(oe["target"], oe["code"], oe["tag"], oe["payload"])
            both = self.slots((T, B))
            keep = [s for s in both if self.O.inst_slot_of(self.iid(s)) >= 0] if self.shadow is not None else []
            leaves = 0
            for c in clients:
                for t, code, tag, payload in self.BW.close_client(int(c), keep=keep):
                    want.setdefault(t, []).append((code, tag, payload))
                    leaves += 1
                self.W.close_client(int(c), keep=keep)
            if self.engine:
                assert (ev["pos"] == 0xFFFFFFFF).all() and (ev["src"] == abi.CC_EVSRC_CLOSE).all()
                assert _per_target(ev["target"], ev["code"], ev["tag"], ev["payload"]) == want
                self.check_open()
            return closed, oe, leaves

        def open_slots(self):
            """the instance slots still open by the references: the oracle's own, and the models' buses and topics"""
            o = [s for s in self.slots(ORACLE_TYPES) if self.O.inst_slot_of(self.iid(s)) >= 0]
            return sorted(o + list(self.BW.inst) + list(self.W.inst))

        def check_open(self):
            every = [s for r in range(len(self.types)) if r not in self.absent for s in self.inst[r]]
            got = [s for s in every if self.E.instance_slot(self.iid(s)) >= 0]
            assert got == self.open_slots()

    return _CoordBusWorld


def CoordBusWorld(types, K, flags, **cfg):
    """The world of this suite (see _world_class): CoordBusWorld(types, K, flags, shadow=False, absent=(), engine=True,
    **engine configuration)."""
    return _world_class()(types, K, flags, **cfg)


# ---- layouts --------------------------------------------------------------------------------------------------------
def layout_types(name):
    if name == "mixed":  # one 64-slot quarter with bus lanes, one without, in the same engine
        return [L, E_, G, V] * 15 + [B, B, T, T] + [L, E_, G, V] * 16
    if name == "uniform":  # every specialised walk in its <..., true> form; the buses in another super-bucket
        return [L] * 64 + [E_] * 64 + [G] * 64 + [V] * 64 + [B, B]
    raise ValueError(name)


VALUES_PLAIN_BUS = 300  # the bus of `values_plain`: in super-bucket 1 (resource slots 256..511)


def layout_world(name, K, flags, **cfg):
    if name == "values_plain":  # 600 values of one instance each, no value events; the bus has 4 instances
        types = [V] * 300 + [B] + [V] * 300
        return CoordBusWorld(types, [1] * 300 + [4] + [1] * 300, flags, **cfg)
    return CoordBusWorld(layout_types(name), K, flags, **cfg)


# ---- streams --------------------------------------------------------------------------------------------------------
def oracle_rows(w, n, seed, index0=1, values=False):
    """coord_random_stream (values: value_random_stream) over the oracle-owned resources of w, in the world's instance
    slots.  max_inst lies above every bus and topic instance slot, so the generator's unknown instances stay unknown."""
    from copycat_amd.workload import coord_random_stream, value_random_stream

    if values:
        g = value_random_stream(n, len(w.own), w.max_inst, seed=seed, index0=index0)
    else:
        K = w.K[w.own[0]]
        assert all(w.K[r] == K for r in w.own)
        g = coord_random_stream(n, np.array([w.types[r] for r in w.own], np.uint8), K, w.max_inst, seed=seed, index0=index0)
    slot_of = np.array([s for r in w.own for s in w.inst[r]], np.uint32)
    known = g.inst < len(slot_of)
    g.inst[known] = slot_of[g.inst[known]]
    assert (g.inst[~known] >= w.max_inst).all() and max(w.slots((T, B)), default=0) < w.max_inst
    return g


def row_types(w, b):
    """the resource type behind every row's instance slot (0: an unknown slot)"""
    type_of = np.zeros(w.max_inst, np.uint8)
    for r, t in enumerate(w.types):
        type_of[w.inst[r]] = t
    return np.where(b.inst < w.max_inst, type_of[np.minimum(b.inst, w.max_inst - 1)], 0)


def coord_bus_stream(w, n, seed, p_bus, index0=1, base=None, values=False, cap=64, p_topic=0.25):
    """The oracle's random stream with a fraction p_bus of its rows overwritten by bus and topic rows (p_topic of them
    topic rows while the world has topics).  Only rows of elections, groups and values are overwritten: the generator's
    lock client model is what bounds the waiter queues, and it has to go on seeing every lock row.  The rows keep the
    generator's index and clock.  base: rows of one longer oracle_rows() draw (a stream continued over several phases
    keeps one lock client model), instead of a draw of its own."""
    b = base if base is not None else oracle_rows(w, n, seed, index0, values)
    assert len(b) == n
    rng = np.random.default_rng(seed)
    rows = BusTopicRows(w, rng, cap)
    if not len(rows.binst) and not len(rows.tinst):
        assert p_bus == 0
        return b
    pick = np.isin(row_types(w, b), (E_, G, V)) & (rng.random(n) < p_bus)
    u, topic = rng.random(n), rng.random(n) < p_topic
    for i in np.nonzero(pick)[0].tolist():
        b.key[i] = b.b[i] = b.aux[i] = 0
        if len(rows.tinst) and (topic[i] or not len(rows.binst)):
            rows.topic(b, i, float(u[i]))
        else:
            rows.bus(b, i, float(u[i]))
    return b


def concat(*parts):
    return Batch.from_columns(**{name: np.concatenate([getattr(p, name) for p in parts]) for name, _ in abi.BATCH_COLUMNS})


# ---- the walk through the references that the CPU file asserts on ---------------------------------------------------
class Facts:
    """What a stream did in the references (walk): the preconditions that make a GPU comparison meaningful."""

    def __init__(self):
        self.status = set()        # status codes on rows of oracle-owned instances and of unknown instances
        self.max_queue = 0         # the longest lock queue after any lock row
        self.queues = {}           # lock -> its longest queue after any of its rows
        self.expired = 0           # waiters that left a queue between two rows of their lock: their timeout fired
        self.promoted = 0          # elections: an unlisten of the leader that made the first listener the leader
        self.executed = 0          # GROUP_EXECUTE rows that published "execute" to a member
        self.changes = 0           # "change" events to value listeners
        self.bus_ops_on_oracle = 0  # rows of an election, group or value that carry a bus op code (85-88)
        self.fan_events = 0        # bus register / unregister events
        self.join_rows = 0         # result rows of bus joins
        self.max_entries = 0       # the fullest bus block after any join or register
        self.max_list = {L: 0, E_: 0, G: 0}  # the longest queue / listener list / member list at a walk's end
        self.rows = 0


def walk(w, b, facts=None):
    """Applies b to the references of w (w.expect) in runs that end after every lock row and after every bus join or
    register, and records Facts.  The lock of every lock row is read before and after the row: a waiter that was queued
    after the lock's last row and is gone before its next one left by timeout, since nothing else in these streams
    changes a lock between two of its rows (no Delete and no foreign op reaches a lock, a close does nothing to one)."""
    f = facts or Facts()
    n = len(b)
    if n == 0:
        return f
    ty = row_types(w, b)
    res_of = {s: r for r in range(len(w.types)) for s in w.inst[r]}
    f.bus_ops_on_oracle += int((np.isin(b.op, BUS_OPS) & np.isin(ty, (E_, G, V))).sum())
    cut = (ty == L) | ((ty == B) & np.isin(b.op, (JOIN, REG)))
    ends = (np.nonzero(cut)[0] + 1).tolist()
    if not ends or ends[-1] != n:
        ends.append(n)
    last = w.__dict__.setdefault("_queue_after", {})  # lock -> its queue after its last row (kept from walk to walk)
    lo = 0
    for hi in ends:
        i = hi - 1
        if ty[i] == L:
            r = res_of[int(b.inst[i])]
            _walk_run(w, b, lo, i, ty, f)
            before = w.O.lock_state(r)[3]
            f.expired += len(set(last.get(r, ())) - set(before))
            _walk_run(w, b, i, hi, ty, f)
            last[r] = w.O.lock_state(r)[3]
            f.max_queue = max(f.max_queue, len(last[r]))
            f.queues[r] = max(f.queues.get(r, 0), len(last[r]))
        else:
            _walk_run(w, b, lo, hi, ty, f)
            if ty[i] == B and w.BW.buses:
                f.max_entries = max(f.max_entries, max(m.entries() for m in w.BW.buses.values()))
        lo = hi
    f.rows += n
    for r in w.own:
        t = w.types[r]
        if t == L:
            f.max_list[L] = max(f.max_list[L], len(w.O.lock_state(r)[3]))
        elif t == E_:
            f.max_list[E_] = max(f.max_list[E_], len(w.O.election_state(r)[2]))
        elif t == G:
            f.max_list[G] = max(f.max_list[G], len(w.O.group_members(r)))
    return f


def _walk_run(w, b, lo, hi, ty, f):
    if hi <= lo:
        return
    s, v, tev, (oe, apos, amem), bev, brows = w.expect(b, lo, hi)
    mine = np.isin(ty[lo:hi], ORACLE_TYPES + (0,))
    f.status.update(abi.status_code(s[mine]).tolist())
    op = b.op[lo:hi]
    commit = oe["src"] == abi.CC_EVSRC_COMMIT
    f.promoted += int((commit & (oe["code"] == abi.CC_EV_ELECT) & (op[oe["pos"]] == abi.CC_OP_ELECT_UNLISTEN)).sum())
    f.executed += int((commit & (oe["code"] == abi.CC_EV_EXECUTE) & (op[oe["pos"]] == abi.CC_OP_GROUP_EXECUTE)).sum())
    f.changes += int((oe["code"] == abi.CC_EV_CHANGE).sum())
    f.fan_events += len(bev)
    f.join_rows += sum(len(rr) for rr in brows.values())


# ---- the scenarios of tests/test_gpu_coord_bus.py -------------------------------------------------------------------
SUB_BATCH = 16384

# 1. random parity
PARITY = dict(n=40_000, K=6, p_bus=0.15, slices=[(0, 1), (1, 17_500), (17_500, 17_500), (17_500, 40_000)],
              seed={"mixed": 102, "uniform": 201})
PARITY_CASES = [(lay, fl) for lay in ("mixed", "uniform") for fl in ("deferred", "module")]


def parity_world(layout, flags, **cfg):
    return layout_world(layout, PARITY["K"], FLAG_SETS[flags], sub_batch=SUB_BATCH, **cfg)


def parity_stream(w, layout):
    return coord_bus_stream(w, PARITY["n"], PARITY["seed"][layout], PARITY["p_bus"])


# 2. values_plain
VALUES_PLAIN = dict(n=60_000, seed=103, p_bus=0.05, cuts=[0, 25_000, 60_000])


def values_plain_world(**cfg):
    return layout_world("values_plain", None, DEFERRED, sub_batch=SUB_BATCH, **cfg)


def values_plain_stream(w):
    return coord_bus_stream(w, VALUES_PLAIN["n"], VALUES_PLAIN["seed"], VALUES_PLAIN["p_bus"], values=True, p_topic=0.0)


# 3. large blocks
LARGE = dict(cap=256, K=200, n=8_000, seed=302, p_bus=0.3, types=[L, E_, G, V, B, L, E_, G], max_events=1 << 25)


def large_world(**cfg):
    return CoordBusWorld(LARGE["types"], LARGE["K"], DEFERRED | EVENTS, coord_cap=LARGE["cap"],
                         max_events=LARGE["max_events"], **cfg)


def large_stream(w):
    return coord_bus_stream(w, LARGE["n"], LARGE["seed"], LARGE["p_bus"], cap=LARGE["cap"])


# 4. instantiation switches
SWITCH = dict(K=6, seed=401, p_bus=0.15, phases=[10_000, 10_000, 10_000, 5_000], buses=(60, 61), topics=(62, 63))


def switch_world(**cfg):
    """the `mixed` layout with both bus slots and both topic slots left empty"""
    return layout_world("mixed", SWITCH["K"], DEFERRED | EVENTS | RETAINED, sub_batch=SUB_BATCH,
                        absent=SWITCH["buses"] + SWITCH["topics"], **cfg)


def switch_base(w):
    """the oracle's rows of all four phases: one index sequence, one clock, one lock client model"""
    return oracle_rows(w, sum(SWITCH["phases"]), SWITCH["seed"])


def switch_enter(w, phase):
    """the registry changes before phase 1..4 on the world's engine and references"""
    if phase == 2:
        for r in SWITCH["topics"] + SWITCH["buses"]:
            w.create_absent(r)
    elif phase == 3:
        for r in SWITCH["buses"]:
            w.delete_bus(r)
    elif phase == 4:
        w.create_absent(SWITCH["buses"][0])


def switch_stream(w, base, phase):
    lo = sum(SWITCH["phases"][:phase - 1])
    n = SWITCH["phases"][phase - 1]
    return coord_bus_stream(w, n, SWITCH["seed"] + phase, 0.0 if phase == 1 else SWITCH["p_bus"], base=base.slice(lo, lo + n))


# 5. close and expire under a bus
CLOSE = dict(K=5, n=20_000, seed=501, p_bus=0.15)


def close_world(**cfg):
    """64 oracle resources [L, E, G, V] * 16 as in test_close_fanout_random at R = 64, with the mixed layout's two buses
    and two topics in the same quarter's last slots (so 60 oracle resources there and 4 in the next quarter)"""
    types = [L, E_, G, V] * 15 + [B, B, T, T] + [L, E_, G, V]
    return CoordBusWorld(types, CLOSE["K"], DEFERRED | EVENTS, shadow=True, **cfg)


def close_clients():
    """[(clients, expire)]: one client closed, two closed in one call, one expired through the bitmap"""
    clients = [7 + k for k in range(CLOSE["K"])]
    np.random.default_rng(CLOSE["seed"]).shuffle(clients)
    return [(clients[:1], False), (clients[1:3], False), (clients[3:4], True)]


def close_follow_up(w, first):
    """the batch after the closes, through tests/test_gpu_close._follow_up's lock rewrite: the lock rows on instances
    that are still open become isLeader (UNKNOWN_OP on a lock), since the generator's lock clients know nothing of the
    closes (every resource has K instances on r * K + k, which is the registry _follow_up expects)"""
    from tests.test_gpu_close import _follow_up

    n = CLOSE["n"] // 2
    b = coord_bus_stream(w, n, CLOSE["seed"] + 100, CLOSE["p_bus"], index0=CLOSE["n"] + 1)
    b.time[:] = np.maximum(b.time, first.time[-1])
    return _follow_up(b, np.array(w.types, np.uint8), CLOSE["K"], w.max_inst, np.array(w.open_slots(), np.uint32))


# 6. retained sets
RETAIN = dict(n=2_000, R=16, K=3, seed=679, p_bus=0.35, schedules=40)


def retain_world(**cfg):
    types = [L, E_, G, V] * (RETAIN["R"] // 4) + [B, B]
    return CoordBusWorld(types, RETAIN["K"], DEFERRED | EVENTS | RETAINED, shadow=True, **cfg)


def retain_stream(w):
    from tests.test_gpu_retained import _with_schedules

    n, K = RETAIN["n"], RETAIN["K"]
    b = coord_bus_stream(w, n, RETAIN["seed"], RETAIN["p_bus"])
    types = np.array(w.types, np.uint8)  # (every resource has K instances on r * K + k, the bus included)
    return _with_schedules(b, types, K, w.max_inst, np.random.default_rng(RETAIN["seed"]), RETAIN["schedules"])


# 7. both prefix forms
PREFIX = dict(K=6, n=3_000, seed=731, p_bus=0.3, cap=64, lock=0, bus=60)


def prefix_world(**cfg):
    return layout_world("mixed", PREFIX["K"], DEFERRED | EVENTS, coord_cap=PREFIX["cap"], **cfg)


def prefix_batches(w):
    """(fill, stream, stop, rest): `fill` takes lock 0 and queues 64 waiters behind it, by hand; `stream` is a random
    stream whose rows on lock 0 are isLeader (UNKNOWN_OP) except row `stop`, a 65th waiter, with a bus join at stop - 2
    and that member's register, a fan-out, at stop - 1; `rest` is an unlock by the holder and then stream[stop:]."""
    K, cap, n = PREFIX["K"], PREFIX["cap"], PREFIX["n"]
    lock = w.inst[PREFIX["lock"]]
    m = cap + 1
    fill = Batch.from_columns(index=np.arange(1, m + 1), time=np.ones(m), inst=[lock[i % K] for i in range(m)],
                              op=np.full(m, abi.CC_OP_LOCK_LOCK, np.uint8), aux=np.full(m, 2**64 - 1, np.uint64))
    b = coord_bus_stream(w, n, PREFIX["seed"], PREFIX["p_bus"], index0=m + 1)
    ty = row_types(w, b)
    b.op[np.isin(b.inst, lock)] = abi.CC_OP_ELECT_ISLEADER
    free = ty != L  # (a lock row of another lock stays: the generator's lock clients have to see it happen)
    stop = next(i for i in range(2 * n // 3, n) if free[i - 2] and free[i - 1] and free[i])
    member = w.inst[PREFIX["bus"]][1]
    H = abi.cc_flags(abi.CC_TAG_HANDLE)
    for i, (s, op, a, fl, aux) in zip((stop - 2, stop - 1, stop), ((member, JOIN, 509, H, 0), (member, REG, 3, H, 0),
                                                               (lock[2], abi.CC_OP_LOCK_LOCK, 0, 0, 2**64 - 1))):
        b.inst[i], b.op[i], b.a[i], b.flags[i], b.aux[i], b.key[i], b.b[i] = s, op, a, fl, aux, 0, 0
    unlock = Batch.from_columns(index=[int(b.index[stop])], time=[int(b.time[stop])], inst=[lock[0]],
                                op=np.array([abi.CC_OP_LOCK_UNLOCK], np.uint8))
    tail = b.slice(stop, n)
    tail.index += 1
    return fill, b, stop, concat(unlock, tail)
