"""MessageBusState restated in Python: the reference for the engine's bus state machine (the C++ oracle has no bus).

Written from coordination/src/main/java/io/atomix/coordination/state/MessageBusState.java, one object per bus:
  members    :31      HashMap<Long, Commit<Join>> keyed by commit.session().id() — the instance's ManagedResourceSession,
                      whose id() is the instance id (ManagedResourceSession.java:59-61)
  topics     :32      HashMap<String, HashMap<Long, Commit<Register>>>
  close      :35-40   members.remove(id) with no clean() (the Join commit is retained for good if there was one), the
                      session's registrations stay in `topics`; "leave"(id) to every remaining member, whether or not the
                      closed session was one
  join       :45-65   members.put (a replaced Join is not clean()ed: leaked); the result has one key per entry of
                      `topics` — an empty registration map or registrants that are no members give an empty set — and
                      under it the distinct addresses of the registrants that are members (:53-56); no event
  leave      :70-97   a non-member: nothing.  Else the member is removed and its Join clean()ed (:72-74); for every topic
                      the leaver is registered on the registration is removed without clean() (:82, leaked),
                      "unregister"(ConsumerInfo(topic, the leaver's address)) goes to every remaining member (:84-86), and
                      the topic is dropped if it is now empty (:88-90; a topic that was already empty stays).  The Leave
                      commit is always clean()ed (:95)
  register   :102-119 a non-member: IllegalStateException (:105-107), the commit clean()ed (:116).  Else
                      registrations.put (:110, a replaced Register is leaked) and "register"(ConsumerInfo(topic, the
                      registrant's address)) to every member, the registrant included (:112-114)
  unregister :124-144 the Unregister commit is clean()ed only on the exception path (:140-143), so the log retains every
                      one.  A registration of the session on the topic is removed and clean()ed (:128-130); if the session
                      is still a member, "unregister"(ConsumerInfo) goes to every member (:132-137).  The topic is not
                      dropped when it becomes empty: only leave drops topics
  delete     :147-151 every member's Join clean()ed but `members` not cleared (the members stay, with a cleaned commit);
                      every registration clean()ed and `topics` cleared
Any other op is CC_ST_UNKNOWN_OP (ResourceStateMachineExecutor.java:78); every void result is
CC_STATUS(CC_ST_OK, CC_TAG_NULL), value 0; a join answers CC_STATUS(CC_ST_OK, CC_TAG_MAP) with the topic count.

Orders the reference takes from HashMap iteration, fixed here as the engine fixes them: one fan-out in ascending member
instance id (each event goes to a different session); the fan-outs of one leave in ascending topic handle
(DistributedMessageBus.unregisterConsumer, DistributedMessageBus.java:199-206, updates one topic's entry per event, so no
client state depends on the order between topics); a join's topics and addresses ascending.  Tests compare events per
target.

Addresses and topics are handles below 2^32 (CC_BUS_HANDLE_BITS); a ConsumerInfo payload is topic << 32 | address.
Instance ids are commit indices, so never 0.
"""
import numpy as np

from copycat_amd import abi
from copycat_amd.batch import Batch

OK_NULL = abi.cc_status(abi.CC_ST_OK, abi.CC_TAG_NULL)
OK_MAP = abi.cc_status(abi.CC_ST_OK, abi.CC_TAG_MAP)
UNKNOWN_OP = abi.cc_status(abi.CC_ST_UNKNOWN_OP, abi.CC_TAG_NULL)
ILLEGAL_STATE = abi.cc_status(abi.CC_ST_ILLEGAL_STATE, abi.CC_TAG_NULL)


def info(topic, addr):
    return (int(topic) << 32) | int(addr)


class Bus:
    def __init__(self):
        self.members = {}  # instance id -> [address, Join index, cleaned]
        self.topics = {}   # topic -> {instance id: Register index}
        self.leaked = []   # commits dropped without clean()

    # every method returns (status, value, events, rows): events = [(target instance id, code, tag, payload)],
    # rows = the join's result rows [(code, payload)]
    def join(self, iid, index, addr):
        old = self.members.get(iid)
        if old is not None and not old[2]:
            self.leaked.append(old[1])  # :47 members.put over an entry
        self.members[iid] = [int(addr), index, False]
        rows = []
        for t in sorted(self.topics):
            rows.append((abi.CC_EV_BUS_TOPIC, t))
            addrs = {self.members[i][0] for i in self.topics[t] if i in self.members}
            rows.extend((abi.CC_EV_BUS_ADDRESS, a) for a in sorted(addrs))
        return OK_MAP, len(self.topics), [], rows

    def _fan(self, code, payload):
        return [(m, code, abi.CC_TAG_HANDLE, payload) for m in sorted(self.members)]

    def leave(self, iid):
        prev = self.members.pop(iid, None)
        ev = []
        if prev is not None:
            for t in sorted(self.topics):
                regs = self.topics[t]
                if iid in regs:
                    self.leaked.append(regs.pop(iid))  # :82 removed, never clean()ed
                    ev.extend(self._fan(abi.CC_EV_BUS_UNREGISTER, info(t, prev[0])))
                    if not regs:
                        del self.topics[t]
        return OK_NULL, 0, ev, []

    def register(self, iid, index, topic):
        parent = self.members.get(iid)
        if parent is None:
            return ILLEGAL_STATE, 0, [], []
        regs = self.topics.setdefault(int(topic), {})
        if iid in regs:
            self.leaked.append(regs[iid])  # :110 registrations.put over an entry
        regs[iid] = index
        return OK_NULL, 0, self._fan(abi.CC_EV_BUS_REGISTER, info(topic, parent[0])), []

    def unregister(self, iid, index, topic):
        self.leaked.append(index)  # :140-143 clean()ed only on the exception path
        regs = self.topics.get(int(topic))
        ev = []
        if regs is not None and iid in regs:
            del regs[iid]
            parent = self.members.get(iid)
            if parent is not None:
                ev = self._fan(abi.CC_EV_BUS_UNREGISTER, info(topic, parent[0]))
        return OK_NULL, 0, ev, []

    def close(self, iid):
        """[(target instance id, code, tag, payload)]: "leave"(iid) to every remaining member"""
        old = self.members.pop(iid, None)
        if old is not None and not old[2]:
            self.leaked.append(old[1])
        return [(m, abi.CC_EV_BUS_LEAVE, abi.CC_TAG_LONG, iid) for m in sorted(self.members)]

    def delete(self):
        for m in self.members.values():
            m[2] = True
        self.topics.clear()
        return OK_NULL, 0, [], []

    def apply(self, op, iid, index, a=0):
        """One commit: (status, value, events, result rows)."""
        if op == abi.CC_OP_BUS_JOIN:
            return self.join(iid, index, a)
        if op == abi.CC_OP_BUS_LEAVE:
            return self.leave(iid)
        if op == abi.CC_OP_BUS_REGISTER:
            return self.register(iid, index, a)
        if op == abi.CC_OP_BUS_UNREGISTER:
            return self.unregister(iid, index, a)
        if op == abi.CC_OP_DELETE:
            return self.delete()
        return UNKNOWN_OP, 0, [], []

    def member_list(self):
        """[(instance id, address, Join index, cleaned)] ascending — cc_read_bus_members"""
        return [(i, m[0], m[1], m[2]) for i, m in sorted(self.members.items())]

    def registration_list(self):
        """[(topic, instance id, Register index)] ascending; an empty topic is (topic, 0, 0) — cc_read_bus_registrations"""
        out = []
        for t in sorted(self.topics):
            regs = self.topics[t]
            out.extend((t, i, regs[i]) for i in sorted(regs))
            if not regs:
                out.append((t, 0, 0))
        return out

    def entries(self):
        return len(self.members) + len(self.registration_list())

    def retained(self):
        joins = [m[1] for m in self.members.values() if not m[2]]
        regs = [x for r in self.topics.values() for x in r.values()]
        return sorted(joins + regs + self.leaked)


class BusWorld:
    """Buses by resource slot and the instances on them: applies the bus rows of a batch (any object with the columns
    inst / op / flags / index / a), as tests/topic_model.TopicWorld does for topics."""

    def __init__(self):
        self.buses = {}    # resource slot -> Bus
        self.inst = {}     # instance slot -> (resource slot, instance id, client)
        self.slot_of = {}  # instance id -> instance slot

    def create(self, res):
        self.buses[res] = Bus()

    def delete_resource(self, res):
        del self.buses[res]
        for s in [s for s, (r, _, _) in self.inst.items() if r == res]:
            del self.slot_of[self.inst.pop(s)[1]]

    def open(self, slot, res, iid, client):
        self.inst[slot] = (res, iid, client)
        self.slot_of[iid] = slot

    def close_client(self, client, keep=()):
        """the close fan-out's events [(target instance slot, code, tag, payload)], instances in ascending slot; the
        slots in `keep` stay open (a close loop that an exception ended early leaves the client's later instances)"""
        ev = []
        for s in sorted(s for s, (_, _, c) in self.inst.items() if c == client and s not in keep):
            res, iid, _ = self.inst.pop(s)
            del self.slot_of[iid]
            ev.extend((self.slot_of[t], c, g, p) for t, c, g, p in self.buses[res].close(iid))
        return ev

    def apply(self, b, lo=0, hi=None):
        """Rows [lo, hi) of `b` that sit on a bus instance: {row: (status, value)}, the events as (row, target instance
        slot, code, tag, payload) in log order, and the result rows {row: [(code, payload)]} of the joins."""
        hi = len(b.op) if hi is None else hi
        res, events, rows = {}, [], {}
        for i in range(lo, hi):
            s = int(b.inst[i])
            if s not in self.inst:
                continue
            r, iid, _ = self.inst[s]
            st, v, ev, rr = self.buses[r].apply(int(b.op[i]), iid, int(b.index[i]), int(b.a[i]))
            res[i] = (st, v)
            events.extend((i, self.slot_of[t], c, g, p) for t, c, g, p in ev)
            if st == OK_MAP:
                rows[i] = rr
        return res, events, rows


def bus_rows(spec, index0=1, tag=abi.CC_TAG_HANDLE):
    """[(instance slot, op[, operand a])] as a Batch: the operand a HANDLE, index and clock advancing by one per row"""
    n = len(spec)
    b = Batch(n)
    b.index[:] = np.arange(index0, index0 + n, dtype=np.uint64)
    b.time[:] = np.arange(index0, index0 + n, dtype=np.uint64)
    b.inst[:] = [x[0] for x in spec]
    b.op[:] = [x[1] for x in spec]
    b.flags[:] = [abi.cc_flags(tag if len(x) > 2 else 0) for x in spec]
    b.a[:] = np.array([x[2] if len(x) > 2 else 0 for x in spec], np.uint64)
    return b
