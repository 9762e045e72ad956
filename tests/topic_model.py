"""TopicState restated in Python: the reference for the engine's topic state machine (the C++ oracle has no topic).

Written from coordination/src/main/java/io/atomix/coordination/state/TopicState.java, one object per topic:
  listeners  :32     HashMap<Long, Commit<Listen>> keyed by commit.session().id() — the instance's
                     ManagedResourceSession, whose id() is the instance id (ManagedResourceSession.java:59-61)
  close      :35-37  listeners.remove(id): no clean(), no event — the listen commit is retained for good (leaked)
  listen     :42-48  no entry: store the commit; an entry: the new commit is clean()ed, the first one stays
  unlisten   :53-62  remove the entry if there is one and clean its commit; the unlisten commit is always cleaned
  publish    :67-82  "message"(message) to every listener's session; the publish commit is cleaned
  delete     :85-88  every listener commit cleaned, the map emptied
Every result is void: status CC_STATUS(CC_ST_OK, CC_TAG_NULL), value 0.  An op the type does not register (anything but
Delete and 125-127) is CC_ST_UNKNOWN_OP (ResourceStateMachineExecutor.java:78).

Order inside one publish: the reference iterates a HashMap, but each event of a publish goes to a different session,
so no session observes an order between them; this model lists them in ascending listener instance id, which is the
engine's (documented) emission order.  Tests compare events per target.

publish's !isOpen() branch (:74-77): a ManagedResourceSession leaves OPEN only when its parent session closes
(ManagedResourceSession.java:129-131), and that close runs TopicState.close for the instance in the same step, so a
publish never meets a closed listener.  The model asserts this instead of implementing the branch.
"""
import numpy as np

from copycat_amd import abi

OK_NULL = abi.cc_status(abi.CC_ST_OK, abi.CC_TAG_NULL)
UNKNOWN_OP = abi.cc_status(abi.CC_ST_UNKNOWN_OP, abi.CC_TAG_NULL)


class Topic:
    def __init__(self):
        self.listeners = {}  # instance id -> the index of its Listen commit
        self.leaked = []     # Listen commits close() dropped without clean()
        self.closed = set()  # instance ids whose session closed (only to assert publish never meets one)

    def listen(self, iid, index):
        if iid not in self.listeners:
            self.listeners[iid] = index

    def unlisten(self, iid):
        self.listeners.pop(iid, None)

    def publish(self, tag, payload):
        """[(listener instance id, tag, canonical payload)] in ascending listener id"""
        assert not (self.closed & set(self.listeners)), "a publish met a listener whose session closed"
        pl = 0 if tag == abi.CC_TAG_NULL else int(payload)
        return [(iid, int(tag), pl) for iid in sorted(self.listeners)]

    def close(self, iid):
        self.closed.add(iid)
        if iid in self.listeners:
            self.leaked.append(self.listeners.pop(iid))

    def delete(self):
        self.listeners.clear()

    def apply(self, op, iid, index, tag=0, payload=0):
        """One commit: (status, value, events)."""
        if op == abi.CC_OP_TOPIC_LISTEN:
            self.listen(iid, index)
        elif op == abi.CC_OP_TOPIC_UNLISTEN:
            self.unlisten(iid)
        elif op == abi.CC_OP_TOPIC_PUBLISH:
            return OK_NULL, 0, self.publish(tag, payload)
        elif op == abi.CC_OP_DELETE:
            self.delete()
        else:
            return UNKNOWN_OP, 0, []
        return OK_NULL, 0, []

    def listener_list(self):
        return sorted(self.listeners.items())

    def retained(self):
        return sorted(list(self.listeners.values()) + self.leaked)


class TopicWorld:
    """Topics by resource slot and the instances on them: applies the topic rows of a Batch."""

    def __init__(self):
        self.topics = {}     # resource slot -> Topic
        self.inst = {}       # instance slot -> (resource slot, instance id, client)
        self.slot_of = {}    # instance id -> instance slot

    def create(self, res):
        self.topics[res] = Topic()

    def delete_resource(self, res):
        del self.topics[res]
        for s in [s for s, (r, _, _) in self.inst.items() if r == res]:
            del self.slot_of[self.inst.pop(s)[1]]

    def open(self, slot, res, iid, client):
        self.inst[slot] = (res, iid, client)
        self.slot_of[iid] = slot

    def close_client(self, client, keep=()):
        """the slots in `keep` stay open (a close loop that an exception ended early leaves the client's later instances)"""
        for s in sorted(s for s, (_, _, c) in self.inst.items() if c == client and s not in keep):
            res, iid, _ = self.inst.pop(s)
            del self.slot_of[iid]
            self.topics[res].close(iid)

    def apply(self, b, lo=0, hi=None):
        """Rows [lo, hi) of `b` that sit on a topic instance: {row: (status, value)} and the events as
        (row, target instance slot, tag, payload) in log order (within a publish: ascending listener id)."""
        hi = len(b) if hi is None else hi
        res, events = {}, []
        for i in range(lo, hi):
            s = int(b.inst[i])
            if s not in self.inst:
                continue
            r, iid, _ = self.inst[s]
            fl = int(b.flags[i])
            st, v, ev = self.topics[r].apply(int(b.op[i]), iid, int(b.index[i]), abi.flag_tag_a(fl), int(b.a[i]))
            res[i] = (st, v)
            events.extend((i, self.slot_of[t], g, p) for t, g, p in ev)
        return res, events


def per_target(rows, targets, tags, payloads):
    """{target: [(row, tag, payload)]} in stream order"""
    out = {}
    cols = [c.tolist() if isinstance(c, np.ndarray) else list(c) for c in (rows, targets, tags, payloads)]
    for r, t, g, p in zip(*cols):  # (python ints throughout: a payload past 2^63 must not pass through a float)
        out.setdefault(int(t), []).append((int(r), int(g), int(p)))
    return out
