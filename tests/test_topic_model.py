"""TopicState without a device: the Python model (tests/topic_model.py) against the hand-derived KATs
(tests/golden/topic_kats.json), the topic constants of abi.py against the header, and the topic ops through the
host-only wire decoder (cc_wire_decode needs no engine)."""
import json
import os
import re
import struct

import numpy as np
import pytest

from copycat_amd import abi
from tests.topic_model import OK_NULL, UNKNOWN_OP, Topic

HERE = os.path.dirname(os.path.abspath(__file__))


def load_kats():
    with open(os.path.join(HERE, "golden", "topic_kats.json")) as f:
        return json.load(f)["kats"]


KATS = load_kats()


def test_kats_cover_the_listed_cases():
    names = {k["name"] for k in KATS}
    assert names >= {"duplicate_listen_keeps_first_commit", "unlisten_of_a_non_listener", "publish_to_nobody",
                     "publish_order_per_target_across_two_publishes", "close_leaks_the_listen_commit",
                     "delete_cleans_every_listener", "topic_ops_on_a_group_are_unknown",
                     "group_join_on_a_topic_is_unknown"}
    assert all(k["source"] for k in KATS)


@pytest.mark.parametrize("kat", [k for k in KATS if k["type"] == "TOPIC"], ids=lambda k: k["name"])
def test_model_against_kats(kat):
    t = Topic()
    for s in kat["steps"]:
        if "close" in s:
            t.close(1000 + (s["close"] - 7))
            continue
        st, v, ev = t.apply(s["op"], 1000 + s["k"], s["index"], s["tag"], s["payload"])
        assert (st, v) == (s["status"], s["value"]), s
        assert [[iid - 1000, g, p] for iid, g, p in ev] == s["events"], s
    f = kat["final"]
    assert [list(x) for x in t.listener_list()] == f["listeners"]
    assert t.retained() == f["retained"] and sorted(t.leaked) == f["leaked"]


def test_model_statuses_and_closed_listener_assertion():
    assert (OK_NULL, UNKNOWN_OP) == (0, 2)
    t = Topic()
    assert t.apply(abi.CC_OP_GROUP_JOIN, 1, 1) == (UNKNOWN_OP, 0, [])
    t.listen(5, 1)
    t.closed.add(5)  # a closed session still listed: cannot happen under the engine's session model
    with pytest.raises(AssertionError):
        t.publish(abi.CC_TAG_LONG, 1)


def test_abi_topic_constants_match_header():
    with open(os.path.join(HERE, "..", "include", "copycat_apply.h")) as f:
        hdr = f.read()
    want = {"CC_RES_TOPIC": 9, "CC_OP_TOPIC_LISTEN": 125, "CC_OP_TOPIC_UNLISTEN": 126, "CC_OP_TOPIC_PUBLISH": 127,
            "CC_EV_MESSAGE": 8, "CC_TOPIC_LISTENERS": 64, "CC_ABI_VERSION": 6}
    for name, val in want.items():
        m = re.search(r"#define\s+%s\s+(\d+)" % name, hdr)
        assert m and int(m.group(1)) == val == getattr(abi, name), name
    assert abi.TOPIC_OPS == {abi.CC_OP_DELETE, 125, 126, 127}
    assert "cc_read_topic_listeners" in hdr
    assert int(re.search(r"#define\s+CC_PROFILE_KERNELS\s+(\d+)", hdr).group(1)) == abi.CC_PROFILE_KERNELS == 8


def topic_entry(iid, op, message=None):
    """InstanceCommand bytes of a topic op, built with make_wire's helpers: Listen / Unlisten carry nothing, Publish
    one object, the message (TopicCommands.java:100-108)."""
    from tests.golden.make_wire import ident, obj

    body = obj(message, []) if op == abi.CC_OP_TOPIC_PUBLISH else b""
    return ident(30) + struct.pack(">Q", iid) + ident(op) + body


def test_wire_decodes_topic_ops():
    from copycat_amd.wire import Interner, WireDecoder

    d = WireDecoder(engine=None, interner=Interner(1))
    msgs = [("LONG", -3), ("INT", 7), ("BOOL", True), None, ("LONG", 1 << 62)]
    entries = [topic_entry(11, abi.CC_OP_TOPIC_LISTEN), topic_entry(12, abi.CC_OP_TOPIC_UNLISTEN)]
    entries += [topic_entry(13 + i, abi.CC_OP_TOPIC_PUBLISH, m) for i, m in enumerate(msgs)]
    b, iid, kind = d.decode(entries=entries)
    assert iid.tolist() == [11, 12, 13, 14, 15, 16, 17] and (kind == 0).all()
    assert b.op.tolist() == [125, 126] + [127] * 5
    tags = [abi.flag_tag_a(int(f)) for f in b.flags]
    assert tags == [0, 0, abi.CC_TAG_LONG, abi.CC_TAG_INT, abi.CC_TAG_BOOL, abi.CC_TAG_NULL, abi.CC_TAG_LONG]
    assert b.a.tolist()[2:] == [(1 << 64) - 3, 7, 1, 0, 1 << 62]
    assert not b.key.any() and not b.aux.any() and not b.b.any()
    assert np.all(b.flags >> 3 == 0)
