"""MessageBusState without a device: the Python model (tests/bus_model.py) against the hand-derived KATs
(tests/golden/bus_kats.json) and the bus constants of abi.py against the header."""
import json
import os
import re

import pytest

from copycat_amd import abi
from copycat_amd.batch import untagged
from tests.bus_model import ILLEGAL_STATE, OK_MAP, OK_NULL, UNKNOWN_OP, Bus, BusWorld, bus_rows, info

HERE = os.path.dirname(os.path.abspath(__file__))


def load_kats():
    with open(os.path.join(HERE, "golden", "bus_kats.json")) as f:
        return json.load(f)["kats"]


KATS = load_kats()


def test_kats_cover_the_listed_cases():
    names = {k["name"] for k in KATS}
    assert names >= {"K1_join_results_unregister_leave", "K2_close_of_a_member_and_of_a_non_member",
                     "K3_delete_keeps_the_members", "K4_reregister_leaks_the_old_register",
                     "K5_join_result_lists_a_shared_address_once", "rejoin_leaks_the_old_join",
                     "leave_of_a_non_member_changes_nothing", "leave_leaks_registrations_and_drops_only_emptied_topics",
                     "register_by_a_non_member_is_illegal_state", "unregister_commit_is_always_retained",
                     "unregister_keeps_the_emptied_topic_and_leave_keeps_an_empty_one",
                     "close_leaves_the_registrations_retained_and_unreported",
                     "delete_then_rejoin_of_a_cleaned_member_leaks_nothing", "other_ops_on_a_bus_are_unknown"}
    assert all("MessageBusState.java:" in k["source"] or "Executor.java:" in k["source"] for k in KATS)


@pytest.mark.parametrize("kat", KATS, ids=lambda k: k["name"])
def test_model_against_kats(kat):
    b = Bus()
    for s in kat["steps"]:
        if "close" in s:
            ev = b.close(s["close"])
            assert all(g == abi.CC_TAG_LONG for _, _, g, _ in ev)
            assert [[t, c, p] for t, c, _, p in ev] == s["events"], s
        else:
            st, v, ev, rows = b.apply(s["op"], s["m"], s["index"], s["a"])
            assert (st, v) == (s["status"], s["value"]), s
            assert all(g == abi.CC_TAG_HANDLE for _, _, g, _ in ev)
            assert [[t, c, p] for t, c, _, p in ev] == s["events"], s
            assert [list(r) for r in rows] == s["rows"], s
        if "retained" in s:
            assert b.retained() == s["retained"], s
    f = kat["final"]
    assert [list(x) for x in b.member_list()] == f["members"]
    assert [list(x) for x in b.registration_list()] == f["registrations"]
    assert b.retained() == f["retained"]


def test_statuses_and_payload():
    assert (OK_NULL, UNKNOWN_OP, ILLEGAL_STATE, OK_MAP) == (0, 2, 3, 0x70)
    assert info(7, 501) == (7 << 32) | 501
    assert untagged(abi.CC_TAG_MAP, 3) == ("map", 3)
    assert abi.status_tag(OK_MAP) == abi.CC_TAG_MAP and abi.status_code(OK_MAP) == abi.CC_ST_OK


def test_world_routes_rows_and_closes():
    """BusWorld: rows by instance slot, events by target slot, a client's close over its instances."""
    w = BusWorld()
    w.create(0)
    for s in range(3):
        w.open(s, 0, 50 - s, 7 + s)  # instance ids descend with the slot
    b = bus_rows([(0, abi.CC_OP_BUS_JOIN, 501), (2, abi.CC_OP_BUS_JOIN, 502), (0, abi.CC_OP_BUS_REGISTER, 7),
                  (1, abi.CC_OP_BUS_REGISTER, 7), (1, abi.CC_OP_BUS_JOIN, 501)])
    res, ev, rows = w.apply(b)
    assert res == {0: (OK_MAP, 0), 1: (OK_MAP, 0), 2: (OK_NULL, 0), 3: (ILLEGAL_STATE, 0), 4: (OK_MAP, 1)}
    # ascending member id: id 48 (slot 2) before id 50 (slot 0)
    assert ev == [(2, 2, abi.CC_EV_BUS_REGISTER, abi.CC_TAG_HANDLE, info(7, 501)),
                  (2, 0, abi.CC_EV_BUS_REGISTER, abi.CC_TAG_HANDLE, info(7, 501))]
    assert rows == {0: [], 1: [], 4: [(abi.CC_EV_BUS_TOPIC, 7), (abi.CC_EV_BUS_ADDRESS, 501)]}
    assert w.close_client(7) == [(2, abi.CC_EV_BUS_LEAVE, abi.CC_TAG_LONG, 50), (1, abi.CC_EV_BUS_LEAVE, abi.CC_TAG_LONG, 50)]
    assert w.buses[0].retained() == [1, 2, 3, 5]


def test_abi_bus_constants_match_header():
    with open(os.path.join(HERE, "..", "include", "copycat_apply.h")) as f:
        hdr = f.read()
    want = {"CC_RES_BUS": 10, "CC_OP_BUS_JOIN": 85, "CC_OP_BUS_LEAVE": 86, "CC_OP_BUS_REGISTER": 87,
            "CC_OP_BUS_UNREGISTER": 88, "CC_BUS_HANDLE_BITS": 32, "CC_TAG_MAP": 7, "CC_EV_BUS_LEAVE": 9,
            "CC_EV_BUS_REGISTER": 10, "CC_EV_BUS_UNREGISTER": 11, "CC_EV_BUS_TOPIC": 12, "CC_EV_BUS_ADDRESS": 13,
            "CC_BUS_ENTRIES": 64, "CC_ABI_VERSION": 6}
    for name, val in want.items():
        m = re.search(r"#define\s+%s\s+(\d+)" % name, hdr)
        assert m and int(m.group(1)) == val == getattr(abi, name), name
    assert abi.BUS_OPS == {abi.CC_OP_DELETE, 85, 86, 87, 88}
    assert abi.CC_RES_BUS not in abi.TYPE_OPS  # (the wire fixture requires every op of TYPE_OPS; see abi.py)
    assert "cc_read_bus_members" in hdr and "cc_read_bus_registrations" in hdr
