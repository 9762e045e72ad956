"""ctypes mirror of include/copycat_apply.h (constants and structs).

tests/test_abi.py checks every constant here against the #defines of the header, so the two cannot drift.
"""
import ctypes as C

CC_ABI_VERSION = 6
CC_MEMCPY_H2D, CC_MEMCPY_D2H, CC_MEMCPY_D2D = 1, 2, 3
CC_PROFILE_KERNELS = 8
CC_PHASES = 8  # phase clocks per kernel of the diagnostics build (cc_debug_phases)

CC_OK = 0
CC_ERR_INVALID = -1
CC_ERR_HIP = -2
CC_ERR_CAPACITY = -3
CC_ERR_UNSUPPORTED = -4
CC_ERR_STATE = -5

CC_RES_NONE = 0
CC_RES_VALUE = 1
CC_RES_MAP = 2
CC_RES_LOCK = 3
CC_RES_ELECTION = 4
CC_RES_GROUP = 5
CC_RES_SET = 6
CC_RES_QUEUE = 7
CC_RES_MULTIMAP = 8
CC_RES_TOPIC = 9
CC_RES_BUS = 10
CC_QUEUE_CAP = 64

CC_OP_DELETE = 1
CC_OP_VALUE_GET = 50
CC_OP_VALUE_SET = 51
CC_OP_VALUE_CAS = 52
CC_OP_VALUE_GETANDSET = 53
CC_OP_VALUE_LISTEN = 54
CC_OP_VALUE_UNLISTEN = 55
CC_OP_MAP_CONTAINSKEY = 60
CC_OP_MAP_CONTAINSVALUE = 61
CC_OP_MAP_PUT = 62
CC_OP_MAP_PUTIFABSENT = 63
CC_OP_MAP_GET = 64
CC_OP_MAP_GETORDEFAULT = 65
CC_OP_MAP_REMOVE = 66
CC_OP_MAP_REMOVEIFPRESENT = 67
CC_OP_MAP_REPLACE = 68
CC_OP_MAP_REPLACEIFPRESENT = 69
CC_OP_MAP_ISEMPTY = 70
CC_OP_MAP_SIZE = 71
CC_OP_MAP_CLEAR = 72
CC_OP_QUEUE_CONTAINS = 90
CC_OP_QUEUE_ADD = 91
CC_OP_QUEUE_OFFER = 92
CC_OP_QUEUE_PEEK = 93
CC_OP_QUEUE_POLL = 94
CC_OP_QUEUE_ELEMENT = 95
CC_OP_QUEUE_REMOVE = 96
CC_OP_QUEUE_SIZE = 97
CC_OP_QUEUE_ISEMPTY = 98
CC_OP_QUEUE_CLEAR = 99
CC_OP_SET_CONTAINS = 100
CC_OP_SET_ADD = 101
CC_OP_SET_REMOVE = 102
CC_OP_SET_SIZE = 103
CC_OP_SET_ISEMPTY = 104
CC_OP_SET_CLEAR = 105
CC_OP_MMAP_CONTAINSKEY = 75
CC_OP_MMAP_CONTAINSENTRY = 76
CC_OP_MMAP_CONTAINSVALUE = 77
CC_OP_MMAP_PUT = 78
CC_OP_MMAP_GET = 79
CC_OP_MMAP_REMOVE = 80
CC_OP_MMAP_REMOVEVALUE = 81
CC_OP_MMAP_ISEMPTY = 82
CC_OP_MMAP_SIZE = 83
CC_OP_MMAP_CLEAR = 84
CC_OP_ELECT_LISTEN = 110
CC_OP_ELECT_UNLISTEN = 111
CC_OP_ELECT_ISLEADER = 112
CC_OP_LOCK_LOCK = 115
CC_OP_LOCK_UNLOCK = 116
CC_OP_GROUP_JOIN = 120
CC_OP_GROUP_LEAVE = 121
CC_OP_GROUP_SCHEDULE = 122
CC_OP_GROUP_EXECUTE = 123
CC_OP_TOPIC_LISTEN = 125
CC_OP_TOPIC_UNLISTEN = 126
CC_OP_TOPIC_PUBLISH = 127
CC_OP_BUS_JOIN = 85
CC_OP_BUS_LEAVE = 86
CC_OP_BUS_REGISTER = 87
CC_OP_BUS_UNREGISTER = 88
CC_BUS_HANDLE_BITS = 32

CC_TAG_NULL = 0
CC_TAG_LONG = 1
CC_TAG_INT = 2
CC_TAG_BOOL = 3
CC_TAG_HANDLE = 4
CC_TAG_SET = 5
CC_TAG_LIST = 6
CC_TAG_MAP = 7

CC_ST_OK = 0
CC_ST_UNKNOWN_SESSION = 1
CC_ST_UNKNOWN_OP = 2
CC_ST_ILLEGAL_STATE = 3
CC_ST_ILLEGAL_ARGUMENT = 4
CC_ST_NULL_POINTER = 5
CC_ST_TYPE_MISMATCH = 6
CC_ST_UNKNOWN_RESOURCE = 7
CC_ST_NO_SUCH_ELEMENT = 8

CC_EV_CHANGE = 1
CC_EV_LOCK = 2
CC_EV_ELECT = 3
CC_EV_JOIN = 4
CC_EV_LEAVE = 5
CC_EV_EXECUTE = 6
CC_EV_MEMBER = 7
CC_EV_MESSAGE = 8
CC_EV_BUS_LEAVE = 9
CC_EV_BUS_REGISTER = 10
CC_EV_BUS_UNREGISTER = 11
CC_EV_BUS_TOPIC = 12
CC_EV_BUS_ADDRESS = 13

CC_EVSRC_COMMIT = 0
CC_EVSRC_TIMER = 1
CC_EVSRC_CLOSE = 2
CC_EVSRC_RESULT = 3

CC_CFG_TIMERS_DEFERRED = 1
CC_CFG_VALUE_EVENTS = 2
CC_CFG_VALUE_RETAINED = 4
CC_LOCK_QUEUE = 64
CC_ELECTION_LISTENERS = 64
CC_GROUP_MEMBERS = 64
CC_VALUE_LISTENERS = 64
CC_TOPIC_LISTENERS = 64
CC_BUS_ENTRIES = 64

# ops each resource type registers (ResourceStateMachine.init + Copycat reflection `configure`)
TYPE_OPS = {
    CC_RES_VALUE: {CC_OP_DELETE, 50, 51, 52, 53, 54, 55},
    CC_RES_MAP: {CC_OP_DELETE} | set(range(60, 73)),
    CC_RES_LOCK: {CC_OP_DELETE, 115, 116},
    CC_RES_ELECTION: {CC_OP_DELETE, 110, 111, 112},
    CC_RES_GROUP: {CC_OP_DELETE, 120, 121, 122, 123},
    CC_RES_SET: {CC_OP_DELETE} | set(range(100, 106)),
    CC_RES_QUEUE: {CC_OP_DELETE} | set(range(90, 100)),
    CC_RES_MULTIMAP: {CC_OP_DELETE, 75} | set(range(78, 85)),
}
# TopicState's ops (TopicCommands.java:53,64,80); kept beside TYPE_OPS, whose ops the wire fixture must all contain
TOPIC_OPS = {CC_OP_DELETE, 125, 126, 127}
# MessageBusState's ops (MessageBusCommands.java; 89 is ConsumerInfo, not an op)
BUS_OPS = {CC_OP_DELETE, 85, 86, 87, 88}
# key tags of the flags column (keys are never null)
KTAG_OF_TAG = {CC_TAG_LONG: 0, CC_TAG_INT: 1, CC_TAG_BOOL: 2, CC_TAG_HANDLE: 3}
TAG_OF_KTAG = {v: k for k, v in KTAG_OF_TAG.items()}


def cc_flags(tag_a=0, tag_b=0, ktag=0):
    return (tag_a & 7) | ((tag_b & 7) << 3) | ((ktag & 3) << 6)


def flag_tag_a(f):
    return f & 7


def flag_tag_b(f):
    return (f >> 3) & 7


def flag_ktag(f):
    return (f >> 6) & 3


def cc_status(code, tag):
    return (code & 15) | ((tag & 15) << 4)


def status_code(s):
    return s & 15


def status_tag(s):
    return (s >> 4) & 15


class cc_config(C.Structure):
    _fields_ = [
        ("max_resources", C.c_uint32),
        ("max_instances", C.c_uint32),
        ("max_batch", C.c_uint64),
        ("max_events", C.c_uint64),
        ("map_capacity", C.c_uint64),
        ("device", C.c_int32),
        ("flags", C.c_uint32),
        ("sub_batch", C.c_uint64),
        ("coord_cap", C.c_uint32),
        ("reserved32", C.c_uint32),
        ("reserved", C.c_uint64 * 3),
    ]


class cc_batch(C.Structure):
    _fields_ = [
        ("index", C.c_void_p),
        ("time", C.c_void_p),
        ("inst", C.c_void_p),
        ("op", C.c_void_p),
        ("flags", C.c_void_p),
        ("key", C.c_void_p),
        ("a", C.c_void_p),
        ("b", C.c_void_p),
        ("aux", C.c_void_p),
    ]


class cc_batch_out(C.Structure):
    _fields_ = cc_batch._fields_


class cc_results(C.Structure):
    _fields_ = [("status", C.c_void_p), ("value", C.c_void_p)]


class cc_events(C.Structure):
    _fields_ = [
        ("pos", C.c_void_p),
        ("target", C.c_void_p),
        ("code", C.c_void_p),
        ("src", C.c_void_p),
        ("tag", C.c_void_p),
        ("payload", C.c_void_p),
        ("capacity", C.c_uint64),
        ("count", C.c_void_p),
    ]


# Catalyst wire format (include/copycat_apply.h "Catalyst wire format"; copycat_amd/csrc/wire.cpp)
CC_WIRE_ID_BOOLEAN = 129
CC_WIRE_ID_INTEGER = 132
CC_WIRE_ID_LONG = 133
CC_WIRE_ID_STRING = 136


class cc_wire_codec(C.Structure):
    _fields_ = [
        ("big_endian", C.c_uint8),
        ("utf8_presence_byte", C.c_uint8),
        ("utf8_len_bytes", C.c_uint8),
        ("reserved8", C.c_uint8),
        ("id_bool", C.c_int32),
        ("id_int", C.c_int32),
        ("id_long", C.c_int32),
        ("id_string", C.c_int32),
        ("reserved", C.c_uint64 * 4),
    ]


class cc_wire_out(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in ("inst", "iid", "op", "flags", "key", "a", "b", "aux", "kind")]


# the GPU wire decoder (include/copycat_apply.h "the same decode on the GPU"; copycat_amd/csrc/wire_gpu.hip)
CC_WIRE_TILE_ROWS = 2048

# the device split (include/copycat_apply.h "the same split and merge on the device"; copycat_amd/csrc/split_gpu.hip)
CC_SPLIT_TILE_ROWS = 4096

# the event merge (include/copycat_apply.h "the per-rank event streams back into log order"; csrc/evmerge.cpp,
# evmerge_gpu.hip; the prototypes are in engine.lib()'s table, as every call's):
#   cc_merge_events(parts, rows, row_counts, n, world, threads, out, total)
#   cc_merge_events_device_bound(n, world, work_bytes)
#   cc_merge_events_device(parts, d_rows, row_counts, n, world, d_out, total, d_work, work_bytes, stream)
CC_EVMERGE_TILE_ROWS = 4096
CC_EVMERGE_WINDOW_EVENTS = 1024

# the route (include/copycat_apply.h "an event stream to its client sessions"; csrc/route.cpp, route_gpu.hip):
#   cc_route_events(in, n_events, session_of_inst, id_of_inst, n_inst, n_sessions, threads, out, out_instance, dir,
#                   n_active)
#   cc_route_events_device_bound(n_events, n_sessions, work_bytes)
#   cc_route_events_device(d_in, n_events, d_session_of_inst, d_id_of_inst, n_inst, n_sessions, d_out, d_out_instance,
#                          d_dir, n_active, d_work, work_bytes, stream)
CC_ROUTE_DIGIT_BITS = 8
CC_ROUTE_TILE_EVENTS = 4096
CC_ROUTE_TIMING_SLOTS = 6


class cc_route_dir(C.Structure):
    _fields_ = [("session", C.c_void_p), ("start", C.c_void_p), ("capacity", C.c_uint64), ("count", C.c_void_p)]


class cc_snapshot_info_t(C.Structure):
    """What a snapshot was taken from (cc_snapshot_info)."""
    _fields_ = [("max_resources", C.c_uint32), ("max_instances", C.c_uint32), ("map_capacity", C.c_uint64),
                ("coord_cap", C.c_uint32), ("flags", C.c_uint32), ("applied", C.c_uint64)]


CC_SNAP_COORD, CC_SNAP_TTL, CC_SNAP_VALUE_RETAINED = 1, 2, 4  # cc_snapshot_info_t.flags

SNAPSHOT_GROW_PROTOTYPES = {
    # (h_buf, size, out)
    "cc_snapshot_info": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p]),
    # (e, h_buf, size)
    "cc_snapshot_restore_grow": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    # (enable, ms[3])
    "cc_snapshot_grow_timing": (C.c_int, [C.c_int, C.c_void_p]),
}


class cc_wire_control(C.Structure):
    _fields_ = [(name, C.c_uint64) for name in ("row", "kind", "key", "a", "b")]


# cc_apply_wire_host_packed's input (include/copycat_apply.h "the log segment through the pipeline")
class cc_wire_segment(C.Structure):
    _fields_ = [
        ("buf", C.c_void_p),
        ("buf_len", C.c_uint64),
        ("offsets", C.c_void_p),
        ("n", C.c_uint64),
        ("aux_blob", C.c_void_p),
        ("aux_bytes", C.c_uint64),
    ]


class cc_wire_stats(C.Structure):
    _fields_ = [(name, C.c_uint64) for name in ("rows", "device_rows", "host_rows")]


# the device String dictionary (include/copycat_apply.h "the device String dictionary")
CC_WIRE_STR_MAX = 256


class cc_wire_dict_info(C.Structure):
    _fields_ = [(name, C.c_uint64) for name in ("strings", "long_strings", "pool_bytes", "cells", "full_uploads",
                                                "last_sync_strings", "last_str_rows")]


# packed host batches (include/copycat_apply.h "packed host batches"; copycat_amd/csrc/pack.cpp, unpack.hip)
CC_PACK_BLOCK_ROWS = 4096
CC_PACK_VERSION = 1
CC_PACK_MAGIC = 1263551299
CC_PACK_COLUMNS = 9
CC_PK_FOR = 0
CC_PK_REL_A = 1
CC_PACKED_TIMELINE = 1


class cc_pack_header(C.Structure):
    _fields_ = [
        ("magic", C.c_uint32),
        ("version", C.c_uint32),
        ("n", C.c_uint64),
        ("blocks", C.c_uint64),
        ("bytes", C.c_uint64),
        ("present", C.c_uint32),
        ("block_rows", C.c_uint32),
        ("reserved", C.c_uint64 * 3),
    ]


class cc_pack_col(C.Structure):
    _fields_ = [
        ("mode", C.c_uint8),
        ("width", C.c_uint8),
        ("reserved16", C.c_uint16),
        ("offset", C.c_uint32),
        ("base", C.c_uint64),
    ]


class cc_pack_block(C.Structure):
    _fields_ = [("rows", C.c_uint32), ("bytes", C.c_uint32), ("offset", C.c_uint64), ("col", cc_pack_col * 9)]


# packed result blobs (include/copycat_apply.h "packed result blobs"; copycat_amd/csrc/respack.cpp, respack.hip)
CC_RESPACK_MAGIC = 1380991811
CC_RESPACK_VERSION = 1
CC_RESPACK_COLUMNS = 2
RESULT_COLUMNS = ("status", "value")  # cc_respack_block.col order


class cc_respack_block(C.Structure):
    _fields_ = [("rows", C.c_uint32), ("bytes", C.c_uint32), ("offset", C.c_uint64), ("col", cc_pack_col * 2)]


# packed event blobs (include/copycat_apply.h "packed event blobs"; copycat_amd/csrc/evpack.cpp, evpack.hip)
CC_EVPACK_MAGIC = 1162888003
CC_EVPACK_VERSION = 1
CC_EVPACK_COLUMNS = 6
CC_PK_BY_POS = 2
EVENT_COLUMNS = (("pos", "u4"), ("target", "u4"), ("code", "u1"), ("src", "u1"), ("tag", "u1"), ("payload", "u8"))  # col order


class cc_evpack_block(C.Structure):
    _fields_ = [("rows", C.c_uint32), ("bytes", C.c_uint32), ("offset", C.c_uint64), ("col", cc_pack_col * 6)]


# packed blobs both ways on the device (include/copycat_apply.h: cc_pack_from_device under "packed host batches",
# cc_respack_to_device under "packed result blobs", cc_evpack_to_device under "packed event blobs"; csrc/pack_enc.hip,
# unpack_res.hip).  name -> (result, arguments); engine.lib() binds them with the rest of its table.
PACK_DEVICE_PROTOTYPES = {
    # (e, d_cols, n, h_blob, cap, bytes, stream)
    "cc_pack_from_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    # (e, h_blob, bytes, d_out, stream)
    "cc_respack_to_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "cc_evpack_to_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
}


class cc_packed_opts(C.Structure):
    _fields_ = [
        ("chunk_rows", C.c_uint64),
        ("flags", C.c_uint32),
        ("reserved32", C.c_uint32),
        ("reserved", C.c_uint64 * 2),
    ]


BATCH_COLUMNS = (
    ("index", "u8"),
    ("time", "u8"),
    ("inst", "u4"),
    ("op", "u1"),
    ("flags", "u1"),
    ("key", "u8"),
    ("a", "u8"),
    ("b", "u8"),
    ("aux", "u8"),
)
