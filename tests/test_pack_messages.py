"""The exact text of every refusal of the three blob validators (cc_pack_check, cc_respack_check, cc_evpack_check).

The three share one validator (copycat_amd/csrc/pack_host.h) over a format description; a consumer may log or match
cc_last_error, so the texts are pinned here as literals, prefix included.  Per format: one well-formed blob of two blocks
(4,096 + 9 rows), one mutation per condition the validator tests, in the order it tests them.  (Its last condition,
"rows do not sum to n", cannot be reached: once the block count matches n and every block has the rows its place
demands, they do.)"""
import ctypes as C

import numpy as np
import pytest

from copycat_amd import abi
from copycat_amd.batch import _aligned_bytes, pack, pack_events, pack_results
from copycat_amd.engine import lib
from tests import evpack_cases as ec
from tests import pack_cases as pc

B = pc.B
N = B + 9
HDR = 64
ROWS, AREA_BYTES, AREA_OFFSET = 0, 4, 8        # a directory entry: rows u32, bytes u32, offset u64, then the columns
MODE, WIDTH, ENTRIES, OFFSET = 0, 1, 2, 4      # a column's entry: mode u8, width u8, reserved16, offset u32, base u64
REL_A, BY_POS = abi.CC_PK_REL_A, abi.CC_PK_BY_POS


def _put(blob, at, value, size):
    blob[at:at + size] = np.frombuffer(int(value).to_bytes(size, "little"), np.uint8)


def _get(blob, at, size):
    return int.from_bytes(blob[at:at + size].tobytes(), "little")


def _add(blob, at, delta, size):
    _put(blob, at, _get(blob, at, size) + delta, size)


def _col(c):
    return 16 + 16 * c


def _common(entry, other_magic):
    """The conditions every format words alike: (name, mutation, reason)."""
    e0, e1 = HDR, HDR + entry
    return [
        ("magic", lambda b: _put(b, 0, other_magic, 4), "bad magic"),
        ("version", lambda b: _put(b, 4, 2, 4), "unknown format version"),
        ("header_block_rows", lambda b: _put(b, 36, 2048, 4), "block_rows is not CC_PACK_BLOCK_ROWS"),
        ("bytes_more", lambda b: _add(b, 24, 16, 8), "total bytes larger than the buffer"),
        ("bytes_tiny", lambda b: _put(b, 24, 32, 8), "total bytes shorter than the header"),
        ("blocks", lambda b: _put(b, 16, 3, 8), "block count does not match n"),
        ("n", lambda b: _add(b, 8, B, 8), "block count does not match n"),
        ("directory", lambda b: _put(b, 24, HDR + entry, 8), "directory outside the blob"),
        ("block_rows", lambda b: _put(b, e0 + ROWS, B - 1, 4),
         "a block's rows are not CC_PACK_BLOCK_ROWS (or the tail's): rows do not sum to n"),
        ("tail_rows", lambda b: _add(b, e1 + ROWS, 1, 4),
         "a block's rows are not CC_PACK_BLOCK_ROWS (or the tail's): rows do not sum to n"),
        ("n_plus_one", lambda b: _add(b, 8, 1, 8),
         "a block's rows are not CC_PACK_BLOCK_ROWS (or the tail's): rows do not sum to n"),
        ("area_offset_misaligned", lambda b: _add(b, e1 + AREA_OFFSET, 8, 8), "a block's data area is not 16-byte aligned"),
        ("area_bytes_misaligned", lambda b: _add(b, e0 + AREA_BYTES, 8, 4), "a block's data area is not 16-byte aligned"),
        ("area_in_directory", lambda b: _put(b, e0 + AREA_OFFSET, HDR, 8),
         "a block's data area overlaps the directory or an earlier block"),
        ("area_overlaps", lambda b: _put(b, e1 + AREA_OFFSET, _get(b, e0 + AREA_OFFSET, 8), 8),
         "a block's data area overlaps the directory or an earlier block"),
        ("area_outside", lambda b: _put(b, e1 + AREA_OFFSET, _get(b, 24, 8), 8), "a block's data area is outside the blob"),
        ("area_too_long", lambda b: _add(b, e1 + AREA_BYTES, 16, 4), "a block's data area is outside the blob"),
    ]


# ---- the batch blob ------------------------------------------------------------------------------------------------------
PK = 160
COL = {name: _col(c) for c, (name, _) in enumerate(abi.BATCH_COLUMNS)}


def _batch(columns=pc.ALL):
    b = pc.random_batch(N, 11)
    b.inst[:] = b.inst % 1000 + 5  # (inst at width 2, so a wider width can be written into its entry)
    return pack(b, columns=columns)


def _rel(at, width):
    def mutate(b):
        _put(b, at + MODE, REL_A, 1)
        _put(b, at + WIDTH, width, 1)
    return mutate


PACK = _common(PK, abi.CC_RESPACK_MAGIC) + [
    ("present", lambda b: _put(b, 32, 0x3FF, 4), "present mask names a column past aux"),
    ("rel_a_on_key", _rel(HDR + COL["key"], 1), "REL_A on a column other than b"),
    ("rel_a_width_8", _rel(HDR + COL["b"], 8), "REL_A width is not 1, 2 or 4"),
    ("width_3", lambda b: _put(b, HDR + COL["key"] + WIDTH, 3, 1), "width is not 0, 1, 2, 4 or 8"),
    ("inst_width_8", lambda b: _put(b, HDR + COL["inst"] + WIDTH, 8, 1), "width above the column's native width"),
    ("op_width_2", lambda b: _put(b, HDR + PK + COL["op"] + WIDTH, 2, 1), "width above the column's native width"),
    ("mode_2", lambda b: _put(b, HDR + COL["key"] + MODE, 2, 1), "unknown mode"),
    ("column_misaligned", lambda b: _add(b, HDR + PK + COL["key"] + OFFSET, 8, 4), "a column's offset is not 16-byte aligned"),
    ("column_outside", lambda b: _put(b, HDR + COL["a"] + OFFSET, _get(b, HDR + AREA_BYTES, 4), 4),
     "a column's rows are outside its block's data area"),
    ("columns_overlap", lambda b: _put(b, HDR + COL["a"] + OFFSET, _get(b, HDR + COL["index"] + OFFSET, 4), 4),
     "two columns' rows overlap"),
]


# ---- the result blob -----------------------------------------------------------------------------------------------------
RS = 48
STATUS, VALUE = _col(0), _col(1)


def _results():
    """Status raw and value 2 bytes wide in both blocks, so both columns have rows to overlap."""
    status = (np.arange(N) % 3 * 0x10).astype(np.uint8)
    value = (np.arange(N, dtype=np.uint64) * np.uint64(7)) % np.uint64(50000) + np.uint64(1 << 33)
    return pack_results(status, value)


RESULT = _common(RS, abi.CC_PACK_MAGIC) + [
    ("present", lambda b: _put(b, 32, 1, 4), "present is not 3 (status and value)"),
    ("mode_rel_a", lambda b: _put(b, HDR + VALUE + MODE, REL_A, 1), "a mode other than CC_PK_FOR"),
    ("value_width_3", lambda b: _put(b, HDR + VALUE + WIDTH, 3, 1), "width is not 0, 1, 2, 4 or 8"),
    ("status_width_2", lambda b: _put(b, HDR + STATUS + WIDTH, 2, 1), "width above the column's native width"),
    ("column_misaligned", lambda b: _add(b, HDR + VALUE + OFFSET, 8, 4), "a column's offset is not 16-byte aligned"),
    ("column_outside", lambda b: _put(b, HDR + RS + VALUE + OFFSET, _get(b, HDR + RS + AREA_BYTES, 4), 4),
     "a column's rows are outside its block's data area"),
    ("columns_overlap", lambda b: _put(b, HDR + VALUE + OFFSET, 0, 4), "the two columns' rows overlap"),
]


# ---- the event blob ------------------------------------------------------------------------------------------------------
EV = 112
POS, TARGET, CODE, PAYLOAD = _col(0), _col(1), _col(2), _col(5)


def _events():
    """A fan-out (pos 1 byte, target 2, payload a table of 64 entries, each referred to), then a tail of 9 rows with pos
    4 bytes wide, target 2, the three byte columns raw and payload 2."""
    mixed = (np.arange(9) % 3).astype(np.uint8)
    tail = ec.events(np.array([5, 90000] * 4 + [5], np.uint32), target=np.arange(7, 7 + 9 * 30, 30, dtype=np.uint32),
                     code=mixed, src=mixed, tag=mixed, payload=np.uint64(1 << 33) + np.arange(9, dtype=np.uint64) * np.uint64(5000))
    return pack_events(ec.concat([ec.fanout(64, 64, seed=9), tail]))


EVENT = _common(EV, abi.CC_RESPACK_MAGIC) + [
    ("present", lambda b: _put(b, 32, 3, 4), "present is not 0x3F (the six event columns)"),
    ("mode_rel_a", lambda b: _put(b, HDR + PAYLOAD + MODE, REL_A, 1), "a mode other than CC_PK_FOR and CC_PK_BY_POS"),
    ("by_pos_on_target", lambda b: _put(b, HDR + TARGET + MODE, BY_POS, 1), "CC_PK_BY_POS on a column other than payload"),
    ("payload_width_3", lambda b: _put(b, HDR + EV + PAYLOAD + WIDTH, 3, 1), "width is not 0, 1, 2, 4 or 8"),
    ("pos_width_8", lambda b: _put(b, HDR + POS + WIDTH, 8, 1), "width above the column's native width"),
    ("code_width_2", lambda b: _put(b, HDR + EV + CODE + WIDTH, 2, 1), "width above the column's native width"),
    ("column_misaligned", lambda b: _add(b, HDR + TARGET + OFFSET, 8, 4), "a column's offset is not 16-byte aligned"),
    ("by_pos_with_pos_width_4", lambda b: _put(b, HDR + EV + PAYLOAD + MODE, BY_POS, 1),
     "CC_PK_BY_POS with a pos column wider than 2 bytes"),
    ("by_pos_width_0", lambda b: _put(b, HDR + PAYLOAD + WIDTH, 0, 1), "CC_PK_BY_POS with width 0"),
    ("by_pos_entries_0", lambda b: _put(b, HDR + PAYLOAD + ENTRIES, 0, 2), "a CC_PK_BY_POS table of no entry or of more than 4096"),
    ("by_pos_entries_4097", lambda b: _put(b, HDR + PAYLOAD + ENTRIES, 4097, 2),
     "a CC_PK_BY_POS table of no entry or of more than 4096"),
    ("column_outside", lambda b: _put(b, HDR + TARGET + OFFSET, _get(b, HDR + AREA_BYTES, 4), 4),
     "a column's rows are outside its block's data area"),
    ("columns_overlap", lambda b: _put(b, HDR + TARGET + OFFSET, 0, 4), "two columns' rows overlap"),
    ("by_pos_entries_below_a_pos_offset", lambda b: _put(b, HDR + PAYLOAD + ENTRIES, 63, 2),
     "a pos offset outside its CC_PK_BY_POS table"),
]


FORMATS = {
    "packed blob": (_batch, PACK, lambda L, p, n: L.cc_pack_check(p, n, None, None)),
    "result blob": (_results, RESULT, lambda L, p, n: L.cc_respack_check(p, n, None)),
    "event blob": (_events, EVENT, lambda L, p, n: L.cc_evpack_check(p, n, None)),
}
_GOOD = {}


def _good(prefix):
    if prefix not in _GOOD:
        _GOOD[prefix] = FORMATS[prefix][0]()
    out = _aligned_bytes(len(_GOOD[prefix]))
    out[:] = _GOOD[prefix]
    return out


def _says(prefix, ptr, nbytes, reason):
    L = lib()
    assert FORMATS[prefix][2](L, ptr, nbytes) == abi.CC_ERR_INVALID
    assert L.cc_last_error().decode() == f"{prefix}: {reason}"


CASES = [(prefix, name, mutate, reason) for prefix, (_, muts, _) in FORMATS.items() for name, mutate, reason in muts]


@pytest.mark.parametrize("prefix,name,mutate,reason", CASES, ids=[f"{c[0].split()[0]}-{c[1]}" for c in CASES])
def test_refusal_text(prefix, name, mutate, reason):
    blob = _good(prefix)
    assert FORMATS[prefix][2](lib(), blob.ctypes.data, len(blob)) == abi.CC_OK
    assert _get(blob, 8, 8) == N and _get(blob, 16, 8) == 2
    mutate(blob)
    _says(prefix, blob.ctypes.data, len(blob), reason)


@pytest.mark.parametrize("prefix", list(FORMATS))
def test_refusal_text_of_the_buffer_itself(prefix):
    blob = _good(prefix)
    _says(prefix, None, len(blob), "null pointer")
    shifted = _aligned_bytes(len(blob) + 16)[8:8 + len(blob)]
    shifted[:] = blob
    _says(prefix, shifted.ctypes.data, len(blob), "not 16-byte aligned")
    _says(prefix, blob.ctypes.data, HDR - 1, "shorter than its header")
    _says(prefix, blob.ctypes.data, len(blob) - 16, "total bytes larger than the buffer")


def test_refusal_text_rel_a_without_a():
    packed = _batch(columns=("inst", "op", "flags", "b"))
    blob = _aligned_bytes(len(packed))
    blob[:] = packed
    _rel(HDR + COL["b"], 1)(blob)
    _says("packed blob", blob.ctypes.data, len(blob), "REL_A without column a")
