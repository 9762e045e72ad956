// value_group.h — the group / segment arithmetic of the value-only apply (apply_batch.hip, value_path.hip).  Host
// code without a HIP call, so the C entry points over it (cc_value_group_*) run on a machine without a GPU.
//
// A value-only call is cut twice.  A *segment* is the stretch one LDS run table of k_apply_value_v3 covers: at most
// kV3MaxTiles tiles, the engine's sub-batch.  A *group* is the stretch one k_part_v4 launch and one k_unpermute_v3
// launch cover: whole segments (the last one of a call may be short), as many as the group staging holds.  The
// partition's output is tile-local (records, cpos and the ttab row of tile T depend on tile T alone), so segment j of
// a group is the group's staging arrays from tile j * seg_tiles on; positions inside it, the dummy rows' among them,
// are counted from that tile.
#pragma once
#include <cstdint>
#include <cstdlib>

#include "common.h"

namespace cc {

// Staging positions a group may hold.  k_apply_value_v3 keeps positions and their byte offsets in 32 bits (v3_at:
// position * 8 < 2^32) and reads and writes kVgDummyRows dummy rows behind the staging area, so the first dummy
// position + kVgDummyRows stays at or below 2^29 (launch_apply_value_v3 checks the same).
constexpr uint64_t kVgPosLimit = 1ull << 29;
constexpr uint64_t kVgDummyRows = 1024;                // one per thread of the apply's workgroup
constexpr uint64_t kVgMaxRows = kVgPosLimit - 4096;    // the upper limit of a group, before rounding to segments
constexpr uint64_t kVgNoCap = ~0ull;                   // CC_VALUE_GROUP_TILES unset: groups as large as the limit allows

// CC_VALUE_GROUP_TILES as text: unset or empty -> kVgNoCap; "0" -> 0 (the per-sub-batch path); "k" -> k tiles.
// Anything else (a sign, a letter, a number past 2^32) is refused, not guessed at.
inline bool vg_parse_knob(const char* text, uint64_t& tiles) {
  tiles = kVgNoCap;
  if (!text || !*text) return true;
  uint64_t v = 0;
  for (const char* p = text; *p; ++p) {
    if (*p < '0' || *p > '9') return false;
    v = v * 10 + (uint64_t)(*p - '0');
    if (v > 0xFFFFFFFFull) return false;
  }
  tiles = v;
  return true;
}

// Rows one group covers at most: whole segments of seg_rows rows (a multiple of the tile), at least one, at most
// what kVgMaxRows and the knob (tiles, rounded down to whole segments) allow.  0: the knob is 0.
inline uint64_t vg_group_rows(uint64_t seg_rows, uint64_t knob_tiles) {
  if (knob_tiles == 0 || seg_rows == 0) return 0;
  uint64_t segs = kVgMaxRows / seg_rows;
  if (knob_tiles != kVgNoCap) {
    const uint64_t k = knob_tiles / (seg_rows / kV3Tile);
    segs = k < segs ? k : segs;
  }
  return (segs ? segs : 1) * seg_rows;
}

struct VgPlan {
  uint64_t group_rows;    // rows per group at most (0: the per-sub-batch path)
  uint64_t groups;        // groups a call of n rows runs
  uint64_t staging_rows;  // positions the group staging needs for it: min(n, max_batch, group_rows) in whole tiles
};
// false: the sizes make no plan (seg_rows no multiple of the tile, or past kV3MaxTiles tiles)
inline bool vg_plan(uint64_t n, uint64_t seg_rows, uint64_t max_batch, uint64_t knob_tiles, VgPlan& p) {
  p = VgPlan{0, 0, 0};
  if (seg_rows == 0 || seg_rows % kV3Tile || seg_rows / kV3Tile > (uint64_t)kV3MaxTiles) return false;
  p.group_rows = vg_group_rows(seg_rows, knob_tiles);
  if (!p.group_rows) return true;
  p.groups = (n + p.group_rows - 1) / p.group_rows;
  uint64_t rows = n < p.group_rows ? n : p.group_rows;
  if (max_batch && max_batch < rows) rows = max_batch;
  p.staging_rows = (rows + kV3Tile - 1) / kV3Tile * kV3Tile;
  return true;
}

struct VgSegment {
  uint64_t row0;   // first row, counted from the group's first
  uint64_t rows;
  uint64_t tile0;  // first tile of the group's staging arrays
  uint64_t tiles;
  uint64_t dummy;  // first dummy position, counted from tile0's first position
};
inline uint64_t vg_segments(uint64_t rows, uint64_t seg_rows) { return (rows + seg_rows - 1) / seg_rows; }
// Segment j of a group of `rows` rows staged in arrays of staging_rows positions.  CC_ERR_CAPACITY when the group
// does not fit its staging or its dummy rows would pass kVgPosLimit (never a wrapped 32-bit position);
// CC_ERR_INVALID for a segment the group does not have.
inline int vg_segment(uint64_t rows, uint64_t seg_rows, uint64_t staging_rows, uint64_t j, VgSegment& s) {
  s = VgSegment{0, 0, 0, 0, 0};
  if (seg_rows == 0 || seg_rows % kV3Tile || seg_rows / kV3Tile > (uint64_t)kV3MaxTiles || staging_rows % kV3Tile)
    return CC_ERR_INVALID;
  if (staging_rows > kVgPosLimit - kVgDummyRows || rows > staging_rows) return CC_ERR_CAPACITY;
  if (j >= vg_segments(rows, seg_rows)) return CC_ERR_INVALID;
  s.row0 = j * seg_rows;
  s.rows = rows - s.row0 < seg_rows ? rows - s.row0 : seg_rows;
  s.tile0 = s.row0 / kV3Tile;
  s.tiles = (s.rows + kV3Tile - 1) / kV3Tile;
  s.dummy = staging_rows - s.row0;
  return CC_OK;
}

}  // namespace cc
