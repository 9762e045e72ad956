// evpack.cpp — packed event blobs: per-block base + narrow offsets for the six cc_events columns, and a payload table
// indexed by pos for fan-outs (include/copycat_apply.h "packed event blobs").  Host code only, no HIP call: the
// reference encoder, the validator and the decoder work on a machine with no GPU.
//
// The format over the shared core (pack_host.h): six columns, all always present, and besides CC_PK_FOR one mode of
// its own, CC_PK_BY_POS, on the payload.  cc_evpack_pack is the reference the GPU encoder (evpack.hip) is tested
// against byte for byte; cc_evpack_check is the one validator every consumer runs before it reads a directory entry;
// cc_evpack_unpack is the host decoder.  A block is 78 KiB of input.
#include "pack_host.h"

namespace {

using namespace cc::pk;

constexpr uint32_t kCols = CC_EVPACK_COLUMNS;
constexpr uint32_t kPos = 0, kPayload = 5;

static_assert(sizeof(cc_evpack_block) == 112, "evpack ABI");

struct Fmt : Format {
  using Block = cc_evpack_block;
  static constexpr const char* name = "event blob";
  static constexpr uint32_t magic = (uint32_t)CC_EVPACK_MAGIC, version = CC_EVPACK_VERSION, all = 0x3F;
  static constexpr uint32_t native[kCols] = {4, 4, 1, 1, 1, 8};  // pos, target, code, src, tag, payload
  static const char* present(uint32_t p) { return p != all ? "present is not 0x3F (the six event columns)" : nullptr; }
  static const char* mode(const cc_pack_header&, const Block& b, uint32_t c) {
    const uint8_t m = b.col[c].mode;
    if (m != CC_PK_FOR && m != CC_PK_BY_POS) return "a mode other than CC_PK_FOR and CC_PK_BY_POS";
    if (m == CC_PK_BY_POS && c != kPayload) return "CC_PK_BY_POS on a column other than payload";
    return nullptr;
  }
  static const char* units(const Block& b, uint32_t c, uint64_t* u) {  // (BY_POS: the table's entries)
    const cc_pack_col& e = b.col[c];
    *u = b.rows;
    if (e.mode != CC_PK_BY_POS) return nullptr;
    if (b.col[kPos].width > 2) return "CC_PK_BY_POS with a pos column wider than 2 bytes";
    if (e.width == 0) return "CC_PK_BY_POS with width 0";
    if (e.reserved16 < 1 || e.reserved16 > kRows) return "a CC_PK_BY_POS table of no entry or of more than 4096";
    *u = e.reserved16;
    return nullptr;
  }
  static const char* rows(const Block& b, const uint8_t* area) {
    const cc_pack_col& p = b.col[kPayload];
    if (p.mode != CC_PK_BY_POS || !b.col[kPos].width) return nullptr;  // (pos width 0: every offset is 0 < E)
    for (uint32_t i = 0; i < b.rows; ++i)
      if (get(area + b.col[kPos].offset, b.col[kPos].width, i) >= p.reserved16) return "a pos offset outside its CC_PK_BY_POS table";
    return nullptr;
  }
};

// a block's six directory entries and its area's bytes
cc_evpack_block measure(const cc_events* h, uint64_t r0, uint32_t m) {
  cc_evpack_block b{};
  b.rows = m;
  b.col[0] = choose_small(h->pos + r0, m);
  b.col[1] = choose_small(h->target + r0, m);
  b.col[2] = choose_small(h->code + r0, m);
  b.col[3] = choose_small(h->src + r0, m);
  b.col[4] = choose_small(h->tag + r0, m);
  cc_pack_col& p = b.col[kPayload];
  p = choose64(h->payload + r0, m);
  if (p.width && b.col[kPos].width <= 2) {  // a payload that is a function of a non-decreasing pos: a table by pos
    const uint32_t* pos = h->pos + r0;
    const uint64_t* pay = h->payload + r0;
    bool ok = true;
    for (uint32_t i = 1; i < m && ok; ++i) ok = pos[i] > pos[i - 1] || (pos[i] == pos[i - 1] && pay[i] == pay[i - 1]);
    const uint64_t E = (uint64_t)pos[m - 1] - pos[0] + 1;  // (non-decreasing: first = min, last = max)
    if (ok && r16(E * p.width) < r16((uint64_t)m * p.width)) p.mode = CC_PK_BY_POS, p.reserved16 = (uint16_t)E;
  }
  for (uint32_t c = 0; c < kCols; ++c) {
    b.col[c].offset = b.bytes;
    const uint64_t units = b.col[c].mode == CC_PK_BY_POS ? b.col[c].reserved16 : m;
    b.bytes += (uint32_t)r16(units * b.col[c].width);
  }
  return b;
}

void write_block(const cc_events* h, uint64_t r0, const cc_evpack_block& b, uint8_t* area) {
  const uint32_t m = b.rows;
  write_for(b.col[0], h->pos + r0, m, area + b.col[0].offset);
  write_for(b.col[1], h->target + r0, m, area + b.col[1].offset);
  write_for(b.col[2], h->code + r0, m, area + b.col[2].offset);
  write_for(b.col[3], h->src + r0, m, area + b.col[3].offset);
  write_for(b.col[4], h->tag + r0, m, area + b.col[4].offset);
  const cc_pack_col& p = b.col[kPayload];
  if (p.mode != CC_PK_BY_POS) return write_for(p, h->payload + r0, m, area + p.offset);
  uint8_t* const t = area + p.offset;
  const uint32_t pos_lo = (uint32_t)b.col[kPos].base;  // (pos width <= 2: the base is the block's smallest pos)
  std::memset(t, 0, r16((uint64_t)p.reserved16 * p.width));
  for (uint32_t i = 0; i < m; ++i) put(t, p.width, h->pos[r0 + i] - pos_lo, h->payload[r0 + i] - p.base);
}

}  // namespace

extern "C" int cc_evpack_bound(uint64_t n, uint64_t* bytes) {
  if (!bytes) return cc::pack_err(CC_ERR_INVALID, "event blob bound: null argument");
  if (n > (1ull << 48)) return cc::pack_err(CC_ERR_INVALID, "event blob bound: n too large");
  // every column raw (a table is taken only when it is smaller); a tail block's columns are each rounded up to 16 bytes
  *bytes = sizeof(cc_pack_header) + blocks_of(n) * sizeof(cc_evpack_block) + n * 19 + (n % kRows ? 16ull * kCols : 0);
  return CC_OK;
}

extern "C" int cc_evpack_pack(const cc_events* h, uint64_t n, void* h_blob, uint64_t cap, uint32_t threads,
                              uint64_t* bytes) {
  if (!h || !bytes || (cap && !h_blob) || (n && (!h->pos || !h->target || !h->code || !h->src || !h->tag || !h->payload)))
    return cc::pack_err(CC_ERR_INVALID, "event blob pack: null argument");
  if ((uintptr_t)h_blob & 15) return cc::pack_err(CC_ERR_INVALID, "event blob pack: the blob must be 16-byte aligned");
  if (n > (1ull << 48)) return cc::pack_err(CC_ERR_INVALID, "event blob pack: n too large");
  uint64_t bound = 0;
  (void)cc_evpack_bound(n, &bound);
  return encode<Fmt>(
      "event blob pack", n, Fmt::all, bound, h_blob, cap, threads, bytes,
      [&](uint64_t r0, uint32_t m) { return measure(h, r0, m); },
      [&](uint64_t r0, const cc_evpack_block& b, uint8_t* area) { write_block(h, r0, b, area); });
}

extern "C" int cc_evpack_check(const void* h_blob, uint64_t bytes, uint64_t* n) {
  cc_pack_header h;
  if (int rc = checked<Fmt>(h_blob, bytes, &h)) return rc;
  if (n) *n = h.n;
  return CC_OK;
}

extern "C" int cc_evpack_unpack(const void* h_blob, uint64_t bytes, const cc_events* out, uint32_t threads) {
  cc_pack_header h;
  if (int rc = checked<Fmt>(h_blob, bytes, &h)) return rc;
  if (!out || (h.n && (!out->pos || !out->target || !out->code || !out->src || !out->tag || !out->payload)))
    return cc::pack_err(CC_ERR_INVALID, "event blob unpack: null argument");
  if (out->capacity < h.n) return cc::pack_err(CC_ERR_CAPACITY, "event blob unpack: more events than h_out->capacity");
  decode<Fmt>(h_blob, h, threads, [&](uint64_t r0, const cc_evpack_block& b, const uint8_t* area) {
    read_for(b.col[0], area + b.col[0].offset, b.rows, out->pos + r0);
    read_for(b.col[1], area + b.col[1].offset, b.rows, out->target + r0);
    read_for(b.col[2], area + b.col[2].offset, b.rows, out->code + r0);
    read_for(b.col[3], area + b.col[3].offset, b.rows, out->src + r0);
    read_for(b.col[4], area + b.col[4].offset, b.rows, out->tag + r0);
    const cc_pack_col& p = b.col[kPayload];
    if (p.mode != CC_PK_BY_POS) return read_for(p, area + p.offset, b.rows, out->payload + r0);
    const uint8_t* const pos = area + b.col[kPos].offset;  // (the validator bounded every pos offset by the table)
    const uint8_t* const table = area + p.offset;
    for (uint32_t i = 0; i < b.rows; ++i)
      out->payload[r0 + i] = p.base + get(table, p.width, get(pos, b.col[kPos].width, i));
  });
  if (out->count) *out->count = h.n;
  return CC_OK;
}
