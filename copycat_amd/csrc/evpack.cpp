// evpack.cpp — packed event blobs: per-block base + narrow offsets for the six cc_events columns, and a payload table
// indexed by pos for fan-outs (include/copycat_apply.h "packed event blobs").  Host code only, no HIP call: the
// reference encoder, the validator and the decoder work on a machine with no GPU.
//
// The format is the result blob's (respack.cpp) widened to six columns, with one more mode, CC_PK_BY_POS.
// cc_evpack_pack is the reference the GPU encoder (evpack.hip) is tested against byte for byte; cc_evpack_check is the
// one validator every consumer runs before it reads a directory entry; cc_evpack_unpack is the host decoder.
//
// cc_evpack_pack is one pass, as cc_respack_pack: a thread takes the next block, measures its six columns (78 KiB of
// input, in cache), sizes the block's data area, takes its place in the blob in block order (a ticket) and writes the
// narrow rows.  The layout depends on the event columns alone, never on the thread count.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/copycat_apply.h"

namespace cc {
int pack_err(int code, const char* what);  // the engine's cc_last_error store (unpack.hip)
}

namespace {

constexpr uint32_t kRows = CC_PACK_BLOCK_ROWS;
constexpr uint32_t kCols = CC_EVPACK_COLUMNS;
constexpr uint32_t kNative[kCols] = {4, 4, 1, 1, 1, 8};  // pos, target, code, src, tag, payload
constexpr uint32_t kPos = 0, kPayload = 5;

static_assert(sizeof(cc_pack_header) == 64 && sizeof(cc_pack_col) == 16 && sizeof(cc_evpack_block) == 112, "evpack ABI");

inline uint64_t r16(uint64_t x) { return (x + 15) & ~15ull; }
inline uint64_t blocks_of(uint64_t n) { return n / kRows + (n % kRows != 0); }
inline uint8_t width_of(uint64_t span) {
  return span == 0 ? 0 : span <= 0xFFu ? 1 : span <= 0xFFFFu ? 2 : span <= 0xFFFFFFFFull ? 4 : 8;
}

uint32_t pick_threads(uint32_t threads, uint64_t blocks) {
  uint32_t t = threads ? threads : std::max(1u, std::thread::hardware_concurrency());
  t = std::min<uint32_t>(t, 256);
  return (uint32_t)std::min<uint64_t>(t, std::max<uint64_t>(1, blocks / 4));  // no thread for less than 4 blocks
}

template <class F>
void parallel(uint32_t threads, F f) {
  if (threads == 1) {
    f(0u);
    return;
  }
  std::vector<std::thread> th;
  th.reserve(threads);
  for (uint32_t t = 0; t < threads; ++t) th.emplace_back(f, t);
  for (auto& x : th) x.join();
}

// one offset of a narrow image
inline uint64_t get(const uint8_t* in, uint32_t w, uint64_t i) {
  switch (w) {
    case 1: return in[i];
    case 2: { uint16_t x; std::memcpy(&x, in + 2 * i, 2); return x; }
    case 4: { uint32_t x; std::memcpy(&x, in + 4 * i, 4); return x; }
    case 8: { uint64_t x; std::memcpy(&x, in + 8 * i, 8); return x; }
    default: return 0;
  }
}
inline void put(uint8_t* out, uint32_t w, uint64_t i, uint64_t v) {  // (little-endian hosts: the low w bytes)
  std::memcpy(out + (uint64_t)w * i, &v, w);
}

// ---- encoder ---------------------------------------------------------------------------------------------------------
// pos / target: base = the unsigned minimum; the native width is the raw column
cc_pack_col choose_u32(const uint32_t* v, uint32_t m, uint32_t* lo_out) {
  uint32_t lo = v[0], hi = v[0];
  for (uint32_t i = 1; i < m; ++i) lo = std::min(lo, v[i]), hi = std::max(hi, v[i]);
  cc_pack_col c{};
  c.mode = CC_PK_FOR;
  c.width = width_of(hi - lo);
  c.base = c.width == 4 ? 0 : lo;
  *lo_out = lo;
  return c;
}

cc_pack_col choose_u8(const uint8_t* v, uint32_t m) {
  uint8_t lo = v[0], hi = v[0];
  for (uint32_t i = 1; i < m; ++i) lo = std::min(lo, v[i]), hi = std::max(hi, v[i]);
  cc_pack_col c{};
  c.mode = CC_PK_FOR;
  c.width = hi != lo;
  c.base = c.width ? 0 : lo;
  return c;
}

// the narrowest exact encoding of one block's payloads: base = the unsigned or the signed minimum, ties to the unsigned
cc_pack_col choose_payload(const uint64_t* v, uint32_t m) {
  uint64_t ulo = v[0], uhi = v[0];
  int64_t slo = (int64_t)v[0], shi = (int64_t)v[0];
  for (uint32_t i = 1; i < m; ++i) {
    ulo = std::min(ulo, v[i]), uhi = std::max(uhi, v[i]);
    slo = std::min(slo, (int64_t)v[i]), shi = std::max(shi, (int64_t)v[i]);
  }
  cc_pack_col c{};
  c.mode = CC_PK_FOR;
  c.width = width_of(uhi - ulo);
  c.base = ulo;
  const uint8_t ws = width_of((uint64_t)shi - (uint64_t)slo);
  if (ws < c.width) c.width = ws, c.base = (uint64_t)slo;
  if (c.width == 8) c.base = 0;  // the native width is the raw column
  return c;
}

// a block's six directory entries and its area's bytes; *pos_lo = the block's smallest pos
void measure(const cc_events* h, uint64_t r0, uint32_t m, cc_evpack_block* b, uint32_t* pos_lo) {
  uint32_t tlo;
  b->rows = m;
  b->col[0] = choose_u32(h->pos + r0, m, pos_lo);
  b->col[1] = choose_u32(h->target + r0, m, &tlo);
  b->col[2] = choose_u8(h->code + r0, m);
  b->col[3] = choose_u8(h->src + r0, m);
  b->col[4] = choose_u8(h->tag + r0, m);
  cc_pack_col& p = b->col[kPayload];
  p = choose_payload(h->payload + r0, m);
  if (p.width && b->col[kPos].width <= 2) {  // a payload that is a function of a non-decreasing pos: a table by pos
    const uint32_t* pos = h->pos + r0;
    const uint64_t* pay = h->payload + r0;
    bool ok = true;
    for (uint32_t i = 1; i < m && ok; ++i) ok = pos[i] > pos[i - 1] || (pos[i] == pos[i - 1] && pay[i] == pay[i - 1]);
    const uint64_t E = (uint64_t)pos[m - 1] - pos[0] + 1;  // (non-decreasing: first = min, last = max)
    if (ok && r16(E * p.width) < r16((uint64_t)m * p.width)) p.mode = CC_PK_BY_POS, p.reserved16 = (uint16_t)E;
  }
  uint32_t at = 0;
  for (uint32_t c = 0; c < kCols; ++c) {
    b->col[c].offset = at;
    const uint64_t units = b->col[c].mode == CC_PK_BY_POS ? b->col[c].reserved16 : m;
    at += (uint32_t)r16(units * b->col[c].width);
  }
  b->bytes = at;
}

template <class T>
void write_for(const cc_pack_col& c, const T* v, uint32_t m, uint8_t* out) {
  if (!c.width) return;
  const size_t used = (size_t)m * c.width;
  if (c.width == sizeof(T)) std::memcpy(out, v, used);
  else
    for (uint32_t i = 0; i < m; ++i) put(out, c.width, i, (uint64_t)v[i] - c.base);
  std::memset(out + used, 0, r16(used) - used);  // (the blob is byte-for-byte a function of the input)
}

void write_block(const cc_events* h, uint64_t r0, const cc_evpack_block& b, uint32_t pos_lo, uint8_t* area) {
  const uint32_t m = b.rows;
  write_for(b.col[0], h->pos + r0, m, area + b.col[0].offset);
  write_for(b.col[1], h->target + r0, m, area + b.col[1].offset);
  write_for(b.col[2], h->code + r0, m, area + b.col[2].offset);
  write_for(b.col[3], h->src + r0, m, area + b.col[3].offset);
  write_for(b.col[4], h->tag + r0, m, area + b.col[4].offset);
  const cc_pack_col& p = b.col[kPayload];
  if (p.mode != CC_PK_BY_POS) {
    write_for(p, h->payload + r0, m, area + p.offset);
    return;
  }
  uint8_t* const t = area + p.offset;
  std::memset(t, 0, r16((uint64_t)p.reserved16 * p.width));
  for (uint32_t i = 0; i < m; ++i) put(t, p.width, h->pos[r0 + i] - pos_lo, h->payload[r0 + i] - p.base);
}

// ---- validator -------------------------------------------------------------------------------------------------------
// nullptr: the blob is well formed
const char* check(const void* blob, uint64_t bytes) {
  if (!blob) return "event blob: null pointer";
  if ((uintptr_t)blob & 15) return "event blob: not 16-byte aligned";
  if (bytes < sizeof(cc_pack_header)) return "event blob: shorter than its header";
  cc_pack_header h;
  std::memcpy(&h, blob, sizeof h);
  if (h.magic != (uint32_t)CC_EVPACK_MAGIC) return "event blob: bad magic";
  if (h.version != CC_EVPACK_VERSION) return "event blob: unknown format version";
  if (h.block_rows != kRows) return "event blob: block_rows is not CC_PACK_BLOCK_ROWS";
  if (h.present != 0x3F) return "event blob: present is not 0x3F (the six event columns)";
  if (h.bytes > bytes) return "event blob: total bytes larger than the buffer";
  if (h.bytes < sizeof(cc_pack_header)) return "event blob: total bytes shorter than the header";
  if (h.blocks != blocks_of(h.n)) return "event blob: block count does not match n";
  if (h.blocks > (h.bytes - sizeof(cc_pack_header)) / sizeof(cc_evpack_block)) return "event blob: directory outside the blob";
  const uint8_t* dir = (const uint8_t*)blob + sizeof(cc_pack_header);
  uint64_t prev_end = sizeof(cc_pack_header) + h.blocks * sizeof(cc_evpack_block), rows_sum = 0;
  for (uint64_t k = 0; k < h.blocks; ++k) {
    cc_evpack_block b;
    std::memcpy(&b, dir + k * sizeof b, sizeof b);
    const uint64_t want = std::min<uint64_t>(kRows, h.n - k * kRows);
    if (b.rows != want) return "event blob: a block's rows are not CC_PACK_BLOCK_ROWS (or the tail's): rows do not sum to n";
    rows_sum += b.rows;
    if ((b.offset & 15) || (b.bytes & 15)) return "event blob: a block's data area is not 16-byte aligned";
    if (b.offset < prev_end) return "event blob: a block's data area overlaps the directory or an earlier block";
    if (b.offset > h.bytes || b.bytes > h.bytes - b.offset) return "event blob: a block's data area is outside the blob";
    prev_end = b.offset + b.bytes;
    uint64_t lo[kCols], hi[kCols];
    for (uint32_t c = 0; c < kCols; ++c) {
      const cc_pack_col& e = b.col[c];
      if (e.mode != CC_PK_FOR && e.mode != CC_PK_BY_POS) return "event blob: a mode other than CC_PK_FOR and CC_PK_BY_POS";
      if (e.mode == CC_PK_BY_POS && c != kPayload) return "event blob: CC_PK_BY_POS on a column other than payload";
      if (e.width != 0 && e.width != 1 && e.width != 2 && e.width != 4 && e.width != 8)
        return "event blob: width is not 0, 1, 2, 4 or 8";
      if (e.width > kNative[c]) return "event blob: width above the column's native width";
      if (e.offset & 15) return "event blob: a column's offset is not 16-byte aligned";
      uint64_t units = b.rows;
      if (e.mode == CC_PK_BY_POS) {
        if (b.col[kPos].width > 2) return "event blob: CC_PK_BY_POS with a pos column wider than 2 bytes";
        if (e.width == 0) return "event blob: CC_PK_BY_POS with width 0";
        if (e.reserved16 < 1 || e.reserved16 > kRows) return "event blob: a CC_PK_BY_POS table of no entry or of more than 4096";
        units = e.reserved16;
      }
      const uint64_t len = r16(units * e.width);  // (BY_POS: the table's bytes, r16(E * width))
      if (e.offset > b.bytes || len > b.bytes - e.offset) return "event blob: a column's rows are outside its block's data area";
      lo[c] = e.offset, hi[c] = e.offset + len;
    }
    for (uint32_t c = 0; c < kCols; ++c)
      for (uint32_t d = c + 1; d < kCols; ++d)
        if (lo[c] < hi[c] && lo[d] < hi[d] && lo[c] < hi[d] && lo[d] < hi[c]) return "event blob: two columns' rows overlap";
    const cc_pack_col& p = b.col[kPayload];
    if (p.mode == CC_PK_BY_POS && b.col[kPos].width) {  // (pos width 0: every offset is 0 < E)
      const uint8_t* pos = (const uint8_t*)blob + b.offset + b.col[kPos].offset;
      for (uint32_t i = 0; i < b.rows; ++i)
        if (get(pos, b.col[kPos].width, i) >= p.reserved16) return "event blob: a pos offset outside its CC_PK_BY_POS table";
    }
  }
  if (rows_sum != h.n) return "event blob: rows do not sum to n";
  return nullptr;
}

// ---- decoder ---------------------------------------------------------------------------------------------------------
template <class T>
void read_for(const cc_pack_col& c, const uint8_t* in, uint32_t m, T* out) {
  if (c.width == 0) std::fill(out, out + m, (T)c.base);
  else if (c.width == sizeof(T)) {
    std::memcpy(out, in, (size_t)m * sizeof(T));
    if (c.base)
      for (uint32_t i = 0; i < m; ++i) out[i] = (T)(out[i] + c.base);
  } else
    for (uint32_t i = 0; i < m; ++i) out[i] = (T)(c.base + get(in, c.width, i));
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
  const uint64_t blocks = blocks_of(n);
  const uint64_t dir_end = sizeof(cc_pack_header) + blocks * sizeof(cc_evpack_block);
  uint8_t* const blob = (uint8_t*)h_blob;
  std::atomic<uint64_t> next{0}, turn{0};
  uint64_t cursor = dir_end;  // written by the thread whose turn it is
  // A cap too small writes nothing, so a pass sizes the blob first whenever the cap is below the bound (the measuring
  // pass alone); a caller that passes cc_evpack_bound never pays it.
  uint64_t bound = 0;
  (void)cc_evpack_bound(n, &bound);
  for (int pass = cap >= bound ? 1 : 0; pass < 2; ++pass) {
    const bool write = pass == 1;
    next = 0, turn = 0, cursor = dir_end;
    parallel(pick_threads(threads, blocks), [&](uint32_t) {
      for (;;) {
        const uint64_t k = next.fetch_add(1, std::memory_order_relaxed);
        if (k >= blocks) return;
        const uint64_t r0 = k * kRows;
        const uint32_t m = (uint32_t)std::min<uint64_t>(kRows, n - r0);
        cc_evpack_block b{};
        uint32_t pos_lo = 0;
        measure(h, r0, m, &b, &pos_lo);
        // (with more threads than cores the thread whose turn it is may not be running: give the core away)
        for (uint32_t spins = 0; turn.load(std::memory_order_acquire) != k; ++spins)
          if (spins >= 64) std::this_thread::yield();
        b.offset = cursor;
        cursor += b.bytes;
        turn.store(k + 1, std::memory_order_release);
        if (!write) continue;
        std::memcpy(blob + sizeof(cc_pack_header) + k * sizeof b, &b, sizeof b);
        write_block(h, r0, b, pos_lo, blob + b.offset);
      }
    });
    *bytes = cursor;
    if (cursor > cap) return cc::pack_err(CC_ERR_CAPACITY, "event blob pack: the blob buffer is too small (*bytes = the size needed)");
  }
  cc_pack_header hd{};
  hd.magic = (uint32_t)CC_EVPACK_MAGIC;
  hd.version = CC_EVPACK_VERSION;
  hd.n = n;
  hd.blocks = blocks;
  hd.bytes = cursor;
  hd.present = 0x3F;
  hd.block_rows = kRows;
  std::memcpy(blob, &hd, sizeof hd);
  return CC_OK;
}

extern "C" int cc_evpack_check(const void* h_blob, uint64_t bytes, uint64_t* n) {
  if (const char* why = check(h_blob, bytes)) return cc::pack_err(CC_ERR_INVALID, why);
  if (n) {
    cc_pack_header h;
    std::memcpy(&h, h_blob, sizeof h);
    *n = h.n;
  }
  return CC_OK;
}

extern "C" int cc_evpack_unpack(const void* h_blob, uint64_t bytes, const cc_events* out, uint32_t threads) {
  if (const char* why = check(h_blob, bytes)) return cc::pack_err(CC_ERR_INVALID, why);
  cc_pack_header h;
  std::memcpy(&h, h_blob, sizeof h);
  if (!out || (h.n && (!out->pos || !out->target || !out->code || !out->src || !out->tag || !out->payload)))
    return cc::pack_err(CC_ERR_INVALID, "event blob unpack: null argument");
  if (out->capacity < h.n) return cc::pack_err(CC_ERR_CAPACITY, "event blob unpack: more events than h_out->capacity");
  const uint8_t* const blob = (const uint8_t*)h_blob;
  const uint32_t T = pick_threads(threads, h.blocks);
  parallel(T, [&](uint32_t t) {
    for (uint64_t k = h.blocks * t / T; k < h.blocks * (t + 1) / T; ++k) {
      cc_evpack_block b;
      std::memcpy(&b, blob + sizeof h + k * sizeof b, sizeof b);
      const uint64_t r0 = k * kRows;
      const uint8_t* const area = blob + b.offset;
      read_for(b.col[0], area + b.col[0].offset, b.rows, out->pos + r0);
      read_for(b.col[1], area + b.col[1].offset, b.rows, out->target + r0);
      read_for(b.col[2], area + b.col[2].offset, b.rows, out->code + r0);
      read_for(b.col[3], area + b.col[3].offset, b.rows, out->src + r0);
      read_for(b.col[4], area + b.col[4].offset, b.rows, out->tag + r0);
      const cc_pack_col& p = b.col[kPayload];
      if (p.mode != CC_PK_BY_POS) {
        read_for(p, area + p.offset, b.rows, out->payload + r0);
        continue;
      }
      const uint8_t* const pos = area + b.col[kPos].offset;  // (the validator bounded every pos offset by the table)
      const uint8_t* const table = area + p.offset;
      for (uint32_t i = 0; i < b.rows; ++i)
        out->payload[r0 + i] = p.base + get(table, p.width, get(pos, b.col[kPos].width, i));
    }
  });
  if (out->count) *out->count = h.n;
  return CC_OK;
}
