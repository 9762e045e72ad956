// respack.cpp — packed result blobs: per-block base + narrow offsets for cc_results (include/copycat_apply.h "packed
// result blobs").  Host code only, no HIP call: the reference encoder, the validator and the decoder work on a machine
// with no GPU.
//
// The format is the batch blob's (pack.cpp) cut down to two columns, status and value, and one mode, CC_PK_FOR.
// cc_respack_pack is the reference the GPU encoder (respack.hip) is tested against byte for byte; cc_respack_check is
// the one validator every consumer runs before it reads a directory entry; cc_respack_unpack is the host decoder.
//
// cc_respack_pack is one pass, as cc_pack_batch: a thread takes the next block, computes both columns' min / max (the
// block, 36 KiB of input, stays in cache), sizes the block's data area, takes its place in the blob in block order (a
// ticket) and writes the narrow rows.  The layout depends on the result columns alone, never on the thread count.
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
constexpr uint32_t kCols = CC_RESPACK_COLUMNS;
constexpr uint32_t kNative[kCols] = {1, 8};  // status, value

static_assert(sizeof(cc_pack_header) == 64 && sizeof(cc_pack_col) == 16 && sizeof(cc_respack_block) == 48, "respack ABI");

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

// ---- encoder ---------------------------------------------------------------------------------------------------------
// the narrowest exact encoding of one block's values: base = the unsigned or the signed minimum, ties to the unsigned
cc_pack_col choose_value(const uint64_t* v, uint32_t m) {
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

cc_pack_col choose_status(const uint8_t* v, uint32_t m) {
  uint8_t lo = v[0], hi = v[0];
  for (uint32_t i = 1; i < m; ++i) lo = std::min(lo, v[i]), hi = std::max(hi, v[i]);
  cc_pack_col c{};
  c.mode = CC_PK_FOR;
  c.width = hi != lo;
  c.base = c.width ? 0 : lo;
  return c;
}

template <class W>
void narrow(const uint64_t* v, uint32_t m, uint64_t base, uint8_t* out) {
  W* o = (W*)out;
  for (uint32_t i = 0; i < m; ++i) o[i] = (W)(v[i] - base);
}

void write_value(const cc_pack_col& c, const uint64_t* v, uint32_t m, uint8_t* out) {
  const size_t used = (size_t)m * c.width;
  if (c.width == 8) std::memcpy(out, v, used);
  else if (c.width == 1) narrow<uint8_t>(v, m, c.base, out);
  else if (c.width == 2) narrow<uint16_t>(v, m, c.base, out);
  else if (c.width == 4) narrow<uint32_t>(v, m, c.base, out);
  std::memset(out + used, 0, r16(used) - used);  // (the blob is byte-for-byte a function of the input)
}

// ---- decoder ---------------------------------------------------------------------------------------------------------
template <class W>
void widen(const uint8_t* in, uint32_t m, uint64_t base, uint64_t* out) {
  const W* p = (const W*)in;
  for (uint32_t i = 0; i < m; ++i) out[i] = base + (uint64_t)p[i];
}

void read_value(const cc_pack_col& c, const uint8_t* in, uint32_t m, uint64_t* out) {
  if (c.width == 0) std::fill(out, out + m, c.base);
  else if (c.width == 1) widen<uint8_t>(in, m, c.base, out);
  else if (c.width == 2) widen<uint16_t>(in, m, c.base, out);
  else if (c.width == 4) widen<uint32_t>(in, m, c.base, out);
  else widen<uint64_t>(in, m, c.base, out);
}

void read_status(const cc_pack_col& c, const uint8_t* in, uint32_t m, uint8_t* out) {
  if (c.width == 0) std::memset(out, (int)(uint8_t)c.base, m);
  else
    for (uint32_t i = 0; i < m; ++i) out[i] = (uint8_t)(c.base + in[i]);
}

// ---- validator -------------------------------------------------------------------------------------------------------
// nullptr: the blob is well formed
const char* check(const void* blob, uint64_t bytes) {
  if (!blob) return "result blob: null pointer";
  if ((uintptr_t)blob & 15) return "result blob: not 16-byte aligned";
  if (bytes < sizeof(cc_pack_header)) return "result blob: shorter than its header";
  cc_pack_header h;
  std::memcpy(&h, blob, sizeof h);
  if (h.magic != (uint32_t)CC_RESPACK_MAGIC) return "result blob: bad magic";
  if (h.version != CC_RESPACK_VERSION) return "result blob: unknown format version";
  if (h.block_rows != kRows) return "result blob: block_rows is not CC_PACK_BLOCK_ROWS";
  if (h.present != 3) return "result blob: present is not 3 (status and value)";
  if (h.bytes > bytes) return "result blob: total bytes larger than the buffer";
  if (h.bytes < sizeof(cc_pack_header)) return "result blob: total bytes shorter than the header";
  if (h.blocks != blocks_of(h.n)) return "result blob: block count does not match n";
  if (h.blocks > (h.bytes - sizeof(cc_pack_header)) / sizeof(cc_respack_block)) return "result blob: directory outside the blob";
  const uint8_t* dir = (const uint8_t*)blob + sizeof(cc_pack_header);
  uint64_t prev_end = sizeof(cc_pack_header) + h.blocks * sizeof(cc_respack_block), rows_sum = 0;
  for (uint64_t k = 0; k < h.blocks; ++k) {
    cc_respack_block b;
    std::memcpy(&b, dir + k * sizeof b, sizeof b);
    const uint64_t want = std::min<uint64_t>(kRows, h.n - k * kRows);
    if (b.rows != want) return "result blob: a block's rows are not CC_PACK_BLOCK_ROWS (or the tail's): rows do not sum to n";
    rows_sum += b.rows;
    if ((b.offset & 15) || (b.bytes & 15)) return "result blob: a block's data area is not 16-byte aligned";
    if (b.offset < prev_end) return "result blob: a block's data area overlaps the directory or an earlier block";
    if (b.offset > h.bytes || b.bytes > h.bytes - b.offset) return "result blob: a block's data area is outside the blob";
    prev_end = b.offset + b.bytes;
    uint64_t lo[kCols], hi[kCols];
    for (uint32_t c = 0; c < kCols; ++c) {
      const cc_pack_col& e = b.col[c];
      if (e.mode != CC_PK_FOR) return "result blob: a mode other than CC_PK_FOR";
      if (e.width != 0 && e.width != 1 && e.width != 2 && e.width != 4 && e.width != 8)
        return "result blob: width is not 0, 1, 2, 4 or 8";
      if (e.width > kNative[c]) return "result blob: width above the column's native width";
      if (e.offset & 15) return "result blob: a column's offset is not 16-byte aligned";
      const uint64_t len = r16((uint64_t)b.rows * e.width);
      if (e.offset > b.bytes || len > b.bytes - e.offset) return "result blob: a column's rows are outside its block's data area";
      lo[c] = e.offset, hi[c] = e.offset + len;
    }
    if (lo[0] < hi[0] && lo[1] < hi[1] && lo[0] < hi[1] && lo[1] < hi[0]) return "result blob: the two columns' rows overlap";
  }
  if (rows_sum != h.n) return "result blob: rows do not sum to n";
  return nullptr;
}

}  // namespace

extern "C" int cc_respack_bound(uint64_t n, uint64_t* bytes) {
  if (!bytes) return cc::pack_err(CC_ERR_INVALID, "result blob bound: null argument");
  if (n > (1ull << 48)) return cc::pack_err(CC_ERR_INVALID, "result blob bound: n too large");
  // both columns raw; a tail block's columns are each rounded up to 16 bytes
  *bytes = sizeof(cc_pack_header) + blocks_of(n) * sizeof(cc_respack_block) + n * 9 + (n % kRows ? 16ull * kCols : 0);
  return CC_OK;
}

extern "C" int cc_respack_pack(const cc_results* h, uint64_t n, void* h_blob, uint64_t cap, uint32_t threads,
                               uint64_t* bytes) {
  if (!h || !bytes || (cap && !h_blob) || (n && (!h->status || !h->value)))
    return cc::pack_err(CC_ERR_INVALID, "result blob pack: null argument");
  if ((uintptr_t)h_blob & 15) return cc::pack_err(CC_ERR_INVALID, "result blob pack: the blob must be 16-byte aligned");
  if (n > (1ull << 48)) return cc::pack_err(CC_ERR_INVALID, "result blob pack: n too large");
  const uint64_t blocks = blocks_of(n);
  const uint64_t dir_end = sizeof(cc_pack_header) + blocks * sizeof(cc_respack_block);
  uint8_t* const blob = (uint8_t*)h_blob;
  std::atomic<uint64_t> next{0}, turn{0};
  uint64_t cursor = dir_end;  // written by the thread whose turn it is
  // A cap too small writes nothing, so a pass sizes the blob first whenever the cap is below the bound (the min / max
  // pass alone: a ninth of the work); a caller that passes cc_respack_bound never pays it.
  uint64_t bound = 0;
  (void)cc_respack_bound(n, &bound);
  for (int pass = cap >= bound ? 1 : 0; pass < 2; ++pass) {
    const bool write = pass == 1;
    next = 0, turn = 0, cursor = dir_end;
    parallel(pick_threads(threads, blocks), [&](uint32_t) {
      for (;;) {
        const uint64_t k = next.fetch_add(1, std::memory_order_relaxed);
        if (k >= blocks) return;
        const uint64_t r0 = k * kRows;
        const uint32_t m = (uint32_t)std::min<uint64_t>(kRows, n - r0);
        cc_respack_block b{};
        b.rows = m;
        b.col[0] = choose_status(h->status + r0, m);
        b.col[1] = choose_value(h->value + r0, m);
        b.col[0].offset = 0;
        b.col[1].offset = (uint32_t)r16((uint64_t)m * b.col[0].width);
        b.bytes = b.col[1].offset + (uint32_t)r16((uint64_t)m * b.col[1].width);
        // (the blocks before k are at most one min / max pass behind; with more threads than cores the thread whose
        // turn it is may not be running: give the core away instead of spinning on it)
        for (uint32_t spins = 0; turn.load(std::memory_order_acquire) != k; ++spins)
          if (spins >= 64) std::this_thread::yield();
        b.offset = cursor;
        cursor += b.bytes;
        turn.store(k + 1, std::memory_order_release);
        if (!write) continue;
        std::memcpy(blob + sizeof(cc_pack_header) + k * sizeof b, &b, sizeof b);
        uint8_t* const out = blob + b.offset;
        if (b.col[0].width) {
          std::memcpy(out, h->status + r0, m);
          std::memset(out + m, 0, r16(m) - m);
        }
        if (b.col[1].width) write_value(b.col[1], h->value + r0, m, out + b.col[1].offset);
      }
    });
    *bytes = cursor;
    if (cursor > cap) return cc::pack_err(CC_ERR_CAPACITY, "result blob pack: the blob buffer is too small (*bytes = the size needed)");
  }
  cc_pack_header hd{};
  hd.magic = (uint32_t)CC_RESPACK_MAGIC;
  hd.version = CC_RESPACK_VERSION;
  hd.n = n;
  hd.blocks = blocks;
  hd.bytes = cursor;
  hd.present = 3;
  hd.block_rows = kRows;
  std::memcpy(blob, &hd, sizeof hd);
  return CC_OK;
}

extern "C" int cc_respack_check(const void* h_blob, uint64_t bytes, uint64_t* n) {
  if (const char* why = check(h_blob, bytes)) return cc::pack_err(CC_ERR_INVALID, why);
  if (n) {
    cc_pack_header h;
    std::memcpy(&h, h_blob, sizeof h);
    *n = h.n;
  }
  return CC_OK;
}

extern "C" int cc_respack_unpack(const void* h_blob, uint64_t bytes, const cc_results* out, uint32_t threads) {
  if (const char* why = check(h_blob, bytes)) return cc::pack_err(CC_ERR_INVALID, why);
  cc_pack_header h;
  std::memcpy(&h, h_blob, sizeof h);
  if (!out || (h.n && (!out->status || !out->value))) return cc::pack_err(CC_ERR_INVALID, "result blob unpack: null argument");
  const uint8_t* const blob = (const uint8_t*)h_blob;
  const uint32_t T = pick_threads(threads, h.blocks);
  parallel(T, [&](uint32_t t) {
    for (uint64_t k = h.blocks * t / T; k < h.blocks * (t + 1) / T; ++k) {
      cc_respack_block b;
      std::memcpy(&b, blob + sizeof h + k * sizeof b, sizeof b);
      const uint64_t r0 = k * kRows;
      const uint8_t* const area = blob + b.offset;
      read_status(b.col[0], area + b.col[0].offset, b.rows, out->status + r0);
      read_value(b.col[1], area + b.col[1].offset, b.rows, out->value + r0);
    }
  });
  return CC_OK;
}
