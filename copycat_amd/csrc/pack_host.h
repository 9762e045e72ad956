// pack_host.h — the host core of the packed blob formats (include/copycat_apply.h "packed host batches", "packed
// result blobs", "packed event blobs"): what pack.cpp, respack.cpp and evpack.cpp share.  Header only, no HIP call.
//
// A blob is a cc_pack_header, a directory of one entry per block of CC_PACK_BLOCK_ROWS rows ({rows, bytes, offset,
// col[]}: cc_pack_block, cc_respack_block, cc_evpack_block) and the blocks' data areas in block order.  Per block and
// column the encoder keeps the narrowest exact encoding: a base and offsets of 0, 1, 2, 4 or 8 bytes.  Here:
//   - the two width rules (choose64, choose_small) and the typed narrow / widen loops (write_for, read_for);
//   - encode(): the one-pass block-order encoder.  A thread takes the next block, measures it (the block stays in
//     cache), takes its place in the blob in block order (a ticket: offsets ascend with the block number, so a run of
//     blocks is one contiguous piece for a copy) and writes the narrow rows.  The layout depends on the input alone,
//     never on the thread count;
//   - check(): the validator every consumer runs before it reads a directory entry, over a format description (a
//     struct derived from Format) that names the format's constants and the rules only that format has;
//   - checked() and decode(): the entry points' validate-then-read-the-header step and the decoder's block loop.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/copycat_apply.h"

namespace cc {

int pack_err(int code, const char* what);  // the engine's cc_last_error store (unpack.hip)

namespace pk {

constexpr uint32_t kRows = CC_PACK_BLOCK_ROWS;
static_assert(sizeof(cc_pack_header) == 64 && sizeof(cc_pack_col) == 16, "packed ABI");

inline uint64_t r16(uint64_t x) { return (x + 15) & ~15ull; }
inline uint64_t blocks_of(uint64_t n) { return n / kRows + (n % kRows != 0); }
inline uint8_t width_of(uint64_t span) {
  return span == 0 ? 0 : span <= 0xFFu ? 1 : span <= 0xFFFFu ? 2 : span <= 0xFFFFFFFFull ? 4 : 8;
}

inline uint32_t pick_threads(uint32_t threads, uint64_t blocks) {
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

// ---- the width rules -------------------------------------------------------------------------------------------------
// a 64-bit column of one block: the narrowest exact width among base = the unsigned and base = the signed minimum, a
// tie goes to the unsigned base; the native width is the raw column (base 0)
inline cc_pack_col choose64(const uint64_t* v, uint32_t m) {
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
  if (c.width == 8) c.base = 0;
  return c;
}

// a u8 or u32 column of one block: base = the minimum, the width from the span; the native width is the raw column
template <class T>
cc_pack_col choose_small(const T* v, uint32_t m) {
  T lo = v[0], hi = v[0];
  for (uint32_t i = 1; i < m; ++i) lo = std::min(lo, v[i]), hi = std::max(hi, v[i]);
  cc_pack_col c{};
  c.mode = CC_PK_FOR;
  c.width = width_of((T)(hi - lo));
  c.base = c.width == sizeof(T) ? 0 : lo;
  return c;
}

// ---- typed write and read of a CC_PK_FOR column -----------------------------------------------------------------------
template <class W, class T>
void narrow(const T* v, uint32_t m, T base, uint8_t* out) {
  W* o = (W*)out;
  for (uint32_t i = 0; i < m; ++i) o[i] = (W)(T)(v[i] - base);
}
template <class W, class T>
void widen(const uint8_t* in, uint32_t m, T base, T* out) {
  const W* p = (const W*)in;
  for (uint32_t i = 0; i < m; ++i) out[i] = (T)(base + (T)p[i]);
}

// the tail of `used` bytes up to 16 is zero: the blob is byte for byte a function of the input
inline void zero_tail(uint8_t* out, size_t used) { std::memset(out + used, 0, r16(used) - used); }

template <class T>
void write_for(const cc_pack_col& c, const T* v, uint32_t m, uint8_t* out) {
  if (!c.width) return;
  if (c.width == sizeof(T)) std::memcpy(out, v, (size_t)m * sizeof(T));
  else if (c.width == 1) narrow<uint8_t>(v, m, (T)c.base, out);
  else if (c.width == 2) narrow<uint16_t>(v, m, (T)c.base, out);
  else if (c.width == 4) narrow<uint32_t>(v, m, (T)c.base, out);
  zero_tail(out, (size_t)m * c.width);
}

template <class T>
void read_for(const cc_pack_col& c, const uint8_t* in, uint32_t m, T* out) {
  if (c.width == 0) std::fill(out, out + m, (T)c.base);
  else if (c.width == 1) widen<uint8_t>(in, m, (T)c.base, out);
  else if (c.width == 2) widen<uint16_t>(in, m, (T)c.base, out);
  else if (c.width == 4) widen<uint32_t>(in, m, (T)c.base, out);
  else widen<uint64_t>(in, m, (T)c.base, out);
}

// ---- the format description ------------------------------------------------------------------------------------------
// A format derives from this and names: Block (its directory entry), name (the prefix of its messages), magic,
// version, native[] (the columns' native widths), present(p) (nullptr, or why the header's present mask is refused)
// and mode(h, b, c) (nullptr, or why column c of block b may not have its mode).  It overrides the rest where it
// differs.
struct Format {
  static constexpr const char* overlap = "two columns' rows overlap";
  // the units column c of block b holds (rows, unless its mode says otherwise), or why its entry is refused
  template <class Block>
  static const char* units(const Block& b, uint32_t, uint64_t* u) {
    *u = b.rows;
    return nullptr;
  }
  // what is left to check once every column of block b lies inside the block's area
  template <class Block>
  static const char* rows(const Block&, const uint8_t*) {
    return nullptr;
  }
};

// ---- encoder ---------------------------------------------------------------------------------------------------------
// measure(r0, m) -> the directory entry of rows r0 .. r0 + m (rows, col[], bytes); write(r0, entry, area) writes its
// area.  A cap too small returns CC_ERR_CAPACITY with *bytes = the size needed and writes nothing, so a pass sizes the
// blob first whenever the cap is below `bound` (the measuring alone); a caller that passes the format's bound never
// pays it.  `who` starts the message ("pack", "result blob pack", ...).
template <class F, class Measure, class Write>
int encode(const char* who, uint64_t n, uint32_t present, uint64_t bound, void* h_blob, uint64_t cap, uint32_t threads,
           uint64_t* bytes, Measure measure, Write write) {
  using Block = typename F::Block;
  const uint64_t blocks = blocks_of(n);
  const uint64_t dir_end = sizeof(cc_pack_header) + blocks * sizeof(Block);
  uint8_t* const blob = (uint8_t*)h_blob;
  std::atomic<uint64_t> next{0}, turn{0};
  uint64_t cursor = dir_end;  // written by the thread whose turn it is
  for (int pass = cap >= bound ? 1 : 0; pass < 2; ++pass) {
    next = 0, turn = 0, cursor = dir_end;
    parallel(pick_threads(threads, blocks), [&](uint32_t) {
      for (;;) {
        const uint64_t k = next.fetch_add(1, std::memory_order_relaxed);
        if (k >= blocks) return;
        const uint64_t r0 = k * kRows;
        Block b = measure(r0, (uint32_t)std::min<uint64_t>(kRows, n - r0));
        // (the blocks before k are at most one measuring pass behind; with more threads than cores the thread whose
        // turn it is may not be running: give the core away instead of spinning on it)
        for (uint32_t spins = 0; turn.load(std::memory_order_acquire) != k; ++spins)
          if (spins >= 64) std::this_thread::yield();
        b.offset = cursor;
        cursor += b.bytes;
        turn.store(k + 1, std::memory_order_release);
        if (pass == 0) continue;
        std::memcpy(blob + sizeof(cc_pack_header) + k * sizeof b, &b, sizeof b);
        write(r0, b, blob + b.offset);
      }
    });
    *bytes = cursor;
    if (cursor > cap)
      return pack_err(CC_ERR_CAPACITY, (std::string(who) + ": the blob buffer is too small (*bytes = the size needed)").c_str());
  }
  cc_pack_header hd{};
  hd.magic = F::magic;
  hd.version = F::version;
  hd.n = n;
  hd.blocks = blocks;
  hd.bytes = cursor;
  hd.present = present;
  hd.block_rows = kRows;
  std::memcpy(blob, &hd, sizeof hd);
  return CC_OK;
}

// ---- validator -------------------------------------------------------------------------------------------------------
// nullptr: the blob is well formed; else the reason, to go after "<F::name>: "
template <class F>
const char* check(const void* blob, uint64_t bytes) {
  using Block = typename F::Block;
  constexpr uint32_t kCols = sizeof(F::native) / sizeof(F::native[0]);
  if (!blob) return "null pointer";
  if ((uintptr_t)blob & 15) return "not 16-byte aligned";
  if (bytes < sizeof(cc_pack_header)) return "shorter than its header";
  cc_pack_header h;
  std::memcpy(&h, blob, sizeof h);
  if (h.magic != F::magic) return "bad magic";
  if (h.version != F::version) return "unknown format version";
  if (h.block_rows != kRows) return "block_rows is not CC_PACK_BLOCK_ROWS";
  if (const char* why = F::present(h.present)) return why;
  if (h.bytes > bytes) return "total bytes larger than the buffer";
  if (h.bytes < sizeof(cc_pack_header)) return "total bytes shorter than the header";
  if (h.blocks != blocks_of(h.n)) return "block count does not match n";
  if (h.blocks > (h.bytes - sizeof(cc_pack_header)) / sizeof(Block)) return "directory outside the blob";
  const uint8_t* dir = (const uint8_t*)blob + sizeof(cc_pack_header);
  uint64_t prev_end = sizeof(cc_pack_header) + h.blocks * sizeof(Block), rows_sum = 0;
  for (uint64_t k = 0; k < h.blocks; ++k) {
    Block b;
    std::memcpy(&b, dir + k * sizeof b, sizeof b);
    const uint64_t want = std::min<uint64_t>(kRows, h.n - k * kRows);
    if (b.rows != want) return "a block's rows are not CC_PACK_BLOCK_ROWS (or the tail's): rows do not sum to n";
    rows_sum += b.rows;
    if ((b.offset & 15) || (b.bytes & 15)) return "a block's data area is not 16-byte aligned";
    if (b.offset < prev_end) return "a block's data area overlaps the directory or an earlier block";
    if (b.offset > h.bytes || b.bytes > h.bytes - b.offset) return "a block's data area is outside the blob";
    prev_end = b.offset + b.bytes;
    uint64_t lo[kCols], hi[kCols];
    uint32_t used = 0;
    for (uint32_t c = 0; c < kCols; ++c) {
      if (!((h.present >> c) & 1)) continue;
      const cc_pack_col& e = b.col[c];
      if (const char* why = F::mode(h, b, c)) return why;
      if (e.width != 0 && e.width != 1 && e.width != 2 && e.width != 4 && e.width != 8) return "width is not 0, 1, 2, 4 or 8";
      if (e.width > F::native[c]) return "width above the column's native width";
      if (e.offset & 15) return "a column's offset is not 16-byte aligned";
      uint64_t units;
      if (const char* why = F::units(b, c, &units)) return why;
      const uint64_t len = r16(units * e.width);
      if (e.offset > b.bytes || len > b.bytes - e.offset) return "a column's rows are outside its block's data area";
      if (len) lo[used] = e.offset, hi[used] = e.offset + len, ++used;
    }
    for (uint32_t i = 0; i < used; ++i)
      for (uint32_t j = i + 1; j < used; ++j)
        if (lo[i] < hi[j] && lo[j] < hi[i]) return F::overlap;
    if (const char* why = F::rows(b, (const uint8_t*)blob + b.offset)) return why;
  }
  if (rows_sum != h.n) return "rows do not sum to n";
  return nullptr;
}

// validate, then hand out the header; CC_ERR_INVALID with "<F::name>: <reason>" in cc_last_error otherwise
template <class F>
int checked(const void* h_blob, uint64_t bytes, cc_pack_header* h) {
  if (const char* why = check<F>(h_blob, bytes)) return pack_err(CC_ERR_INVALID, (std::string(F::name) + ": " + why).c_str());
  std::memcpy(h, h_blob, sizeof *h);
  return CC_OK;
}

// the decoder's loop over a validated blob: each thread a contiguous range of blocks, f(r0, entry, area)
template <class F, class Fn>
void decode(const void* h_blob, const cc_pack_header& h, uint32_t threads, Fn f) {
  using Block = typename F::Block;
  const uint8_t* const blob = (const uint8_t*)h_blob;
  const uint32_t T = pick_threads(threads, h.blocks);
  parallel(T, [&](uint32_t t) {
    for (uint64_t k = h.blocks * t / T; k < h.blocks * (t + 1) / T; ++k) {
      Block b;
      std::memcpy(&b, blob + sizeof h + k * sizeof b, sizeof b);
      f(k * kRows, b, blob + b.offset);
    }
  });
}

}  // namespace pk
}  // namespace cc
