// pack.cpp — packed host batches: per-block base + narrow offsets (include/copycat_apply.h "packed host batches").
// Host code only, no HIP call: the encoder, the validator and the host decoder work on a machine with no GPU.
//
// A host that holds no device pointers ships every column over PCIe; the wide columns are mostly zeros (a run of
// consecutive log rows has indices, instance slots and operands close to each other).  cc_pack_batch writes, per block
// of CC_PACK_BLOCK_ROWS rows and per column, the narrowest exact encoding; cc_pack_check is the one validator every
// consumer (cc_unpack_batch here, cc_unpack_to_device and cc_apply_batch_host_packed on the device side) runs before
// it reads a directory entry; cc_unpack_batch is the host decoder the kernel (unpack.hip) is tested against.
//
// cc_pack_batch is one pass: a thread takes the next block, computes every column's min / max (the block, at most
// 216 KiB of input, stays in cache), sizes the block's data area, takes its place in the blob in block order (a ticket:
// offsets ascend with the block number, so a run of blocks is one contiguous piece for the H2D) and writes the narrow
// rows.  The layout depends on the input alone, never on the thread count.
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
constexpr uint32_t kCols = CC_PACK_COLUMNS;
constexpr uint32_t kNative[kCols] = {8, 8, 4, 1, 1, 8, 8, 8, 8};
constexpr uint32_t kColA = 6, kColB = 7;
constexpr uint8_t kNone = 9;  // no encoding of that kind

static_assert(sizeof(cc_pack_header) == 64 && sizeof(cc_pack_col) == 16 && sizeof(cc_pack_block) == 160, "packed ABI");

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
template <class T>
void minmax(const T* v, uint32_t m, uint64_t* lo, uint64_t* hi) {
  T a = v[0], b = v[0];
  for (uint32_t i = 1; i < m; ++i) a = std::min(a, v[i]), b = std::max(b, v[i]);
  *lo = a, *hi = b;
}

// the narrowest exact encoding of one 64-bit column of one block (`a`: the block's a column when the column is b)
cc_pack_col choose64(const uint64_t* v, const uint64_t* a, uint32_t m) {
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
  if (a && c.width > 1) {  // REL_A: only when it is strictly narrower than FOR
    int64_t dlo = (int64_t)(v[0] - a[0]), dhi = dlo;
    for (uint32_t i = 1; i < m; ++i) {
      const int64_t d = (int64_t)(v[i] - a[i]);
      dlo = std::min(dlo, d), dhi = std::max(dhi, d);
    }
    const uint8_t wr = dlo >= -128 && dhi <= 127               ? 1
                       : dlo >= -32768 && dhi <= 32767         ? 2
                       : dlo >= INT32_MIN && dhi <= INT32_MAX ? 4
                                                               : kNone;
    if (wr < c.width) c.mode = CC_PK_REL_A, c.width = wr, c.base = 0;
  }
  if (c.width == 8) c.base = 0;  // the native width is the raw column
  return c;
}

template <class T>
cc_pack_col choose_small(const T* v, uint32_t m) {
  uint64_t lo, hi;
  minmax(v, m, &lo, &hi);
  cc_pack_col c{};
  c.mode = CC_PK_FOR;
  c.width = width_of(hi - lo);
  c.base = c.width == sizeof(T) ? 0 : lo;
  return c;
}

template <class W, class T>
void narrow(const T* v, uint32_t m, T base, uint8_t* out) {
  W* o = (W*)out;
  for (uint32_t i = 0; i < m; ++i) o[i] = (W)(T)(v[i] - base);
}
template <class W>
void narrow_rel(const uint64_t* v, const uint64_t* a, uint32_t m, uint8_t* out) {
  W* o = (W*)out;
  for (uint32_t i = 0; i < m; ++i) o[i] = (W)(v[i] - a[i]);
}

template <class T>
void write_col(const cc_pack_col& c, const T* v, const uint64_t* a, uint32_t m, uint8_t* out) {
  const size_t used = (size_t)m * c.width;
  if (c.mode == CC_PK_REL_A) {
    const uint64_t* b = (const uint64_t*)(const void*)v;
    if (c.width == 1) narrow_rel<uint8_t>(b, a, m, out);
    else if (c.width == 2) narrow_rel<uint16_t>(b, a, m, out);
    else narrow_rel<uint32_t>(b, a, m, out);
  } else if (c.width == sizeof(T)) {
    std::memcpy(out, v, used);
  } else if (c.width == 1) {
    narrow<uint8_t>(v, m, (T)c.base, out);
  } else if (c.width == 2) {
    narrow<uint16_t>(v, m, (T)c.base, out);
  } else if (c.width == 4) {
    narrow<uint32_t>(v, m, (T)c.base, out);
  }
  std::memset(out + used, 0, r16(used) - used);  // (the blob is byte-for-byte a function of the input)
}

// ---- decoder ---------------------------------------------------------------------------------------------------------
template <class W, class T>
void widen(const uint8_t* in, uint32_t m, T base, T* out) {
  const W* p = (const W*)in;
  for (uint32_t i = 0; i < m; ++i) out[i] = (T)(base + (T)p[i]);
}
template <class W>
void widen_rel(const uint8_t* in, const uint64_t* a, uint32_t m, uint64_t* out) {
  const W* p = (const W*)in;  // W is signed: the offset is sign-extended
  for (uint32_t i = 0; i < m; ++i) out[i] = a[i] + (uint64_t)(int64_t)p[i];
}

template <class T>
void read_col(const cc_pack_col& c, const uint8_t* in, const uint64_t* a, uint32_t m, T* out) {
  if (c.mode == CC_PK_REL_A) {
    uint64_t* b = (uint64_t*)(void*)out;
    if (c.width == 1) widen_rel<int8_t>(in, a, m, b);
    else if (c.width == 2) widen_rel<int16_t>(in, a, m, b);
    else widen_rel<int32_t>(in, a, m, b);
  } else if (c.width == 0) {
    std::fill(out, out + m, (T)c.base);
  } else if (c.width == 1) {
    widen<uint8_t>(in, m, (T)c.base, out);
  } else if (c.width == 2) {
    widen<uint16_t>(in, m, (T)c.base, out);
  } else if (c.width == 4) {
    widen<uint32_t>(in, m, (T)c.base, out);
  } else {
    widen<uint64_t>(in, m, (T)c.base, out);
  }
}

// ---- validator -------------------------------------------------------------------------------------------------------
// nullptr: the blob is well formed
const char* check(const void* blob, uint64_t bytes) {
  if (!blob) return "packed blob: null pointer";
  if ((uintptr_t)blob & 15) return "packed blob: not 16-byte aligned";
  if (bytes < sizeof(cc_pack_header)) return "packed blob: shorter than its header";
  cc_pack_header h;
  std::memcpy(&h, blob, sizeof h);
  if (h.magic != (uint32_t)CC_PACK_MAGIC) return "packed blob: bad magic";
  if (h.version != CC_PACK_VERSION) return "packed blob: unknown format version";
  if (h.block_rows != kRows) return "packed blob: block_rows is not CC_PACK_BLOCK_ROWS";
  if (h.present >> kCols) return "packed blob: present mask names a column past aux";
  if (h.bytes > bytes) return "packed blob: total bytes larger than the buffer";
  if (h.bytes < sizeof(cc_pack_header)) return "packed blob: total bytes shorter than the header";
  if (h.blocks != blocks_of(h.n)) return "packed blob: block count does not match n";
  if (h.blocks > (h.bytes - sizeof(cc_pack_header)) / sizeof(cc_pack_block)) return "packed blob: directory outside the blob";
  const uint8_t* dir = (const uint8_t*)blob + sizeof(cc_pack_header);
  uint64_t prev_end = sizeof(cc_pack_header) + h.blocks * sizeof(cc_pack_block), rows_sum = 0;
  for (uint64_t k = 0; k < h.blocks; ++k) {
    cc_pack_block b;
    std::memcpy(&b, dir + k * sizeof b, sizeof b);
    const uint64_t want = std::min<uint64_t>(kRows, h.n - k * kRows);
    if (b.rows != want) return "packed blob: a block's rows are not CC_PACK_BLOCK_ROWS (or the tail's): rows do not sum to n";
    rows_sum += b.rows;
    if ((b.offset & 15) || (b.bytes & 15)) return "packed blob: a block's data area is not 16-byte aligned";
    if (b.offset < prev_end) return "packed blob: a block's data area overlaps the directory or an earlier block";
    if (b.offset > h.bytes || b.bytes > h.bytes - b.offset) return "packed blob: a block's data area is outside the blob";
    prev_end = b.offset + b.bytes;
    uint32_t lo[kCols], hi[kCols], used = 0;
    for (uint32_t c = 0; c < kCols; ++c) {
      if (!((h.present >> c) & 1)) continue;
      const cc_pack_col& e = b.col[c];
      if (e.mode == CC_PK_REL_A) {
        if (c != kColB) return "packed blob: REL_A on a column other than b";
        if (!((h.present >> kColA) & 1)) return "packed blob: REL_A without column a";
        if (e.width != 1 && e.width != 2 && e.width != 4) return "packed blob: REL_A width is not 1, 2 or 4";
      } else if (e.mode == CC_PK_FOR) {
        if (e.width != 0 && e.width != 1 && e.width != 2 && e.width != 4 && e.width != 8)
          return "packed blob: width is not 0, 1, 2, 4 or 8";
        if (e.width > kNative[c]) return "packed blob: width above the column's native width";
      } else {
        return "packed blob: unknown mode";
      }
      if (e.offset & 15) return "packed blob: a column's offset is not 16-byte aligned";
      const uint64_t len = r16((uint64_t)b.rows * e.width);
      if (e.offset > b.bytes || len > b.bytes - e.offset) return "packed blob: a column's rows are outside its block's data area";
      if (len) lo[used] = e.offset, hi[used] = e.offset + (uint32_t)len, ++used;
    }
    for (uint32_t i = 0; i < used; ++i)
      for (uint32_t j = i + 1; j < used; ++j)
        if (lo[i] < hi[j] && lo[j] < hi[i]) return "packed blob: two columns' rows overlap";
  }
  if (rows_sum != h.n) return "packed blob: rows do not sum to n";
  return nullptr;
}

}  // namespace

extern "C" int cc_pack_bound(uint64_t n, uint32_t present, uint64_t* bytes) {
  if (!bytes || (present >> kCols)) return cc::pack_err(CC_ERR_INVALID, "pack bound: null argument or bad present mask");
  if (n > (1ull << 48)) return cc::pack_err(CC_ERR_INVALID, "pack bound: n too large");
  uint64_t row = 0;
  for (uint32_t c = 0; c < kCols; ++c)
    if ((present >> c) & 1) row += kNative[c];
  const uint64_t blocks = blocks_of(n);
  // every column raw; a tail block's columns are each rounded up to 16 bytes
  *bytes = sizeof(cc_pack_header) + blocks * sizeof(cc_pack_block) + n * row + (n % kRows ? 16ull * kCols : 0);
  return CC_OK;
}

extern "C" int cc_pack_batch(const cc_batch* h, uint64_t n, void* h_blob, uint64_t cap, uint32_t threads, uint64_t* bytes) {
  if (!h || !bytes || (cap && !h_blob)) return cc::pack_err(CC_ERR_INVALID, "pack: null argument");
  if ((uintptr_t)h_blob & 15) return cc::pack_err(CC_ERR_INVALID, "pack: the blob must be 16-byte aligned");
  if (n > (1ull << 48)) return cc::pack_err(CC_ERR_INVALID, "pack: n too large");
  const void* const col[kCols] = {h->index, h->time, h->inst, h->op, h->flags, h->key, h->a, h->b, h->aux};
  uint32_t present = 0;
  for (uint32_t c = 0; c < kCols; ++c)
    if (col[c]) present |= 1u << c;
  const uint64_t blocks = blocks_of(n);
  const uint64_t dir_end = sizeof(cc_pack_header) + blocks * sizeof(cc_pack_block);
  uint8_t* const blob = (uint8_t*)h_blob;
  const bool has_dir = dir_end <= cap;  // (else only the size is computed)
  std::atomic<uint64_t> next{0}, turn{0};
  uint64_t cursor = dir_end;  // written by the thread whose turn it is
  parallel(pick_threads(threads, blocks), [&](uint32_t) {
    for (;;) {
      const uint64_t k = next.fetch_add(1, std::memory_order_relaxed);
      if (k >= blocks) return;
      const uint64_t r0 = k * kRows;
      const uint32_t m = (uint32_t)std::min<uint64_t>(kRows, n - r0);
      cc_pack_block b{};
      b.rows = m;
      uint32_t area = 0;
      const uint64_t* a_col = h->a ? h->a + r0 : nullptr;
      for (uint32_t c = 0; c < kCols; ++c) {
        if (!col[c]) continue;
        cc_pack_col e;
        if (c == 2) e = choose_small((const uint32_t*)col[c] + r0, m);
        else if (c == 3 || c == 4) e = choose_small((const uint8_t*)col[c] + r0, m);
        else e = choose64((const uint64_t*)col[c] + r0, c == kColB ? a_col : nullptr, m);
        e.offset = area;
        area += (uint32_t)r16((uint64_t)m * e.width);
        b.col[c] = e;
      }
      b.bytes = area;
      // (the blocks before k are at most one min / max pass behind; with more threads than cores the thread whose
      // turn it is may not be running: give the core away instead of spinning on it)
      for (uint32_t spins = 0; turn.load(std::memory_order_acquire) != k; ++spins)
        if (spins >= 64) std::this_thread::yield();
      b.offset = cursor;
      cursor += area;
      turn.store(k + 1, std::memory_order_release);
      if (b.offset + area > cap || !has_dir) continue;  // too small: the size is still summed up
      std::memcpy(blob + sizeof(cc_pack_header) + k * sizeof b, &b, sizeof b);
      uint8_t* const out = blob + b.offset;
      for (uint32_t c = 0; c < kCols; ++c) {
        if (!col[c] || !b.col[c].width) continue;
        uint8_t* o = out + b.col[c].offset;
        if (c == 2) write_col(b.col[c], (const uint32_t*)col[c] + r0, nullptr, m, o);
        else if (c == 3 || c == 4) write_col(b.col[c], (const uint8_t*)col[c] + r0, nullptr, m, o);
        else write_col(b.col[c], (const uint64_t*)col[c] + r0, a_col, m, o);
      }
    }
  });
  *bytes = cursor;
  if (cursor > cap) return cc::pack_err(CC_ERR_CAPACITY, "pack: the blob buffer is too small (*bytes = the size needed)");
  cc_pack_header hd{};
  hd.magic = (uint32_t)CC_PACK_MAGIC;
  hd.version = CC_PACK_VERSION;
  hd.n = n;
  hd.blocks = blocks;
  hd.bytes = cursor;
  hd.present = present;
  hd.block_rows = kRows;
  std::memcpy(blob, &hd, sizeof hd);
  return CC_OK;
}

extern "C" int cc_pack_check(const void* h_blob, uint64_t bytes, uint64_t* n, uint32_t* present) {
  if (const char* why = check(h_blob, bytes)) return cc::pack_err(CC_ERR_INVALID, why);
  cc_pack_header h;
  std::memcpy(&h, h_blob, sizeof h);
  if (n) *n = h.n;
  if (present) *present = h.present;
  return CC_OK;
}

extern "C" int cc_unpack_batch(const void* h_blob, uint64_t bytes, const cc_batch_out* out, uint32_t threads) {
  if (const char* why = check(h_blob, bytes)) return cc::pack_err(CC_ERR_INVALID, why);
  if (!out) return cc::pack_err(CC_ERR_INVALID, "unpack: null argument");
  cc_pack_header h;
  std::memcpy(&h, h_blob, sizeof h);
  void* const col[kCols] = {out->index, out->time, out->inst, out->op, out->flags, out->key, out->a, out->b, out->aux};
  for (uint32_t c = 0; c < kCols; ++c)
    if (h.n && ((h.present >> c) & 1) && !col[c]) return cc::pack_err(CC_ERR_INVALID, "unpack: null output column");
  const uint8_t* const blob = (const uint8_t*)h_blob;
  const uint32_t T = pick_threads(threads, h.blocks);
  parallel(T, [&](uint32_t t) {
    for (uint64_t k = h.blocks * t / T; k < h.blocks * (t + 1) / T; ++k) {
      cc_pack_block b;
      std::memcpy(&b, blob + sizeof h + k * sizeof b, sizeof b);
      const uint64_t r0 = k * kRows;
      const uint64_t* a_out = out->a ? out->a + r0 : nullptr;  // (decoded before b: column order)
      for (uint32_t c = 0; c < kCols; ++c) {
        if (!((h.present >> c) & 1)) continue;
        const uint8_t* in = blob + b.offset + b.col[c].offset;
        if (c == 2) read_col(b.col[c], in, nullptr, b.rows, (uint32_t*)col[c] + r0);
        else if (c == 3 || c == 4) read_col(b.col[c], in, nullptr, b.rows, (uint8_t*)col[c] + r0);
        else read_col(b.col[c], in, a_out, b.rows, (uint64_t*)col[c] + r0);
      }
    }
  });
  return CC_OK;
}
