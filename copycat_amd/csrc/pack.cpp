// pack.cpp — packed host batches: per-block base + narrow offsets (include/copycat_apply.h "packed host batches").
// Host code only, no HIP call: the encoder, the validator and the host decoder work on a machine with no GPU.
//
// A host that holds no device pointers ships every column over PCIe; the wide columns are mostly zeros (a run of
// consecutive log rows has indices, instance slots and operands close to each other).  cc_pack_batch writes, per block
// of CC_PACK_BLOCK_ROWS rows and per column, the narrowest exact encoding; cc_pack_check is the one validator every
// consumer (cc_unpack_batch here, cc_unpack_to_device and cc_apply_batch_host_packed on the device side) runs before
// it reads a directory entry; cc_unpack_batch is the host decoder the kernel (unpack.hip) is tested against.
//
// The format over the shared core (pack_host.h: the width rules, the one-pass block-order encoder, the validator, the
// decoder's loop): nine columns, each present or absent, and besides CC_PK_FOR one mode of its own, CC_PK_REL_A, on b.
// A block is at most 216 KiB of input.
#include "pack_host.h"

namespace {

using namespace cc::pk;

constexpr uint32_t kCols = CC_PACK_COLUMNS;
constexpr uint32_t kColA = 6, kColB = 7;
constexpr uint8_t kNone = 9;  // no encoding of that kind

static_assert(sizeof(cc_pack_block) == 160, "packed ABI");

struct Fmt : Format {
  using Block = cc_pack_block;
  static constexpr const char* name = "packed blob";
  static constexpr uint32_t magic = (uint32_t)CC_PACK_MAGIC, version = CC_PACK_VERSION;
  static constexpr uint32_t native[kCols] = {8, 8, 4, 1, 1, 8, 8, 8, 8};
  static const char* present(uint32_t p) { return p >> kCols ? "present mask names a column past aux" : nullptr; }
  static const char* mode(const cc_pack_header& h, const Block& b, uint32_t c) {
    const cc_pack_col& e = b.col[c];
    if (e.mode == CC_PK_FOR) return nullptr;
    if (e.mode != CC_PK_REL_A) return "unknown mode";
    if (c != kColB) return "REL_A on a column other than b";
    if (!((h.present >> kColA) & 1)) return "REL_A without column a";
    if (e.width != 1 && e.width != 2 && e.width != 4) return "REL_A width is not 1, 2 or 4";
    return nullptr;
  }
};

// ---- REL_A: b as a signed offset from the same row's a ---------------------------------------------------------------
// the narrowest exact encoding of one block of b: choose64's, or REL_A when that is strictly narrower
cc_pack_col choose_b(const uint64_t* v, const uint64_t* a, uint32_t m) {
  cc_pack_col c = choose64(v, m);
  if (!a || c.width <= 1) return c;
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
  return c;
}

template <class W>
void narrow_rel(const uint64_t* v, const uint64_t* a, uint32_t m, uint8_t* out) {
  W* o = (W*)out;
  for (uint32_t i = 0; i < m; ++i) o[i] = (W)(v[i] - a[i]);
}
template <class W>
void widen_rel(const uint8_t* in, const uint64_t* a, uint32_t m, uint64_t* out) {
  const W* p = (const W*)in;  // W is signed: the offset is sign-extended
  for (uint32_t i = 0; i < m; ++i) out[i] = a[i] + (uint64_t)(int64_t)p[i];
}

void write_rel(const cc_pack_col& c, const uint64_t* b, const uint64_t* a, uint32_t m, uint8_t* out) {
  if (c.width == 1) narrow_rel<uint8_t>(b, a, m, out);
  else if (c.width == 2) narrow_rel<uint16_t>(b, a, m, out);
  else narrow_rel<uint32_t>(b, a, m, out);
  zero_tail(out, (size_t)m * c.width);
}
void read_rel(const cc_pack_col& c, const uint8_t* in, const uint64_t* a, uint32_t m, uint64_t* b) {
  if (c.width == 1) widen_rel<int8_t>(in, a, m, b);
  else if (c.width == 2) widen_rel<int16_t>(in, a, m, b);
  else widen_rel<int32_t>(in, a, m, b);
}

}  // namespace

extern "C" int cc_pack_bound(uint64_t n, uint32_t present, uint64_t* bytes) {
  if (!bytes || (present >> kCols)) return cc::pack_err(CC_ERR_INVALID, "pack bound: null argument or bad present mask");
  if (n > (1ull << 48)) return cc::pack_err(CC_ERR_INVALID, "pack bound: n too large");
  uint64_t row = 0;
  for (uint32_t c = 0; c < kCols; ++c)
    if ((present >> c) & 1) row += Fmt::native[c];
  // every column raw; a tail block's columns are each rounded up to 16 bytes
  *bytes = sizeof(cc_pack_header) + blocks_of(n) * sizeof(cc_pack_block) + n * row + (n % kRows ? 16ull * kCols : 0);
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
  uint64_t bound = 0;
  (void)cc_pack_bound(n, present, &bound);
  return encode<Fmt>(
      "pack", n, present, bound, h_blob, cap, threads, bytes,
      [&](uint64_t r0, uint32_t m) {
        cc_pack_block b{};
        b.rows = m;
        for (uint32_t c = 0; c < kCols; ++c) {
          if (!col[c]) continue;
          cc_pack_col e;
          if (c == 2) e = choose_small((const uint32_t*)col[c] + r0, m);
          else if (c == 3 || c == 4) e = choose_small((const uint8_t*)col[c] + r0, m);
          else if (c == kColB) e = choose_b(h->b + r0, h->a ? h->a + r0 : nullptr, m);
          else e = choose64((const uint64_t*)col[c] + r0, m);
          e.offset = b.bytes;
          b.bytes += (uint32_t)r16((uint64_t)m * e.width);
          b.col[c] = e;
        }
        return b;
      },
      [&](uint64_t r0, const cc_pack_block& b, uint8_t* area) {
        for (uint32_t c = 0; c < kCols; ++c) {
          if (!col[c] || !b.col[c].width) continue;
          uint8_t* o = area + b.col[c].offset;
          if (c == 2) write_for(b.col[c], (const uint32_t*)col[c] + r0, b.rows, o);
          else if (c == 3 || c == 4) write_for(b.col[c], (const uint8_t*)col[c] + r0, b.rows, o);
          else if (b.col[c].mode == CC_PK_REL_A) write_rel(b.col[c], h->b + r0, h->a + r0, b.rows, o);
          else write_for(b.col[c], (const uint64_t*)col[c] + r0, b.rows, o);
        }
      });
}

extern "C" int cc_pack_check(const void* h_blob, uint64_t bytes, uint64_t* n, uint32_t* present) {
  cc_pack_header h;
  if (int rc = checked<Fmt>(h_blob, bytes, &h)) return rc;
  if (n) *n = h.n;
  if (present) *present = h.present;
  return CC_OK;
}

extern "C" int cc_unpack_batch(const void* h_blob, uint64_t bytes, const cc_batch_out* out, uint32_t threads) {
  cc_pack_header h;
  if (int rc = checked<Fmt>(h_blob, bytes, &h)) return rc;
  if (!out) return cc::pack_err(CC_ERR_INVALID, "unpack: null argument");
  void* const col[kCols] = {out->index, out->time, out->inst, out->op, out->flags, out->key, out->a, out->b, out->aux};
  for (uint32_t c = 0; c < kCols; ++c)
    if (h.n && ((h.present >> c) & 1) && !col[c]) return cc::pack_err(CC_ERR_INVALID, "unpack: null output column");
  decode<Fmt>(h_blob, h, threads, [&](uint64_t r0, const cc_pack_block& b, const uint8_t* area) {
    for (uint32_t c = 0; c < kCols; ++c) {
      if (!((h.present >> c) & 1)) continue;
      const uint8_t* in = area + b.col[c].offset;
      if (c == 2) read_for(b.col[c], in, b.rows, (uint32_t*)col[c] + r0);
      else if (c == 3 || c == 4) read_for(b.col[c], in, b.rows, (uint8_t*)col[c] + r0);
      else if (b.col[c].mode == CC_PK_REL_A) read_rel(b.col[c], in, out->a + r0, b.rows, out->b + r0);  // (a: decoded before b)
      else read_for(b.col[c], in, b.rows, (uint64_t*)col[c] + r0);
    }
  });
  return CC_OK;
}

