// respack.cpp — packed result blobs: per-block base + narrow offsets for cc_results (include/copycat_apply.h "packed
// result blobs").  Host code only, no HIP call: the reference encoder, the validator and the decoder work on a machine
// with no GPU.
//
// The format over the shared core (pack_host.h): two columns, status and value, both always present, one mode,
// CC_PK_FOR.  cc_respack_pack is the reference the GPU encoder (respack.hip) is tested against byte for byte;
// cc_respack_check is the one validator every consumer runs before it reads a directory entry; cc_respack_unpack is
// the host decoder.  A block is 36 KiB of input.
#include "pack_host.h"

namespace {

using namespace cc::pk;

constexpr uint32_t kCols = CC_RESPACK_COLUMNS;

static_assert(sizeof(cc_respack_block) == 48, "respack ABI");

struct Fmt : Format {
  using Block = cc_respack_block;
  static constexpr const char* name = "result blob";
  static constexpr const char* overlap = "the two columns' rows overlap";
  static constexpr uint32_t magic = (uint32_t)CC_RESPACK_MAGIC, version = CC_RESPACK_VERSION, all = 3;
  static constexpr uint32_t native[kCols] = {1, 8};  // status, value
  static const char* present(uint32_t p) { return p != all ? "present is not 3 (status and value)" : nullptr; }
  static const char* mode(const cc_pack_header&, const Block& b, uint32_t c) {
    return b.col[c].mode != CC_PK_FOR ? "a mode other than CC_PK_FOR" : nullptr;
  }
};

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
  uint64_t bound = 0;
  (void)cc_respack_bound(n, &bound);
  return encode<Fmt>(
      "result blob pack", n, Fmt::all, bound, h_blob, cap, threads, bytes,
      [&](uint64_t r0, uint32_t m) {
        cc_respack_block b{};
        b.rows = m;
        b.col[0] = choose_small(h->status + r0, m);
        b.col[1] = choose64(h->value + r0, m);
        b.col[1].offset = (uint32_t)r16((uint64_t)m * b.col[0].width);
        b.bytes = b.col[1].offset + (uint32_t)r16((uint64_t)m * b.col[1].width);
        return b;
      },
      [&](uint64_t r0, const cc_respack_block& b, uint8_t* area) {
        write_for(b.col[0], h->status + r0, b.rows, area);
        write_for(b.col[1], h->value + r0, b.rows, area + b.col[1].offset);
      });
}

extern "C" int cc_respack_check(const void* h_blob, uint64_t bytes, uint64_t* n) {
  cc_pack_header h;
  if (int rc = checked<Fmt>(h_blob, bytes, &h)) return rc;
  if (n) *n = h.n;
  return CC_OK;
}

extern "C" int cc_respack_unpack(const void* h_blob, uint64_t bytes, const cc_results* out, uint32_t threads) {
  cc_pack_header h;
  if (int rc = checked<Fmt>(h_blob, bytes, &h)) return rc;
  if (!out || (h.n && (!out->status || !out->value))) return cc::pack_err(CC_ERR_INVALID, "result blob unpack: null argument");
  decode<Fmt>(h_blob, h, threads, [&](uint64_t r0, const cc_respack_block& b, const uint8_t* area) {
    read_for(b.col[0], area + b.col[0].offset, b.rows, out->status + r0);
    read_for(b.col[1], area + b.col[1].offset, b.rows, out->value + r0);
  });
  return CC_OK;
}
