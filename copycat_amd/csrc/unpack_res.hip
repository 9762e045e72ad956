// unpack_res.hip — a packed result blob / a packed event blob -> the ordinary wide columns in HBM
// (include/copycat_apply.h "packed result blobs", "packed event blobs"); byte for byte what cc_respack_unpack
// (respack.cpp) and cc_evpack_unpack (evpack.cpp) write.  The counterparts of k_unpack (unpack.hip), over the same
// steps of pack_dev.h.
//
// One workgroup of 256 lanes per block of CC_PACK_BLOCK_ROWS rows; the block's directory entry is the same for every
// lane (read through readfirstlane: the branches on mode and width are scalar branches).  Per column the packed rows go
// global -> LDS with 16-byte loads (stage), then each lane widens the rows it owns and writes ONE 16-byte store per
// group (two u64 rows, four u32 rows, sixteen u8 rows); a width-0 column stages nothing and stores the base; the lane
// that holds the tail's last partial group stores row by row.
//   k_res_unpack  status (unpack8), then value (unpack64).  32 KiB LDS: the one image.
//   k_ev_unpack   pos, target (unpack32), code, src, tag (unpack8), payload.  40 KiB LDS: the 32 KiB image and, behind
//                 it, 8 KiB that hold the block's narrow pos image (pos width 1 or 2; a raw pos column, 16 KiB, goes
//                 through the image like any other and cannot come with a table).  A CC_PK_BY_POS payload is decoded
//                 last: the pos image is still where pos was decoded from, the table (at most 4,096 entries of 8 B:
//                 32 KiB) is staged into the image, then payload[row] = base + table[pos_offset[row]], two rows per
//                 lane and one 16-byte store.  A pos column of width 0 has every offset 0: table[0].  Thread 0 of
//                 block 0 writes the device count word (n).
// Each kernel moves (packed + wide) bytes once; its bar is the H2D of the wide columns, an order of magnitude slower.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): k_res_unpack 12 VGPRs, 32 KiB LDS; k_ev_unpack
// 14 VGPRs, 40 KiB LDS; no scratch in either (the build checks it: build.py REPORT_SRCS).
#include "pack_dev.h"

namespace cc {

namespace {

using namespace pkd;

constexpr uint32_t kImage = kRows * 8;     // the shared image
constexpr uint32_t kPosImage = kRows * 2;  // a narrow pos column, kept for the table lookup
static_assert(kImage + kPosImage <= 64 * 1024, "a workgroup's static LDS");

__global__ __launch_bounds__(256) void k_res_unpack(ResUnpackArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kImage];
  const cc_respack_block& b = a.dir[blockIdx.x];
  const uint32_t rows = min(uni(b.rows), kRows);
  const uint8_t* area = a.data + (uni(b.offset) - a.data_base);
  const uint64_t r0 = (uint64_t)blockIdx.x * kRows;
  unpack8(b.col[0], area, lds, a.status + r0, rows);
  unpack64(b.col[1], area, lds, a.value + r0, nullptr, rows);
}

// offset i of a narrow image of wave-uniform width w, zero-extended (w = 0: no image, every offset is 0)
__device__ inline uint64_t offset_at(const uint8_t* img, uint32_t w, uint32_t i) {
  return w == 1 ? narrow_at<1>(img, i) : w == 2 ? narrow_at<2>(img, i) : w == 4 ? narrow_at<4>(img, i) : w == 8 ? narrow_at<8>(img, i) : 0;
}

__global__ __launch_bounds__(256) void k_ev_unpack(EvUnpackArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kImage + kPosImage];
  uint8_t* const pimg = lds + kImage;
  if (blockIdx.x == 0 && threadIdx.x == 0) *a.count = a.n;
  const cc_evpack_block& b = a.dir[blockIdx.x];
  const uint32_t rows = min(uni(b.rows), kRows);
  const uint8_t* area = a.data + (uni(b.offset) - a.data_base);
  const uint64_t r0 = (uint64_t)blockIdx.x * kRows;
  const uint32_t pw = uni((uint32_t)b.col[0].width);
  unpack32(b.col[0], area, pw <= 2 ? pimg : lds, a.pos + r0, rows);
  unpack32(b.col[1], area, lds, a.target + r0, rows);
  unpack8(b.col[2], area, lds, a.code + r0, rows);
  unpack8(b.col[3], area, lds, a.src + r0, rows);
  unpack8(b.col[4], area, lds, a.tag + r0, rows);
  const Col v = col_of(b.col[5]);
  uint64_t* const out = a.payload + r0;
  if (v.mode != CC_PK_BY_POS) return unpack64(b.col[5], area, lds, out, nullptr, rows);
  // (the validator: pos width <= 2, 1 <= E <= 4,096, the width 1, 2, 4 or 8, every row's pos offset < E)
  stage(lds, area + v.offset, r16(uni((uint32_t)b.col[5].reserved16) * v.width));
  for (uint32_t r = threadIdx.x * 2; r < rows; r += kLanes * 2) {
    const uint64_t v0 = v.base + offset_at(lds, v.width, (uint32_t)offset_at(pimg, pw, r));
    if (r + 1 < rows) {  // (a pos offset past the tail is not in the image: never looked up)
      const uint64_t v1 = v.base + offset_at(lds, v.width, (uint32_t)offset_at(pimg, pw, r + 1));
      *(ulonglong2*)(out + r) = make_ulonglong2(v0, v1);
    } else {
      out[r] = v0;
    }
  }
}

}  // namespace

int launch_res_unpack(const ResUnpackArgs& a, uint32_t blocks, hipStream_t st) {
  if (blocks == 0) return 0;
  hipLaunchKernelGGL(k_res_unpack, dim3(blocks), dim3(kLanes), 0, st, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_ev_unpack(const EvUnpackArgs& a, uint32_t blocks, hipStream_t st) {
  if (blocks == 0) return 0;
  hipLaunchKernelGGL(k_ev_unpack, dim3(blocks), dim3(kLanes), 0, st, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace cc
