// respack.hip — the wide result columns in HBM -> the directory and data areas of a packed result blob
// (include/copycat_apply.h "packed result blobs"); byte for byte what cc_respack_pack (respack.cpp) writes.
//
// Three launches on one stream; the kernel boundaries are the only synchronisation (no workgroup waits on another):
//   k_respack_measure  one workgroup of 256 lanes per block of CC_PACK_BLOCK_ROWS rows.  Each lane folds the rows it
//                      owns (two u64 values per 16-byte load, sixteen status bytes per 16-byte load) into the value's
//                      unsigned min / max, its signed min / max (the unsigned ones of v ^ 2^63) and the status
//                      min / max; a wave shuffle reduction, then the four waves through LDS; lane 0 writes the
//                      block's directory entry ({mode, width, base} per column, the area's bytes; offset still 0).
//   k_respack_place    one workgroup: an exclusive scan of the blocks' bytes into their offsets from `data_base` on,
//                      kRespackPlacePass blocks per pass with a carry; the total goes into a device word.
//   k_respack_write    one workgroup per block, the mirror of stage() + dec64 in unpack.hip: each lane reloads its two
//                      rows with one 16-byte load, subtracts the base and writes the pair of narrow offsets as ONE LDS
//                      store at the rows' position (rows past the tail and the padding up to 16 bytes are zero);
//                      after a barrier the image (at most 32 KiB) goes out with 16-byte stores, lane i the i-th 16
//                      bytes, so a wave store is one contiguous KiB whatever the width.  A raw status column has that
//                      row -> lane mapping already and is copied register to register.  Width 0 writes nothing; the
//                      tail block runs the same loop.
// The encoder reads 9 B per row twice and writes at most 9 B per row; its bar is the D2H of the bytes it saves.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): measure 34 VGPRs, 160 B LDS; place 32 VGPRs, 32 B
// LDS; write 13 VGPRs, 32 KiB LDS; no scratch in any of them.
#include <hip/hip_runtime.h>

#include "engine_state.h"

namespace cc {

namespace {

constexpr uint32_t kRows = CC_PACK_BLOCK_ROWS;
constexpr uint32_t kLanes = 256;
constexpr uint64_t kSign = 1ull << 63;
static_assert(kRespackPlacePass == kLanes, "the placement scan holds one block per lane");

__device__ inline uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ inline uint64_t uni(uint64_t v) { return (uint64_t)uni((uint32_t)v) | ((uint64_t)uni((uint32_t)(v >> 32)) << 32); }

__device__ inline uint32_t width_of(uint64_t span) {
  return span == 0 ? 0 : span <= 0xFFu ? 1 : span <= 0xFFFFu ? 2 : span <= 0xFFFFFFFFull ? 4 : 8;
}
__device__ inline uint32_t r16(uint32_t x) { return (x + 15) & ~15u; }
__device__ inline uint32_t rows_of(uint64_t n) {  // this workgroup's rows
  const uint64_t left = n - (uint64_t)blockIdx.x * kRows;
  return left < kRows ? (uint32_t)left : kRows;
}
__device__ inline uint4 col_words(uint32_t width, uint32_t offset, uint64_t base) {  // a cc_pack_col in mode CC_PK_FOR
  return make_uint4(CC_PK_FOR | (width << 8), offset, (uint32_t)base, (uint32_t)(base >> 32));
}

__global__ __launch_bounds__(256) void k_respack_measure(RespackArgs a) {
  __shared__ uint64_t red[4][4];
  __shared__ uint32_t sred[4][2];
  const uint32_t rows = rows_of(a.n);
  const uint64_t r0 = (uint64_t)blockIdx.x * kRows;
  const uint64_t* v = a.value + r0;
  const uint8_t* s = a.status + r0;
  uint64_t ulo = ~0ull, uhi = 0, xlo = ~0ull, xhi = 0;  // x: of v ^ 2^63
  for (uint32_t r = threadIdx.x * 2; r < rows; r += kLanes * 2) {
    uint64_t v0, v1;
    if (r + 1 < rows) {
      const ulonglong2 x = *(const ulonglong2*)(v + r);
      v0 = x.x, v1 = x.y;
    } else {
      v0 = v1 = v[r];
    }
    ulo = min(ulo, min(v0, v1)), uhi = max(uhi, max(v0, v1));
    v0 ^= kSign, v1 ^= kSign;
    xlo = min(xlo, min(v0, v1)), xhi = max(xhi, max(v0, v1));
  }
  uint32_t slo = 255, shi = 0;
  const uint32_t q = threadIdx.x * 16;  // lane t owns status rows 16t .. 16t + 15
  if (q < rows) {
    uint32_t w[4] = {0, 0, 0, 0};
    if (q + 16 <= rows) {
      const uint4 x = *(const uint4*)(s + q);
      w[0] = x.x, w[1] = x.y, w[2] = x.z, w[3] = x.w;
    } else {  // (the tail's last group: its first byte stands in for the rows past the end)
      const uint32_t first = s[q];
#pragma unroll
      for (int j = 0; j < 16; ++j) w[j >> 2] |= (q + j < rows ? (uint32_t)s[q + j] : first) << (8 * (j & 3));
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const uint32_t b = (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
      slo = min(slo, b), shi = max(shi, b);
    }
  }
  for (int off = 32; off; off >>= 1) {
    ulo = min(ulo, (uint64_t)__shfl_xor((unsigned long long)ulo, off));
    uhi = max(uhi, (uint64_t)__shfl_xor((unsigned long long)uhi, off));
    xlo = min(xlo, (uint64_t)__shfl_xor((unsigned long long)xlo, off));
    xhi = max(xhi, (uint64_t)__shfl_xor((unsigned long long)xhi, off));
    slo = min(slo, (uint32_t)__shfl_xor((int)slo, off));
    shi = max(shi, (uint32_t)__shfl_xor((int)shi, off));
  }
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[wave][0] = ulo, red[wave][1] = uhi, red[wave][2] = xlo, red[wave][3] = xhi;
    sred[wave][0] = slo, sred[wave][1] = shi;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int w = 1; w < 4; ++w) {
    ulo = min(ulo, red[w][0]), uhi = max(uhi, red[w][1]);
    xlo = min(xlo, red[w][2]), xhi = max(xhi, red[w][3]);
    slo = min(slo, sred[w][0]), shi = max(shi, sred[w][1]);
  }
  // the narrowest exact width among base = the unsigned and base = the signed minimum; a tie goes to the unsigned base
  uint32_t vw = width_of(uhi - ulo);
  uint64_t vbase = ulo;
  const uint32_t ws = width_of(xhi - xlo);
  if (ws < vw) vw = ws, vbase = xlo ^ kSign;
  if (vw == 8) vbase = 0;  // the native width is the raw column
  const uint32_t sw = shi != slo;
  const uint32_t voff = r16(rows * sw);
  uint4* const e = (uint4*)(a.dir + blockIdx.x);
  e[0] = make_uint4(rows, voff + r16(rows * vw), 0, 0);  // (offset: k_respack_place)
  e[1] = col_words(sw, 0, sw ? 0 : slo);
  e[2] = col_words(vw, voff, vbase);
}

__global__ __launch_bounds__(256) void k_respack_place(RespackArgs a, uint32_t blocks) {
  __shared__ uint64_t wsum[4];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t carry = a.data_base;
  for (uint32_t k0 = 0; k0 < blocks; k0 += kRespackPlacePass) {
    const uint32_t k = k0 + threadIdx.x;
    uint4 w = make_uint4(0, 0, 0, 0);  // {rows, bytes, offset lo, offset hi}
    if (k < blocks) w = *(const uint4*)(a.dir + k);
    uint32_t inc = w.y;  // (a pass sums at most 256 areas of 36 KiB: 32 bits hold it)
    for (uint32_t off = 1; off < 64; off <<= 1) {
      const uint32_t y = (uint32_t)__shfl_up((int)inc, off);
      if (lane >= off) inc += y;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      const uint64_t x = wsum[j];
      before += j < wave ? x : 0;
      all += x;
    }
    const uint64_t at = carry + before + (inc - w.y);
    if (k < blocks) {
      w.z = (uint32_t)at, w.w = (uint32_t)(at >> 32);
      *(uint4*)(a.dir + k) = w;
    }
    carry += all;
    __syncthreads();  // (wsum is written again by the next pass)
  }
  if (threadIdx.x == 0) *a.total = carry - a.data_base;
}

// the value rows as W-byte offsets from `base`: lane t owns rows 2t, 2t + 1 of every 512, written as one LDS store
template <int W>
__device__ inline void enc64(uint8_t* lds, const uint64_t* v, uint64_t base, uint32_t rows, uint32_t bytes) {
  for (uint32_t r = threadIdx.x * 2; r * W < bytes; r += kLanes * 2) {  // (bytes: a multiple of 16, so of 2 W)
    uint64_t v0 = base, v1 = base;  // rows past the tail: the padding is zero
    if (r + 1 < rows) {
      const ulonglong2 x = *(const ulonglong2*)(v + r);
      v0 = x.x, v1 = x.y;
    } else if (r < rows) {
      v0 = v[r];
    }
    v0 -= base, v1 -= base;
    if constexpr (W == 1) *(uint16_t*)(lds + r) = (uint16_t)((v0 & 0xFFu) | ((v1 & 0xFFu) << 8));
    else if constexpr (W == 2) *(uint32_t*)(lds + 2 * r) = (uint32_t)((v0 & 0xFFFFu) | ((v1 & 0xFFFFu) << 16));
    else if constexpr (W == 4) *(uint2*)(lds + 4 * r) = make_uint2((uint32_t)v0, (uint32_t)v1);
    else *(ulonglong2*)(lds + 8 * r) = make_ulonglong2(v0, v1);
  }
}

__global__ __launch_bounds__(256) void k_respack_write(RespackArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kRows * 8];
  const cc_respack_block& b = a.dir[blockIdx.x];
  const uint32_t rows = rows_of(a.n);
  const uint64_t r0 = (uint64_t)blockIdx.x * kRows;
  uint8_t* const area = a.data + (uni(b.offset) - a.data_base);
  if (uni((uint32_t)b.col[0].width)) {  // status, raw: lane t copies rows 16t .. 16t + 15
    const uint8_t* s = a.status + r0;
    const uint32_t q = threadIdx.x * 16;
    if (q < rows) {
      uint4 x;
      if (q + 16 <= rows) {
        x = *(const uint4*)(s + q);
      } else {
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if (q + j < rows) w[j >> 2] |= (uint32_t)s[q + j] << (8 * (j & 3));
        x = make_uint4(w[0], w[1], w[2], w[3]);
      }
      *(uint4*)(area + uni(b.col[0].offset) + q) = x;
    }
  }
  const uint32_t vw = uni((uint32_t)b.col[1].width);
  if (vw == 0) return;
  const uint64_t base = uni(b.col[1].base);
  const uint32_t bytes = r16(rows * vw);
  const uint64_t* v = a.value + r0;
  if (vw == 1) enc64<1>(lds, v, base, rows, bytes);
  else if (vw == 2) enc64<2>(lds, v, base, rows, bytes);
  else if (vw == 4) enc64<4>(lds, v, base, rows, bytes);
  else enc64<8>(lds, v, base, rows, bytes);
  __syncthreads();
  uint8_t* const out = area + uni(b.col[1].offset);
  for (uint32_t i = threadIdx.x * 16; i < bytes; i += kLanes * 16) *(uint4*)(out + i) = *(const uint4*)(lds + i);
}

}  // namespace

int launch_respack(const RespackArgs& a, hipStream_t st) {
  const uint64_t blocks = (a.n + kRows - 1) / kRows;
  if (blocks == 0 || blocks > 0x7FFFFFFFull) return -1;
  hipLaunchKernelGGL(k_respack_measure, dim3((uint32_t)blocks), dim3(kLanes), 0, st, a);
  hipLaunchKernelGGL(k_respack_place, dim3(1), dim3(kLanes), 0, st, a, (uint32_t)blocks);
  hipLaunchKernelGGL(k_respack_write, dim3((uint32_t)blocks), dim3(kLanes), 0, st, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace cc
