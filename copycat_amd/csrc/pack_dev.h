// pack_dev.h — the device core of the packed blob formats: what the three encoders (pack_enc.hip, respack.hip,
// evpack.hip) and the three decoders (unpack.hip; unpack_res.hip for result and event blobs) share.  The host core, and
// the formats' rules, are pack_host.h's.
//
// Every kernel here runs one workgroup of kLanes = 256 lanes per block of kRows = CC_PACK_BLOCK_ROWS rows, and every
// global access of a column is a 16-byte one: lane t owns rows 2t, 2t + 1 of every 512 of a 64-bit column, rows
// 4t .. 4t + 3 of every 1,024 of a 32-bit one and rows 16t .. 16t + 15 of a byte column, so a wave instruction moves
// one contiguous KiB.  Narrow rows pass through ONE LDS image of at most 32 KiB: written (or read) at the rows'
// positions, moved to (or from) the blob lane i the i-th 16 bytes (flush, stage).
// An encoder is three launches: measure (per block: every column's min / max -> the directory entry, offset still 0),
// place (place_blocks: one workgroup scans the blocks' bytes into their offsets) and write (the narrow rows).
#pragma once
#include <hip/hip_runtime.h>

#include "engine_state.h"

namespace cc {
namespace pkd {

constexpr uint32_t kRows = CC_PACK_BLOCK_ROWS;
constexpr uint32_t kLanes = 256;
constexpr uint64_t kSign = 1ull << 63;
static_assert(kPackPlacePass == kLanes, "the placement scan holds one block per lane");

// a value every lane of the wave holds, read through readfirstlane: a branch on it is a scalar branch
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
__device__ inline uint4 col_words(uint32_t mode, uint32_t width, uint32_t entries, uint32_t offset, uint64_t base) {
  return make_uint4(mode | (width << 8) | (entries << 16), offset, (uint32_t)base, (uint32_t)(base >> 32));  // a cc_pack_col
}

// ---- measuring -------------------------------------------------------------------------------------------------------
// sixteen bytes of a u8 column folded into lo / hi: lane t owns rows 16t .. 16t + 15
__device__ inline void fold_bytes(const uint8_t* s, uint32_t rows, uint32_t& lo, uint32_t& hi) {
  const uint32_t q = threadIdx.x * 16;
  if (q >= rows) return;
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
    lo = min(lo, b), hi = max(hi, b);
  }
}

__device__ inline uint32_t shfl_xor(uint32_t v, int off) { return (uint32_t)__shfl_xor((int)v, off); }
__device__ inline uint64_t shfl_xor(uint64_t v, int off) { return (uint64_t)__shfl_xor((unsigned long long)v, off); }

// a 64-bit column's min / max in the unsigned order ([0]) and in the signed one ([1]: the unsigned ones of v ^ 2^63)
struct Range64 {
  uint64_t lo[2] = {~0ull, ~0ull}, hi[2] = {0, 0};
  __device__ void fold(uint64_t v) {
    lo[0] = min(lo[0], v), hi[0] = max(hi[0], v);
    v ^= kSign;
    lo[1] = min(lo[1], v), hi[1] = max(hi[1], v);
  }
  // the narrowest exact width among base = the unsigned and base = the signed minimum; a tie goes to the unsigned base
  __device__ uint32_t pick(uint64_t* base) const {
    uint32_t w = width_of(hi[0] - lo[0]);
    *base = lo[0];
    const uint32_t ws = width_of(hi[1] - lo[1]);
    if (ws < w) w = ws, *base = lo[1] ^ kSign;
    if (w == 8) *base = 0;  // the native width is the raw column
    return w;
  }
};

// (lo, hi) pairs over the workgroup, in three steps around the kernel's one barrier: the wave's by shuffles (every
// lane, for off = 32, 16 .. 1: shuffle_minmax of each pair); lane 0 of each wave parks them in red[wave] (park); after
// the barrier thread 0 merges waves 1 .. 3 into its own (merge).  The kernel keeps ONE loop over `off` for all its
// pairs, and the step takes one pair: a step over whole arrays, or a loop per array, compiles k_evpack_measure to
// 74 - 78 VGPRs instead of 68, one wave per SIMD less.
template <class T>
__device__ inline void shuffle_minmax(T& lo, T& hi, int off) {
  lo = min(lo, shfl_xor(lo, off)), hi = max(hi, shfl_xor(hi, off));
}
template <class T, int N>
__device__ inline void park(const T (&lo)[N], const T (&hi)[N], T (*red)[2 * N]) {
  if (threadIdx.x & 63) return;
#pragma unroll
  for (int i = 0; i < N; ++i) red[threadIdx.x >> 6][2 * i] = lo[i], red[threadIdx.x >> 6][2 * i + 1] = hi[i];
}
template <class T, int N>
__device__ inline void merge(T (&lo)[N], T (&hi)[N], const T (*red)[2 * N]) {
  for (int w = 1; w < 4; ++w)
#pragma unroll
    for (int i = 0; i < N; ++i) lo[i] = min(lo[i], red[w][2 * i]), hi[i] = max(hi[i], red[w][2 * i + 1]);
}

// ---- placing ---------------------------------------------------------------------------------------------------------
// one workgroup: an exclusive scan of the blocks' bytes into their offsets from `data_base` on, kPackPlacePass blocks
// per pass with a carry; the total goes into a device word.  Entry: {rows, bytes, offset lo, offset hi} first.
template <class Entry>
__device__ inline void place_blocks(Entry* dir, uint32_t blocks, uint64_t data_base, unsigned long long* total) {
  __shared__ uint64_t wsum[4];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t carry = data_base;
  for (uint32_t k0 = 0; k0 < blocks; k0 += kPackPlacePass) {
    const uint32_t k = k0 + threadIdx.x;
    uint4 w = make_uint4(0, 0, 0, 0);
    if (k < blocks) w = *(const uint4*)(dir + k);
    uint32_t inc = w.y;  // (a pass sums at most 256 areas of 76 KiB: 32 bits hold it)
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
      *(uint4*)(dir + k) = w;
    }
    carry += all;
    __syncthreads();  // (wsum is written again by the next pass)
  }
  if (threadIdx.x == 0) *total = carry - data_base;
}

// ---- writing ---------------------------------------------------------------------------------------------------------
// `used` bytes of a raw column (a multiple of its element size, from a 16-byte aligned source) register to register,
// the padding up to 16 bytes zero: lane t the t-th 16 bytes of every 4 KiB
__device__ inline void copy_raw(const uint8_t* s, uint8_t* out, uint32_t used) {
  for (uint32_t i = threadIdx.x * 16; i < used; i += kLanes * 16) {
    uint4 x;
    if (i + 16 <= used) {
      x = *(const uint4*)(s + i);
    } else {
      uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (i + j < used) w[j >> 2] |= (uint32_t)s[i + j] << (8 * (j & 3));
      x = make_uint4(w[0], w[1], w[2], w[3]);
    }
    *(uint4*)(out + i) = x;
  }
}

// u32 rows as W-byte offsets from `base` (W = 1, 2): lane t owns rows 4t .. 4t + 3 of every 1,024, one LDS store
template <int W>
__device__ inline void enc32(uint8_t* lds, const uint32_t* v, uint32_t base, uint32_t rows, uint32_t bytes) {
  for (uint32_t r = threadIdx.x * 4; r * W < bytes; r += kLanes * 4) {  // (bytes: a multiple of 16, so of 4 W)
    uint32_t x[4] = {base, base, base, base};  // rows past the tail: the padding is zero
    if (r + 4 <= rows) {
      const uint4 q = *(const uint4*)(v + r);
      x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w;
    } else {
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j)
        if (r + j < rows) x[j] = v[r + j];
    }
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) x[j] -= base;
    if constexpr (W == 1)
      *(uint32_t*)(lds + r) = (x[0] & 0xFFu) | ((x[1] & 0xFFu) << 8) | ((x[2] & 0xFFu) << 16) | (x[3] << 24);
    else
      *(uint2*)(lds + 2 * r) = make_uint2((x[0] & 0xFFFFu) | (x[1] << 16), (x[2] & 0xFFFFu) | (x[3] << 16));
  }
}

// u64 rows as W-byte offsets from `base` (W = 1, 2, 4): lane t owns rows 2t, 2t + 1 of every 512, one LDS store
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
    else *(uint2*)(lds + 4 * r) = make_uint2((uint32_t)v0, (uint32_t)v1);
  }
}

// `bytes` (a multiple of 16) between the LDS image and the blob, lane i the i-th 16 bytes of every 4 KiB.  The barrier
// before completes (flush) or frees (stage) the image, the one after frees (flush) or completes (stage) it.
__device__ inline void image_copy(uint8_t* to, const uint8_t* from, uint32_t bytes) {
  __syncthreads();
  for (uint32_t i = threadIdx.x * 16; i < bytes; i += kLanes * 16) *(uint4*)(to + i) = *(const uint4*)(from + i);
  __syncthreads();
}
__device__ inline void flush(const uint8_t* lds, uint8_t* out, uint32_t bytes) { image_copy(out, lds, bytes); }
__device__ inline void stage(uint8_t* lds, const uint8_t* src, uint32_t bytes) { image_copy(lds, src, bytes); }

// a 64-bit CC_PK_FOR column of `width` bytes: raw rows are copied register to register, narrow ones go through the image
__device__ inline void write_u64(uint8_t* lds, const uint64_t* v, uint32_t width, uint64_t base, uint32_t rows, uint8_t* out) {
  if (width == 0) return;
  if (width == 8) return copy_raw((const uint8_t*)v, out, rows * 8);
  const uint32_t bytes = r16(rows * width);
  if (width == 1) enc64<1>(lds, v, base, rows, bytes);
  else if (width == 2) enc64<2>(lds, v, base, rows, bytes);
  else enc64<4>(lds, v, base, rows, bytes);
  flush(lds, out, bytes);
}

// a 32-bit CC_PK_FOR column by its directory entry: raw rows register to register, narrow ones through the image
__device__ inline void write_u32(uint8_t* lds, const cc_pack_col& c, const uint32_t* v, uint32_t rows, uint8_t* area) {
  const uint32_t w = uni((uint32_t)c.width);
  if (w == 0) return;
  uint8_t* const out = area + uni(c.offset);
  if (w == 4) return copy_raw((const uint8_t*)v, out, rows * 4);
  const uint32_t base = uni((uint32_t)c.base), bytes = r16(rows * w);
  if (w == 1) enc32<1>(lds, v, base, rows, bytes);
  else enc32<2>(lds, v, base, rows, bytes);
  flush(lds, out, bytes);
}

// ---- reading ---------------------------------------------------------------------------------------------------------
// The decoders (unpack.hip, unpack_res.hip): a column's packed rows are staged into the image, then each lane widens
// the rows it owns and issues ONE 16-byte store per group; the lane that holds the tail's last partial group stores
// row by row.  A width-0 column stages nothing and stores the base.
struct Col {  // one directory entry, wave-uniform
  uint32_t mode, width, offset;
  uint64_t base;
};
__device__ inline Col col_of(const cc_pack_col& e) {
  return Col{uni((uint32_t)e.mode), uni((uint32_t)e.width), uni(e.offset), uni(e.base)};
}

template <int W>
__device__ inline uint64_t narrow_at(const uint8_t* lds, uint32_t r) {  // row r's offset, zero-extended
  if constexpr (W == 1) return lds[r];
  else if constexpr (W == 2) return ((const uint16_t*)lds)[r];
  else if constexpr (W == 4) return ((const uint32_t*)lds)[r];
  else if constexpr (W == 8) return ((const uint64_t*)lds)[r];
  else return 0;
}
template <int W>
__device__ inline uint64_t sext(uint64_t v) {
  return (uint64_t)((int64_t)(v << (64 - 8 * W)) >> (64 - 8 * W));
}

// 64-bit columns: lane t owns rows 2t, 2t + 1 of every 512
template <int W, bool REL>
__device__ inline void dec64(const uint8_t* lds, uint64_t* out, const uint64_t* a, uint64_t base, uint32_t rows) {
  for (uint32_t r = threadIdx.x * 2; r < rows; r += kLanes * 2) {
    uint64_t v0 = narrow_at<W>(lds, r), v1 = narrow_at<W>(lds, r + 1);  // (r + 1 < kRows: inside the image)
    const bool pair = r + 1 < rows;
    if constexpr (REL) {
      uint64_t a0, a1 = 0;
      if (pair) {
        const ulonglong2 x = *(const ulonglong2*)(a + r);
        a0 = x.x, a1 = x.y;
      } else {
        a0 = a[r];
      }
      v0 = a0 + sext<W>(v0), v1 = a1 + sext<W>(v1);
    } else {
      v0 += base, v1 += base;
    }
    if (pair) *(ulonglong2*)(out + r) = make_ulonglong2(v0, v1);
    else out[r] = v0;
  }
}

__device__ inline void unpack64(const cc_pack_col& e, const uint8_t* area, uint8_t* lds, uint64_t* out, const uint64_t* a,
                                uint32_t rows) {
  const Col c = col_of(e);
  if (c.width) stage(lds, area + c.offset, r16(rows * c.width));
  if (c.mode == CC_PK_REL_A) {
    if (c.width == 1) dec64<1, true>(lds, out, a, 0, rows);
    else if (c.width == 2) dec64<2, true>(lds, out, a, 0, rows);
    else dec64<4, true>(lds, out, a, 0, rows);
  } else if (c.width == 0) dec64<0, false>(lds, out, nullptr, c.base, rows);
  else if (c.width == 1) dec64<1, false>(lds, out, nullptr, c.base, rows);
  else if (c.width == 2) dec64<2, false>(lds, out, nullptr, c.base, rows);
  else if (c.width == 4) dec64<4, false>(lds, out, nullptr, c.base, rows);
  else dec64<8, false>(lds, out, nullptr, c.base, rows);
}

// the 32-bit column (inst): lane t owns rows 4t .. 4t + 3 of every 1024
template <int W>
__device__ inline void dec32(const uint8_t* lds, uint32_t* out, uint32_t base, uint32_t rows) {
  for (uint32_t r = threadIdx.x * 4; r < rows; r += kLanes * 4) {
    uint32_t v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = base + (uint32_t)narrow_at<W>(lds, r + j);
    if (r + 4 <= rows) {
      *(uint4*)(out + r) = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (r + j < rows) out[r + j] = v[j];
    }
  }
}

__device__ inline void unpack32(const cc_pack_col& e, const uint8_t* area, uint8_t* lds, uint32_t* out, uint32_t rows) {
  const Col c = col_of(e);
  if (c.width) stage(lds, area + c.offset, r16(rows * c.width));
  const uint32_t base = (uint32_t)c.base;
  if (c.width == 0) dec32<0>(lds, out, base, rows);
  else if (c.width == 1) dec32<1>(lds, out, base, rows);
  else if (c.width == 2) dec32<2>(lds, out, base, rows);
  else dec32<4>(lds, out, base, rows);
}

// the 8-bit columns (op, flags): lane t owns rows 16t .. 16t + 15; base is added per byte (modulo 2^8)
__device__ inline uint32_t add_bytes(uint32_t x, uint32_t b) {
  return ((x & 0x7F7F7F7Fu) + (b & 0x7F7F7F7Fu)) ^ ((x ^ b) & 0x80808080u);
}
__device__ inline void unpack8(const cc_pack_col& e, const uint8_t* area, uint8_t* lds, uint8_t* out, uint32_t rows) {
  const Col c = col_of(e);
  if (c.width) stage(lds, area + c.offset, r16(rows));
  const uint32_t b4 = ((uint32_t)c.base & 0xFFu) * 0x01010101u;
  const uint32_t r = threadIdx.x * 16;
  if (r >= rows) return;
  uint4 v = c.width ? *(const uint4*)(lds + r) : make_uint4(0, 0, 0, 0);
  v = make_uint4(add_bytes(v.x, b4), add_bytes(v.y, b4), add_bytes(v.z, b4), add_bytes(v.w, b4));
  if (r + 16 <= rows) {
    *(uint4*)(out + r) = v;
  } else {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (r + j < rows) out[r + j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
  }
}

}  // namespace pkd
}  // namespace cc
