// unpack.hip — packed host batch -> the ordinary wide columns in HBM (include/copycat_apply.h "packed host batches").
//
// k_unpack: one workgroup of 256 lanes per block of CC_PACK_BLOCK_ROWS rows.  The block's directory entry is the same
// for every lane (read through readfirstlane: the branches on mode and width are scalar branches).  Per column:
//   1. the packed rows (at most 32 KiB) go global -> LDS with 16-byte loads, lane i the i-th 16 bytes (pack_dev.h
//      stage): each wave instruction reads one contiguous KiB, whatever the width;
//   2. each lane reads the narrow offsets of the rows it owns from LDS, widens them and writes ONE 16-byte store:
//      two u64 rows, four u32 rows or sixteen u8 rows per lane, so a wave store is one contiguous KiB (narrow stores
//      cost several times a 16-byte store per byte).
// A width-0 column stages nothing and stores the base; the tail block runs the same loop, and the lane that holds the
// last partial group of rows stores them one by one.  b in REL_A mode is decoded after a, and each lane reads back
// the a rows it has just written itself (a and b share the row -> lane mapping), so no fence is needed.
// The kernel moves (packed + wide) bytes once; its bar is the H2D of the same chunk, an order of magnitude slower.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): no scratch, 32 KiB LDS.
#include "pack_dev.h"

namespace cc {

namespace {

using namespace pkd;

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

__global__ __launch_bounds__(256) void k_unpack(UnpackArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kRows * 8];
  const cc_pack_block& b = a.dir[blockIdx.x];
  const uint32_t rows = min(uni(b.rows), kRows);
  const uint8_t* area = a.data + (uni(b.offset) - a.data_base);
  const uint64_t r0 = (uint64_t)blockIdx.x * kRows;
  const uint32_t p = a.present;
  if (p & 1) unpack64(b.col[0], area, lds, a.index + r0, nullptr, rows);
  if (p & 2) unpack64(b.col[1], area, lds, a.time + r0, nullptr, rows);
  if (p & 4) unpack32(b.col[2], area, lds, a.inst + r0, rows);
  if (p & 8) unpack8(b.col[3], area, lds, a.op + r0, rows);
  if (p & 16) unpack8(b.col[4], area, lds, a.flags + r0, rows);
  if (p & 32) unpack64(b.col[5], area, lds, a.key + r0, nullptr, rows);
  if (p & 64) unpack64(b.col[6], area, lds, a.a + r0, nullptr, rows);
  if (p & 128) unpack64(b.col[7], area, lds, a.b + r0, a.a + r0, rows);
  if (p & 256) unpack64(b.col[8], area, lds, a.aux + r0, nullptr, rows);
}

}  // namespace

int launch_unpack(const UnpackArgs& a, uint32_t blocks, hipStream_t st) {
  if (blocks == 0) return 0;
  hipLaunchKernelGGL(k_unpack, dim3(blocks), dim3(kLanes), 0, st, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int pack_err(int code, const char* what) { return set_err(code, what); }

}  // namespace cc

extern "C" int cc_host_register(void* h_ptr, uint64_t bytes) {
  if (!h_ptr || !bytes) return set_err(CC_ERR_INVALID, "host register: null pointer or zero bytes");
  HIPCHECK(hipHostRegister(h_ptr, bytes, hipHostRegisterDefault));
  return CC_OK;
}

extern "C" int cc_host_unregister(void* h_ptr) {
  if (!h_ptr) return set_err(CC_ERR_INVALID, "host unregister: null pointer");
  HIPCHECK(hipHostUnregister(h_ptr));
  return CC_OK;
}
