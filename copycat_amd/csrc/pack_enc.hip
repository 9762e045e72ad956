// pack_enc.hip — the wide batch columns in HBM -> the directory and data areas of a packed batch blob
// (include/copycat_apply.h "packed host batches"); byte for byte what cc_pack_batch (pack.cpp) writes.
//
// Three launches on one stream (pack_dev.h: the lanes' rows, the LDS image, the shared steps); the kernel boundaries
// are the only synchronisation (no workgroup waits on another):
//   k_pack_measure  one workgroup per block.  The columns `present` names are measured ONE AFTER THE OTHER (the mask is
//                   a kernel argument: the column loop is a chain of scalar branches): a lane folds the rows it owns
//                   into the column's min / max (a 64-bit column: the unsigned and the signed order; b with a present:
//                   also the signed min / max of b - a modulo 2^64, from the same pass over b and one more 16-byte load
//                   of a), the wave reduces them by shuffles and lane 0 of each wave parks them in the column's own LDS
//                   cells.  One barrier after the last column; then lane 0 merges the four waves column by column,
//                   applies the format's rules (choose64, choose_small, choose_b of pack.cpp) and writes the block's
//                   directory entry (offset still 0; the entries of absent columns 0).
//                   Column by column, not all columns in one pass: six 64-bit ranges in two orders plus the REL_A range
//                   are about 60 VGPRs of accumulators alone (counted, not compiled: the one-pass shape was not
//                   built); one column at a time holds 12, the kernel compiles to 37 VGPRs, which is full occupancy
//                   (8 waves per SIMD), and each row's bytes are read once in both shapes.
//   k_pack_place    one workgroup: place_blocks.
//   k_pack_write    one workgroup per block, one column at a time through ONE LDS image of at most 32 KiB, as
//                   k_evpack_write: narrow offsets into the image at the rows' positions (rows past the tail and the
//                   padding zero), out with 16-byte stores; a raw-width column register to register; width 0 nothing.
//                   REL_A: each lane loads its two rows of b and of a and stores (W)(b - a) as one LDS store.
// The encoder reads each present column's bytes twice (a three times when b is measured for REL_A and written as REL_A)
// and writes at most as many once; its bar is the D2H of the wide columns, an order of magnitude slower per byte.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): measure 37 VGPRs, 928 B LDS; place 34 VGPRs,
// 32 B LDS; write 18 VGPRs, 32 KiB LDS; no scratch in any of them (the build checks it: build.py REPORT_SRCS).
#include "pack_dev.h"

namespace cc {

namespace {

using namespace pkd;

static_assert(sizeof(cc_pack_block) == 160, "a directory entry is ten 16-byte words");

constexpr int kCol64[6] = {0, 1, 5, 6, 7, 8};  // index, time, key, a, b, aux: the 64-bit columns, in red64 order
constexpr int kColA = 6, kColB = 7;

// one 64-bit column of the block measured and parked; `a` non-null: v is b, and b - a is measured with it
__device__ inline void measure64(const uint64_t* v, const uint64_t* a, uint32_t rows, uint64_t (*red)[4], uint64_t (*rel)[2]) {
  Range64 val;
  uint64_t dlo[1] = {~0ull}, dhi[1] = {0};  // the signed order of b - a: the unsigned one of (b - a) ^ 2^63
  for (uint32_t r = threadIdx.x * 2; r < rows; r += kLanes * 2) {
    if (r + 1 < rows) {
      const ulonglong2 x = *(const ulonglong2*)(v + r);
      val.fold(x.x), val.fold(x.y);
      if (a) {
        const ulonglong2 y = *(const ulonglong2*)(a + r);
        const uint64_t d0 = (x.x - y.x) ^ kSign, d1 = (x.y - y.y) ^ kSign;
        dlo[0] = min(dlo[0], min(d0, d1)), dhi[0] = max(dhi[0], max(d0, d1));
      }
    } else {
      val.fold(v[r]);
      if (a) {
        const uint64_t d = (v[r] - a[r]) ^ kSign;
        dlo[0] = min(dlo[0], d), dhi[0] = max(dhi[0], d);
      }
    }
  }
  for (int off = 32; off; off >>= 1) {
#pragma unroll
    for (int i = 0; i < 2; ++i) shuffle_minmax(val.lo[i], val.hi[i], off);
    if (a) shuffle_minmax(dlo[0], dhi[0], off);
  }
  park(val.lo, val.hi, red);
  if (a) park(dlo, dhi, rel);
}

// the u32 column (inst): lane t owns rows 4t .. 4t + 3 of every 1,024
__device__ inline void measure32(const uint32_t* v, uint32_t rows, uint32_t (*red)[2]) {
  uint32_t lo[1] = {~0u}, hi[1] = {0};
  for (uint32_t r = threadIdx.x * 4; r < rows; r += kLanes * 4) {
    uint32_t x[4];
    if (r + 4 <= rows) {
      const uint4 q = *(const uint4*)(v + r);
      x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w;
    } else {  // (the tail's last group: the last row stands in for the rows past the end)
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) x[j] = v[min(r + j, rows - 1)];
    }
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) lo[0] = min(lo[0], x[j]), hi[0] = max(hi[0], x[j]);
  }
  for (int off = 32; off; off >>= 1) shuffle_minmax(lo[0], hi[0], off);
  park(lo, hi, red);
}

__device__ inline void measure8(const uint8_t* v, uint32_t rows, uint32_t (*red)[2]) {
  uint32_t lo[1] = {255}, hi[1] = {0};
  fold_bytes(v, rows, lo[0], hi[0]);
  for (int off = 32; off; off >>= 1) shuffle_minmax(lo[0], hi[0], off);
  park(lo, hi, red);
}

__global__ __launch_bounds__(256) void k_pack_measure(PackEncArgs a) {
  __shared__ uint64_t red64[6][4][4], rel[4][2];
  __shared__ uint32_t red32[3][4][2];  // inst, op, flags
  const uint32_t rows = rows_of(a.n);
  const uint64_t r0 = (uint64_t)blockIdx.x * kRows;
  const uint32_t p = a.present;
  const bool rel_a = (p >> kColA & 1) && (p >> kColB & 1);
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int c = kCol64[k];
    if (!(p >> c & 1)) continue;
    const uint64_t* const av = c == kColB && rel_a ? (const uint64_t*)a.col[kColA] + r0 : nullptr;
    measure64((const uint64_t*)a.col[c] + r0, av, rows, red64[k], rel);
  }
  if (p & 4) measure32((const uint32_t*)a.col[2] + r0, rows, red32[0]);
  if (p & 8) measure8((const uint8_t*)a.col[3] + r0, rows, red32[1]);
  if (p & 16) measure8((const uint8_t*)a.col[4] + r0, rows, red32[2]);
  __syncthreads();
  if (threadIdx.x != 0) return;
  uint4* const e = (uint4*)(a.dir + blockIdx.x);
  uint32_t at = 0;
  for (int c = 0; c < 9; ++c) {
    uint4 words = make_uint4(0, 0, 0, 0);  // an absent column's entry
    if (p >> c & 1) {
      uint32_t mode = CC_PK_FOR, w;
      uint64_t base;
      if (c >= 2 && c <= 4) {  // choose_small: base = the minimum; the native width is the raw column
        const uint32_t(*red)[2] = red32[c - 2];
        uint32_t lo = red[0][0], hi = red[0][1];
        for (int v = 1; v < 4; ++v) lo = min(lo, red[v][0]), hi = max(hi, red[v][1]);
        w = width_of(hi - lo);
        base = w == (c == 2 ? 4u : 1u) ? 0 : lo;
      } else {  // choose64, and on b choose_b
        const uint64_t(*red)[4] = red64[c < 2 ? c : c - 3];
        Range64 val;
        for (int v = 0; v < 4; ++v)
#pragma unroll
          for (int i = 0; i < 2; ++i) val.lo[i] = min(val.lo[i], red[v][2 * i]), val.hi[i] = max(val.hi[i], red[v][2 * i + 1]);
        w = val.pick(&base);
        if (c == kColB && rel_a && w > 1) {  // REL_A only when strictly narrower than FOR, and FOR above one byte
          uint64_t ulo = rel[0][0], uhi = rel[0][1];
          for (int v = 1; v < 4; ++v) ulo = min(ulo, rel[v][0]), uhi = max(uhi, rel[v][1]);
          const int64_t dlo = (int64_t)(ulo ^ kSign), dhi = (int64_t)(uhi ^ kSign);
          const uint32_t wr = dlo >= -128 && dhi <= 127 ? 1 : dlo >= -32768 && dhi <= 32767 ? 2 : dlo >= INT32_MIN && dhi <= INT32_MAX ? 4 : 9;
          if (wr < w) mode = CC_PK_REL_A, w = wr, base = 0;
        }
      }
      words = col_words(mode, w, 0, at, base);
      at += r16(rows * w);
    }
    e[1 + c] = words;
  }
  e[0] = make_uint4(rows, at, 0, 0);  // (offset: k_pack_place)
}

__global__ __launch_bounds__(256) void k_pack_place(PackEncArgs a, uint32_t blocks) {
  place_blocks(a.dir, blocks, a.data_base, a.total);
}

// b as W-byte signed offsets from the same row's a (W = 1, 2, 4): enc64's rows and its one LDS store
template <int W>
__device__ inline void enc_rel(uint8_t* lds, const uint64_t* b, const uint64_t* a, uint32_t rows, uint32_t bytes) {
  for (uint32_t r = threadIdx.x * 2; r * W < bytes; r += kLanes * 2) {
    uint64_t d0 = 0, d1 = 0;  // rows past the tail: the padding is zero
    if (r + 1 < rows) {
      const ulonglong2 x = *(const ulonglong2*)(b + r), y = *(const ulonglong2*)(a + r);
      d0 = x.x - y.x, d1 = x.y - y.y;
    } else if (r < rows) {
      d0 = b[r] - a[r];
    }
    if constexpr (W == 1) *(uint16_t*)(lds + r) = (uint16_t)((d0 & 0xFFu) | ((d1 & 0xFFu) << 8));
    else if constexpr (W == 2) *(uint32_t*)(lds + 2 * r) = (uint32_t)((d0 & 0xFFFFu) | ((d1 & 0xFFFFu) << 16));
    else *(uint2*)(lds + 4 * r) = make_uint2((uint32_t)d0, (uint32_t)d1);
  }
}

__device__ inline void put64(uint8_t* lds, const cc_pack_col& c, const void* v, uint64_t r0, uint32_t rows, uint8_t* area) {
  write_u64(lds, (const uint64_t*)v + r0, uni((uint32_t)c.width), uni(c.base), rows, area + uni(c.offset));
}
__device__ inline void put8(const cc_pack_col& c, const void* v, uint64_t r0, uint32_t rows, uint8_t* area) {
  if (uni((uint32_t)c.width)) copy_raw((const uint8_t*)v + r0, area + uni(c.offset), rows);
}

__global__ __launch_bounds__(256) void k_pack_write(PackEncArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kRows * 8];
  const cc_pack_block& b = a.dir[blockIdx.x];
  const uint32_t rows = rows_of(a.n);
  const uint64_t r0 = (uint64_t)blockIdx.x * kRows;
  uint8_t* const area = a.data + (uni(b.offset) - a.data_base);
  const uint32_t p = a.present;
  if (p & 1) put64(lds, b.col[0], a.col[0], r0, rows, area);
  if (p & 2) put64(lds, b.col[1], a.col[1], r0, rows, area);
  if (p & 4) write_u32(lds, b.col[2], (const uint32_t*)a.col[2] + r0, rows, area);
  if (p & 8) put8(b.col[3], a.col[3], r0, rows, area);
  if (p & 16) put8(b.col[4], a.col[4], r0, rows, area);
  if (p & 32) put64(lds, b.col[5], a.col[5], r0, rows, area);
  if (p & 64) put64(lds, b.col[6], a.col[6], r0, rows, area);
  if (p & 128) {
    const cc_pack_col& c = b.col[kColB];
    if (uni((uint32_t)c.mode) != CC_PK_REL_A) {
      put64(lds, c, a.col[kColB], r0, rows, area);
    } else {  // (the measure pass took REL_A only with a present)
      const uint64_t* const bv = (const uint64_t*)a.col[kColB] + r0;
      const uint64_t* const av = (const uint64_t*)a.col[kColA] + r0;
      const uint32_t w = uni((uint32_t)c.width), bytes = r16(rows * w);
      if (w == 1) enc_rel<1>(lds, bv, av, rows, bytes);
      else if (w == 2) enc_rel<2>(lds, bv, av, rows, bytes);
      else enc_rel<4>(lds, bv, av, rows, bytes);
      flush(lds, area + uni(c.offset), bytes);
    }
  }
  if (p & 256) put64(lds, b.col[8], a.col[8], r0, rows, area);
}

}  // namespace

int launch_pack_enc(const PackEncArgs& a, hipStream_t st) {
  const uint64_t blocks = (a.n + kRows - 1) / kRows;
  if (blocks == 0 || blocks > 0x7FFFFFFFull) return -1;
  hipLaunchKernelGGL(k_pack_measure, dim3((uint32_t)blocks), dim3(kLanes), 0, st, a);
  hipLaunchKernelGGL(k_pack_place, dim3(1), dim3(kLanes), 0, st, a, (uint32_t)blocks);
  hipLaunchKernelGGL(k_pack_write, dim3((uint32_t)blocks), dim3(kLanes), 0, st, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace cc
