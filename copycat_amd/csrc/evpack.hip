// evpack.hip — the wide event columns in HBM -> the directory and data areas of a packed event blob
// (include/copycat_apply.h "packed event blobs"); byte for byte what cc_evpack_pack (evpack.cpp) writes.
//
// Three launches on one stream; the kernel boundaries are the only synchronisation (no workgroup waits on another):
//   k_evpack_measure  one workgroup of 256 lanes per block of CC_PACK_BLOCK_ROWS events.  A lane takes four events per
//                     step (one 16-byte load of pos, one of target, two of payload) and sixteen code / src / tag bytes
//                     (one 16-byte load each), and folds them into every column's min / max, the payload's unsigned
//                     and signed min / max (the unsigned ones of v ^ 2^63) and the AND of the two BY_POS conditions:
//                     each of its rows against the row before it (the row before a lane's first one is read again;
//                     the block's first row has none).  A wave shuffle reduction, then the four waves through LDS;
//                     lane 0 applies the format's rules and writes the block's directory entry (offset still 0).
//   k_evpack_place    one workgroup: an exclusive scan of the blocks' bytes into their offsets from `data_base` on
//                     (k_respack_place's scheme: 256 blocks per pass with a carry); the total goes into a device word.
//   k_evpack_write    one workgroup per block.  One column at a time through ONE LDS image of at most 32 KiB (six
//                     images would be 76 KiB, and a static allocation above 64 KiB costs occupancy for nothing): the
//                     lanes write the narrow offsets of their rows into the image (rows past the tail and the padding
//                     are zero), a barrier, the image goes out with 16-byte stores, lane i the i-th 16 bytes, a barrier
//                     before the next column.  A raw-width column is copied register to register.  A BY_POS payload:
//                     the table image is zeroed, a barrier, the run heads (the block's first row, or pos[i] !=
//                     pos[i-1]) store payload - base at pos - pos.base, a barrier, the store.  Width 0 writes nothing;
//                     the tail block runs the same code.
// The encoder reads 19 B per event twice and writes at most 19 B per event; its bar is the D2H of the bytes it saves.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): measure 68 VGPRs, 304 B LDS; place 32 VGPRs, 32 B
// LDS; write 22 VGPRs, 32 KiB LDS; no scratch in any of them.
#include <hip/hip_runtime.h>

#include "engine_state.h"

namespace cc {

namespace {

constexpr uint32_t kRows = CC_PACK_BLOCK_ROWS;
constexpr uint32_t kLanes = 256;
constexpr uint64_t kSign = 1ull << 63;
constexpr uint32_t kPlacePass = kLanes;  // blocks one pass of the placement scan holds (one per lane)
static_assert(sizeof(cc_evpack_block) == 112, "a directory entry is seven 16-byte words");

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

__global__ __launch_bounds__(256) void k_evpack_measure(EvpackArgs a) {
  __shared__ uint64_t red64[4][4];
  __shared__ uint32_t red32[4][11];
  const uint32_t rows = rows_of(a.n);
  const uint64_t r0 = (uint64_t)blockIdx.x * kRows;
  const uint32_t* pos = a.pos + r0;
  const uint32_t* tgt = a.target + r0;
  const uint64_t* pay = a.payload + r0;
  uint32_t plo = ~0u, phi = 0, tlo = ~0u, thi = 0, ok = 1;
  uint64_t ulo = ~0ull, uhi = 0, xlo = ~0ull, xhi = 0;  // x: of v ^ 2^63
  for (uint32_t r = threadIdx.x * 4; r < rows; r += kLanes * 4) {
    uint32_t p[4], t[4];
    uint64_t v[4];
    if (r + 4 <= rows) {
      const uint4 pp = *(const uint4*)(pos + r), tt = *(const uint4*)(tgt + r);
      const ulonglong2 v01 = *(const ulonglong2*)(pay + r), v23 = *(const ulonglong2*)(pay + r + 2);
      p[0] = pp.x, p[1] = pp.y, p[2] = pp.z, p[3] = pp.w;
      t[0] = tt.x, t[1] = tt.y, t[2] = tt.z, t[3] = tt.w;
      v[0] = v01.x, v[1] = v01.y, v[2] = v23.x, v[3] = v23.y;
    } else {  // (the tail's last group: the last row stands in for the rows past the end)
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t i = min(r + j, rows - 1);
        p[j] = pos[i], t[j] = tgt[i], v[j] = pay[i];
      }
    }
    uint32_t pp = p[0];  // the row before: the block's first row has none
    uint64_t pv = v[0];
    if (r) pp = pos[r - 1], pv = pay[r - 1];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      ok &= (p[j] > pp) | ((p[j] == pp) & (v[j] == pv));
      pp = p[j], pv = v[j];
      plo = min(plo, p[j]), phi = max(phi, p[j]);
      tlo = min(tlo, t[j]), thi = max(thi, t[j]);
      ulo = min(ulo, v[j]), uhi = max(uhi, v[j]);
      const uint64_t x = v[j] ^ kSign;
      xlo = min(xlo, x), xhi = max(xhi, x);
    }
  }
  uint32_t clo = 255, chi = 0, slo = 255, shi = 0, glo = 255, ghi = 0;
  fold_bytes(a.code + r0, rows, clo, chi);
  fold_bytes(a.src + r0, rows, slo, shi);
  fold_bytes(a.tag + r0, rows, glo, ghi);
  for (int off = 32; off; off >>= 1) {
    ulo = min(ulo, (uint64_t)__shfl_xor((unsigned long long)ulo, off));
    uhi = max(uhi, (uint64_t)__shfl_xor((unsigned long long)uhi, off));
    xlo = min(xlo, (uint64_t)__shfl_xor((unsigned long long)xlo, off));
    xhi = max(xhi, (uint64_t)__shfl_xor((unsigned long long)xhi, off));
    plo = min(plo, (uint32_t)__shfl_xor((int)plo, off)), phi = max(phi, (uint32_t)__shfl_xor((int)phi, off));
    tlo = min(tlo, (uint32_t)__shfl_xor((int)tlo, off)), thi = max(thi, (uint32_t)__shfl_xor((int)thi, off));
    clo = min(clo, (uint32_t)__shfl_xor((int)clo, off)), chi = max(chi, (uint32_t)__shfl_xor((int)chi, off));
    slo = min(slo, (uint32_t)__shfl_xor((int)slo, off)), shi = max(shi, (uint32_t)__shfl_xor((int)shi, off));
    glo = min(glo, (uint32_t)__shfl_xor((int)glo, off)), ghi = max(ghi, (uint32_t)__shfl_xor((int)ghi, off));
    ok &= (uint32_t)__shfl_xor((int)ok, off);
  }
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red64[wave][0] = ulo, red64[wave][1] = uhi, red64[wave][2] = xlo, red64[wave][3] = xhi;
    uint32_t* q = red32[wave];
    q[0] = plo, q[1] = phi, q[2] = tlo, q[3] = thi, q[4] = clo, q[5] = chi, q[6] = slo, q[7] = shi, q[8] = glo, q[9] = ghi;
    q[10] = ok;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int w = 1; w < 4; ++w) {
    ulo = min(ulo, red64[w][0]), uhi = max(uhi, red64[w][1]);
    xlo = min(xlo, red64[w][2]), xhi = max(xhi, red64[w][3]);
    const uint32_t* q = red32[w];
    plo = min(plo, q[0]), phi = max(phi, q[1]), tlo = min(tlo, q[2]), thi = max(thi, q[3]);
    clo = min(clo, q[4]), chi = max(chi, q[5]), slo = min(slo, q[6]), shi = max(shi, q[7]);
    glo = min(glo, q[8]), ghi = max(ghi, q[9]);
    ok &= q[10];
  }
  const uint32_t pw = width_of(phi - plo), tw = width_of(thi - tlo);
  const uint32_t cw = chi != clo, sw = shi != slo, gw = ghi != glo;
  // the narrowest exact width among base = the unsigned and base = the signed minimum; a tie goes to the unsigned base
  uint32_t vw = width_of(uhi - ulo);
  uint64_t vbase = ulo;
  const uint32_t ws = width_of(xhi - xlo);
  if (ws < vw) vw = ws, vbase = xlo ^ kSign;
  if (vw == 8) vbase = 0;  // the native width is the raw column
  // a payload that is a function of a non-decreasing pos goes as a table by pos when that is smaller
  const uint32_t E = phi - plo + 1;  // (used only when pw <= 2: at most 65,536)
  const bool by_pos = ok && vw && pw <= 2 && r16(E * vw) < r16(rows * vw);
  uint32_t at = 0;
  uint4* const e = (uint4*)(a.dir + blockIdx.x);
  e[1] = col_words(CC_PK_FOR, pw, 0, at, pw == 4 ? 0 : plo), at += r16(rows * pw);
  e[2] = col_words(CC_PK_FOR, tw, 0, at, tw == 4 ? 0 : tlo), at += r16(rows * tw);
  e[3] = col_words(CC_PK_FOR, cw, 0, at, cw ? 0 : clo), at += r16(rows * cw);
  e[4] = col_words(CC_PK_FOR, sw, 0, at, sw ? 0 : slo), at += r16(rows * sw);
  e[5] = col_words(CC_PK_FOR, gw, 0, at, gw ? 0 : glo), at += r16(rows * gw);
  e[6] = col_words(by_pos ? CC_PK_BY_POS : CC_PK_FOR, vw, by_pos ? E : 0, at, vbase), at += r16((by_pos ? E : rows) * vw);
  e[0] = make_uint4(rows, at, 0, 0);  // (offset: k_evpack_place)
}

__global__ __launch_bounds__(256) void k_evpack_place(EvpackArgs a, uint32_t blocks) {
  __shared__ uint64_t wsum[4];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t carry = a.data_base;
  for (uint32_t k0 = 0; k0 < blocks; k0 += kPlacePass) {
    const uint32_t k = k0 + threadIdx.x;
    uint4 w = make_uint4(0, 0, 0, 0);  // {rows, bytes, offset lo, offset hi}
    if (k < blocks) w = *(const uint4*)(a.dir + k);
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
      *(uint4*)(a.dir + k) = w;
    }
    carry += all;
    __syncthreads();  // (wsum is written again by the next pass)
  }
  if (threadIdx.x == 0) *a.total = carry - a.data_base;
}

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

// the u32 rows as W-byte offsets from `base`: lane t owns rows 4t .. 4t + 3 of every 1,024, written as one LDS store
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

// the payload rows as W-byte offsets from `base`: lane t owns rows 2t, 2t + 1 of every 512, written as one LDS store
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

// the LDS image's first `bytes` (a multiple of 16) to `out`, lane i the i-th 16 bytes; the image is free again after it
__device__ inline void flush(const uint8_t* lds, uint8_t* out, uint32_t bytes) {
  __syncthreads();
  for (uint32_t i = threadIdx.x * 16; i < bytes; i += kLanes * 16) *(uint4*)(out + i) = *(const uint4*)(lds + i);
  __syncthreads();
}

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

__global__ __launch_bounds__(256) void k_evpack_write(EvpackArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kRows * 8];
  const cc_evpack_block& b = a.dir[blockIdx.x];
  const uint32_t rows = rows_of(a.n);
  const uint64_t r0 = (uint64_t)blockIdx.x * kRows;
  uint8_t* const area = a.data + (uni(b.offset) - a.data_base);
  const uint32_t* pos = a.pos + r0;
  write_u32(lds, b.col[0], pos, rows, area);
  write_u32(lds, b.col[1], a.target + r0, rows, area);
  if (uni((uint32_t)b.col[2].width)) copy_raw(a.code + r0, area + uni(b.col[2].offset), rows);
  if (uni((uint32_t)b.col[3].width)) copy_raw(a.src + r0, area + uni(b.col[3].offset), rows);
  if (uni((uint32_t)b.col[4].width)) copy_raw(a.tag + r0, area + uni(b.col[4].offset), rows);
  const cc_pack_col& pc = b.col[5];
  const uint32_t vw = uni((uint32_t)pc.width);
  if (vw == 0) return;
  const uint64_t base = uni(pc.base);
  const uint64_t* v = a.payload + r0;
  uint8_t* const out = area + uni(pc.offset);
  if (uni((uint32_t)pc.mode) != CC_PK_BY_POS) {
    if (vw == 8) return copy_raw((const uint8_t*)v, out, rows * 8);
    const uint32_t bytes = r16(rows * vw);
    if (vw == 1) enc64<1>(lds, v, base, rows, bytes);
    else if (vw == 2) enc64<2>(lds, v, base, rows, bytes);
    else enc64<4>(lds, v, base, rows, bytes);
    return flush(lds, out, bytes);
  }
  // a table by pos: E entries (E < rows, so at most 32 KiB), the entries no row refers to zero
  const uint32_t bytes = r16(uni((uint32_t)pc.reserved16) * vw);
  const uint32_t pbase = uni((uint32_t)b.col[0].base);  // (pos width <= 2: the block's smallest pos)
  for (uint32_t i = threadIdx.x * 16; i < bytes; i += kLanes * 16) *(uint4*)(lds + i) = make_uint4(0, 0, 0, 0);
  __syncthreads();
  for (uint32_t r = threadIdx.x * 4; r < rows; r += kLanes * 4) {
    uint32_t p[4];
    if (r + 4 <= rows) {
      const uint4 q = *(const uint4*)(pos + r);
      p[0] = q.x, p[1] = q.y, p[2] = q.z, p[3] = q.w;
    } else {
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) p[j] = pos[min(r + j, rows - 1)];
    }
    uint32_t before = r ? pos[r - 1] : ~p[0];  // (the block's first row is a run head)
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      if (r + j < rows && p[j] != before) {
        const uint64_t x = v[r + j] - base;
        uint8_t* const t = lds + (p[j] - pbase) * vw;
        if (vw == 1) *t = (uint8_t)x;
        else if (vw == 2) *(uint16_t*)t = (uint16_t)x;
        else if (vw == 4) *(uint32_t*)t = (uint32_t)x;
        else *(uint64_t*)t = x;
      }
      before = p[j];
    }
  }
  flush(lds, out, bytes);
}

}  // namespace

int launch_evpack(const EvpackArgs& a, hipStream_t st) {
  const uint64_t blocks = (a.n + kRows - 1) / kRows;
  if (blocks == 0 || blocks > 0x7FFFFFFFull) return -1;
  hipLaunchKernelGGL(k_evpack_measure, dim3((uint32_t)blocks), dim3(kLanes), 0, st, a);
  hipLaunchKernelGGL(k_evpack_place, dim3(1), dim3(kLanes), 0, st, a, (uint32_t)blocks);
  hipLaunchKernelGGL(k_evpack_write, dim3((uint32_t)blocks), dim3(kLanes), 0, st, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace cc
