// evpack.hip — the wide event columns in HBM -> the directory and data areas of a packed event blob
// (include/copycat_apply.h "packed event blobs"); byte for byte what cc_evpack_pack (evpack.cpp) writes.
//
// Three launches on one stream (pack_dev.h: the lanes' rows, the LDS image, the shared steps); the kernel boundaries
// are the only synchronisation (no workgroup waits on another):
//   k_evpack_measure  one workgroup per block.  A lane takes four events per step (one 16-byte load of pos, one of
//                     target, two of payload) and sixteen code / src / tag bytes (one 16-byte load each), and folds
//                     them into every column's min / max, the payload's unsigned and signed min / max and the AND of
//                     the two BY_POS conditions: each of its rows against the row before it (the row before a lane's
//                     first one is read again; the block's first row has none).  A wave shuffle reduction, then the
//                     four waves through LDS; lane 0 applies the format's rules and writes the block's directory entry
//                     (offset still 0).
//   k_evpack_place    one workgroup: place_blocks.
//   k_evpack_write    one workgroup per block.  One column at a time through ONE LDS image of at most 32 KiB (six
//                     images would be 76 KiB, and a static allocation above 64 KiB costs occupancy for nothing): the
//                     lanes write the narrow offsets of their rows into the image (rows past the tail and the padding
//                     are zero), a barrier, the image goes out with 16-byte stores, lane i the i-th 16 bytes, a barrier
//                     before the next column.  A raw-width column is copied register to register.  A BY_POS payload:
//                     the table image is zeroed, a barrier, the run heads (the block's first row, or pos[i] !=
//                     pos[i-1]) store payload - base at pos - pos.base, a barrier, the store.  Width 0 writes nothing;
//                     the tail block runs the same code.
// The encoder reads 19 B per event twice and writes at most 19 B per event; its bar is the D2H of the bytes it saves.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): measure 68 VGPRs, 304 B LDS; place 34 VGPRs, 32 B
// LDS; write 22 VGPRs, 32 KiB LDS; no scratch in any of them.
#include "pack_dev.h"

namespace cc {

namespace {

using namespace pkd;

static_assert(sizeof(cc_evpack_block) == 112, "a directory entry is seven 16-byte words");

__global__ __launch_bounds__(256) void k_evpack_measure(EvpackArgs a) {
  __shared__ uint64_t red64[4][4];
  __shared__ uint32_t red32[4][10], red_ok[4];
  const uint32_t rows = rows_of(a.n);
  const uint64_t r0 = (uint64_t)blockIdx.x * kRows;
  const uint32_t* pos = a.pos + r0;
  const uint32_t* tgt = a.target + r0;
  const uint64_t* pay = a.payload + r0;
  uint32_t lo[5] = {~0u, ~0u}, hi[5] = {0, 0}, ok = 1;  // pos, target, code, src, tag (the bytes: after the loop)
  Range64 val;
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
      lo[0] = min(lo[0], p[j]), hi[0] = max(hi[0], p[j]);
      lo[1] = min(lo[1], t[j]), hi[1] = max(hi[1], t[j]);
      val.fold(v[j]);
    }
  }
  lo[2] = lo[3] = lo[4] = 255, hi[2] = hi[3] = hi[4] = 0;
  fold_bytes(a.code + r0, rows, lo[2], hi[2]);
  fold_bytes(a.src + r0, rows, lo[3], hi[3]);
  fold_bytes(a.tag + r0, rows, lo[4], hi[4]);
  for (int off = 32; off; off >>= 1) {
#pragma unroll
    for (int i = 0; i < 2; ++i) shuffle_minmax(val.lo[i], val.hi[i], off);
#pragma unroll
    for (int c = 0; c < 5; ++c) shuffle_minmax(lo[c], hi[c], off);
    ok &= shfl_xor(ok, off);
  }
  park(val.lo, val.hi, red64), park(lo, hi, red32);
  if ((threadIdx.x & 63) == 0) red_ok[threadIdx.x >> 6] = ok;
  __syncthreads();
  if (threadIdx.x != 0) return;
  merge(val.lo, val.hi, red64), merge(lo, hi, red32);
  ok &= red_ok[1] & red_ok[2] & red_ok[3];
  uint32_t w[5];  // pos / target: the native width is the raw column; a byte column is constant or raw
#pragma unroll
  for (int c = 0; c < 5; ++c) w[c] = width_of(hi[c] - lo[c]);
  uint64_t vbase;
  const uint32_t vw = val.pick(&vbase);
  // a payload that is a function of a non-decreasing pos goes as a table by pos when that is smaller
  const uint32_t E = hi[0] - lo[0] + 1;  // (used only when the pos width <= 2: at most 65,536)
  const bool by_pos = ok && vw && w[0] <= 2 && r16(E * vw) < r16(rows * vw);
  uint32_t at = 0;
  uint4* const e = (uint4*)(a.dir + blockIdx.x);
#pragma unroll
  for (int c = 0; c < 5; ++c)
    e[1 + c] = col_words(CC_PK_FOR, w[c], 0, at, w[c] == (c < 2 ? 4 : 1) ? 0 : lo[c]), at += r16(rows * w[c]);
  e[6] = col_words(by_pos ? CC_PK_BY_POS : CC_PK_FOR, vw, by_pos ? E : 0, at, vbase), at += r16((by_pos ? E : rows) * vw);
  e[0] = make_uint4(rows, at, 0, 0);  // (offset: k_evpack_place)
}

__global__ __launch_bounds__(256) void k_evpack_place(EvpackArgs a, uint32_t blocks) {
  place_blocks(a.dir, blocks, a.data_base, a.total);
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
  if (uni((uint32_t)pc.mode) != CC_PK_BY_POS) return write_u64(lds, v, vw, base, rows, out);
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
