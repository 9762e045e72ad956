// respack.hip — the wide result columns in HBM -> the directory and data areas of a packed result blob
// (include/copycat_apply.h "packed result blobs"); byte for byte what cc_respack_pack (respack.cpp) writes.
//
// Three launches on one stream (pack_dev.h: the lanes' rows, the LDS image, the shared steps); the kernel boundaries
// are the only synchronisation (no workgroup waits on another):
//   k_respack_measure  one workgroup per block.  Each lane folds the rows it owns (two u64 values per 16-byte load,
//                      sixteen status bytes per 16-byte load) into the value's unsigned and signed min / max and the
//                      status min / max; a wave shuffle reduction, then the four waves through LDS; lane 0 writes the
//                      block's directory entry ({mode, width, base} per column, the area's bytes; offset still 0).
//   k_respack_place    one workgroup: place_blocks.
//   k_respack_write    one workgroup per block.  Narrow values: each lane reloads its two rows with one 16-byte load,
//                      subtracts the base and writes the pair of narrow offsets as ONE LDS store at the rows' position
//                      (rows past the tail and the padding up to 16 bytes are zero); the image goes out with 16-byte
//                      stores.  A raw column (status, width-8 values) has the image's row -> lane mapping already and
//                      is copied register to register.  Width 0 writes nothing; the tail block runs the same code.
// The encoder reads 9 B per row twice and writes at most 9 B per row; its bar is the D2H of the bytes it saves.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): measure 34 VGPRs, 160 B LDS; place 34 VGPRs, 32 B
// LDS; write 17 VGPRs, 32 KiB LDS; no scratch in any of them.
#include "pack_dev.h"

namespace cc {

namespace {

using namespace pkd;

__global__ __launch_bounds__(256) void k_respack_measure(RespackArgs a) {
  __shared__ uint64_t red[4][4];
  __shared__ uint32_t sred[4][2];
  const uint32_t rows = rows_of(a.n);
  const uint64_t r0 = (uint64_t)blockIdx.x * kRows;
  const uint64_t* v = a.value + r0;
  Range64 val;
  for (uint32_t r = threadIdx.x * 2; r < rows; r += kLanes * 2) {
    if (r + 1 < rows) {
      const ulonglong2 x = *(const ulonglong2*)(v + r);
      val.fold(x.x), val.fold(x.y);
    } else {
      val.fold(v[r]);
    }
  }
  uint32_t slo[1] = {255}, shi[1] = {0};
  fold_bytes(a.status + r0, rows, slo[0], shi[0]);
  for (int off = 32; off; off >>= 1) {
#pragma unroll
    for (int i = 0; i < 2; ++i) shuffle_minmax(val.lo[i], val.hi[i], off);
    shuffle_minmax(slo[0], shi[0], off);
  }
  park(val.lo, val.hi, red), park(slo, shi, sred);
  __syncthreads();
  if (threadIdx.x != 0) return;
  merge(val.lo, val.hi, red), merge(slo, shi, sred);
  uint64_t vbase;
  const uint32_t vw = val.pick(&vbase);
  const uint32_t sw = shi[0] != slo[0];
  const uint32_t voff = r16(rows * sw);
  uint4* const e = (uint4*)(a.dir + blockIdx.x);
  e[0] = make_uint4(rows, voff + r16(rows * vw), 0, 0);  // (offset: k_respack_place)
  e[1] = col_words(CC_PK_FOR, sw, 0, 0, sw ? 0 : slo[0]);
  e[2] = col_words(CC_PK_FOR, vw, 0, voff, vbase);
}

__global__ __launch_bounds__(256) void k_respack_place(RespackArgs a, uint32_t blocks) {
  place_blocks(a.dir, blocks, a.data_base, a.total);
}

__global__ __launch_bounds__(256) void k_respack_write(RespackArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kRows * 8];
  const cc_respack_block& b = a.dir[blockIdx.x];
  const uint32_t rows = rows_of(a.n);
  const uint64_t r0 = (uint64_t)blockIdx.x * kRows;
  uint8_t* const area = a.data + (uni(b.offset) - a.data_base);
  if (uni((uint32_t)b.col[0].width)) copy_raw(a.status + r0, area + uni(b.col[0].offset), rows);
  write_u64(lds, a.value + r0, uni((uint32_t)b.col[1].width), uni(b.col[1].base), rows, area + uni(b.col[1].offset));
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
