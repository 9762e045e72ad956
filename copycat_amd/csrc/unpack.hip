// unpack.hip — packed host batch -> the ordinary wide columns in HBM (include/copycat_apply.h "packed host batches").
//
// k_unpack: one workgroup of 256 lanes per block of CC_PACK_BLOCK_ROWS rows.  The block's directory entry is the same
// for every lane (read through readfirstlane: the branches on mode and width are scalar branches).  Per column (the
// steps are pack_dev.h's "reading" section, shared with the result and event decoders of unpack_res.hip):
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
