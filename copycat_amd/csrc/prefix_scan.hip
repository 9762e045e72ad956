// prefix_scan.hip — the stop scan of cc_apply_batch_prefix on device-resident columns (gfx950, wave64).
//
// cc_apply_batch_host_prefix walks the host's inst / op / aux columns on the CPU to find the first row that could
// overflow a coordination collection (host_path.hip).  With the columns in HBM that walk is these kernels: they find,
// without copying a column to the host, the first row in log order of [lo, hi) that
//   * adds an entry (adds_entry, common.h: lock with a timeout != 0, election listen, group join, value listen,
//     queue add / offer, topic listen, bus join / register; a row whose instance slot is out of range or unbound never counts), and
//   * meets its resource's block full: its entry count (coord_used, common.h: CoordHdr.n, a bus's members +
//     registrations) + the adding rows for that resource before it in [lo, hi) equals
//     coord_cap.
// Removals are not counted, as on the host: the row is an upper bound's stop, and the driver reads the block's exact
// count once the rows before it have applied.
//
//   pass 1  k_px_count        one streaming read of inst / op (5 B per row; aux, 8 B, only for lock rows): adding rows
//                             per resource into cnt[slots].  A workgroup first counts into an LDS table of kPxLds
//                             resources (claimed first come, first served, by slot & (kPxLds - 1)) and flushes it with
//                             one global atomic per resource it saw, so a hot resource costs a workgroup one global
//                             atomic, not one per row; a resource that finds its LDS entry taken counts in global
//                             memory directly (many resources: little contention per address).
//   pass 2  k_px_pick         one thread per resource slot: n + cnt > coord_cap puts the resource on the list with its
//                             room (coord_cap - n); cnt[r] becomes its list position + 1 (0: not listed).
//   (host)                    reads the list's length.  Empty -- the normal case -- means no row of [lo, hi) can
//                             overflow.
//   pass 3  only with a non-empty list, per group of kPxGroup listed resources:
//     k_px_block_count        a second streaming read: adding rows per (row chunk, listed resource), LDS counters
//     k_px_block_scan         one thread per listed resource: exclusive scan over the chunks; the chunk in which the
//                             rank reaches the room, and the rank at its start; the earliest such chunk so far bounds
//                             what later groups count and scan
//     k_px_rank               one workgroup per listed resource of that earliest chunk walks it in tiles of kPxBlock
//                             rows, in row order: the rank of an adding row is the rows before the tile + the waves
//                             before its own (LDS) + the lanes before it (ballot, popcount); the row whose rank
//                             equals the room does an atomicMin into the stop row.
// Plain loads, vector stores and C++ atomics only.
#include <algorithm>

#include "common.h"
#include "engine_internal.h"

namespace cc {
namespace {

constexpr uint32_t kPxLds = 4096;  // resources a pass-1 workgroup aggregates in LDS (tags + counters: 32 KiB)
constexpr uint32_t kPxWaves = kPxBlock / kWave;

// row i adds an entry to the coordination block of *res (set whenever the row resolves to a resource slot)
__device__ inline bool px_adds(const PxArgs& a, uint64_t i, uint32_t* res) {
  const uint32_t in = a.inst[i];
  const uint32_t r = in < a.max_inst ? a.inst_res[in] : kNoRes;
  if (r >= a.slots) return false;  // (kNoRes: an unbound instance slot)
  *res = r;
  const uint8_t t = a.res_type[r], op = a.op[i];
  const uint64_t aux = (t == CC_RES_LOCK && op == CC_OP_LOCK_LOCK && a.aux) ? a.aux[i] : 0;  // (only locks read it)
  return adds_entry(t, op, aux);
}

__global__ __launch_bounds__(kPxBlock) void k_px_count(PxArgs a) {
  __shared__ uint32_t tag[kPxLds], cnt[kPxLds];  // tag: resource slot + 1 (0: free)
  for (uint32_t t = threadIdx.x; t < kPxLds; t += kPxBlock) tag[t] = 0, cnt[t] = 0;
  __syncthreads();
  const uint64_t stride = (uint64_t)gridDim.x * kPxBlock;
  for (uint64_t i = a.lo + (uint64_t)blockIdx.x * kPxBlock + threadIdx.x; i < a.hi; i += stride) {
    uint32_t r;
    if (!px_adds(a, i, &r)) continue;
    const uint32_t h = r & (kPxLds - 1);
    const uint32_t old = atomicCAS(&tag[h], 0u, r + 1);
    if (old == 0 || old == r + 1)
      atomicAdd(&cnt[h], 1u);
    else
      atomicAdd(&a.cnt[r], 1u);
  }
  __syncthreads();
  for (uint32_t t = threadIdx.x; t < kPxLds; t += kPxBlock)
    if (cnt[t]) atomicAdd(&a.cnt[tag[t] - 1], cnt[t]);
}

__global__ __launch_bounds__(kPxBlock) void k_px_pick(PxArgs a) {
  const uint32_t r = blockIdx.x * kPxBlock + threadIdx.x;
  if (r >= a.slots) return;
  const uint32_t c = a.cnt[r];
  if (!c) return;
  const CoordHdr* hd = (const CoordHdr*)(a.coord + (size_t)r * coord_block(a.coord_cap));
  const uint32_t n = coord_used(a.res_type[r], hd->n, hd->head, a.coord_cap);  // (a bus: members + registrations)
  uint32_t sel = 0;
  if ((uint64_t)n + c > a.coord_cap) {  // (each slot is listed at most once: the list holds `slots` entries)
    const uint32_t k = atomicAdd(a.list_n, 1u);
    a.list_res[k] = r;
    a.list_room[k] = n < a.coord_cap ? a.coord_cap - n : 0;
    sel = k + 1;
  }
  a.cnt[r] = sel;
}

// rows [lo + b * chunk, lo + (b + 1) * chunk) are chunk b; bcnt[b][k - g0] = its adding rows for listed resource k
__global__ __launch_bounds__(kPxBlock) void k_px_block_count(PxArgs a, uint32_t g0, uint32_t mg, uint64_t chunk) {
  __shared__ uint32_t c[kPxGroup];
  if (blockIdx.x > *a.min_tb) return;  // (an earlier group's stop row lies in a chunk before this one)
  for (uint32_t t = threadIdx.x; t < mg; t += kPxBlock) c[t] = 0;
  __syncthreads();
  const uint64_t b0 = a.lo + (uint64_t)blockIdx.x * chunk, b1 = b0 + chunk < a.hi ? b0 + chunk : a.hi;
  for (uint64_t i = b0 + threadIdx.x; i < b1; i += kPxBlock) {
    uint32_t r;
    if (!px_adds(a, i, &r)) continue;
    const uint32_t k = a.cnt[r] - 1 - g0;  // (not listed, or listed in another group: wraps past mg)
    if (k < mg) atomicAdd(&c[k], 1u);
  }
  __syncthreads();
  for (uint32_t t = threadIdx.x; t < mg; t += kPxBlock) a.bcnt[(size_t)blockIdx.x * mg + t] = c[t];
}

// The stop row is the smallest over the listed resources, so only the chunks up to the earliest target chunk found so
// far (min_tb, over this group and the groups before it) matter: a later group counts and scans those alone, and
// k_px_rank walks only the resources whose target chunk is that one.
__global__ __launch_bounds__(kPxBlock) void k_px_block_scan(PxArgs a, uint32_t g0, uint32_t mg, uint32_t nblk) {
  const uint32_t t = blockIdx.x * kPxBlock + threadIdx.x;
  if (t >= mg) return;
  const uint32_t room = a.list_room[g0 + t];
  const uint32_t mt = __hip_atomic_load(a.min_tb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint32_t lim = mt < nblk ? mt + 1 : nblk;  // (k_px_block_count filled at least these chunks)
  uint32_t run = 0, tb = nblk;
  for (uint32_t b = 0; b < lim && tb == nblk; b += 8) {  // eight independent loads in flight, then the walk
    uint32_t c[8];
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) c[j] = b + j < lim ? a.bcnt[(size_t)(b + j) * mg + t] : 0;
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
      if (tb != nblk) continue;
      if (run + c[j] > room)  // the row of rank `room` lies in chunk b + j
        tb = b + j;
      else
        run += c[j];
    }
  }
  a.tblk[t] = tb;
  a.tbase[t] = run;
  if (tb < nblk) atomicMin(a.min_tb, tb);
}

__global__ __launch_bounds__(kPxBlock) void k_px_rank(PxArgs a, uint32_t g0, uint32_t nblk, uint64_t chunk) {
  __shared__ uint32_t wsum[kPxWaves];
  const uint32_t k = blockIdx.x, tb = a.tblk[k];
  if (tb >= nblk || tb > *a.min_tb) return;
  const uint32_t res = a.list_res[g0 + k], room = a.list_room[g0 + k];
  uint32_t run = a.tbase[k];  // adding rows of `res` before the tile
  const uint64_t b0 = a.lo + (uint64_t)tb * chunk, b1 = b0 + chunk < a.hi ? b0 + chunk : a.hi;
  const uint32_t lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  for (uint64_t t0 = b0; t0 < b1; t0 += kPxBlock) {  // (every condition of this loop is uniform over the workgroup)
    const uint64_t i = t0 + threadIdx.x;
    uint32_t r = kNoRes;
    const bool f = i < b1 && px_adds(a, i, &r) && r == res;
    const uint64_t m = __ballot(f);
    if (lane == 0) wsum[w] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t j = 0; j < kPxWaves; ++j) {
      if (j < w) before += wsum[j];
      total += wsum[j];
    }
    const uint32_t rank = run + before + (uint32_t)__popcll(m & ((1ull << lane) - 1));
    if (f && rank == room) atomicMin(a.stop, (unsigned long long)i);
    run += total;
    __syncthreads();  // (wsum is rewritten by the next tile)
    if (run > room) break;
  }
}

}  // namespace

int launch_px_count(const PxArgs& a, hipStream_t st) {
  if (hipMemsetAsync(a.cnt, 0, sizeof(uint32_t) * a.slots, st) != hipSuccess) return -1;
  if (hipMemsetAsync(a.list_n, 0, sizeof(uint32_t), st) != hipSuccess) return -1;
  if (hipMemsetAsync(a.min_tb, 0xFF, sizeof(uint32_t), st) != hipSuccess) return -1;
  if (hipMemsetAsync(a.stop, 0xFF, sizeof(unsigned long long), st) != hipSuccess) return -1;
  if (a.hi <= a.lo) return 0;
  const uint64_t len = a.hi - a.lo;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(1024, (len + 8 * kPxBlock - 1) / (8 * kPxBlock));
  hipLaunchKernelGGL(k_px_count, dim3(grid), dim3(kPxBlock), 0, st, a);
  hipLaunchKernelGGL(k_px_pick, dim3((a.slots + kPxBlock - 1) / kPxBlock), dim3(kPxBlock), 0, st, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_px_rank(const PxArgs& a, uint32_t g0, uint32_t mg, uint32_t nblk, uint64_t chunk, hipStream_t st) {
  if (mg == 0 || nblk == 0) return 0;
  hipLaunchKernelGGL(k_px_block_count, dim3(nblk), dim3(kPxBlock), 0, st, a, g0, mg, chunk);
  hipLaunchKernelGGL(k_px_block_scan, dim3((mg + kPxBlock - 1) / kPxBlock), dim3(kPxBlock), 0, st, a, g0, mg, nblk);
  hipLaunchKernelGGL(k_px_rank, dim3(mg), dim3(kPxBlock), 0, st, a, g0, nblk, chunk);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace cc
