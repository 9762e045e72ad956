// grow.hip — the device side of cc_snapshot_restore_grow (engine.hip): a snapshot's sections that change shape when the
// engine it restores into has a larger map table or wider coordination blocks (DESIGN "Growing from a snapshot").
//
// The host uploads those sections as they were saved into temporary buffers; three kernels, one launch each, move them
// into the engine's own arrays.  No workgroup reads what another one wrote, so none of them needs an ordering between
// workgroups, and every index is bounded by the kernel itself (the sections come from a host buffer that only had its
// sizes checked).
//   k_grow_table  a workgroup per old region r.  A key's region is the top map_bits bits of map_hash and its first
//                 probe the low 11 bits (common.h tbl_find), so with d more bits r's entries land only in the regions
//                 [r << d, (r + 1) << d), at the same first probe.  The workgroup zeroes those children, then every
//                 bound entry that is not DEAD claims the first free word of its probe chain (one CAS on the word, as
//                 the compaction of apply_map.hip) and stores the other six columns there.  Tombstones and UNSEEN
//                 entries move like present ones, so the move touches no drop counter and no compacted-key set entry.
//                 A child receives a subset of one old region: it cannot fill up.
//   k_grow_cset   a lane per old entry: an occupied entry of its map's current generation is inserted into the zeroed
//                 larger set with cset_insert (an entry of a generation the map has left would be taken over by the
//                 next insert that meets it, and counts nowhere: it stays behind).
//   k_grow_coord  a wave per resource slot, the lanes striding the entries.  Lock waiters and queue elements form a
//                 ring from CoordHdr.head: entry i goes to new entry i and the head to 0.  A MessageBus keeps its
//                 members at the front and its CoordHdr.head registrations at the back: registration j moves from
//                 old_cap - 1 - j to new_cap - 1 - j.  Every other type keeps a list from the front.
#include "engine_internal.h"

namespace cc {
namespace {

constexpr uint32_t kGT = 256;  // threads per workgroup

// Per-kernel times of the calling thread's last grow (cc_snapshot_grow_timing; off by default).
thread_local bool g_time_on = false;
thread_local float g_time_ms[3] = {0.f, 0.f, 0.f};
struct Timed {  // events around one launch; waits for the kernel when timing is on
  hipStream_t st;
  int slot;
  hipEvent_t a = nullptr, b = nullptr;
  Timed(int slot_, hipStream_t st_) : st(st_), slot(slot_) {
    if (!g_time_on) return;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
    (void)hipEventRecord(a, st);
  }
  ~Timed() {
    if (a && b && hipEventRecord(b, st) == hipSuccess && hipEventSynchronize(b) == hipSuccess)
      (void)hipEventElapsedTime(&g_time_ms[slot], a, b);
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

__global__ __launch_bounds__(kGT) void k_grow_table(TblCols old, uint32_t old_bits, TblCols dst, uint32_t new_bits) {
  const uint32_t r = blockIdx.x, t = threadIdx.x, d = new_bits - old_bits;
  const uint64_t ob = (uint64_t)r * kMapRegion;          // the old region's first entry
  const uint64_t cb = ((uint64_t)r << d) * kMapRegion;   // its first child's
  const uint64_t cn = (uint64_t)kMapRegion << d;
  for (uint64_t q = t; q < cn; q += kGT) {
    dst.word[cb + q] = 0u;
    dst.key[cb + q] = 0;
    dst.val[cb + q] = 0;
    dst.ci[cb + q] = 0;
    dst.ins[cb + q] = 0;
    dst.dl[cb + q] = 0;
    dst.claim[cb + q] = 0;
  }
  __syncthreads();  // (the children are this workgroup's alone; the barrier orders its stores to HBM too)
  for (uint32_t q = t; q < (uint32_t)kMapRegion; q += kGT) {
    const uint32_t w = old.word[ob + q];
    if (!(w & kMwUsed) || (w & kMwDead)) continue;
    const uint64_t key = old.key[ob + q];
    const uint64_t h = map_hash(w & kMwSlotMask, (w >> 17) & 3u, key);
    // (the child bits only: an entry of a damaged snapshot that sat in the wrong region still lands in a child of r)
    const uint64_t base = cb + ((h >> (64 - new_bits)) & ((1ull << d) - 1)) * kMapRegion;
    uint32_t p = (uint32_t)h & (kMapRegion - 1);
    for (int step = 0; step < kMapRegion; ++step, p = (p + 1) & (kMapRegion - 1)) {
      if (atomicCAS(&dst.word[base + p], 0u, w) != 0u) continue;
      dst.key[base + p] = key;
      dst.val[base + p] = old.val[ob + q];
      dst.ci[base + p] = old.ci[ob + q];
      dst.ins[base + p] = old.ins[ob + q];
      dst.dl[base + p] = old.dl[ob + q];
      dst.claim[base + p] = old.claim[ob + q];
      break;
    }
  }
}

__global__ __launch_bounds__(kGT) void k_grow_cset(const CsetEnt* __restrict__ old, uint64_t old_n, CsetEnt* __restrict__ dst,
                                                   uint64_t new_mask, uint32_t* __restrict__ full,
                                                   const uint64_t* __restrict__ cgen, uint32_t max_resources) {
  const uint64_t i = (uint64_t)blockIdx.x * kGT + threadIdx.x;
  if (i >= old_n) return;
  const uint32_t m = old[i].meta;
  if (!(m & 0x80000000u)) return;
  const uint32_t slot = m & kMwSlotMask;
  if (slot >= max_resources) return;
  if (((m >> 19) & 0xFFFu) != (uint32_t)(cgen[slot] & 0xFFFu)) return;  // (a generation its map has left)
  cset_insert(dst, new_mask, full, slot, (m >> 17) & 3u, old[i].key, cgen, old[i].claim);
}

__global__ __launch_bounds__(kGT) void k_grow_coord(const uint8_t* __restrict__ old, uint32_t old_cap, uint8_t* __restrict__ dst,
                                                    uint32_t new_cap, const uint8_t* __restrict__ res_type, uint64_t slots) {
  const uint64_t s = (uint64_t)blockIdx.x * (kGT / kWave) + (threadIdx.x / kWave);
  const uint32_t l = threadIdx.x % kWave;
  if (s >= slots) return;
  const uint8_t* ob = old + s * coord_block(old_cap);
  uint8_t* nb = dst + s * coord_block(new_cap);
  CoordHdr h = *reinterpret_cast<const CoordHdr*>(ob);
  const CoordEnt* oe = reinterpret_cast<const CoordEnt*>(ob + sizeof(CoordHdr));
  CoordEnt* ne = reinterpret_cast<CoordEnt*>(nb + sizeof(CoordHdr));
  const uint32_t type = res_type[s], n = h.n < old_cap ? h.n : old_cap;
  if (type == CC_RES_BUS) {
    const uint32_t regs = h.head < old_cap - n ? h.head : old_cap - n;
    for (uint32_t i = l; i < n; i += kWave) ne[i] = oe[i];
    for (uint32_t j = l; j < regs; j += kWave) ne[new_cap - 1 - j] = oe[old_cap - 1 - j];
  } else {
    const bool ring = type == CC_RES_LOCK || type == CC_RES_QUEUE;
    const uint32_t head = ring ? h.head & (old_cap - 1) : 0u;
    for (uint32_t i = l; i < n; i += kWave) ne[i] = oe[(head + i) & (old_cap - 1)];
    if (ring) h.head = 0;
  }
  if (l == 0) *reinterpret_cast<CoordHdr*>(nb) = h;
}

}  // namespace

int launch_grow_table(const TblCols& old, uint32_t old_bits, const TblCols& dst, uint32_t new_bits, hipStream_t st) {
  const Timed tm(0, st);
  hipLaunchKernelGGL(k_grow_table, dim3(1u << old_bits), dim3(kGT), 0, st, old, old_bits, dst, new_bits);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_grow_cset(const CsetEnt* old, uint64_t old_n, CsetEnt* dst, uint64_t new_mask, uint32_t* full, const uint64_t* cgen,
                     uint32_t max_resources, hipStream_t st) {
  const Timed tm(1, st);
  hipLaunchKernelGGL(k_grow_cset, dim3((uint32_t)((old_n + kGT - 1) / kGT)), dim3(kGT), 0, st, old, old_n, dst, new_mask, full, cgen,
                     max_resources);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_grow_coord(const uint8_t* old, uint32_t old_cap, uint8_t* dst, uint32_t new_cap, const uint8_t* res_type,
                      uint64_t slots, hipStream_t st) {
  const Timed tm(2, st);
  constexpr uint32_t per = kGT / kWave;
  hipLaunchKernelGGL(k_grow_coord, dim3((uint32_t)((slots + per - 1) / per)), dim3(kGT), 0, st, old, old_cap, dst, new_cap,
                     res_type, slots);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace cc

extern "C" int cc_snapshot_grow_timing(int enable, float* ms) {
  if (ms)
    for (int k = 0; k < 3; ++k) ms[k] = cc::g_time_ms[k];
  cc::g_time_on = enable != 0;
  for (int k = 0; k < 3; ++k) cc::g_time_ms[k] = 0.f;
  return CC_OK;
}
