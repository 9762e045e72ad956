// split_gpu.hip — one global log, many engines, on the device (DESIGN §6 "The split on the device").
//
// cc_split_batch_device / cc_merge_results_device are split.cpp's two calls for columns that already sit in HBM: a
// stable split of the batch columns by the rank that owns the row's resource, and the inverse merge of the per-rank
// result columns, byte for byte what the host calls give.  Three launches, none of which has a workgroup wait for
// another:
//   k_split_count    a workgroup per tile of CC_SPLIT_TILE_ROWS rows: owner byte per row (kept in the workspace, so the
//                    table is gathered once), the tile's rows per rank cnt[tile][rank], "owner >= world" -> error word
//   k_split_scan     per rank, the exclusive prefix of cnt over the tiles: base[tile][rank], counts[rank]
//   k_split_scatter  per tile: a stable rank of every row among the tile's rows of its owner, every present column
//   (k_merge_gather)            staged through LDS in rank order and each rank's run stored contiguously at
//                               out[rank] + base[tile][rank]  (the merge reads parts[rank] at the same places)
// The host waits once, after the scan, for `world` counts and the error word: nothing may be written before the
// capacity and owner checks have passed.
//
// The rank of a row comes from wave ballots (the lanes of a 64-row step that share an owner, counted below the lane)
// plus wave-private running counters in LDS that one elected lane advances, plus one scan over the waves' totals: it is
// stable by construction and does not rest on the order in which LDS serves same-address atomics (these calls have no
// engine, so no k_selfcheck_lds_order has run before them).
#include <cstdio>
#include <vector>

#include "engine_state.h"

namespace cc {
namespace {

constexpr uint32_t kST = CC_SPLIT_TILE_ROWS;  // rows per tile
constexpr uint32_t kSThreads = 256;
constexpr uint32_t kSWaves = kSThreads / kWave;
constexpr uint32_t kSSpan = kST / kSWaves;  // consecutive rows of a tile that one wave ranks
constexpr uint32_t kRanks = 256;            // LDS counters are sized for every owner byte, whatever `world` is
constexpr uint32_t kCols = 10;              // the nine batch columns (cc_batch order) + the source-row output
constexpr uint32_t kMaxGrid = 1u << 16;
static_assert(kST % (kSThreads * 16) == 0 && kST <= 65536, "16 rows per thread and step; u16 staging slots");

// ---- workspace layout (every part 256-byte aligned) -----------------------------------------------------------------
//   header  u32 error word; u64 counts[256] at byte 64
//   ptab    kCols x world output pointers (the merge: 2 x world part pointers)
//   own     u8 per row
//   cnt     u32 [tiles][world]
//   base    u64 [tiles][world]
constexpr uint64_t kHdrCounts = 64;
constexpr uint64_t kHdrBytes = 2304;
struct Layout {
  uint64_t tiles, ptab, own, cnt, base, total;
};
inline uint64_t up256(uint64_t x) { return (x + 255) & ~(uint64_t)255; }
inline Layout layout(uint64_t n, uint32_t world) {
  Layout l;
  l.tiles = (n + kST - 1) / kST;
  l.ptab = kHdrBytes;
  l.own = l.ptab + up256((uint64_t)kCols * world * 8);
  l.cnt = l.own + up256(n);
  l.base = l.cnt + up256(l.tiles * world * 4);
  l.total = l.base + up256(l.tiles * world * 8);
  return l;
}

// The lanes of the wave that hold the same owner as the next unserved lane: one round of the match loop.  `rem` (the
// lanes not yet served) is wave-uniform, so the leader's owner is read with a uniform lane index.
__device__ inline uint64_t match_round(uint64_t rem, uint32_t o, bool valid, uint32_t& r) {
  const uint32_t leader = (uint32_t)__builtin_ctzll(rem);
  r = (uint32_t)__builtin_amdgcn_readlane((int)o, (int)leader);
  return ballot(valid && o == r);
}

__global__ __launch_bounds__(kSThreads) void k_split_count(const uint32_t* __restrict__ inst, uint64_t n,
                                                           const uint8_t* __restrict__ tab, uint32_t n_inst,
                                                           uint32_t world, uint64_t tiles, uint8_t* __restrict__ own,
                                                           uint32_t* __restrict__ cnt, uint32_t* __restrict__ err) {
  __shared__ uint32_t wc[kSWaves][kRanks];
  const uint32_t t = threadIdx.x, l = t & 63, w = t >> 6;
  bool bad = false;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    for (uint32_t i = t; i < kSWaves * kRanks; i += kSThreads) (&wc[0][0])[i] = 0;
    __syncthreads();
    const uint64_t row0 = tile * kST + (uint64_t)w * kSSpan;
#pragma unroll
    for (uint32_t s = 0; s < kSSpan / 256; ++s) {
      const uint64_t row = row0 + s * 256 + l * 4;  // a multiple of 4: the 16-byte load is aligned
      uint32_t v[4] = {0, 0, 0, 0};
      uint32_t have = 0;
      if (row + 4 <= n) {
        const uint4 q = *reinterpret_cast<const uint4*>(inst + row);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        have = 4;
      } else if (row < n) {
        have = (uint32_t)(n - row);
        for (uint32_t j = 0; j < have; ++j) v[j] = inst[row + j];
      }
      uint32_t o[4];
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        o[j] = (j < have && v[j] < n_inst) ? tab[v[j]] : 0u;  // an unknown instance: rank 0 answers UNKNOWN_SESSION
        bad |= o[j] >= world;
      }
      if (have == 4) {
        *reinterpret_cast<uint32_t*>(own + row) = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
      } else {
        for (uint32_t j = 0; j < have; ++j) own[row + j] = (uint8_t)o[j];
      }
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        const bool valid = j < have;
        uint64_t rem = ballot(valid);
        while (rem) {
          uint32_t r;
          const uint64_t m = match_round(rem, o[j], valid, r);
          if (l == (uint32_t)__builtin_ctzll(rem)) atomicAdd(&wc[w][r], (uint32_t)__popcll(m));  // one lane, its wave's row
          rem &= ~m;
        }
      }
    }
    __syncthreads();
    if (t < world) cnt[tile * world + t] = wc[0][t] + wc[1][t] + wc[2][t] + wc[3][t];
    __syncthreads();
  }
  if (__any(bad) && l == 0) atomicOr(err, 1u);
}

// One workgroup per rank: thread t sums a contiguous chunk of the rank's tile counters, the 256 sums are scanned in
// LDS, and the thread walks its chunk again writing the bases.
__global__ __launch_bounds__(kSThreads) void k_split_scan(const uint32_t* __restrict__ cnt, uint64_t tiles, uint32_t world,
                                                          uint64_t* __restrict__ base, uint64_t* __restrict__ counts) {
  __shared__ uint64_t part[kSThreads];
  const uint32_t r = blockIdx.x, t = threadIdx.x;
  const uint64_t chunk = (tiles + kSThreads - 1) / kSThreads;
  const uint64_t lo = (uint64_t)t * chunk < tiles ? (uint64_t)t * chunk : tiles;
  const uint64_t hi = lo + chunk < tiles ? lo + chunk : tiles;
  uint64_t s = 0;
  for (uint64_t i = lo; i < hi; ++i) s += cnt[i * world + r];
  part[t] = s;
  __syncthreads();
  for (uint32_t d = 1; d < kSThreads; d <<= 1) {
    const uint64_t y = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += y;
    __syncthreads();
  }
  uint64_t run = part[t] - s;
  for (uint64_t i = lo; i < hi; ++i) {
    base[i * world + r] = run;
    run += cnt[i * world + r];
  }
  if (t == kSThreads - 1) counts[r] = part[t];
}

// The stable rank of each of the tile's m rows among the tile's rows of its owner.  Wave w ranks rows
// [w * kSSpan, (w + 1) * kSSpan) in 64-row steps: a row's rank inside its wave is the wave's running counter of that
// owner (wc[w][r], read by every lane of the round, advanced by the round's first lane) plus the equal lanes below it.
// On return loc[i] = that rank, wc[w][r] = the tile's rows of rank r in the waves before w, and tc (thread r's) = the
// tile's rows of rank r.  Ends with a barrier.
__device__ inline void tile_rank(const uint8_t* __restrict__ own, uint32_t m, uint32_t (*wc)[kRanks], uint16_t* loc,
                                 uint32_t& tc) {
  const uint32_t t = threadIdx.x, l = t & 63, w = t >> 6;
  for (uint32_t i = t; i < kSWaves * kRanks; i += kSThreads) (&wc[0][0])[i] = 0;
  __syncthreads();
  const uint64_t below = lanemask_lt();
  uint32_t* const mine = wc[w];
  for (uint32_t s = 0; s < kSSpan / 64; ++s) {
    const uint32_t i = w * kSSpan + s * 64 + l;
    const bool valid = i < m;
    const uint32_t o = valid ? own[i] : 0u;
    uint32_t rank = 0;
    uint64_t rem = ballot(valid);
    while (rem) {
      uint32_t r;
      const uint64_t mk = match_round(rem, o, valid, r);
      const uint32_t old = mine[r];  // every lane reads the round's counter before its first lane advances it
      if (valid && o == r) rank = old + (uint32_t)__popcll(mk & below);
      if (l == (uint32_t)__builtin_ctzll(rem)) mine[r] = old + (uint32_t)__popcll(mk);
      __builtin_amdgcn_wave_barrier();
      rem &= ~mk;
    }
    if (valid) loc[i] = (uint16_t)rank;
  }
  __syncthreads();
  const uint32_t c0 = wc[0][t], c1 = wc[1][t], c2 = wc[2][t], c3 = wc[3][t];  // thread t: rank t (kSThreads == kRanks)
  wc[0][t] = 0, wc[1][t] = c0, wc[2][t] = c0 + c1, wc[3][t] = c0 + c1 + c2;
  tc = c0 + c1 + c2 + c3;
  __syncthreads();
}
static_assert(kSThreads == kRanks && kSWaves == 4, "tile_rank: one thread per rank, four waves");

struct SplitArgs {
  const void* in[kCols - 1];  // cc_batch order; null: absent
  void* const* ptab;          // [kCols][world]
  const uint8_t* own;
  const uint64_t* base;
  uint64_t n, tiles;
  uint32_t world, rows;  // rows: the source-row output is wanted
};

// One column of one tile: loaded in row order (16-byte loads on a full tile), stored at the rows' staging slots, then
// read back in slot order and stored to the ranks' outputs.  Two barriers: the staging area is reused by the next column.
// Thread r first publishes where rank r's staging positions go: position p belongs at obase[r] + p elements, obase[r] =
// out[r] + delta (delta = base[tile][r] - the rank's first staging slot, modulo 2^64), 0 for a NULL output.
template <class T, bool kRowIds>
__device__ inline void scatter_col(const T* __restrict__ in, uint64_t row0, uint32_t m, T* const* __restrict__ out,
                                   uint32_t world, T* st, const uint16_t* slot, const uint8_t* rk, uint64_t* obase,
                                   uint64_t delta) {
  const uint32_t t = threadIdx.x;
  constexpr uint32_t V = 16 / sizeof(T);
  {
    T* const o = t < world ? out[t] : nullptr;
    obase[t] = o ? (uint64_t)(uintptr_t)o + delta * sizeof(T) : 0;
  }
  if constexpr (kRowIds) {
    for (uint32_t i = t; i < m; i += kSThreads) st[slot[i]] = (T)(row0 + i);
  } else if (m == kST) {
    const uint4* __restrict__ in4 = reinterpret_cast<const uint4*>(in + row0);
#pragma unroll
    for (uint32_t k = 0; k < kST / V / kSThreads; ++k) {
      const uint32_t q = k * kSThreads + t;
      const uint4 v = in4[q];
      T e[V];
      __builtin_memcpy(e, &v, 16);
#pragma unroll
      for (uint32_t j = 0; j < V; ++j) st[slot[q * V + j]] = e[j];
    }
  } else {
    for (uint32_t i = t; i < m; i += kSThreads) st[slot[i]] = in[row0 + i];
  }
  __syncthreads();
  for (uint32_t p = t; p < m; p += kSThreads) {
    const uint64_t ob = obase[rk[p]];
    if (ob) reinterpret_cast<T*>((uintptr_t)ob)[p] = st[p];
  }
  __syncthreads();
}

__global__ __launch_bounds__(kSThreads) void k_split_scatter(const SplitArgs a) {
  __shared__ __attribute__((aligned(16))) uint64_t stage[kST];
  __shared__ uint16_t slot[kST];
  __shared__ uint8_t rk[kST];
  __shared__ uint32_t wc[kSWaves][kRanks];
  __shared__ uint32_t boff[kRanks];
  __shared__ uint64_t obase[kRanks];
  __shared__ uint32_t wsum[kSWaves];
  const uint32_t t = threadIdx.x, l = t & 63, w = t >> 6;
  for (uint64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const uint64_t row0 = tile * kST;
    const uint32_t m = (uint32_t)(a.n - row0 < kST ? a.n - row0 : kST);
    const uint8_t* __restrict__ own = a.own + row0;
    uint32_t tc;
    tile_rank(own, m, wc, slot, tc);
    // exclusive scan of the tile's rank counts: rank r's run starts at staging slot boff[r]
    uint32_t inc = tc;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const uint32_t y = __shfl_up(inc, d, kWave);
      if (l >= (uint32_t)d) inc += y;
    }
    if (l == kWave - 1) wsum[w] = inc;
    const uint64_t gbase = t < a.world ? a.base[tile * a.world + t] : 0;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t k = 0; k < w; ++k) before += wsum[k];
    boff[t] = before + inc - tc;
    const uint64_t delta = gbase - boff[t];  // thread r's: rank r's staging position p is output row p + delta
    __syncthreads();
    for (uint32_t s = 0; s < kSSpan / 64; ++s) {
      const uint32_t i = w * kSSpan + s * 64 + l;
      if (i < m) {
        const uint32_t o = own[i];
        const uint32_t p = boff[o] + wc[w][o] + slot[i];
        slot[i] = (uint16_t)p;
        rk[p] = (uint8_t)o;
      }
    }
    __syncthreads();
    void* const* pt = a.ptab;
    const uint32_t W = a.world;
#define CC_SPLIT_COL(k, T)                                                                                      \
  if (a.in[k])                                                                                                  \
    scatter_col<T, false>((const T*)a.in[k], row0, m, (T* const*)(pt + (uint64_t)(k) * W), W, (T*)stage, slot, \
                          rk, obase, delta)
    CC_SPLIT_COL(0, uint64_t);
    CC_SPLIT_COL(1, uint64_t);
    CC_SPLIT_COL(2, uint32_t);
    CC_SPLIT_COL(3, uint8_t);
    CC_SPLIT_COL(4, uint8_t);
    CC_SPLIT_COL(5, uint64_t);
    CC_SPLIT_COL(6, uint64_t);
    CC_SPLIT_COL(7, uint64_t);
    CC_SPLIT_COL(8, uint64_t);
#undef CC_SPLIT_COL
    if (a.rows)
      scatter_col<uint64_t, true>(nullptr, row0, m, (uint64_t* const*)(pt + (uint64_t)(kCols - 1) * W), W, stage, slot,
                                  rk, obase, delta);
  }
}

// Row i of the merged columns takes row base[tile][r] + (its rank among the tile's rows of r) of parts[r]: within a
// tile each rank's reads are one contiguous run.
__global__ __launch_bounds__(kSThreads) void k_merge_gather(const uint8_t* __restrict__ own, const uint64_t* __restrict__ base,
                                                            uint64_t n, uint64_t tiles, uint32_t world,
                                                            const void* const* __restrict__ ptab,
                                                            uint8_t* __restrict__ status, uint64_t* __restrict__ value) {
  __shared__ uint16_t loc[kST];
  __shared__ uint32_t wc[kSWaves][kRanks];
  __shared__ uint64_t gbase[kRanks];
  const uint32_t t = threadIdx.x, l = t & 63, w = t >> 6;
  const uint8_t* const* __restrict__ ps = reinterpret_cast<const uint8_t* const*>(ptab);
  const uint64_t* const* __restrict__ pv = reinterpret_cast<const uint64_t* const*>(ptab + world);
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t row0 = tile * kST;
    const uint32_t m = (uint32_t)(n - row0 < kST ? n - row0 : kST);
    uint32_t tc;
    tile_rank(own + row0, m, wc, loc, tc);
    gbase[t] = t < world ? base[tile * world + t] : 0;
    __syncthreads();
    for (uint32_t s = 0; s < kSSpan / 64; ++s) {
      const uint32_t i = w * kSSpan + s * 64 + l;
      if (i < m) {
        const uint32_t o = own[row0 + i];
        const uint64_t src = gbase[o] + wc[w][o] + loc[i];
        status[row0 + i] = ps[o][src];
        value[row0 + i] = pv[o][src];
      }
    }
    __syncthreads();
  }
}

uint32_t grid_for_tiles(uint64_t tiles) { return (uint32_t)(tiles < kMaxGrid ? tiles : kMaxGrid); }

// the arguments both calls share, checked before any HIP call
int check_common(const char* who, uint64_t n, const uint32_t* d_inst, const uint8_t* d_tab, uint32_t n_inst, uint32_t world,
                 const void* d_work, uint64_t work_bytes) {
  auto fail = [&](const char* what) {
    char msg[96];
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return set_err(CC_ERR_INVALID, msg);
  };
  if (world == 0 || world > 256) return fail("world must be in [1, 256]");
  if ((n && !d_inst) || (n_inst && !d_tab)) return fail("null argument");
  if ((uintptr_t)d_inst & 15) return fail("the inst column must be 16-byte aligned");
  if (!d_work || ((uintptr_t)d_work & 15)) return fail("the workspace is null or not 16-byte aligned");
  if (work_bytes < layout(n, world).total) return fail("the workspace is smaller than cc_split_device_bound");
  return CC_OK;
}

// Launches on the device that owns `stream` (the current device for the null stream), restoring the caller's device.
struct DeviceOf {
  int prev = -1, dev = -1;
  hipError_t enter(hipStream_t st) {
    hipError_t e = hipGetDevice(&prev);
    if (e != hipSuccess) return e;
    dev = prev;
    if (st) {
      e = hipStreamGetDevice(st, &dev);
      if (e != hipSuccess) return e;
      if (dev != prev) e = hipSetDevice(dev);
    }
    return e;
  }
  ~DeviceOf() {
    if (prev >= 0 && dev != prev) (void)hipSetDevice(prev);
  }
};

// Per-kernel times of the calling thread's last device call (cc_split_device_timing; off by default): events
// before the count kernel, between count and scan, after the scan, and around the scatter / gather.
struct Timing {
  bool on = false;
  int dev = -1;
  hipEvent_t ev[5] = {};
  bool scanned = false, moved = false;  // which spans the last call recorded
  int prepare(int device) {
    scanned = moved = false;
    if (dev == device) return CC_OK;
    for (hipEvent_t& e : ev) {
      if (e) (void)hipEventDestroy(e);
      e = nullptr;
      HIPCHECK(hipEventCreate(&e));
    }
    dev = device;
    return CC_OK;
  }
};
thread_local Timing g_timing;

// count + scan, then the one host wait: h_hdr = the error word and the counts
int count_and_scan(const uint32_t* d_inst, uint64_t n, const uint8_t* d_tab, uint32_t n_inst, uint32_t world,
                   const Layout& L, uint8_t* work, hipStream_t st, const void* h_ptab, uint64_t ptab_bytes,
                   uint64_t* h_counts, int device) {
  uint32_t* d_err = reinterpret_cast<uint32_t*>(work);
  uint64_t* d_counts = reinterpret_cast<uint64_t*>(work + kHdrCounts);
  Timing& tm = g_timing;
  if (tm.on) TRY(tm.prepare(device));
  HIPCHECK(hipMemsetAsync(work, 0, kHdrBytes, st));
  if (ptab_bytes) HIPCHECK(hipMemcpyAsync(work + L.ptab, h_ptab, ptab_bytes, hipMemcpyHostToDevice, st));
  if (tm.on) HIPCHECK(hipEventRecord(tm.ev[0], st));
  hipLaunchKernelGGL(k_split_count, dim3(grid_for_tiles(L.tiles)), dim3(kSThreads), 0, st, d_inst, n, d_tab, n_inst, world,
                     L.tiles, work + L.own, reinterpret_cast<uint32_t*>(work + L.cnt), d_err);
  if (tm.on) HIPCHECK(hipEventRecord(tm.ev[1], st));
  hipLaunchKernelGGL(k_split_scan, dim3(world), dim3(kSThreads), 0, st, reinterpret_cast<const uint32_t*>(work + L.cnt),
                     L.tiles, world, reinterpret_cast<uint64_t*>(work + L.base), d_counts);
  if (tm.on) {
    HIPCHECK(hipEventRecord(tm.ev[2], st));
    tm.scanned = true;
  }
  HIPCHECK(hipGetLastError());
  uint64_t h_hdr[kHdrCounts / 8 + 256];
  HIPCHECK(hipMemcpyAsync(h_hdr, work, kHdrCounts + 8ull * world, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  for (uint32_t r = 0; r < world; ++r) h_counts[r] = h_hdr[kHdrCounts / 8 + r];
  return (uint32_t)h_hdr[0] ? CC_ERR_INVALID : CC_OK;
}

}  // namespace
}  // namespace cc

extern "C" int cc_split_device_bound(uint64_t n, uint32_t world, uint64_t* work_bytes) {
  using namespace cc;
  if (!work_bytes) return set_err(CC_ERR_INVALID, "split bound: null argument");
  if (world == 0 || world > 256) return set_err(CC_ERR_INVALID, "split bound: world must be in [1, 256]");
  if (n > (1ull << 48)) return set_err(CC_ERR_INVALID, "split bound: n is beyond 2^48 rows");
  *work_bytes = layout(n, world).total;
  return CC_OK;
}

extern "C" int cc_split_device_timing(int enable, float* ms) {
  using namespace cc;
  Timing& tm = g_timing;
  if (ms) {
    ms[0] = ms[1] = ms[2] = 0.f;
    if (tm.scanned) {
      HIPCHECK(hipEventElapsedTime(&ms[0], tm.ev[0], tm.ev[1]));
      HIPCHECK(hipEventElapsedTime(&ms[1], tm.ev[1], tm.ev[2]));
    }
    if (tm.moved) {
      HIPCHECK(hipEventSynchronize(tm.ev[4]));
      HIPCHECK(hipEventElapsedTime(&ms[2], tm.ev[3], tm.ev[4]));
    }
  }
  tm.on = enable != 0;
  return CC_OK;
}

extern "C" int cc_split_batch_device(const cc_batch* d_in, uint64_t n, const uint8_t* d_rank_of_inst, uint32_t n_inst,
                                     uint32_t world, const cc_batch_out* outs, const uint64_t* out_cap, uint64_t* counts,
                                     uint64_t* const* d_rows, void* d_work, uint64_t work_bytes, void* stream) {
  using namespace cc;
  if (!d_in || !counts) return set_err(CC_ERR_INVALID, "split (device): null argument");
  if (n > (1ull << 48)) return set_err(CC_ERR_INVALID, "split (device): n is beyond 2^48 rows");
  if (const int rc = check_common("split (device)", n, d_in->inst, d_rank_of_inst, n_inst, world, d_work, work_bytes)) return rc;
  if (outs && !out_cap) return set_err(CC_ERR_INVALID, "split (device): null out_cap");
  const void* const icol[9] = {d_in->index, d_in->time, d_in->inst, d_in->op, d_in->flags,
                               d_in->key,   d_in->a,    d_in->b,    d_in->aux};
  for (int k = 0; k < 9; ++k)
    if ((uintptr_t)icol[k] & 15) return set_err(CC_ERR_INVALID, "split (device): input columns must be 16-byte aligned");
  if (n == 0) {
    for (uint32_t r = 0; r < world; ++r) counts[r] = 0;
    return CC_OK;
  }
  const Layout L = layout(n, world);
  // every column the input has, every output has (a missing input column stays missing)
  std::vector<void*> ptab;
  bool want_rows = false;
  if (outs) {
    ptab.assign((size_t)kCols * world, nullptr);
    for (uint32_t r = 0; r < world; ++r) {
      void* const ocol[9] = {outs[r].index, outs[r].time, outs[r].inst, outs[r].op, outs[r].flags,
                             outs[r].key,   outs[r].a,    outs[r].b,    outs[r].aux};
      for (uint32_t k = 0; k < 9; ++k) ptab[(size_t)k * world + r] = icol[k] ? ocol[k] : nullptr;
      if (d_rows && d_rows[r]) ptab[(size_t)(kCols - 1) * world + r] = d_rows[r], want_rows = true;
    }
  }
  hipStream_t st = (hipStream_t)stream;
  DeviceOf dev;
  HIPCHECK(dev.enter(st));
  uint8_t* work = static_cast<uint8_t*>(d_work);
  const int rc = count_and_scan(d_in->inst, n, d_rank_of_inst, n_inst, world, L, work, st, ptab.data(), ptab.size() * 8,
                                counts, dev.dev);
  if (rc == CC_ERR_INVALID) return set_err(CC_ERR_INVALID, "split (device): rank_of_inst names a rank >= world");
  if (rc != CC_OK || !outs) return rc;
  for (uint32_t r = 0; r < world; ++r) {
    if (counts[r] > out_cap[r]) return set_err(CC_ERR_CAPACITY, "split (device): a rank's output columns are too small");
    for (uint32_t k = 0; k < 9; ++k)
      if (icol[k] && counts[r] && !ptab[(size_t)k * world + r]) return set_err(CC_ERR_INVALID, "split (device): null output column");
  }
  SplitArgs a;
  for (int k = 0; k < 9; ++k) a.in[k] = icol[k];
  a.ptab = reinterpret_cast<void* const*>(work + L.ptab);
  a.own = work + L.own;
  a.base = reinterpret_cast<const uint64_t*>(work + L.base);
  a.n = n, a.tiles = L.tiles, a.world = world, a.rows = want_rows;
  Timing& tm = g_timing;
  if (tm.on) HIPCHECK(hipEventRecord(tm.ev[3], st));
  hipLaunchKernelGGL(k_split_scatter, dim3(grid_for_tiles(L.tiles)), dim3(kSThreads), 0, st, a);
  if (tm.on) {
    HIPCHECK(hipEventRecord(tm.ev[4], st));
    tm.moved = true;
  }
  HIPCHECK(hipGetLastError());
  return CC_OK;
}

extern "C" int cc_merge_results_device(const uint32_t* d_inst, uint64_t n, const uint8_t* d_rank_of_inst, uint32_t n_inst,
                                       uint32_t world, const cc_results* parts, const cc_results* d_out, void* d_work,
                                       uint64_t work_bytes, void* stream) {
  using namespace cc;
  if (n > (1ull << 48)) return set_err(CC_ERR_INVALID, "merge (device): n is beyond 2^48 rows");
  if (const int rc = check_common("merge (device)", n, d_inst, d_rank_of_inst, n_inst, world, d_work, work_bytes)) return rc;
  if (n && (!parts || !d_out || !d_out->status || !d_out->value)) return set_err(CC_ERR_INVALID, "merge (device): null argument");
  if (n == 0) return CC_OK;
  const Layout L = layout(n, world);
  std::vector<const void*> ptab((size_t)2 * world);
  for (uint32_t r = 0; r < world; ++r) ptab[r] = parts[r].status, ptab[world + r] = parts[r].value;
  hipStream_t st = (hipStream_t)stream;
  DeviceOf dev;
  HIPCHECK(dev.enter(st));
  uint8_t* work = static_cast<uint8_t*>(d_work);
  uint64_t counts[256];
  const int rc = count_and_scan(d_inst, n, d_rank_of_inst, n_inst, world, L, work, st, ptab.data(), ptab.size() * 8, counts,
                                dev.dev);
  if (rc == CC_ERR_INVALID) return set_err(CC_ERR_INVALID, "merge (device): rank_of_inst names a rank >= world");
  if (rc != CC_OK) return rc;
  for (uint32_t r = 0; r < world; ++r)
    if (counts[r] && (!parts[r].status || !parts[r].value)) return set_err(CC_ERR_INVALID, "merge (device): null part column");
  Timing& tm = g_timing;
  if (tm.on) HIPCHECK(hipEventRecord(tm.ev[3], st));
  hipLaunchKernelGGL(k_merge_gather, dim3(grid_for_tiles(L.tiles)), dim3(kSThreads), 0, st, work + L.own,
                     reinterpret_cast<const uint64_t*>(work + L.base), n, L.tiles, world,
                     reinterpret_cast<const void* const*>(work + L.ptab), d_out->status, d_out->value);
  if (tm.on) {
    HIPCHECK(hipEventRecord(tm.ev[4], st));
    tm.moved = true;
  }
  HIPCHECK(hipGetLastError());
  return CC_OK;
}
