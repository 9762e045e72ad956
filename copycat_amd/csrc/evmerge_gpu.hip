// evmerge_gpu.hip — the per-rank event streams of a sharded log back into log order, on the device (DESIGN §6 "The
// event merge").  cc_merge_events_device is evmerge.cpp's cc_merge_events for streams that sit in HBM, byte for byte.
//
// A log row belongs to one rank and a rank's events are ordered by pos, so the merged stream is, log row by log row,
// the owning rank's run of events for that row.  Four kernels in separate launches, none of which has a workgroup wait
// for another, and no result that rests on the order in which an atomic is served:
//   k_evm_mark    grid (x, rank): every event of every rank (the counts are read on the device).  The preconditions
//                 go to the error word; the head of each run of equal pos stores one 8-byte record at the run's log
//                 row (the run's first event index, the rank, "present", and "single" when the head is the tail
//                 too); the tail of a longer run stores the run's end.  Plain stores to distinct rows (the records
//                 are cleared before; an end is read only where a record says that it was written).
//   k_evm_sums    a workgroup per tile of CC_EVMERGE_TILE_ROWS log rows: the tile's events (1, or end - first, per
//                 present row)
//   k_evm_scan    one workgroup: exclusive prefix of the tile sums, and the total
//   k_evm_gather  a workgroup per tile: the rows' offsets rebuilt in LDS, then the tile's contiguous output range is
//                 filled CC_EVMERGE_WINDOW_EVENTS at a time: an output event finds its row by a search of the offsets
//                 and reads parts[owner][first[row] + k - off[row]].  Within a tile each rank's reads are one
//                 contiguous run; every store is in output order.
// The host waits once, after k_evm_scan, for the counts, the total and the error word: nothing may be written before
// every check has passed.  The error word is an atomicMax over the complement of evmerge_key (the lowest rank's first
// failing event wins whatever the order of service).
#include <cstdio>
#include <vector>

#include "engine_state.h"
#include "evmerge.h"

namespace cc {
namespace {

constexpr uint32_t kET = CC_EVMERGE_TILE_ROWS;
constexpr uint32_t kEWin = CC_EVMERGE_WINDOW_EVENTS;
constexpr uint32_t kEThreads = 256;
constexpr uint32_t kEWaves = kEThreads / kWave;
constexpr uint32_t kERows = kET / kEThreads;  // consecutive rows of a tile per thread
constexpr uint32_t kEMaxGrid = 1u << 16;
static_assert(kERows == 16 && kEWin % kEThreads == 0 && (kET & (kET - 1)) == 0, "16 rows per thread; a power-of-two tile");

// one rank's stream as the kernels see it
struct PartDev {
  const uint32_t *pos, *target;
  const uint8_t *code, *src, *tag;
  const uint64_t *payload, *rows, *count;
  uint64_t row_count, capacity;
};

// ---- workspace layout (every part 256-byte aligned) -----------------------------------------------------------------
//   header  u64 error word, u64 total at byte 8, u64 counts[256] at byte 64
//   rec     u64 per log row: bits 0-31 the first event of the row's run in its rank's stream, 32-39 the rank,
//           bit 40 present (0: a silent row), bit 41 single (the run is one event; else its length is end - first)
//   end     u32 per log row: one past the last event of a run of two or more events; not cleared, and read only for
//           a present row that is not single
//   tsum    u64 per tile; tbase u64 per tile
//   ptab    PartDev[world]
// header and rec are cleared by one memset per call.
constexpr uint64_t kHdrTotal = 8, kHdrCounts = 64, kHdrBytes = 2304;
constexpr uint64_t kRecPresent = 1ull << 40, kRecSingle = 1ull << 41;
struct Layout {
  uint64_t tiles, rec, end, tsum, tbase, ptab, total;
};
inline uint64_t up256(uint64_t x) { return (x + 255) & ~(uint64_t)255; }
inline Layout layout(uint64_t n, uint32_t world) {
  Layout l;
  l.tiles = (n + kET - 1) / kET;
  l.rec = kHdrBytes;
  l.end = l.rec + up256(n * 8);
  l.tsum = l.end + up256(n * 4);
  l.tbase = l.tsum + up256(l.tiles * 8);
  l.ptab = l.tbase + up256(l.tiles * 8);
  l.total = l.ptab + up256((uint64_t)world * sizeof(PartDev));
  return l;
}

__global__ __launch_bounds__(kEThreads) void k_evm_mark(const PartDev* __restrict__ pt, uint64_t n, uint64_t* __restrict__ rec,
                                                        uint32_t* __restrict__ end, unsigned long long* __restrict__ hdr) {
  const uint32_t r = blockIdx.y;
  const PartDev p = pt[r];
  const uint64_t c = p.count ? *p.count : 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) hdr[kHdrCounts / 8 + r] = c;
  // a stream beyond its capacity, or without columns, is refused by the host after the wait: only what exists is read
  const uint64_t m = (p.pos && p.rows) ? (c < p.capacity ? c : p.capacity) : 0;
  unsigned long long bad = 0;  // the complement of the lowest failing key
  for (uint64_t j = (uint64_t)blockIdx.x * kEThreads + threadIdx.x; j < m; j += (uint64_t)gridDim.x * kEThreads) {
    const uint32_t x = p.pos[j];
    const uint32_t prev = j ? p.pos[j - 1] : x;
    const bool last = j + 1 == m;
    const uint32_t next = last ? x : p.pos[j + 1];
    uint64_t key = ~0ull;
    if (x >= p.row_count) {
      key = evmerge_key(r, j, kEvmPosRange);
    } else if (prev > x) {
      key = evmerge_key(r, j, kEvmPosOrder);
    } else {
      const bool head = j == 0 || prev != x, tail = last || next != x;
      if (head || tail) {
        const uint64_t row = p.rows[x];  // x < row_count: inside the rank's row ids
        if (row >= n) {
          key = evmerge_key(r, j, kEvmRowRange);
        } else {
          if (head) rec[row] = (uint32_t)j | (uint64_t)r << 32 | kRecPresent | (tail ? kRecSingle : 0);
          else end[row] = (uint32_t)(j + 1);  // the tail of a run of two or more
        }
      }
    }
    if (~key > bad) bad = ~key;
  }
  if (bad) atomicMax(hdr, bad);
}

// the tile's rows [16 t, 16 t + 16) of thread t: their records' low and high words and their event counts (0 for a
// silent row and beyond the log's last row)
__device__ inline void load_counts(const uint64_t* __restrict__ rec, const uint32_t* __restrict__ end, uint64_t row0,
                                   uint32_t m, uint32_t (&f)[kERows], uint32_t (&h)[kERows], uint32_t (&c)[kERows]) {
  const uint32_t i0 = threadIdx.x * kERows;
  if (i0 + kERows <= m) {
    const uint4* __restrict__ r4 = reinterpret_cast<const uint4*>(rec + row0 + i0);
#pragma unroll
    for (uint32_t q = 0; q < kERows / 2; ++q) {
      const uint4 a = r4[q];
      f[2 * q] = a.x, h[2 * q] = a.y, f[2 * q + 1] = a.z, h[2 * q + 1] = a.w;
    }
  } else {
#pragma unroll
    for (uint32_t q = 0; q < kERows; ++q) {
      const uint64_t v = i0 + q < m ? rec[row0 + i0 + q] : 0;
      f[q] = (uint32_t)v, h[q] = (uint32_t)(v >> 32);
    }
  }
  constexpr uint32_t present = (uint32_t)(kRecPresent >> 32), single = (uint32_t)(kRecSingle >> 32);
#pragma unroll
  for (uint32_t q = 0; q < kERows; ++q) {
    c[q] = (h[q] & present) ? 1u : 0u;
    if ((h[q] & (present | single)) == present) c[q] = end[row0 + i0 + q] - f[q];  // a present row is below m
  }
}

__global__ __launch_bounds__(kEThreads) void k_evm_sums(const uint64_t* __restrict__ rec, const uint32_t* __restrict__ end,
                                                        uint64_t n, uint64_t tiles, uint64_t* __restrict__ tsum) {
  __shared__ uint64_t red[kEThreads];
  const uint32_t t = threadIdx.x;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t row0 = tile * kET;
    const uint32_t m = (uint32_t)(n - row0 < kET ? n - row0 : kET);
    uint32_t f[kERows], h[kERows], c[kERows];
    load_counts(rec, end, row0, m, f, h, c);
    uint64_t s = 0;
#pragma unroll
    for (uint32_t q = 0; q < kERows; ++q) s += c[q];
    red[t] = s;
    __syncthreads();
    for (uint32_t d = kEThreads / 2; d; d >>= 1) {
      if (t < d) red[t] += red[t + d];
      __syncthreads();
    }
    if (t == 0) tsum[tile] = red[0];
    __syncthreads();
  }
}

// One workgroup: thread t sums a contiguous chunk of the tile sums, the 256 sums are scanned in LDS, and the thread
// walks its chunk again writing the bases (k_split_scan for one rank).
__global__ __launch_bounds__(kEThreads) void k_evm_scan(const uint64_t* __restrict__ tsum, uint64_t tiles,
                                                        uint64_t* __restrict__ tbase, unsigned long long* __restrict__ hdr) {
  __shared__ uint64_t part[kEThreads];
  const uint32_t t = threadIdx.x;
  const uint64_t chunk = (tiles + kEThreads - 1) / kEThreads;
  const uint64_t lo = (uint64_t)t * chunk < tiles ? (uint64_t)t * chunk : tiles;
  const uint64_t hi = lo + chunk < tiles ? lo + chunk : tiles;
  uint64_t s = 0;
  for (uint64_t i = lo; i < hi; ++i) s += tsum[i];
  part[t] = s;
  __syncthreads();
  for (uint32_t d = 1; d < kEThreads; d <<= 1) {
    const uint64_t y = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += y;
    __syncthreads();
  }
  uint64_t run = part[t] - s;
  for (uint64_t i = lo; i < hi; ++i) {
    tbase[i] = run;
    run += tsum[i];
  }
  if (t == kEThreads - 1) hdr[kHdrTotal / 8] = part[t];
}

struct GatherArgs {
  const PartDev* pt;
  const uint64_t* rec;
  const uint32_t* end;
  const uint64_t* tbase;
  const unsigned long long* hdr;
  uint64_t n, tiles, total;
  uint32_t *pos, *target;
  uint8_t *code, *src, *tag;
  uint64_t *payload, *count;
};

__global__ __launch_bounds__(kEThreads) void k_evm_gather(const GatherArgs a) {
  __shared__ uint32_t off[kET + 1];
  __shared__ uint32_t fst[kET];
  __shared__ uint8_t ow[kET];
  __shared__ uint32_t wsum[kEWaves];
  const uint32_t t = threadIdx.x, l = t & 63, w = t >> 6;
  if (blockIdx.x == 0 && t == 0 && a.count) *a.count = a.total;
  for (uint64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const uint64_t row0 = tile * kET;
    const uint32_t m = (uint32_t)(a.n - row0 < kET ? a.n - row0 : kET);
    uint32_t f[kERows], h[kERows], c[kERows];
    load_counts(a.rec, a.end, row0, m, f, h, c);
    uint32_t s = 0;
#pragma unroll
    for (uint32_t q = 0; q < kERows; ++q) s += c[q];
    uint32_t inc = s;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const uint32_t y = __shfl_up(inc, d, kWave);
      if (l >= (uint32_t)d) inc += y;
    }
    if (l == kWave - 1) wsum[w] = inc;
    __syncthreads();
    uint32_t run = inc - s;
    for (uint32_t k = 0; k < w; ++k) run += wsum[k];
#pragma unroll
    for (uint32_t q = 0; q < kERows; ++q) {
      const uint32_t i = t * kERows + q;
      off[i] = run, fst[i] = f[q];
      ow[i] = (uint8_t)h[q];
      run += c[q];
    }
    if (t == kEThreads - 1) off[kET] = run;
    __syncthreads();
    const uint32_t tot = off[kET];
    const uint64_t base = a.tbase[tile];
    for (uint64_t k0 = 0; k0 < tot; k0 += kEWin) {  // one window: every thread's events are independent of each other
#pragma unroll
      for (uint32_t u = 0; u < kEWin / kEThreads; ++u) {
        const uint64_t k = k0 + u * kEThreads + t;
        if (k < tot) {
          uint32_t i = 0;  // the last row whose offset is <= k: the row that holds output event k
#pragma unroll
          for (uint32_t step = kET / 2; step; step >>= 1)
            if (off[i + step] <= (uint32_t)k) i += step;
          const uint32_t r = ow[i];
          const uint64_t srcj = (uint64_t)fst[i] + ((uint32_t)k - off[i]);
          const PartDev* __restrict__ p = a.pt + r;
          if (srcj < a.hdr[kHdrCounts / 8 + r]) {  // always, for rows that are the split's; never a read past a stream
            const uint64_t d = base + k;
            a.pos[d] = (uint32_t)(row0 + i);
            a.target[d] = p->target[srcj];
            a.code[d] = p->code[srcj];
            a.src[d] = p->src[srcj];
            a.tag[d] = p->tag[srcj];
            a.payload[d] = p->payload[srcj];
          }
        }
      }
    }
    __syncthreads();
  }
}

__global__ void k_evm_store_count(uint64_t* count, uint64_t total) { *count = total; }

uint32_t grid_for_tiles(uint64_t tiles) { return (uint32_t)(tiles < kEMaxGrid ? tiles : kEMaxGrid); }

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

// Per-step times of the calling thread's last device call (cc_merge_events_device_timing; off by default): events
// around the clear, the mark kernel, the two scan kernels and the gather.
struct Timing {
  bool on = false;
  int dev = -1;
  hipEvent_t ev[6] = {};
  bool scanned = false, moved = false;
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

int fail(const char* what) {
  char msg[128];
  snprintf(msg, sizeof msg, "merge events (device): %s", what);
  return set_err(CC_ERR_INVALID, msg);
}

}  // namespace
}  // namespace cc

extern "C" int cc_merge_events_device_bound(uint64_t n, uint32_t world, uint64_t* work_bytes) {
  using namespace cc;
  if (!work_bytes) return set_err(CC_ERR_INVALID, "merge events bound: null argument");
  if (world == 0 || world > 256) return set_err(CC_ERR_INVALID, "merge events bound: world must be in [1, 256]");
  if (n >= (1ull << 32)) return set_err(CC_ERR_INVALID, "merge events bound: n must be below 2^32");
  *work_bytes = layout(n, world).total;
  return CC_OK;
}

extern "C" int cc_merge_events_device_timing(int enable, float* ms) {
  using namespace cc;
  Timing& tm = g_timing;
  if (ms) {
    ms[0] = ms[1] = ms[2] = ms[3] = 0.f;
    if (tm.scanned) {
      HIPCHECK(hipEventElapsedTime(&ms[0], tm.ev[0], tm.ev[1]));
      HIPCHECK(hipEventElapsedTime(&ms[1], tm.ev[1], tm.ev[2]));
      HIPCHECK(hipEventElapsedTime(&ms[2], tm.ev[2], tm.ev[3]));
    }
    if (tm.moved) {
      HIPCHECK(hipEventSynchronize(tm.ev[5]));
      HIPCHECK(hipEventElapsedTime(&ms[3], tm.ev[4], tm.ev[5]));
    }
  }
  tm.on = enable != 0;
  return CC_OK;
}

extern "C" int cc_merge_events_device(const cc_events* parts, uint64_t* const* d_rows, const uint64_t* row_counts, uint64_t n,
                                      uint32_t world, const cc_events* d_out, uint64_t* total, void* d_work,
                                      uint64_t work_bytes, void* stream) {
  using namespace cc;
  // ---- every check that does not need the counts, before the first HIP call
  if (world == 0 || world > 256) return fail("world must be in [1, 256]");
  if (n >= (1ull << 32)) return fail("n must be below 2^32 (pos is 32 bits wide)");
  if (!parts || !d_rows || !row_counts || !d_out || !total) return fail("null argument");
  if (!d_work || ((uintptr_t)d_work & 15)) return fail("the workspace is null or not 16-byte aligned");
  const Layout L = layout(n, world);
  if (work_bytes < L.total) return fail("the workspace is smaller than cc_merge_events_device_bound");
  auto misaligned = [](const cc_events& e) {
    return (((uintptr_t)e.pos | (uintptr_t)e.target) & 3) || (((uintptr_t)e.payload | (uintptr_t)e.count) & 7);
  };
  if (misaligned(*d_out)) return fail("an output column lacks its natural alignment");
  if (d_out->capacity && (!d_out->pos || !d_out->target || !d_out->code || !d_out->src || !d_out->tag || !d_out->payload))
    return fail("null output column");
  std::vector<PartDev> ptab(world);
  bool any = false;
  uint64_t max_cap = 0;
  for (uint32_t r = 0; r < world; ++r) {
    const cc_events& e = parts[r];
    if (misaligned(e) || ((uintptr_t)d_rows[r] & 7)) return fail("a part's column or row ids lack their natural alignment");
    if (row_counts[r] > n) return fail("a rank's row count exceeds n");
    ptab[r] = PartDev{e.pos, e.target, e.code, e.src, e.tag, e.payload, d_rows[r], e.count, row_counts[r], e.capacity};
    any |= e.count != nullptr;
    if (e.count && e.capacity > max_cap) max_cap = e.capacity;
  }
  *total = 0;
  if (n == 0 || !any) return CC_OK;
  // ---- clear, mark, scan, then the one host wait
  hipStream_t st = (hipStream_t)stream;
  DeviceOf dev;
  HIPCHECK(dev.enter(st));
  uint8_t* work = static_cast<uint8_t*>(d_work);
  unsigned long long* d_hdr = reinterpret_cast<unsigned long long*>(work);
  uint64_t* d_rec = reinterpret_cast<uint64_t*>(work + L.rec);
  uint32_t* d_end = reinterpret_cast<uint32_t*>(work + L.end);
  uint64_t* d_tsum = reinterpret_cast<uint64_t*>(work + L.tsum);
  uint64_t* d_tbase = reinterpret_cast<uint64_t*>(work + L.tbase);
  const PartDev* d_pt = reinterpret_cast<const PartDev*>(work + L.ptab);
  Timing& tm = g_timing;
  if (tm.on) {
    TRY(tm.prepare(dev.dev));
    HIPCHECK(hipEventRecord(tm.ev[0], st));
  }
  HIPCHECK(hipMemsetAsync(work, 0, L.end, st));
  HIPCHECK(hipMemcpyAsync(work + L.ptab, ptab.data(), (uint64_t)world * sizeof(PartDev), hipMemcpyHostToDevice, st));
  if (tm.on) HIPCHECK(hipEventRecord(tm.ev[1], st));
  uint64_t gx = (max_cap + 8 * kEThreads - 1) / (8 * kEThreads);  // about 8 events per thread of the fullest stream
  gx = gx < 1 ? 1 : gx > 2048 ? 2048 : gx;
  hipLaunchKernelGGL(k_evm_mark, dim3((uint32_t)gx, world), dim3(kEThreads), 0, st, d_pt, n, d_rec, d_end, d_hdr);
  if (tm.on) HIPCHECK(hipEventRecord(tm.ev[2], st));
  hipLaunchKernelGGL(k_evm_sums, dim3(grid_for_tiles(L.tiles)), dim3(kEThreads), 0, st, d_rec, d_end, n, L.tiles, d_tsum);
  hipLaunchKernelGGL(k_evm_scan, dim3(1), dim3(kEThreads), 0, st, d_tsum, L.tiles, d_tbase, d_hdr);
  if (tm.on) {
    HIPCHECK(hipEventRecord(tm.ev[3], st));
    tm.scanned = true;
  }
  HIPCHECK(hipGetLastError());
  uint64_t h_hdr[kHdrCounts / 8 + 256];
  HIPCHECK(hipMemcpyAsync(h_hdr, work, kHdrCounts + 8ull * world, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  // ---- the checks that need the counts, in the host call's order
  const uint64_t* counts = h_hdr + kHdrCounts / 8;
  uint64_t sum = 0;
  bool over = false;
  for (uint32_t r = 0; r < world; ++r) sum += counts[r], over |= counts[r] > ptab[r].capacity;
  *total = sum;
  if (over)
    return set_err(CC_ERR_CAPACITY, "merge events (device): a part holds more events than its capacity (that rank's apply overflowed)");
  for (uint32_t r = 0; r < world; ++r) {
    const PartDev& p = ptab[r];
    if (counts[r] >= (1ull << 32)) return fail("a part's count must be below 2^32");
    if (counts[r] && (!p.pos || !p.target || !p.code || !p.src || !p.tag || !p.payload || !p.rows))
      return fail("null column in a part that holds events");
  }
  if (sum >= (1ull << 32)) return fail("the total must be below 2^32");
  if (h_hdr[0]) return evmerge_fail("merge events (device)", ~h_hdr[0]);
  if (h_hdr[kHdrTotal / 8] != sum) return fail("the rows' runs do not add up to the events (rows is not the split's)");
  if (sum > d_out->capacity) return set_err(CC_ERR_CAPACITY, "merge events (device): the output stream is too small");
  if (sum == 0) {
    if (d_out->count) hipLaunchKernelGGL(k_evm_store_count, dim3(1), dim3(1), 0, st, d_out->count, (uint64_t)0);
    HIPCHECK(hipGetLastError());
    return CC_OK;
  }
  GatherArgs a;
  a.pt = d_pt, a.rec = d_rec, a.end = d_end, a.tbase = d_tbase, a.hdr = d_hdr;
  a.n = n, a.tiles = L.tiles, a.total = sum;
  a.pos = d_out->pos, a.target = d_out->target, a.code = d_out->code, a.src = d_out->src, a.tag = d_out->tag;
  a.payload = d_out->payload, a.count = d_out->count;
  if (tm.on) HIPCHECK(hipEventRecord(tm.ev[4], st));
  hipLaunchKernelGGL(k_evm_gather, dim3(grid_for_tiles(L.tiles)), dim3(kEThreads), 0, st, a);
  if (tm.on) {
    HIPCHECK(hipEventRecord(tm.ev[5], st));
    tm.moved = true;
  }
  HIPCHECK(hipGetLastError());
  return CC_OK;
}
