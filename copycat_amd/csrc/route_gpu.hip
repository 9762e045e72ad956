// route_gpu.hip — an event stream grouped by owning client session, on the device (DESIGN §6 "The route").
// cc_route_events_device is route.cpp's cc_route_events for a stream that sits in HBM, byte for byte.
//
// A stable least-significant-digit radix ordering of (session ordinal, event number) is built in the workspace, then
// one gather moves the rows.  Separate launches, none of which has a workgroup wait for another:
//   k_route_key      one lane per event: key = session_of_inst[target] (target checked before it addresses the table,
//                    the entry before it is used), the identity permutation, the lowest bad event -> error word
//   per round of CC_ROUTE_DIGIT_BITS bits (ceil(bits(n_sessions - 1) / CC_ROUTE_DIGIT_BITS) rounds, none for one session):
//   k_route_count    a workgroup per tile of CC_ROUTE_TILE_EVENTS events: cnt[digit][tile]
//   k_route_scan_*   exclusive scan of cnt in (digit, tile) order, in place: per-chunk sums, one workgroup over the
//                    sums, per-chunk scan + base
//   k_route_scatter  per tile: the stable rank of every event among the tile's events of its digit, the (key,
//                    permutation) pairs staged through LDS in digit order and stored run by run to the other buffer
//   k_route_heads    per tile: the positions where the sorted key changes; the same scan; k_route_compact writes the
//                    directory in order
//   k_route_gather   every lane owns four consecutive output rows: random reads through the permutation, 16-byte
//                    stores in output order (a wave's store covers 1 KiB of whole lines; 4-byte words for the byte
//                    columns), so the stores need no staging
// The host waits once, at the end, for the error word and the number of active sessions.  k_route_compact and
// k_route_gather, the only kernels that store outside the workspace, read the error word and the directory capacity on
// the device and store nothing when either refuses the call.
//
// The rank of an event comes from wave ballots (the lanes of a 64-event step that share a digit: one ballot per digit
// bit), wave-private running counters in LDS that the lowest lane of each digit advances, and one scan over the waves'
// totals: stable by construction.  The only atomics are integer sums whose value is not read back and the atomicMin of
// the error word: no result rests on the order in which LDS or L2 serves them (these calls have no engine, so no
// k_selfcheck_lds_order has run before them).
#include <cstdio>

#include "route.h"

namespace cc {
namespace {

constexpr uint32_t kRT = CC_ROUTE_TILE_EVENTS;
constexpr uint32_t kRD = 1u << CC_ROUTE_DIGIT_BITS;
constexpr uint32_t kRThreads = 256;
constexpr uint32_t kRWaves = kRThreads / kWave;
constexpr uint32_t kRSpan = kRT / kRWaves;      // consecutive events of a tile that one wave ranks
constexpr uint32_t kRSteps = kRSpan / kWave;    // 64-event steps per wave
constexpr uint32_t kRPer = kRT / kRThreads;     // events per thread
constexpr uint32_t kScanChunk = kRThreads * 16; // elements of a scan chunk (one workgroup)
constexpr uint32_t kRMaxGrid = 1u << 16;
constexpr uint32_t kRMaxRounds = (32 + CC_ROUTE_DIGIT_BITS - 1) / CC_ROUTE_DIGIT_BITS;
static_assert(kRD == kRThreads && kRWaves == 4 && kRSteps == 16 && kRPer == 16, "one thread per digit value; four waves");
static_assert(kRT % 1024 == 0, "the gather moves 1024 rows per step");

// ---- workspace layout (every part 256-byte aligned) -----------------------------------------------------------------
//   header  u64 error word (all ones: none), u64 active sessions at byte 8, u64 scratch total at byte 16
//   key[2], perm[2]  u32 per event each: the ping-pong buffers
//   cnt     u32 [kRD][tiles]; its first `tiles` words are reused for the heads per tile
//   part    u32 per scan chunk
constexpr uint64_t kHdrBytes = 256;
struct Layout {
  uint64_t tiles, chunks, key[2], perm[2], cnt, part, total;
};
inline uint64_t up256(uint64_t x) { return (x + 255) & ~(uint64_t)255; }
inline Layout layout(uint64_t n) {
  Layout l;
  l.tiles = (n + kRT - 1) / kRT;
  l.chunks = (l.tiles * kRD + kScanChunk - 1) / kScanChunk;
  l.key[0] = kHdrBytes;
  l.perm[0] = l.key[0] + up256(n * 4);
  l.key[1] = l.perm[0] + up256(n * 4);
  l.perm[1] = l.key[1] + up256(n * 4);
  l.cnt = l.perm[1] + up256(n * 4);
  l.part = l.cnt + up256(l.tiles * kRD * 4);
  l.total = l.part + up256(l.chunks * 4);
  return l;
}

// ---- block helpers ----------------------------------------------------------------------------------------------------
// exclusive prefix of s over the workgroup's threads; `all` = the workgroup's sum.  Two barriers.
__device__ inline uint32_t block_exclusive(uint32_t s, uint32_t* wsum, uint32_t& all) {
  const uint32_t t = threadIdx.x, l = t & 63, w = t >> 6;
  uint32_t inc = s;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const uint32_t y = __shfl_up(inc, d, kWave);
    if (l >= (uint32_t)d) inc += y;
  }
  __syncthreads();  // (wsum may still be read from the call before)
  if (l == kWave - 1) wsum[w] = inc;
  __syncthreads();
  uint32_t before = 0;
  all = 0;
#pragma unroll
  for (uint32_t k = 0; k < kRWaves; ++k) {
    if (k < w) before += wsum[k];
    all += wsum[k];
  }
  return before + inc - s;
}

__device__ inline void load16(const uint32_t* __restrict__ a, uint64_t i0, uint64_t m, uint32_t (&v)[16]) {
  if (i0 + 16 <= m) {
    const uint4* __restrict__ p = reinterpret_cast<const uint4*>(a + i0);  // i0 is a multiple of 16, `a` 256-byte aligned
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      const uint4 x = p[q];
      v[4 * q] = x.x, v[4 * q + 1] = x.y, v[4 * q + 2] = x.z, v[4 * q + 3] = x.w;
    }
  } else {
#pragma unroll
    for (uint32_t q = 0; q < 16; ++q) v[q] = i0 + q < m ? a[i0 + q] : 0u;
  }
}

// The lanes of the wave that are valid and hold digit d: one ballot per digit bit.  Only valid lanes may use the result.
__device__ inline uint64_t match_digit(uint32_t d, bool valid) {
  uint64_t m = ballot(valid);
#pragma unroll
  for (uint32_t b = 0; b < CC_ROUTE_DIGIT_BITS; ++b) {
    const bool bit = (d >> b) & 1u;
    const uint64_t bb = ballot(bit);
    m &= bit ? bb : ~bb;
  }
  return m;
}

// ---- the generic exclusive scan of a u32 array, in place, in three launches -------------------------------------------
__global__ __launch_bounds__(kRThreads) void k_route_scan_part(const uint32_t* __restrict__ a, uint64_t m, uint64_t chunks,
                                                               uint32_t* __restrict__ part) {
  __shared__ uint32_t wsum[kRWaves];
  for (uint64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    uint32_t v[16];
    load16(a, c * kScanChunk + threadIdx.x * 16, m, v);
    uint32_t s = 0, all;
#pragma unroll
    for (uint32_t q = 0; q < 16; ++q) s += v[q];
    (void)block_exclusive(s, wsum, all);
    if (threadIdx.x == 0) part[c] = all;
  }
}

// One workgroup: thread t sums a contiguous run of the chunk sums, the 256 sums are scanned in LDS, and the thread walks
// its run again writing the bases (k_evm_scan's shape).  The grand total (below 2^32: it counts events) goes to *total.
__global__ __launch_bounds__(kRThreads) void k_route_scan(uint32_t* __restrict__ part, uint64_t chunks,
                                                          unsigned long long* __restrict__ total) {
  __shared__ uint32_t wsum[kRWaves];
  const uint32_t t = threadIdx.x;
  const uint64_t run = (chunks + kRThreads - 1) / kRThreads;
  const uint64_t lo = (uint64_t)t * run < chunks ? (uint64_t)t * run : chunks;
  const uint64_t hi = lo + run < chunks ? lo + run : chunks;
  uint32_t s = 0, all;
  for (uint64_t i = lo; i < hi; ++i) s += part[i];
  uint32_t at = block_exclusive(s, wsum, all);
  for (uint64_t i = lo; i < hi; ++i) {
    const uint32_t c = part[i];
    part[i] = at;
    at += c;
  }
  if (t == 0) *total = all;
}

__global__ __launch_bounds__(kRThreads) void k_route_scan_add(uint32_t* __restrict__ a, uint64_t m, uint64_t chunks,
                                                              const uint32_t* __restrict__ part) {
  __shared__ uint32_t wsum[kRWaves];
  for (uint64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const uint64_t i0 = c * kScanChunk + threadIdx.x * 16;
    uint32_t v[16];
    load16(a, i0, m, v);
    uint32_t s = 0, all;
#pragma unroll
    for (uint32_t q = 0; q < 16; ++q) s += v[q];
    uint32_t at = block_exclusive(s, wsum, all) + part[c];
#pragma unroll
    for (uint32_t q = 0; q < 16; ++q) {
      const uint32_t x = v[q];
      v[q] = at;
      at += x;
    }
    if (i0 + 16 <= m) {
      uint4* __restrict__ p = reinterpret_cast<uint4*>(a + i0);
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q) p[q] = make_uint4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    } else {
#pragma unroll
      for (uint32_t q = 0; q < 16; ++q)
        if (i0 + q < m) a[i0 + q] = v[q];
    }
  }
}

// ---- the key -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRThreads) void k_route_key(const uint32_t* __restrict__ target, uint64_t n,
                                                         const uint32_t* __restrict__ tab, uint32_t n_inst, uint32_t n_sessions,
                                                         uint32_t* __restrict__ key, uint32_t* __restrict__ perm,
                                                         unsigned long long* __restrict__ hdr) {
  unsigned long long bad = kRouteNoErr;  // the lowest bad event of this lane
  for (uint64_t j = (uint64_t)blockIdx.x * kRThreads + threadIdx.x; j < n; j += (uint64_t)gridDim.x * kRThreads) {
    const uint32_t x = target[j];
    uint32_t s = 0;
    unsigned long long e = kRouteNoErr;
    if (x >= n_inst) {
      e = route_key(j, kRouteTarget);
    } else {
      s = tab[x];
      if (s >= n_sessions) e = route_key(j, kRouteSession), s = 0;
    }
    if (e < bad) bad = e;
    key[j] = s;  // a bad event sorts as session 0; nothing leaves the workspace once the error word is set
    perm[j] = (uint32_t)j;
  }
  if (bad != kRouteNoErr) atomicMin(hdr, bad);  // the minimum: whatever order the atomics are served in
}

// ---- one round -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRThreads) void k_route_count(const uint32_t* __restrict__ key, uint64_t n, uint64_t tiles,
                                                           uint32_t shift, uint32_t* __restrict__ cnt) {
  __shared__ uint32_t h[kRD];
  const uint32_t t = threadIdx.x;
  const uint64_t below = lanemask_lt();
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    h[t] = 0;
    __syncthreads();
    const uint64_t row0 = tile * kRT;
    const uint32_t m = (uint32_t)(n - row0 < kRT ? n - row0 : kRT);
    uint32_t k[kRPer];
#pragma unroll
    for (uint32_t q = 0; q < kRPer; ++q) {
      const uint32_t i = q * kRThreads + t;
      k[q] = i < m ? key[row0 + i] : 0u;
    }
#pragma unroll
    for (uint32_t q = 0; q < kRPer; ++q) {
      const bool valid = q * kRThreads + t < m;
      const uint32_t d = (k[q] >> shift) & (kRD - 1);
      const uint64_t mk = match_digit(d, valid);
      if (valid && (mk & below) == 0) atomicAdd(&h[d], (uint32_t)__popcll(mk));  // a sum: its value is not read back
    }
    __syncthreads();
    cnt[(uint64_t)t * tiles + tile] = h[t];
    __syncthreads();
  }
}

__global__ __launch_bounds__(kRThreads) void k_route_scatter(const uint32_t* __restrict__ key_in, const uint32_t* __restrict__ perm_in,
                                                             uint32_t* __restrict__ key_out, uint32_t* __restrict__ perm_out,
                                                             const uint32_t* __restrict__ base, uint64_t n, uint64_t tiles,
                                                             uint32_t shift) {
  __shared__ uint32_t skey[kRT];
  __shared__ uint32_t sperm[kRT];
  __shared__ uint32_t wc[kRWaves][kRD];
  __shared__ uint32_t boff[kRD];   // the first staging slot of digit d
  __shared__ uint32_t delta[kRD];  // staging slot p of digit d goes to output position p + delta[d] (modulo 2^32)
  __shared__ uint32_t wsum[kRWaves];
  const uint32_t t = threadIdx.x, l = t & 63, w = t >> 6;
  const uint64_t below = lanemask_lt();
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t row0 = tile * kRT;
    const uint32_t m = (uint32_t)(n - row0 < kRT ? n - row0 : kRT);
#pragma unroll
    for (uint32_t k = 0; k < kRWaves; ++k) wc[k][t] = 0;
    __syncthreads();
    // wave w ranks events [w * kRSpan, (w + 1) * kRSpan) in 64-event steps: an event's rank inside its wave is the
    // wave's running counter of its digit (read by every lane of the step before the digit's lowest lane advances it)
    // plus the equal lanes below it
    uint32_t k[kRSteps], rk[kRSteps];
#pragma unroll
    for (uint32_t s = 0; s < kRSteps; ++s) {
      const uint32_t i = w * kRSpan + s * kWave + l;
      k[s] = i < m ? key_in[row0 + i] : 0u;
    }
    uint32_t* const mine = wc[w];
#pragma unroll
    for (uint32_t s = 0; s < kRSteps; ++s) {
      const bool valid = w * kRSpan + s * kWave + l < m;
      const uint32_t d = (k[s] >> shift) & (kRD - 1);
      const uint64_t mk = match_digit(d, valid);
      const uint32_t old = mine[d];
      rk[s] = old + (uint32_t)__popcll(mk & below);
      if (valid && (mk & below) == 0) mine[d] = old + (uint32_t)__popcll(mk);
      __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    // thread d: the waves' counts of digit d become the waves' offsets inside the digit's run
    const uint32_t c0 = wc[0][t], c1 = wc[1][t], c2 = wc[2][t], c3 = wc[3][t];
    wc[0][t] = 0, wc[1][t] = c0, wc[2][t] = c0 + c1, wc[3][t] = c0 + c1 + c2;
    uint32_t all;
    const uint32_t first = block_exclusive(c0 + c1 + c2 + c3, wsum, all);
    boff[t] = first;
    delta[t] = base[(uint64_t)t * tiles + tile] - first;
    __syncthreads();
#pragma unroll
    for (uint32_t s = 0; s < kRSteps; ++s) {
      const uint32_t i = w * kRSpan + s * kWave + l;
      if (i < m) {
        const uint32_t d = (k[s] >> shift) & (kRD - 1);
        const uint32_t p = boff[d] + mine[d] + rk[s];  // below m: the ranks of a digit are 0 .. its count - 1
        if (p < kRT) {
          skey[p] = k[s];
          sperm[p] = perm_in[row0 + i];
        }
      }
    }
    __syncthreads();
    for (uint32_t p = t; p < m; p += kRThreads) {
      const uint32_t kk = skey[p];
      const uint32_t dst = p + delta[(kk >> shift) & (kRD - 1)];
      if (dst < n) {  // always: base is the scan of the same keys' counts
        key_out[dst] = kk;
        perm_out[dst] = sperm[p];
      }
    }
    __syncthreads();
  }
}

// ---- the directory -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRThreads) void k_route_heads(const uint32_t* __restrict__ key, uint64_t n, uint64_t tiles,
                                                           uint32_t* __restrict__ hcnt) {
  __shared__ uint32_t wsum[kRWaves];
  const uint32_t t = threadIdx.x;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t row0 = tile * kRT;
    const uint32_t m = (uint32_t)(n - row0 < kRT ? n - row0 : kRT);
    uint32_t c = 0, all;
#pragma unroll
    for (uint32_t q = 0; q < kRPer; ++q) {
      const uint32_t i = q * kRThreads + t;
      const uint64_t j = row0 + i;
      if (i < m) c += (j == 0 || key[j] != key[j - 1]) ? 1u : 0u;
    }
    (void)block_exclusive(c, wsum, all);
    if (t == 0) hcnt[tile] = all;
  }
}

struct DirDev {
  uint32_t *session, *start;
  uint64_t capacity;
  uint64_t* count;
};

// nothing leaves the workspace when the error word is set or the directory is too small
__device__ inline bool refused(const unsigned long long* __restrict__ hdr, uint64_t dir_capacity) {
  return hdr[0] != kRouteNoErr || hdr[1] > dir_capacity;
}

__global__ __launch_bounds__(kRThreads) void k_route_compact(const uint32_t* __restrict__ key, uint64_t n, uint64_t tiles,
                                                             const uint32_t* __restrict__ hbase,
                                                             const unsigned long long* __restrict__ hdr, const DirDev dir) {
  __shared__ uint32_t wsum[kRWaves];
  if (refused(hdr, dir.capacity)) return;
  const uint32_t t = threadIdx.x, l = t & 63, w = t >> 6;
  const uint64_t below = lanemask_lt();
  if (blockIdx.x == 0 && t == 0) {
    dir.start[hdr[1]] = (uint32_t)n;
    *dir.count = hdr[1];
  }
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t row0 = tile * kRT;
    const uint32_t m = (uint32_t)(n - row0 < kRT ? n - row0 : kRT);
    uint32_t run = hbase[tile];
    for (uint32_t q = 0; q < kRPer; ++q) {
      const uint32_t i = q * kRThreads + t;
      const uint64_t j = row0 + i;
      uint32_t kk = 0;
      bool head = false;
      if (i < m) {
        kk = key[j];
        head = j == 0 || kk != key[j - 1];
      }
      const uint64_t b = ballot(head);
      if (l == 0) wsum[w] = (uint32_t)__popcll(b);
      __syncthreads();
      uint32_t at = run + (uint32_t)__popcll(b & below);
#pragma unroll
      for (uint32_t k = 0; k < kRWaves; ++k) {
        if (k < w) at += wsum[k];
        run += wsum[k];
      }
      if (head && at < dir.capacity) {  // always: hbase is the scan of the same heads
        dir.session[at] = kk;
        dir.start[at] = (uint32_t)j;
      }
      __syncthreads();
    }
  }
}

// ---- the rows ------------------------------------------------------------------------------------------------------------
struct GatherArgs {
  const uint32_t *pos, *target;
  const uint8_t *code, *src, *tag;
  const uint64_t *payload, *id_of_inst;
  uint32_t *opos, *otarget;
  uint8_t *ocode, *osrc, *otag;
  uint64_t *opayload, *oinst, *ocount;
  const uint32_t* perm;
  const unsigned long long* hdr;
  uint64_t n, tiles, dir_capacity;
  uint32_t wide;  // every output column takes 16-byte (the byte columns: 4-byte) stores at a multiple of four rows
};

__global__ __launch_bounds__(kRThreads) void k_route_gather(const GatherArgs a) {
  if (refused(a.hdr, a.dir_capacity)) return;
  const uint32_t t = threadIdx.x;
  if (blockIdx.x == 0 && t == 0 && a.ocount) *a.ocount = a.n;
  for (uint64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
#pragma unroll 1
    for (uint32_t step = 0; step < kRT / 1024; ++step) {
      const uint64_t j0 = tile * kRT + step * 1024 + 4 * t;  // a multiple of 4
      if (j0 >= a.n) break;
      const bool full = j0 + 4 <= a.n;
      uint32_t s[4] = {0, 0, 0, 0};
      if (full) {
        const uint4 p = *reinterpret_cast<const uint4*>(a.perm + j0);
        s[0] = p.x, s[1] = p.y, s[2] = p.z, s[3] = p.w;
      } else {
        for (uint32_t q = 0; q < 4; ++q)
          if (j0 + q < a.n) s[q] = a.perm[j0 + q];
      }
      uint32_t po[4], ta[4], co[4], sr[4], tg[4];
      uint64_t pa[4], id[4];
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q) {
        const uint32_t r = s[q] < a.n ? s[q] : 0u;  // always below n: a permutation
        po[q] = a.pos[r], ta[q] = a.target[r], co[q] = a.code[r], sr[q] = a.src[r], tg[q] = a.tag[r], pa[q] = a.payload[r];
      }
      if (a.oinst) {
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) id[q] = a.id_of_inst[ta[q]];  // below n_inst: the error word is clear
      }
      if (full && a.wide) {
        *reinterpret_cast<uint4*>(a.opos + j0) = make_uint4(po[0], po[1], po[2], po[3]);
        *reinterpret_cast<uint4*>(a.otarget + j0) = make_uint4(ta[0], ta[1], ta[2], ta[3]);
        *reinterpret_cast<uint32_t*>(a.ocode + j0) = co[0] | co[1] << 8 | co[2] << 16 | co[3] << 24;
        *reinterpret_cast<uint32_t*>(a.osrc + j0) = sr[0] | sr[1] << 8 | sr[2] << 16 | sr[3] << 24;
        *reinterpret_cast<uint32_t*>(a.otag + j0) = tg[0] | tg[1] << 8 | tg[2] << 16 | tg[3] << 24;
        ulonglong2* const op = reinterpret_cast<ulonglong2*>(a.opayload + j0);
        op[0] = make_ulonglong2(pa[0], pa[1]);
        op[1] = make_ulonglong2(pa[2], pa[3]);
        if (a.oinst) {
          ulonglong2* const oi = reinterpret_cast<ulonglong2*>(a.oinst + j0);
          oi[0] = make_ulonglong2(id[0], id[1]);
          oi[1] = make_ulonglong2(id[2], id[3]);
        }
      } else {
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
          if (j0 + q < a.n) {
            a.opos[j0 + q] = po[q], a.otarget[j0 + q] = ta[q];
            a.ocode[j0 + q] = (uint8_t)co[q], a.osrc[j0 + q] = (uint8_t)sr[q], a.otag[j0 + q] = (uint8_t)tg[q];
            a.opayload[j0 + q] = pa[q];
            if (a.oinst) a.oinst[j0 + q] = id[q];
          }
        }
      }
    }
  }
}

uint32_t grid_for(uint64_t blocks) { return (uint32_t)(blocks < 1 ? 1 : blocks < kRMaxGrid ? blocks : kRMaxGrid); }

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

// Per-kernel times of the calling thread's last device call (cc_route_events_device_timing; off by default): an event
// before k_route_key and one after every step: the key, per round the count, the scan and the scatter, the directory,
// the gather.
constexpr uint32_t kTimingEvents = 2 + 3 * kRMaxRounds + 2;
struct Timing {
  bool on = false;
  int dev = -1;
  hipEvent_t ev[kTimingEvents] = {};
  uint32_t rounds = 0;
  bool done = false;
  int prepare(int device) {
    done = false;
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
  snprintf(msg, sizeof msg, "route events (device): %s", what);
  return set_err(CC_ERR_INVALID, msg);
}

// exclusive scan of a[0, m) in place on `st`; the sum goes to *d_total
void scan_u32(uint32_t* a, uint64_t m, uint32_t* part, unsigned long long* d_total, hipStream_t st) {
  const uint64_t chunks = (m + kScanChunk - 1) / kScanChunk;
  hipLaunchKernelGGL(k_route_scan_part, dim3(grid_for(chunks)), dim3(kRThreads), 0, st, a, m, chunks, part);
  hipLaunchKernelGGL(k_route_scan, dim3(1), dim3(kRThreads), 0, st, part, chunks, d_total);
  hipLaunchKernelGGL(k_route_scan_add, dim3(grid_for(chunks)), dim3(kRThreads), 0, st, a, m, chunks, part);
}

}  // namespace
}  // namespace cc

extern "C" int cc_route_events_device_bound(uint64_t n_events, uint32_t n_sessions, uint64_t* work_bytes) {
  using namespace cc;
  if (!work_bytes) return set_err(CC_ERR_INVALID, "route events bound: null argument");
  if (n_events >= (1ull << 32)) return set_err(CC_ERR_INVALID, "route events bound: n_events must be below 2^32");
  if (n_events && n_sessions == 0) return set_err(CC_ERR_INVALID, "route events bound: n_sessions is 0 with events to route");
  *work_bytes = layout(n_events).total;  // (the session count sets the number of rounds, not the size of anything)
  return CC_OK;
}

extern "C" int cc_route_events_device_timing(int enable, float* ms) {
  using namespace cc;
  Timing& tm = g_timing;
  if (ms) {
    for (int k = 0; k < CC_ROUTE_TIMING_SLOTS; ++k) ms[k] = 0.f;
    if (tm.done) {
      const uint32_t last = 2 + 3 * tm.rounds + 1;
      HIPCHECK(hipEventSynchronize(tm.ev[last]));
      auto span = [&](uint32_t i, float& acc) {
        float x = 0.f;
        const hipError_t e = hipEventElapsedTime(&x, tm.ev[i], tm.ev[i + 1]);
        acc += x;
        return e;
      };
      HIPCHECK(span(0, ms[0]));
      for (uint32_t r = 0; r < tm.rounds; ++r)
        for (uint32_t k = 0; k < 3; ++k) HIPCHECK(span(1 + 3 * r + k, ms[1 + k]));
      HIPCHECK(span(1 + 3 * tm.rounds, ms[4]));
      HIPCHECK(span(2 + 3 * tm.rounds, ms[5]));
    }
  }
  tm.on = enable != 0;
  return CC_OK;
}

extern "C" int cc_route_events_device(const cc_events* d_in, uint64_t n, const uint32_t* d_session_of_inst,
                                      const uint64_t* d_id_of_inst, uint32_t n_inst, uint32_t n_sessions,
                                      const cc_events* d_out, uint64_t* d_out_instance, const cc_route_dir* d_dir,
                                      uint64_t* n_active, void* d_work, uint64_t work_bytes, void* stream) {
  using namespace cc;
  // ---- every argument check, before the first HIP call
  if (n < (1ull << 32)) {  // (route_check_args refuses a larger n itself)
    if (!d_work || ((uintptr_t)d_work & 15)) return fail("the workspace is null or not 16-byte aligned");
    if (work_bytes < layout(n).total) return fail("the workspace is smaller than cc_route_events_device_bound");
  }
  if (const int rc = route_check_args("route events (device)", d_in, n, d_session_of_inst, d_id_of_inst, n_inst, n_sessions,
                                      d_out, d_out_instance, d_dir, n_active))
    return rc;
  if (n == 0) {
    *n_active = 0;
    return CC_OK;
  }
  const Layout L = layout(n);
  const uint32_t rounds = route_rounds(n_sessions);
  hipStream_t st = (hipStream_t)stream;
  DeviceOf dev;
  HIPCHECK(dev.enter(st));
  uint8_t* work = static_cast<uint8_t*>(d_work);
  unsigned long long* d_hdr = reinterpret_cast<unsigned long long*>(work);
  uint32_t* key[2] = {reinterpret_cast<uint32_t*>(work + L.key[0]), reinterpret_cast<uint32_t*>(work + L.key[1])};
  uint32_t* perm[2] = {reinterpret_cast<uint32_t*>(work + L.perm[0]), reinterpret_cast<uint32_t*>(work + L.perm[1])};
  uint32_t* cnt = reinterpret_cast<uint32_t*>(work + L.cnt);
  uint32_t* part = reinterpret_cast<uint32_t*>(work + L.part);
  Timing& tm = g_timing;
  uint32_t evi = 0;
  if (tm.on) TRY(tm.prepare(dev.dev));
#define CC_ROUTE_MARK() \
  if (tm.on) HIPCHECK(hipEventRecord(tm.ev[evi++], st))
  HIPCHECK(hipMemsetAsync(work, 0xFF, 8, st));  // the error word: none
  CC_ROUTE_MARK();
  const uint32_t tile_grid = grid_for(L.tiles);
  hipLaunchKernelGGL(k_route_key, dim3(grid_for((n + 4 * kRThreads - 1) / (4 * kRThreads))), dim3(kRThreads), 0, st,
                     d_in->target, n, d_session_of_inst, n_inst, n_sessions, key[0], perm[0], d_hdr);
  CC_ROUTE_MARK();
  int cur = 0;
  for (uint32_t r = 0; r < rounds; ++r, cur ^= 1) {
    const uint32_t shift = r * CC_ROUTE_DIGIT_BITS;
    hipLaunchKernelGGL(k_route_count, dim3(tile_grid), dim3(kRThreads), 0, st, key[cur], n, L.tiles, shift, cnt);
    CC_ROUTE_MARK();
    scan_u32(cnt, L.tiles * kRD, part, d_hdr + 2, st);
    CC_ROUTE_MARK();
    hipLaunchKernelGGL(k_route_scatter, dim3(tile_grid), dim3(kRThreads), 0, st, key[cur], perm[cur], key[cur ^ 1],
                       perm[cur ^ 1], cnt, n, L.tiles, shift);
    CC_ROUTE_MARK();
  }
  const DirDev dir{d_dir->session, d_dir->start, d_dir->capacity, d_dir->count};
  hipLaunchKernelGGL(k_route_heads, dim3(tile_grid), dim3(kRThreads), 0, st, key[cur], n, L.tiles, cnt);
  scan_u32(cnt, L.tiles, part, d_hdr + 1, st);
  hipLaunchKernelGGL(k_route_compact, dim3(tile_grid), dim3(kRThreads), 0, st, key[cur], n, L.tiles, cnt, d_hdr, dir);
  CC_ROUTE_MARK();
  GatherArgs a;
  a.pos = d_in->pos, a.target = d_in->target, a.code = d_in->code, a.src = d_in->src, a.tag = d_in->tag;
  a.payload = d_in->payload, a.id_of_inst = d_id_of_inst;
  a.opos = d_out->pos, a.otarget = d_out->target, a.ocode = d_out->code, a.osrc = d_out->src, a.otag = d_out->tag;
  a.opayload = d_out->payload, a.oinst = d_out_instance, a.ocount = d_out->count;
  a.perm = perm[cur], a.hdr = d_hdr;
  a.n = n, a.tiles = L.tiles, a.dir_capacity = d_dir->capacity;
  a.wide = ((((uintptr_t)a.opos | (uintptr_t)a.otarget | (uintptr_t)a.opayload | (uintptr_t)a.oinst) & 15) == 0 &&
            (((uintptr_t)a.ocode | (uintptr_t)a.osrc | (uintptr_t)a.otag) & 3) == 0)
               ? 1u
               : 0u;
  hipLaunchKernelGGL(k_route_gather, dim3(tile_grid), dim3(kRThreads), 0, st, a);
  CC_ROUTE_MARK();
#undef CC_ROUTE_MARK
  if (tm.on) tm.rounds = rounds, tm.done = true;
  HIPCHECK(hipGetLastError());
  // ---- the one host wait: the error word and the active sessions
  uint64_t h_hdr[2];
  HIPCHECK(hipMemcpyAsync(h_hdr, work, sizeof h_hdr, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  if (h_hdr[0] != kRouteNoErr) return route_fail("route events (device)", h_hdr[0]);
  *n_active = h_hdr[1];
  if (h_hdr[1] > d_dir->capacity) return set_err(CC_ERR_CAPACITY, "route events (device): the directory is too small");
  return CC_OK;
}
