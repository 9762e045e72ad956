// topic_fanout.hip — TopicState.publish (TopicState.java:67-82) expanded into its "message" events.
//
// k_apply_coord applies a publish in O(1): it writes the commit's event count (ev_cnt[g] = n listeners) and appends one
// FanRec (common.h) — the staging position g, the canonical message, n, and where the listeners' instance slots as
// they stood at that row lie in the sub-batch's listener log (a snapshot shared by every publish between two changes
// of the list).  k_topic_fanout, launched after the coordination apply and before the order pass (events.hip), writes
// the n events of every record into the sub-batch's event arena:
//   EvRec{g, target = log[snap + i], payload, k = first + i, code, tag, CC_EVSRC_COMMIT},  i = 0 .. n - 1,
// with the code and `first` from the record (FanRec.tag; a topic's records carry CC_EV_MESSAGE and 0),
// i.e. in ascending listener instance id (engine-defined: each event of one publish goes to a different session).  The
// order pass then sees only real events, each with its (g, k) and a matching ev_cnt.
//
// MessageBusState's register / unregister / leave (MessageBusState.java:84-86,112-114,134-136) publish a
// ConsumerInfo(topic, address) to every member of the bus: the same records with CC_EV_BUS_REGISTER / _UNREGISTER, the
// payload topic << 32 | address, against a snapshot of the members.  A leave leaves one record per topic of the leaver
// for the same commit g; `first` runs on across them (0, n, 2n, ...), so the commit's emission indices are dense.
//
// A workgroup takes kFT records at a time: a scan of their n, one arena reservation for all their events (never one
// per event), then (record, i) flattened over the lanes — lane e of a pass handles event e of the chunk, found by a
// search of the scanned counts in LDS — so a publish to 0, 1 or 2 listeners (the common pub/sub case) costs a lane or
// two, not a wave, while the lanes of a long record read a contiguous run of its snapshot.  A pass's events are
// assembled in LDS as 8-byte words and stored to the arena (24-byte records, contiguous for the whole chunk) as
// 16-byte words; only the first and last 8 bytes of a pass may go alone (an odd event index is 8 mod 16).
//
// Overflow: the fan records and the listener log are sized like the arena (FanCtx) and overflow only if the arena does;
// then, or when a chunk's reservation passes the arena's end, nothing partial is written: the arena count ends past
// its capacity, k_ev_tiles reports kErrEvents, and the call fails (or the prefix form rolls back) as for any other
// event overflow.
#include "common.h"
#include "engine_internal.h"

namespace cc {

constexpr int kFT = 256;            // threads per workgroup = fan records per chunk = events per pass
constexpr int kFanMaxGrid = 2048;   // workgroups (each strides over the chunks)

__global__ __launch_bounds__(kFT) void k_topic_fanout(const FanCtx* __restrict__ fx, EvRec* __restrict__ arena,
                                                      unsigned long long* __restrict__ arena_n, uint64_t arena_cap,
                                                      uint32_t* __restrict__ err_out) {
  __shared__ uint32_t pre[kFT + 1];     // exclusive prefix of the chunk's n
  __shared__ uint32_t rg[kFT], rsnap[kFT], rtag[kFT];
  __shared__ uint64_t rpay[kFT];
  __shared__ uint32_t wsum[kFT / kWave];
  __shared__ unsigned long long sbase;
  __shared__ uint64_t stage[kFT * 3];   // one pass's events as 8-byte words
  const uint32_t t = threadIdx.x, w = t >> 6, l = t & 63;
  const unsigned long long nrec = fx->rec_n, nlog = fx->log_n;
  const uint64_t cap = fx->cap;
  if (nrec > cap || nlog > cap) {  // more fan-out than the arena holds: the call fails, nothing is expanded
    if (blockIdx.x == 0 && t == 0) {
      atomicAdd(arena_n, (unsigned long long)arena_cap + 1ull);
      atomicOr(err_out, kErrEvents);
    }
    return;
  }
  const FanRec* __restrict__ rec = fx->rec;
  const uint32_t* __restrict__ lg = fx->log;
  for (uint64_t c0 = (uint64_t)blockIdx.x * kFT; c0 < nrec; c0 += (uint64_t)gridDim.x * kFT) {  // block-uniform
    uint32_t n = 0;
    if (c0 + t < nrec) {
      const FanRec r = rec[c0 + t];
      n = r.n;
      rg[t] = r.g;
      rsnap[t] = r.snap;
      rtag[t] = r.tag;
      rpay[t] = r.payload;
    }
    uint32_t inc = n;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t y = __shfl_up(inc, d, 64);
      if (l >= (uint32_t)d) inc += y;
    }
    if (l == 63) wsum[w] = inc;
    __syncthreads();
    uint32_t run = inc - n, total = 0;
#pragma unroll
    for (int q = 0; q < kFT / kWave; ++q) {
      if ((uint32_t)q < w) run += wsum[q];
      total += wsum[q];
    }
    pre[t] = run;
    if (t == 0) {
      pre[kFT] = total;
      sbase = total ? atomicAdd(arena_n, (unsigned long long)total) : 0ull;  // one reservation per chunk
    }
    __syncthreads();
    const unsigned long long base = sbase;
    if (base + total <= arena_cap) {  // (else counted past capacity: kErrEvents from k_ev_tiles)
      for (uint32_t e0 = 0; e0 < total; e0 += kFT) {  // block-uniform
        const uint32_t cnt = total - e0 < (uint32_t)kFT ? total - e0 : (uint32_t)kFT;
        if (t < cnt) {
          const uint32_t e = e0 + t;
          uint32_t lo = 0, hi = kFT;  // the record holding event e: pre[lo] <= e < pre[lo + 1]
          while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (pre[mid] <= e) lo = mid; else hi = mid;
          }
          const uint32_t i = e - pre[lo];
          const uint32_t target = lg[(uint64_t)rsnap[lo] + i];
          stage[3 * t + 0] = (uint64_t)rg[lo] | ((uint64_t)target << 32);
          stage[3 * t + 1] = rpay[lo];
          // FanRec.tag = tag | code << 8 | first emission index << 16 (a topic's: CC_EV_MESSAGE, 0)
          const uint32_t tg = rtag[lo];
          stage[3 * t + 2] = (uint64_t)((i + (tg >> 16)) & 0xFFFFu) | ((uint64_t)((tg >> 8) & 0xFFu) << 16) |
                             ((uint64_t)(tg & 0xFFu) << 24) | ((uint64_t)CC_EVSRC_COMMIT << 32);
        }
        __syncthreads();
        // the pass's 3 * cnt words, contiguous in the arena from event base + e0
        const uint64_t w0 = (base + e0) * 3;
        uint64_t* const out = reinterpret_cast<uint64_t*>(arena) + w0;
        const uint32_t nw = cnt * 3, head = (uint32_t)(w0 & 1);
        if (head && t == 0) out[0] = stage[0];
        const uint32_t pairs = (nw - head) >> 1;
        for (uint32_t p = t; p < pairs; p += kFT) {
          const uint32_t x = head + 2 * p;
          *reinterpret_cast<u64x2*>(out + x) = u64x2{stage[x], stage[x + 1]};
        }
        if (((nw - head) & 1u) && t == 0) out[nw - 1] = stage[nw - 1];
        __syncthreads();
      }
    }
    __syncthreads();  // (pre / the record planes are rewritten by the next chunk)
  }
}

int launch_topic_fanout(const FanoutArgs& a, hipStream_t st) {
  const uint64_t chunks = (a.arena_cap + kFT - 1) / kFT;
  const uint32_t grid = (uint32_t)(chunks < (uint64_t)kFanMaxGrid ? (chunks ? chunks : 1) : (uint64_t)kFanMaxGrid);
  a.mark(K_TOPIC_FANOUT, 1, st);
  hipLaunchKernelGGL(k_topic_fanout, dim3(grid), dim3(kFT), 0, st, a.fx, a.arena, a.arena_n, a.arena_cap, a.err);
  a.mark(K_TOPIC_FANOUT, 0, st);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace cc
