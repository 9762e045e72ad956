// host_path.hip — the host-memory entry points of the C-ABI (host code only).
//
// A JVM host (Panama FFM / JNI) hands the engine Java heap or off-heap host memory, not HBM
// pointers.  These calls stage host columns into engine-owned device buffers (grown on demand and kept between
// calls: no hipMalloc / hipFree per batch), run the device entry point, and copy results AND events back, so every
// reference path that publishes -- Session.publish -> InstanceEvent{instance, msg}
// (manager/src/main/java/io/atomix/manager/ManagedResourceSession.java:64-71,
//  manager/src/main/java/io/atomix/resource/InstanceEvent.java:29-80) -- has a host-memory route:
//   cc_apply_batch_host / cc_apply_batch_host_events   ResourceManager.operateResource per entry (:56-72)
//   cc_sessions_close_host / cc_sessions_expire_host    ResourceManager.close / expire (:237-264)
//   cc_advance_time_events_host                         timer callbacks (ResourceManagerStateMachineExecutor :104-116)
//   cc_retained_bitmap_host                             the compaction feed (ResourceManagerCommit.clean :79-81)
// plus a plain device-memory API (cc_device_alloc / cc_memcpy ...) for the stateless device calls
// (cc_quorum_commit, cc_expire_sweep) and for hosts that keep columns resident.
#include <algorithm>
#include <cstring>
#include <functional>
#include <string>

#include <unordered_map>

#include "engine_state.h"

namespace {

enum HwSlot : int {
  kHwCol = 0,  // 9 input columns
  kHwStatus = 9,
  kHwValue,
  kHwEvPos,
  kHwEvTarget,
  kHwEvCode,
  kHwEvSrc,
  kHwEvTag,
  kHwEvPayload,
  kHwEvCount,
  kHwBitmap,
  kHwNum
};
static_assert(kHwNum <= 32, "cc_engine::hw_buf");

// Device buffer `slot` with room for `bytes` (the previous contents are not kept).  The callers are synchronous, so
// no launch of an earlier call still reads a buffer that is replaced here.
int hw(cc_engine* e, int slot, size_t bytes, void** out) {
  bytes = std::max<size_t>(bytes, 256);
  if (e->hw_cap[slot] < bytes) {
    const size_t cap = std::max(bytes, e->hw_cap[slot] * 3 / 2);  // grow by half: no free + malloc per call
    if (e->hw_buf[slot]) (void)hipFree(e->hw_buf[slot]);
    e->hw_buf[slot] = nullptr;
    e->hw_cap[slot] = 0;
    hipError_t x = hipMalloc(&e->hw_buf[slot], cap);
    if (x != hipSuccess) return set_err(CC_ERR_HIP, "hipMalloc (host-path staging)", x);
    e->hw_cap[slot] = cap;
  }
  *out = e->hw_buf[slot];
  return CC_OK;
}

// Device event columns of `cap` rows mirroring the host cc_events `h` (null: no event stream).
int hw_events(cc_engine* e, const cc_events* h, cc_events* d) {
  std::memset(d, 0, sizeof *d);
  if (!h) return CC_OK;
  if (!h->count || (h->capacity && (!h->pos || !h->target || !h->code || !h->src || !h->tag || !h->payload)))
    return set_err(CC_ERR_INVALID, "host event stream: null column or count");
  const size_t c = std::max<uint64_t>(h->capacity, 1);
  int rc;
  void* p;
  if ((rc = hw(e, kHwEvPos, 4 * c, &p))) return rc;
  d->pos = (uint32_t*)p;
  if ((rc = hw(e, kHwEvTarget, 4 * c, &p))) return rc;
  d->target = (uint32_t*)p;
  if ((rc = hw(e, kHwEvCode, c, &p))) return rc;
  d->code = (uint8_t*)p;
  if ((rc = hw(e, kHwEvSrc, c, &p))) return rc;
  d->src = (uint8_t*)p;
  if ((rc = hw(e, kHwEvTag, c, &p))) return rc;
  d->tag = (uint8_t*)p;
  if ((rc = hw(e, kHwEvPayload, 8 * c, &p))) return rc;
  d->payload = (uint64_t*)p;
  if ((rc = hw(e, kHwEvCount, 8, &p))) return rc;
  d->count = (uint64_t*)p;
  d->capacity = h->capacity;
  HIPCHECK(hipMemsetAsync(d->count, 0, sizeof(uint64_t), e->own_stream));
  return CC_OK;
}

// Events back to the host: *h->count = the events published (may exceed capacity: then the call fails with
// CC_ERR_CAPACITY, and the first `capacity` rows are still copied).
int hw_events_back(cc_engine* e, const cc_events* h, const cc_events* d) {
  if (!h) return CC_OK;
  hipStream_t st = e->own_stream;
  uint64_t cnt = 0;
  HIPCHECK(hipMemcpyAsync(&cnt, d->count, sizeof cnt, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  *h->count = cnt;
  const uint64_t m = std::min<uint64_t>(cnt, h->capacity);
  if (m) {
    HIPCHECK(hipMemcpyAsync(h->pos, d->pos, 4 * m, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(h->target, d->target, 4 * m, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(h->code, d->code, m, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(h->src, d->src, m, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(h->tag, d->tag, m, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(h->payload, d->payload, 8 * m, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
  }
  if (cnt <= h->capacity) return CC_OK;
  e->last_err_bits |= kErrEvents;  // (cc_apply_batch_host_prefix: a full event stream, like a full max_events arena)
  return set_err(CC_ERR_CAPACITY, "more events than the host event stream holds");
}

int apply_staged(cc_engine* e, void* const* dcol, uint64_t n, const cc_results* hout, const cc_events* hev, cc_events& dev);

int apply_host(cc_engine* e, const cc_batch* h, uint64_t n, const cc_results* hout, const cc_events* hev) {
  if (!e || !h || !hout || (n && (!hout->status || !hout->value))) return set_err(CC_ERR_INVALID, "null argument");
  HIPCHECK(hipSetDevice(e->device));
  e->last_err_bits = 0;
  hipStream_t st = e->own_stream;
  if (st != e->last_stream) HIPCHECK(hipStreamSynchronize(e->last_stream));
  e->last_stream = st;
  cc_events dev{};
  int rc = hw_events(e, hev, &dev);
  if (rc) return rc;
  if (n == 0) {
    if (hev) *hev->count = 0;
    return CC_OK;
  }
  const void* src[9] = {h->index, h->time, h->inst, h->op, h->flags, h->key, h->a, h->b, h->aux};
  const size_t esz[9] = {8, 8, 4, 1, 1, 8, 8, 8, 8};
  void* dcol[9] = {};
  for (int c = 0; c < 9; ++c) {
    if (!src[c]) continue;
    if ((rc = hw(e, kHwCol + c, esz[c] * n, &dcol[c]))) return rc;
    HIPCHECK(hipMemcpyAsync(dcol[c], src[c], esz[c] * n, hipMemcpyHostToDevice, st));
  }
  return apply_staged(e, dcol, n, hout, hev, dev);
}

// the rest of apply_host, on staged device columns (also cc_apply_wire_host's, whose columns the GPU decoder wrote)
int apply_staged(cc_engine* e, void* const* dcol, uint64_t n, const cc_results* hout, const cc_events* hev, cc_events& dev) {
  hipStream_t st = e->own_stream;
  int rc;
  void *d_status, *d_value;
  if ((rc = hw(e, kHwStatus, n, &d_status)) || (rc = hw(e, kHwValue, 8 * n, &d_value))) return rc;
  // sentinel prefill: status 0xFF is no legal status (tag nibble 15), so a row the kernels never wrote comes back as
  // 0xFF instead of passing for a legal NULL result (status 0, value 0)
  HIPCHECK(hipMemsetAsync(d_status, 0xFF, n, st));
  HIPCHECK(hipMemsetAsync(d_value, 0xA5, 8 * n, st));
  cc_batch d{};
  d.index = (const uint64_t*)dcol[0];
  d.time = (const uint64_t*)dcol[1];
  d.inst = (const uint32_t*)dcol[2];
  d.op = (const uint8_t*)dcol[3];
  d.flags = (const uint8_t*)dcol[4];
  d.key = (const uint64_t*)dcol[5];
  d.a = (const uint64_t*)dcol[6];
  d.b = (const uint64_t*)dcol[7];
  d.aux = (const uint64_t*)dcol[8];
  cc_results r{(uint8_t*)d_status, (uint64_t*)d_value};
  rc = cc_apply_batch(e, &d, n, &r, hev ? &dev : nullptr, st);
  if (rc) {
    (void)hipStreamSynchronize(st);
    return rc;
  }
  HIPCHECK(hipMemcpyAsync(hout->status, d_status, n, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipMemcpyAsync(hout->value, d_value, 8 * n, hipMemcpyDeviceToHost, st));
  const int rs = cc_sync(e);  // device-side checks (capacity, unsupported ops, time order) after the D2H
  const int re = hw_events_back(e, hev, &dev);
  return rs ? rs : re;
}

}  // namespace

// The log segment itself: decoded on the GPU into the staging columns (wire_gpu.hip), rows before the first manager
// entry applied.
extern "C" int cc_apply_wire_host(cc_engine* e, const cc_wire_codec* codec, cc_wire_interner* in, const uint8_t* h_buf,
                                  uint64_t buf_len, const uint64_t* h_offsets, uint64_t n, const uint64_t* h_index,
                                  const uint64_t* h_time, const cc_results* hout, const cc_events* hev,
                                  uint64_t* h_applied, cc_wire_control* ctl) {
  if (!e || !hout || !h_applied || !ctl || (n && (!hout->status || !hout->value || !h_index)))
    return set_err(CC_ERR_INVALID, "null argument");
  *h_applied = 0;
  HIPCHECK(hipSetDevice(e->device));
  e->last_err_bits = 0;
  hipStream_t st = e->own_stream;
  if (st != e->last_stream) HIPCHECK(hipStreamSynchronize(e->last_stream));
  e->last_stream = st;
  const size_t esz[9] = {8, 8, 4, 1, 1, 8, 8, 8, 8};
  void* dcol[9] = {};
  uint64_t r = 0;
  if (n) {
    for (int c = 0; c < 9; ++c)
      if (c != 1 || h_time) TRY(hw(e, kHwCol + c, esz[c] * n, &dcol[c]));
    const cc_batch_out cols{nullptr, nullptr, (uint32_t*)dcol[2], (uint8_t*)dcol[3], (uint8_t*)dcol[4],
                            (uint64_t*)dcol[5], (uint64_t*)dcol[6], (uint64_t*)dcol[7], (uint64_t*)dcol[8]};
    uint64_t nctl = 0;
    TRY(wire_to_device(e, codec, in, h_buf, buf_len, h_offsets, n, &cols, nullptr, ctl, 1, &nctl, nullptr, st, nullptr,
                       true, &r));
    if (r) HIPCHECK(hipMemcpyAsync(dcol[0], h_index, 8 * r, hipMemcpyHostToDevice, st));
    if (r && h_time) HIPCHECK(hipMemcpyAsync(dcol[1], h_time, 8 * r, hipMemcpyHostToDevice, st));
  }
  cc_events dev{};
  TRY(hw_events(e, hev, &dev));
  if (r == 0) {
    if (hev) *hev->count = 0;
    return CC_OK;
  }
  TRY(apply_staged(e, dcol, r, hout, hev, dev));
  *h_applied = r;
  return CC_OK;
}

extern "C" int cc_apply_batch_host(cc_engine* e, const cc_batch* h_cols, uint64_t n, const cc_results* h_out) {
  return apply_host(e, h_cols, n, h_out, nullptr);
}

extern "C" int cc_apply_batch_host_events(cc_engine* e, const cc_batch* h_cols, uint64_t n, const cc_results* h_out,
                                          const cc_events* h_events) {
  if (!h_events) return set_err(CC_ERR_INVALID, "null event stream (use cc_apply_batch_host)");
  return apply_host(e, h_cols, n, h_out, h_events);
}

// ---- a batch applied up to the first commit the engine cannot hold (ABI 5) ------------------------------------------
// Java's collections are unbounded (LockState's ArrayDeque, LeaderElectionState's LinkedHashMap, MembershipGroupState's
// HashMap, QueueState, AtomicValueState's listeners: LockState.java:35, ...); the engine's coordination blocks hold
// coord_cap entries.  cc_apply_batch fails such a batch after applying it (CC_ERR_CAPACITY).  This call instead applies
// exactly the rows before the first commit that would overflow a collection and reports them: *applied = that row
// (n when every row applied), the state is the one after rows [0, *applied), and the row itself and every row after
// it are not applied (their results are not written), so the host can act (a larger engine from a snapshot, or the
// commit failed) and resume at that row.
//   1. Rows that can add an entry (lock with a timeout != 0, election listen, group join, value listen, queue
//      add / offer, topic listen, bus join / register) are the only ones that can overflow.  Every resource they address starts with its block's entry
//      count (one strided copy of the block headers), and one pass over the batch keeps an upper bound per resource
//      (+1 per adding row; removals are not counted, so it never falls short).  The rows before the first adding
//      row whose bound would pass coord_cap go as one call.
//   2. At that row the resource's count is read again (after the rows before it: the bound's slack is gone); if the
//      row fits, the pass goes on.  Else the row goes alone: if the device reports a full collection (kErrCoordFull,
//      and nothing else), its resource block, the clock, the applied index and the pending group timers are restored
//      (the engine skips the entry it cannot hold, so nothing else moved) and the call stops there; if it applied
//      (the op did not add after all), the count is read once more and the pass goes on.
// Each row is scanned once, and the collection scan itself costs one header read per stop: a queue that stays near
// coord_cap under churn costs a call per stop, not a rescan of the batch.  On an engine with maps or with an event
// stream every part (the single row of step 2 included) also runs under a device checkpoint (ckpt_save, engine.hip:
// a device-to-device copy of every snapshot section into a second allocation of that size, kept until the engine is
// destroyed), taken whether or not the part then succeeds; a full map table region or a full event stream costs
// about log2(rows of the part) restores and re-applies on top of it (`attempt` below).
//
// cc_apply_batch_prefix (ABI 6) is the same call on device-resident columns: the control flow (prefix_flow) is shared,
// and what differs -- how a part is applied, how the caller's result rows are kept and put back, and how the next stop
// is found -- is a PrefixPath.  Its scan runs on the device (prefix_scan.hip): 5 B per row (13 B on lock rows) in one
// streaming pass plus one thread per resource slot and one 4-byte read back; a non-empty list costs a second streaming
// pass that ranks the listed resources' rows.  The scan starts from exact block counts, so unlike the host's it is run
// again on the rest of the batch after every stop: one rescan per stop at streaming speed, which a queue held at
// coord_cap under churn pays once per add (the host path pays one header read there).
namespace {

struct PrefixPath {
  uint64_t ev_n = 0;  // events of the rows applied so far
  virtual ~PrefixPath() = default;
  // rows [lo, hi) applied: their results written, their events appended with rows as batch positions (ev_n moves by
  // the part's events, whether or not they fit)
  virtual int apply(uint64_t lo, uint64_t hi) = 0;
  // the caller's result rows [lo, hi) kept aside; rows [from, hi) of the kept ones put back
  virtual int save(uint64_t lo, uint64_t hi) = 0;
  virtual int putback(uint64_t from, uint64_t hi) = 0;
  // rows [0, pos) are applied: the first row from pos on whose resource's bound would pass coord_cap (n: none)
  virtual int next_stop(uint64_t pos, uint64_t* stop) = 0;
  virtual int row_res(uint64_t row, uint32_t* r) = 0;  // the resource slot a row addresses (kNoRes: none)
  virtual void counted(uint32_t, uint32_t) {}          // a block's exact count, read with the rows before applied
  virtual int finish() = 0;                            // the event count, to where the caller reads it
};

// apply host rows [lo, hi) appending to the host event stream `hev` (rows shifted to batch positions); *ev_n = events
// so far
int apply_part(cc_engine* e, const cc_batch* h, uint64_t lo, uint64_t hi, const cc_results* hout, const cc_events* hev,
               uint64_t* ev_n) {
  auto sh = [lo](const auto* p) { return p ? p + lo : p; };
  const cc_batch part{sh(h->index), sh(h->time), sh(h->inst), sh(h->op), sh(h->flags), sh(h->key), sh(h->a), sh(h->b),
                      sh(h->aux)};
  const cc_results o{hout->status + lo, hout->value + lo};
  if (!hev) return apply_host(e, &part, hi - lo, &o, nullptr);
  uint64_t cnt = 0;
  cc_events v = *hev;
  const uint64_t k = std::min(*ev_n, hev->capacity);
  v.pos += k, v.target += k, v.code += k, v.src += k, v.tag += k, v.payload += k;
  v.capacity -= k;
  v.count = &cnt;
  const int rc = apply_host(e, &part, hi - lo, &o, &v);
  for (uint64_t i = 0; i < std::min(cnt, v.capacity); ++i) v.pos[i] += (uint32_t)lo;
  *ev_n += cnt;
  return rc;
}

// The control flow of both prefix applies.  `ck`: the parts run under a device checkpoint (an engine with maps, or a
// call with an event stream).
int prefix_flow(cc_engine* e, uint64_t n, bool ck, PrefixPath& p, uint64_t* h_applied) {
  *h_applied = 0;
  auto finish = [&](int rc) {
    const int rf = p.finish();
    return rc ? rc : rf;
  };
  if (ck && n) {  // (a call that cannot have its checkpoint fails here, before any row is applied)
    const int rc = ckpt_reserve(e);
    if (rc) return finish(rc);
  }
  // Rows [lo, hi) as one part.  On an engine with maps or with an event stream, a part may also fail on a full map
  // table region or a full event stream (kErrCapacity / kErrEvents, and nothing else): the state before the part is a
  // device checkpoint (ckpt_save), and the longest prefix of the part that applies is found by bisection (restore, apply
  // [lo, mid)); the state is then the one after that prefix, its results and events written, the rows after it keep
  // what the caller had there.  *done = the first row not applied (hi on success).
  auto cap_only = [&](int rc) {
    const uint32_t b = e->last_err_bits;
    return rc == CC_ERR_CAPACITY && b && !(b & ~(kErrCapacity | kErrEvents));
  };
  auto attempt = [&](uint64_t lo, uint64_t hi, uint64_t* done) -> int {
    *done = lo;
    if (!ck) {
      const int rc = p.apply(lo, hi);
      if (!rc) *done = hi;
      return rc;
    }
    int rc = p.save(lo, hi);  // (the caller's rows, for the rows not applied)
    if (rc) return rc;
    const uint64_t ev0 = p.ev_n;
    if ((rc = ckpt_save(e))) return rc;
    rc = p.apply(lo, hi);
    if (!rc) {
      *done = hi;
      return CC_OK;
    }
    if (!cap_only(rc)) return rc;
    uint64_t good = lo, bad = hi;  // [lo, good) applies, [lo, bad) does not
    bool at_good = false;          // the engine's state is the one after [lo, good)
    while (bad - good > 1) {
      const uint64_t mid = good + (bad - good) / 2;
      if ((rc = ckpt_restore(e))) return rc;
      p.ev_n = ev0;
      rc = p.apply(lo, mid);
      if (!rc) {
        good = mid;
        at_good = true;
      } else if (cap_only(rc)) {
        bad = mid;
        at_good = false;
      } else {
        return rc;
      }
    }
    if (!at_good) {
      if ((rc = ckpt_restore(e))) return rc;
      p.ev_n = ev0;
      if (good > lo && (rc = p.apply(lo, good))) return rc;
    }
    if ((rc = p.putback(good, hi))) return rc;
    *done = good;
    return CC_ERR_CAPACITY;
  };
  auto full = [&](uint64_t row) {
    *h_applied = row;
    return finish(set_err(CC_ERR_CAPACITY, "a map table region or the event stream is full: *applied rows were applied"));
  };
  if (!e->coord_on) {  // no coordination collection to overflow: one part
    uint64_t done = 0;
    const int rc = n ? attempt(0, n, &done) : CC_OK;
    if (rc == CC_ERR_CAPACITY && done < n) return full(done);
    if (!rc) *h_applied = n;
    return finish(rc);
  }
  const uint32_t cap = e->coord_cap;
  const size_t blk = coord_block(cap);
  auto entries = [&](uint32_t r, uint32_t* out) -> int {  // one block's current entry count (CoordHdr.n)
    CoordHdr hd{};
    HIPCHECK(hipMemcpy(&hd, e->d_coord + (uint64_t)r * blk, sizeof hd, hipMemcpyDeviceToHost));
    *out = coord_used(e->res_type[r], hd.n, hd.head, cap);  // (a bus: members + registrations, common.h)
    return CC_OK;
  };
  uint64_t pos = 0;  // rows [0, pos) applied
  while (pos < n) {
    uint64_t stop = n;  // the first row whose bound would pass coord_cap
    {
      const int rc = p.next_stop(pos, &stop);
      if (rc) return finish(rc);
    }
    if (stop > pos) {
      uint64_t done = pos;
      const int rc = attempt(pos, stop, &done);
      if (rc == CC_ERR_CAPACITY && done < stop) return full(done);
      if (rc) return finish(rc);
      pos = stop;
      *h_applied = pos;
      if (pos == n) break;
    }
    // row pos (= stop) may overflow: its resource's count now (rows before it applied)
    uint32_t r = kNoRes, cur = 0;
    {
      int rc = p.row_res(pos, &r);
      if (!rc && r == kNoRes)
        rc = set_err(CC_ERR_STATE, "internal check: the stop row of a prefix apply addresses no resource");
      if (!rc) rc = entries(r, &cur);
      if (rc) return finish(rc);
    }
    if ((uint64_t)cur + 1 <= cap) {  // it fits: the pass goes on from this row with the exact count
      p.counted(r, cur);
      continue;
    }
    // row pos alone: its resource's block, the clock, the applied index and the group timers are saved first
    std::vector<uint8_t> saved(blk);
    uint64_t clock = 0, last = 0;
    HIPCHECK(hipMemcpy(saved.data(), e->d_coord + (uint64_t)r * blk, blk, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(&clock, e->d_clock, sizeof clock, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(&last, e->d_last_index, sizeof last, hipMemcpyDeviceToHost));
    const bool pending = e->applied_pending;
    const uint64_t applied0 = e->applied;
    const auto gtimers = e->gtimers;
    const uint64_t ev0 = p.ev_n;
    if (!ck) {  // (under a checkpoint the attempt keeps the row itself)
      const int rc = p.save(pos, pos + 1);
      if (rc) return finish(rc);
    }
    uint64_t done1 = pos;
    const int rc = attempt(pos, pos + 1, &done1);
    if (rc == CC_ERR_CAPACITY && e->last_err_bits != kErrCoordFull) return full(pos);
    // (only a full coordination collection, and nothing else, is rolled back: any other failure is returned as is)
    if (rc == CC_ERR_CAPACITY && e->last_err_bits == kErrCoordFull) {
      // (the row is not applied: its result row keeps what the caller had there)
      const int rp = p.putback(pos, pos + 1);
      if (rp) return finish(rp);
      HIPCHECK(hipMemcpy(e->d_coord + (uint64_t)r * blk, saved.data(), blk, hipMemcpyHostToDevice));
      HIPCHECK(hipMemcpy(e->d_clock, &clock, sizeof clock, hipMemcpyHostToDevice));
      HIPCHECK(hipMemcpy(e->d_last_index, &last, sizeof last, hipMemcpyHostToDevice));
      e->applied_pending = pending;
      e->applied = applied0;
      e->gtimers = gtimers;
      p.ev_n = ev0;
      return finish(set_err(CC_ERR_CAPACITY, "a coordination collection is full (coord_cap): *applied rows were applied"));
    }
    if (rc) return finish(rc);
    pos += 1;
    *h_applied = pos;
    {
      const int rc2 = entries(r, &cur);
      if (rc2) return finish(rc2);
    }
    p.counted(r, cur);
  }
  return finish(CC_OK);
}

// ---- host columns: staged per part by apply_host, results and events in the caller's host memory ---------------------
struct HostPrefix : PrefixPath {
  cc_engine* e;
  const cc_batch* h;
  uint64_t n;
  const cc_results* hout;
  const cc_events* hev;
  std::vector<uint8_t> s0;  // the kept result rows [s_lo, s_lo + size)
  std::vector<uint64_t> v0;
  uint64_t s_lo = 0;
  std::unordered_map<uint32_t, uint64_t> bound;  // per resource: an upper bound of its block's entry count
  bool bounded = false;
  uint64_t i = 0;  // rows before i are scanned (their adds are in the bounds)
  HostPrefix(cc_engine* e_, const cc_batch* h_, uint64_t n_, const cc_results* o_, const cc_events* v_)
      : e(e_), h(h_), n(n_), hout(o_), hev(v_) {}

  int apply(uint64_t lo, uint64_t hi) override { return apply_part(e, h, lo, hi, hout, hev, &ev_n); }
  int save(uint64_t lo, uint64_t hi) override {
    s0.assign(hout->status + lo, hout->status + hi);
    v0.assign(hout->value + lo, hout->value + hi);
    s_lo = lo;
    return CC_OK;
  }
  int putback(uint64_t from, uint64_t hi) override {
    std::copy(s0.begin() + (from - s_lo), s0.begin() + (hi - s_lo), hout->status + from);
    std::copy(v0.begin() + (from - s_lo), v0.begin() + (hi - s_lo), hout->value + from);
    return CC_OK;
  }
  uint32_t res_of(uint64_t row) const {
    const uint32_t in = h->inst[row];
    return in < e->cfg.max_instances ? e->inst_res[in] : kNoRes;
  }
  bool adds(uint64_t row, uint32_t r) const {
    return r != kNoRes && r < e->res_type.size() && adds_entry(e->res_type[r], h->op[row], h->aux ? h->aux[row] : 0);
  }
  // the upper bound of every addressed resource's entry count, from one strided copy of the block headers over the
  // slot range the adding rows address
  int bounds() {
    const size_t blk = coord_block(e->coord_cap);
    uint32_t rlo = ~0u, rhi = 0;
    for (uint64_t k = 0; k < n; ++k) {
      const uint32_t r = res_of(k);
      if (adds(k, r)) rlo = std::min(rlo, r), rhi = std::max(rhi, r);
    }
    if (rlo <= rhi) {
      std::vector<CoordHdr> hdr(rhi - rlo + 1);
      HIPCHECK(hipMemcpy2D(hdr.data(), sizeof(CoordHdr), e->d_coord + (uint64_t)rlo * blk, blk, sizeof(CoordHdr),
                           hdr.size(), hipMemcpyDeviceToHost));
      for (uint64_t k = 0; k < n; ++k) {
        const uint32_t r = res_of(k);
        if (adds(k, r) && !bound.count(r))
          bound[r] = coord_used(e->res_type[r], hdr[r - rlo].n, hdr[r - rlo].head, e->coord_cap);
      }
    }
    bounded = true;
    return CC_OK;
  }
  int next_stop(uint64_t pos, uint64_t* stop) override {
    if (!bounded) {
      const int rc = bounds();
      if (rc) return rc;
    }
    if (i < pos) i = pos;  // (a row applied alone is not scanned again)
    for (; i < n; ++i) {
      const uint32_t r = res_of(i);
      if (!adds(i, r)) continue;
      uint64_t& b = bound[r];
      if (b + 1 > e->coord_cap) break;
      ++b;
    }
    *stop = i;
    return CC_OK;
  }
  int row_res(uint64_t row, uint32_t* r) override {
    *r = res_of(row);
    return CC_OK;
  }
  void counted(uint32_t r, uint32_t cur) override { bound[r] = cur; }
  int finish() override {
    if (hev) *hev->count = ev_n;
    return CC_OK;
  }
};

// ---- device-resident columns (cc_apply_batch_prefix): results and events stay in HBM ---------------------------------
enum PxSlot : int { kHwSaveStatus = kHwNum, kHwSaveValue, kPxSlots };
static_assert(kPxSlots <= 32, "cc_engine::hw_buf");

struct DevicePrefix : PrefixPath {
  cc_engine* e;
  const cc_batch* c;
  uint64_t n;
  const cc_results* out;
  const cc_events* ev;
  void* stream;    // as the caller passed it (cc_apply_batch resolves null itself)
  hipStream_t st;  // the stream every part runs on
  uint64_t s_lo = 0;
  DevicePrefix(cc_engine* e_, const cc_batch* c_, uint64_t n_, const cc_results* o_, const cc_events* v_, void* stream_,
               hipStream_t st_)
      : e(e_), c(c_), n(n_), out(o_), ev(v_), stream(stream_), st(st_) {}

  // A part that starts at a multiple of four rows meets cc_apply_batch's alignment rules in place (inst and value 16
  // bytes, status 4).  Any other part (the rest of a batch after a stop, a stop row alone) runs on copies of its
  // columns in the engine's staging buffers, its results on a copy of the caller's rows that is copied back once it
  // applied.
  int apply(uint64_t lo, uint64_t hi) override {
    const uint64_t m = hi - lo;
    const bool staged = (lo & 3) != 0;
    auto sh = [lo](const auto* p) { return p ? p + lo : p; };
    cc_batch part{sh(c->index), sh(c->time), sh(c->inst), sh(c->op), sh(c->flags), sh(c->key), sh(c->a), sh(c->b),
                  sh(c->aux)};
    cc_results o{out->status + lo, out->value + lo};
    int rc;
    if (staged) {
      const void* src[9] = {part.index, part.time, part.inst, part.op, part.flags, part.key, part.a, part.b, part.aux};
      const size_t esz[9] = {8, 8, 4, 1, 1, 8, 8, 8, 8};
      void* d[9] = {};
      for (int k = 0; k < 9; ++k) {
        if (!src[k]) continue;
        if ((rc = hw(e, kHwCol + k, esz[k] * m, &d[k]))) return rc;
        HIPCHECK(hipMemcpyAsync(d[k], src[k], esz[k] * m, hipMemcpyDeviceToDevice, st));
      }
      part = cc_batch{(const uint64_t*)d[0], (const uint64_t*)d[1], (const uint32_t*)d[2], (const uint8_t*)d[3],
                      (const uint8_t*)d[4],  (const uint64_t*)d[5], (const uint64_t*)d[6], (const uint64_t*)d[7],
                      (const uint64_t*)d[8]};
      void *ds, *dv;
      if ((rc = hw(e, kHwStatus, m, &ds)) || (rc = hw(e, kHwValue, 8 * m, &dv))) return rc;
      HIPCHECK(hipMemcpyAsync(ds, out->status + lo, m, hipMemcpyDeviceToDevice, st));
      HIPCHECK(hipMemcpyAsync(dv, out->value + lo, 8 * m, hipMemcpyDeviceToDevice, st));
      o = cc_results{(uint8_t*)ds, (uint64_t*)dv};
    }
    cc_events v{};
    if (ev) {  // the event columns from the events so far on; the part's own count in an engine word
      v = *ev;
      const uint64_t k = std::min(ev_n, ev->capacity);
      v.pos += k, v.target += k, v.code += k, v.src += k, v.tag += k, v.payload += k;
      v.capacity -= k;
      v.count = e->d_px_evn;
      HIPCHECK(hipMemsetAsync(v.count, 0, sizeof(uint64_t), st));
    }
    e->last_err_bits = 0;
    rc = cc_apply_batch(e, &part, m, &o, ev ? &v : nullptr, stream);
    if (rc) {
      (void)hipStreamSynchronize(st);
      return rc;
    }
    const int rs = cc_sync(e);  // device-side checks (capacity, unsupported ops, time order)
    int re = CC_OK;
    if (ev) {
      uint64_t cnt = 0;
      HIPCHECK(hipMemcpyAsync(&cnt, v.count, sizeof cnt, hipMemcpyDeviceToHost, st));
      HIPCHECK(hipStreamSynchronize(st));
      if (lo && launch_ev_shift(v.pos, std::min(cnt, v.capacity), (uint32_t)lo, st))
        return set_err(CC_ERR_HIP, "event row shift launch", hipGetLastError());
      ev_n += cnt;
      if (cnt > v.capacity) {
        e->last_err_bits |= kErrEvents;  // (a full event stream, like a full max_events arena)
        if (!rs) re = set_err(CC_ERR_CAPACITY, "more events than the event stream holds");
      }
    }
    if (staged && !rs && !re) {
      HIPCHECK(hipMemcpyAsync(out->status + lo, o.status, m, hipMemcpyDeviceToDevice, st));
      HIPCHECK(hipMemcpyAsync(out->value + lo, o.value, 8 * m, hipMemcpyDeviceToDevice, st));
    }
    HIPCHECK(hipStreamSynchronize(st));
    return rs ? rs : re;
  }
  int save(uint64_t lo, uint64_t hi) override {
    void *ds, *dv;
    int rc;
    if ((rc = hw(e, kHwSaveStatus, hi - lo, &ds)) || (rc = hw(e, kHwSaveValue, 8 * (hi - lo), &dv))) return rc;
    HIPCHECK(hipMemcpyAsync(ds, out->status + lo, hi - lo, hipMemcpyDeviceToDevice, st));
    HIPCHECK(hipMemcpyAsync(dv, out->value + lo, 8 * (hi - lo), hipMemcpyDeviceToDevice, st));
    s_lo = lo;
    return CC_OK;
  }
  int putback(uint64_t from, uint64_t hi) override {
    if (hi > from) {
      HIPCHECK(hipMemcpyAsync(out->status + from, (const uint8_t*)e->hw_buf[kHwSaveStatus] + (from - s_lo), hi - from,
                              hipMemcpyDeviceToDevice, st));
      HIPCHECK(hipMemcpyAsync(out->value + from, (const uint64_t*)e->hw_buf[kHwSaveValue] + (from - s_lo),
                              8 * (hi - from), hipMemcpyDeviceToDevice, st));
    }
    HIPCHECK(hipStreamSynchronize(st));
    return CC_OK;
  }
  // the scan's buffers: control words (list length, earliest target chunk, stop row), then cnt / list_res /
  // list_room [slots] and tblk / tbase [kPxGroup]
  int scan_args(uint64_t lo, PxArgs* a) {
    const uint32_t slots = (uint32_t)e->sb << kSbShift;
    if (!e->d_px) HIPCHECK(hipMalloc(&e->d_px, sizeof(uint32_t) * (4 + 3ull * slots + 2 * kPxGroup)));
    a->inst = c->inst, a->op = c->op, a->aux = c->aux;
    a->lo = lo, a->hi = n;
    a->inst_res = e->d_inst_res, a->res_type = e->d_res_type;
    a->max_inst = e->cfg.max_instances, a->slots = slots;
    a->coord = e->d_coord, a->coord_cap = e->coord_cap;
    a->list_n = e->d_px;
    a->min_tb = e->d_px + 1;
    a->stop = (unsigned long long*)(e->d_px + 2);
    a->cnt = e->d_px + 4;
    a->list_res = a->cnt + slots;
    a->list_room = a->list_res + slots;
    a->tblk = a->list_room + slots;
    a->tbase = a->tblk + kPxGroup;
    a->bcnt = e->d_px_bcnt;
    return CC_OK;
  }
  int next_stop(uint64_t pos, uint64_t* stop) override {
    PxArgs a{};
    int rc = scan_args(pos, &a);
    if (rc) return rc;
    if (launch_px_count(a, st)) return set_err(CC_ERR_HIP, "prefix scan launch", hipGetLastError());
    uint32_t listed = 0;
    HIPCHECK(hipMemcpyAsync(&listed, a.list_n, sizeof listed, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    *stop = n;
    if (!listed) return CC_OK;  // (the normal case: no resource's bound passes coord_cap in [pos, n))
    // the rank pass: [pos, n) in at most kPxMaxBlocks chunks of whole tiles, kPxGroup listed resources at a time
    const uint64_t len = n - pos, tiles = (len + kPxBlock - 1) / kPxBlock;
    const uint64_t chunk = (tiles + kPxMaxBlocks - 1) / kPxMaxBlocks * kPxBlock;
    const uint32_t nblk = (uint32_t)((len + chunk - 1) / chunk);
    const uint64_t need = (uint64_t)nblk * std::min(listed, kPxGroup);
    if (need > e->px_bcnt_cap) {
      if (e->d_px_bcnt) HIPCHECK(hipFree(e->d_px_bcnt));
      e->d_px_bcnt = nullptr;
      e->px_bcnt_cap = 0;
      HIPCHECK(hipMalloc(&e->d_px_bcnt, sizeof(uint32_t) * need));
      e->px_bcnt_cap = need;
    }
    a.bcnt = e->d_px_bcnt;
    for (uint32_t g0 = 0; g0 < listed; g0 += kPxGroup)
      if (launch_px_rank(a, g0, std::min(listed - g0, kPxGroup), nblk, chunk, st))
        return set_err(CC_ERR_HIP, "prefix rank launch", hipGetLastError());
    unsigned long long row = ~0ull;
    HIPCHECK(hipMemcpyAsync(&row, a.stop, sizeof row, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    if (row < pos || row >= n)
      return set_err(CC_ERR_STATE, "internal check: the prefix scan listed a resource but ranked no stop row");
    *stop = row;
    return CC_OK;
  }
  int row_res(uint64_t row, uint32_t* r) override {
    uint32_t in = 0;
    HIPCHECK(hipMemcpyAsync(&in, c->inst + row, sizeof in, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    *r = in < e->cfg.max_instances ? e->inst_res[in] : kNoRes;
    return CC_OK;
  }
  int finish() override {
    if (!ev) return CC_OK;
    HIPCHECK(hipMemcpyAsync(ev->count, &ev_n, sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIPCHECK(hipStreamSynchronize(st));  // (ev_n is a member of a local)
    return CC_OK;
  }
};

}  // namespace

extern "C" int cc_apply_batch_host_prefix(cc_engine* e, const cc_batch* h, uint64_t n, const cc_results* hout,
                                          const cc_events* hev, uint64_t* h_applied) {
  if (!e || !h || !hout || !h_applied || (n && (!h->inst || !h->op))) return set_err(CC_ERR_INVALID, "null argument");
  if (hev && (!hev->count || (hev->capacity && (!hev->pos || !hev->target || !hev->code || !hev->src || !hev->tag ||
                                                !hev->payload))))
    return set_err(CC_ERR_INVALID, "host event stream: null column or count");
  *h_applied = 0;
  HIPCHECK(hipSetDevice(e->device));
  HostPrefix p(e, h, n, hout, hev);
  return prefix_flow(e, n, e->map_bits != 0 || hev != nullptr, p, h_applied);
}

extern "C" int cc_apply_batch_prefix(cc_engine* e, const cc_batch* c, uint64_t n, const cc_results* out,
                                     const cc_events* ev, void* stream, uint64_t* h_applied) {
  if (!e || !c || !out || !h_applied) return set_err(CC_ERR_INVALID, "null argument");
  if (ev && (!ev->pos || !ev->target || !ev->code || !ev->src || !ev->tag || !ev->payload || !ev->count))
    return set_err(CC_ERR_INVALID, "event stream columns and count are required");
  *h_applied = 0;
  HIPCHECK(hipSetDevice(e->device));
  hipStream_t st = stream ? (hipStream_t)stream : e->own_stream;
  if (n == 0) {
    if (ev) {
      HIPCHECK(hipMemsetAsync(ev->count, 0, sizeof(uint64_t), st));
      HIPCHECK(hipStreamSynchronize(st));
    }
    return CC_OK;
  }
  // cc_apply_batch's own argument rules, checked before the scan reads a column or a checkpoint is taken
  if (n > e->cfg.max_batch) return set_err(CC_ERR_CAPACITY, "batch larger than max_batch");
  if (!c->inst || !c->op || !c->flags || !c->a || !c->b || !out->status || !out->value)
    return set_err(CC_ERR_INVALID, "inst/op/flags/a/b columns and status/value outputs are required");
  if ((((uintptr_t)out->status) & 3) || (((uintptr_t)out->value) & 15) || (((uintptr_t)c->inst) & 15))
    return set_err(CC_ERR_INVALID, "inst and value must be 16-byte aligned, status 4-byte aligned");
  if (st != e->last_stream) HIPCHECK(hipStreamSynchronize(e->last_stream));
  e->last_stream = st;
  if (!e->coord_on && !e->map_bits && !ev) {  // nothing here can fill: the plain call and the final sync
    int rc = cc_apply_batch(e, c, n, out, nullptr, stream);
    if (rc) {
      (void)hipStreamSynchronize(st);
      return rc;
    }
    if (!(rc = cc_sync(e))) *h_applied = n;
    return rc;
  }
  int rc = quiesce(e);  // (queued registry writes: the scan reads the device registry)
  if (rc) return rc;
  if (ev && !e->d_px_evn) HIPCHECK(hipMalloc(&e->d_px_evn, sizeof(uint64_t)));
  DevicePrefix p(e, c, n, out, ev, stream, st);
  return prefix_flow(e, n, e->map_bits != 0 || ev != nullptr, p, h_applied);
}

// ---- packed host batches (pack.cpp, unpack.hip) -----------------------------------------------------------------------
// The decoder on its own (cc_unpack_to_device) and what the packed apply pipeline below shares with it.
namespace {

enum PkSlot : int { kHwBlob0 = kPxSlots, kHwBlob1, kHwStatus1, kHwValue1, kPkSlots };
static_assert(kPkSlots <= 32, "cc_engine::hw_buf");
constexpr uint32_t kPkNeed = 4 | 8 | 16 | 64 | 128;  // inst, op, flags, a, b: the columns cc_apply_batch requires
constexpr size_t kPkEsz[9] = {8, 8, 4, 1, 1, 8, 8, 8, 8};

int pk_init(cc_engine* e) {
  if (!e->pk_in) HIPCHECK(hipStreamCreateWithFlags(&e->pk_in, hipStreamNonBlocking));
  if (!e->pk_out) {
    // The copy-out stream is created at the highest stream priority: the runtime maps a process's streams onto a few
    // hardware queues per priority level (4 by default), and at equal priority the two copy streams landed on one
    // queue, which ran H2D and D2H one after the other (measured: the call took the SUM of the two directions).
    int least = 0, greatest = 0;
    HIPCHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIPCHECK(hipStreamCreateWithPriority(&e->pk_out, hipStreamNonBlocking, greatest));
  }
  for (hipEvent_t* ev : {&e->pk_landed[0], &e->pk_landed[1], &e->pk_drained[0], &e->pk_drained[1]})
    if (!*ev) HIPCHECK(hipEventCreateWithFlags(ev, hipEventDisableTiming));
  return CC_OK;
}

int host_events_ok(const cc_events* h) {
  if (h && (!h->count || (h->capacity && (!h->pos || !h->target || !h->code || !h->src || !h->tag || !h->payload))))
    return set_err(CC_ERR_INVALID, "host event stream: null column or count");
  return CC_OK;
}

UnpackArgs unpack_args(const void* d_dir, const void* d_data, uint64_t data_base, void* const* col, uint32_t present) {
  UnpackArgs a{};
  a.dir = (const cc_pack_block*)d_dir;
  a.data = (const uint8_t*)d_data;
  a.data_base = data_base;
  a.index = (uint64_t*)col[0], a.time = (uint64_t*)col[1], a.inst = (uint32_t*)col[2], a.op = (uint8_t*)col[3];
  a.flags = (uint8_t*)col[4], a.key = (uint64_t*)col[5], a.a = (uint64_t*)col[6], a.b = (uint64_t*)col[7];
  a.aux = (uint64_t*)col[8];
  a.present = present;
  return a;
}

}  // namespace

extern "C" int cc_unpack_to_device(cc_engine* e, const void* h_blob, uint64_t bytes, const cc_batch_out* d_cols,
                                   void* stream) {
  if (!e || !d_cols) return set_err(CC_ERR_INVALID, "null argument");
  uint64_t n = 0;
  uint32_t present = 0;
  TRY(cc_pack_check(h_blob, bytes, &n, &present));  // (a malformed blob never reaches the GPU)
  if (n == 0) return CC_OK;
  void* const col[9] = {d_cols->index, d_cols->time, d_cols->inst, d_cols->op, d_cols->flags,
                        d_cols->key,   d_cols->a,    d_cols->b,    d_cols->aux};
  for (int c = 0; c < 9; ++c)
    if (((present >> c) & 1) && (!col[c] || ((uintptr_t)col[c] & 15)))
      return set_err(CC_ERR_INVALID, "unpack: a present column's device pointer is null or not 16-byte aligned");
  HIPCHECK(hipSetDevice(e->device));
  const cc_pack_header* hd = (const cc_pack_header*)h_blob;
  if (hd->blocks > 0x7FFFFFFFull) return set_err(CC_ERR_CAPACITY, "unpack: more than 2^31 blocks");
  void* d = nullptr;
  TRY(hw(e, kHwBlob0, hd->bytes, &d));
  hipStream_t st = (hipStream_t)stream;
  HIPCHECK(hipMemcpyAsync(d, h_blob, hd->bytes, hipMemcpyHostToDevice, st));
  if (launch_unpack(unpack_args((const uint8_t*)d + sizeof *hd, d, 0, col, present), (uint32_t)hd->blocks, st))
    return set_err(CC_ERR_HIP, "unpack launch", hipGetLastError());
  return CC_OK;
}

// ---- packed result blobs (respack.cpp, respack.hip) -------------------------------------------------------------------
// The encoder (three launches, respack.hip) turns wide result rows into directory entries and data areas in a device
// staging: {total word (16 B) | directory entries | data areas}.  The encoder's total is copied into a pinned host word
// on the same stream, so the host reads it after the synchronisation it makes anyway.
namespace {

enum RpSlot : int { kHwRes0 = kPkSlots, kHwRes1, kRpSlots };
static_assert(kRpSlots <= 32, "cc_engine::hw_buf");
constexpr uint64_t kRpHead = 16;  // the staging's first bytes: the encoder's total word

uint64_t rp_blocks(uint64_t n) { return (n + CC_PACK_BLOCK_ROWS - 1) / CC_PACK_BLOCK_ROWS; }

// rows [0, m) of d_status / d_value encoded into staging `slot` on `st`, the data areas placed from blob offset
// `data_base` on; the total then travels into the pinned word on `st` too.  *stage = the staging.
int rp_encode(cc_engine* e, int slot, const void* d_status, const void* d_value, uint64_t m, uint64_t data_base,
              hipStream_t st, uint8_t** stage) {
  if (!e->rp_pin) HIPCHECK(hipHostMalloc((void**)&e->rp_pin, 16, hipHostMallocDefault));
  const uint64_t db = rp_blocks(m) * sizeof(cc_respack_block);
  void* p = nullptr;
  TRY(hw(e, slot, kRpHead + db + 9 * m + 32, &p));  // (every column raw; the tail block's two paddings)
  RespackArgs a{};
  a.status = (const uint8_t*)d_status, a.value = (const uint64_t*)d_value, a.n = m;
  a.dir = (cc_respack_block*)((uint8_t*)p + kRpHead);
  a.data = (uint8_t*)p + kRpHead + db;
  a.data_base = data_base;
  a.total = (unsigned long long*)p;
  if (launch_respack(a, st)) return set_err(CC_ERR_HIP, "result blob encode launch", hipGetLastError());
  HIPCHECK(hipMemcpyAsync(e->rp_pin, p, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  *stage = (uint8_t*)p;
  return CC_OK;
}

// the header of a result blob or of an event blob of n rows and `bytes` bytes: they differ in magic, version and columns
enum BlobKind { kResultBlob, kEventBlob };

void blob_header(BlobKind kind, void* h_blob, uint64_t n, uint64_t bytes) {
  cc_pack_header hd{};
  hd.magic = kind == kResultBlob ? (uint32_t)CC_RESPACK_MAGIC : (uint32_t)CC_EVPACK_MAGIC;
  hd.version = kind == kResultBlob ? CC_RESPACK_VERSION : CC_EVPACK_VERSION;
  hd.n = n;
  hd.blocks = rp_blocks(n);
  hd.bytes = bytes;
  hd.present = kind == kResultBlob ? 3 : 0x3F;
  hd.block_rows = CC_PACK_BLOCK_ROWS;
  std::memcpy(h_blob, &hd, sizeof hd);
}

}  // namespace

extern "C" int cc_respack_from_device(cc_engine* e, const cc_results* d_results, uint64_t n, void* h_blob, uint64_t cap,
                                      uint64_t* bytes, void* stream) {
  if (!e || !d_results || !bytes || !h_blob) return set_err(CC_ERR_INVALID, "result blob: null argument");
  if ((uintptr_t)h_blob & 15) return set_err(CC_ERR_INVALID, "result blob: the blob must be 16-byte aligned");
  uint64_t bound = 0;
  TRY(cc_respack_bound(n, &bound));
  if (cap < bound) {
    *bytes = bound;
    return set_err(CC_ERR_CAPACITY, "result blob: the blob buffer is smaller than cc_respack_bound (*bytes = the bound)");
  }
  if (n == 0) {
    blob_header(kResultBlob, h_blob, 0, sizeof(cc_pack_header));
    *bytes = sizeof(cc_pack_header);
    return CC_OK;
  }
  if (!d_results->status || !d_results->value || (((uintptr_t)d_results->status | (uintptr_t)d_results->value) & 15))
    return set_err(CC_ERR_INVALID, "result blob: status and value device pointers must be non-null and 16-byte aligned");
  if (rp_blocks(n) > 0x7FFFFFFFull) return set_err(CC_ERR_CAPACITY, "result blob: more than 2^31 blocks");
  HIPCHECK(hipSetDevice(e->device));
  hipStream_t st = (hipStream_t)stream;
  const uint64_t db = rp_blocks(n) * sizeof(cc_respack_block);
  uint8_t* stage = nullptr;
  TRY(rp_encode(e, kHwRes0, d_results->status, d_results->value, n, sizeof(cc_pack_header) + db, st, &stage));
  HIPCHECK(hipStreamSynchronize(st));
  const uint64_t total = *e->rp_pin;
  if (total > 9 * n + 32) return set_err(CC_ERR_STATE, "internal check: the result blob encoder wrote past its bound");
  // directory and data are adjacent in the staging as they are in the blob: one copy
  HIPCHECK(hipMemcpyAsync((uint8_t*)h_blob + sizeof(cc_pack_header), stage + kRpHead, db + total, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  *bytes = sizeof(cc_pack_header) + db + total;
  blob_header(kResultBlob, h_blob, n, *bytes);
  return CC_OK;
}

// ---- packed event blobs (evpack.cpp, evpack.hip) ----------------------------------------------------------------------
// Device event columns (the caller's, or the engine-owned ones the packed apply pipeline accumulates a call's events
// in) encoded into one staging and sent in one D2H.
namespace {

enum EpSlot : int { kHwEvAcc = kRpSlots, kHwEvStage, kEpSlots };
static_assert(kEpSlots <= 32, "cc_engine::hw_buf");
constexpr uint64_t kEpHead = 16;  // the first bytes of both buffers: the count word / the encoder's total word

uint64_t ep_r16(uint64_t x) { return (x + 15) & ~15ull; }

// engine-owned device event columns of `cap` events, each 16-byte aligned, in one allocation behind the count word
int ep_columns(cc_engine* e, uint64_t cap, cc_events* d) {
  const uint64_t c = std::max<uint64_t>(cap, 1);
  void* p = nullptr;
  TRY(hw(e, kHwEvAcc, kEpHead + ep_r16(8 * c) + 2 * ep_r16(4 * c) + 3 * ep_r16(c), &p));
  uint8_t* q = (uint8_t*)p;
  d->count = (uint64_t*)q, q += kEpHead;
  d->payload = (uint64_t*)q, q += ep_r16(8 * c);
  d->pos = (uint32_t*)q, q += ep_r16(4 * c);
  d->target = (uint32_t*)q, q += ep_r16(4 * c);
  d->code = q, q += ep_r16(c);
  d->src = q, q += ep_r16(c);
  d->tag = q;
  d->capacity = cap;
  return CC_OK;
}

int ep_pin(cc_engine* e) {
  if (!e->ep_pin) HIPCHECK(hipHostMalloc((void**)&e->ep_pin, 16, hipHostMallocDefault));
  return CC_OK;
}

// the first m events of the device columns `d` (each 16-byte aligned) as an event blob in h_blob: encoded in the
// engine's staging on `st`, then header + directory + the data bytes used copied out.  Synchronous.  stamp: four HIP
// events (encode begin / end, D2H begin / end) or null.
int ep_encode(cc_engine* e, const cc_events* d, uint64_t m, void* h_blob, hipStream_t st, uint64_t* bytes,
              const hipEvent_t* stamp) {
  auto mark = [&](int i) { return stamp ? hipEventRecord(stamp[i], st) : hipSuccess; };
  const uint64_t db = rp_blocks(m) * sizeof(cc_evpack_block);
  *bytes = sizeof(cc_pack_header);
  HIPCHECK(mark(0));
  uint8_t* p = nullptr;
  if (m) {
    if (rp_blocks(m) > 0x7FFFFFFFull) return set_err(CC_ERR_CAPACITY, "event blob: more than 2^31 blocks");
    TRY(ep_pin(e));
    void* v = nullptr;
    TRY(hw(e, kHwEvStage, kEpHead + db + 19 * m + 96, &v));  // (every column raw; the tail block's six paddings)
    p = (uint8_t*)v;
    EvpackArgs a{};
    a.pos = d->pos, a.target = d->target, a.code = d->code, a.src = d->src, a.tag = d->tag, a.payload = d->payload;
    a.n = m;
    a.dir = (cc_evpack_block*)(p + kEpHead);
    a.data = p + kEpHead + db;
    a.data_base = sizeof(cc_pack_header) + db;
    a.total = (unsigned long long*)p;
    if (launch_evpack(a, st)) return set_err(CC_ERR_HIP, "event blob encode launch", hipGetLastError());
    HIPCHECK(hipMemcpyAsync(e->ep_pin + 1, p, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  }
  HIPCHECK(mark(1));
  HIPCHECK(hipStreamSynchronize(st));
  HIPCHECK(mark(2));
  if (m) {
    const uint64_t total = e->ep_pin[1];
    if (total > 19 * m + 96) return set_err(CC_ERR_STATE, "internal check: the event blob encoder wrote past its bound");
    // directory and data are adjacent in the staging as they are in the blob: one copy
    HIPCHECK(hipMemcpyAsync((uint8_t*)h_blob + sizeof(cc_pack_header), p + kEpHead, db + total, hipMemcpyDeviceToHost, st));
    *bytes += db + total;
  }
  HIPCHECK(mark(3));
  HIPCHECK(hipStreamSynchronize(st));
  blob_header(kEventBlob, h_blob, m, *bytes);
  return CC_OK;
}

}  // namespace

extern "C" int cc_evpack_from_device(cc_engine* e, const cc_events* d, void* h_blob, uint64_t cap_bytes, uint64_t* bytes,
                                     uint64_t* count, void* stream) {
  if (!e || !d || !bytes || !h_blob || !d->count) return set_err(CC_ERR_INVALID, "event blob: null argument");
  if ((uintptr_t)h_blob & 15) return set_err(CC_ERR_INVALID, "event blob: the blob must be 16-byte aligned");
  uint64_t bound = 0;
  TRY(cc_evpack_bound(d->capacity, &bound));
  if (cap_bytes < bound) {
    *bytes = bound;
    return set_err(CC_ERR_CAPACITY, "event blob: the blob buffer is smaller than cc_evpack_bound (*bytes = the bound)");
  }
  HIPCHECK(hipSetDevice(e->device));
  hipStream_t st = (hipStream_t)stream;
  uint64_t cnt = 0;
  HIPCHECK(hipMemcpyAsync(&cnt, d->count, sizeof cnt, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));  // (the stream is drained: the columns and the count are final)
  if (count) *count = cnt;
  const uint64_t m = std::min(cnt, d->capacity);
  if (m && (!d->pos || !d->target || !d->code || !d->src || !d->tag || !d->payload ||
            (((uintptr_t)d->pos | (uintptr_t)d->target | (uintptr_t)d->code | (uintptr_t)d->src | (uintptr_t)d->tag |
              (uintptr_t)d->payload) & 15)))
    return set_err(CC_ERR_INVALID, "event blob: the six device columns must be non-null and 16-byte aligned");
  TRY(ep_encode(e, d, m, h_blob, st, bytes, nullptr));
  if (cnt > d->capacity) return set_err(CC_ERR_CAPACITY, "more events than the event stream holds");
  return CC_OK;
}

// ---- the packed apply pipeline -------------------------------------------------------------------------------------------
// cc_apply_batch_host_packed, cc_apply_batch_host_packed_results, cc_apply_batch_host_packed_events and
// cc_apply_wire_host_packed are one chunked, three-stream pipeline of a PCIe-inclusive step inside the library
// (pk_run); each entry point checks its own arguments, says where the rows come from (PkSource) and where results and
// events go (PkSink), and runs it:
//
//   copy-in  (pk_in)      | H2D 0 | H2D 1 |        H2D 2        |
//   engine   (own_stream)         | dec 0 + apply 0 [+ enc 0] | dec 1 + apply 1 [+ enc 1] | ... [| ev enc | ev D2H |]
//   copy-out (pk_out)                                         | D2H 0 |                   | D2H 1 |
//
// A chunk is a run of whole blocks; its piece of the blob (its directory entries, then its blocks' data areas, which
// are contiguous because offsets ascend with the block number) goes into one of two piece buffers.  The H2D of chunk
// k + 1 is enqueued BEFORE cc_apply_batch of chunk k is called: on an engine with maps that call syncs the host, and
// the copy must already be in flight.  Decode and apply share the engine's stream, so one decoded column set is
// enough.  The host waits for each chunk's device-side checks (cc_sync) before it applies the next one: that is what
// "stop at the first failing chunk" costs, one round trip per chunk of up to 16 Mi rows.  On an engine with maps or
// with an event sink every chunk runs under a device checkpoint (as the parts of cc_apply_batch_host_prefix): a chunk
// that fails on a full event stream or map table region, and on nothing else, is rolled back and copied out nowhere;
// a chunk that fails for any other reason stays applied and its rows are copied out before the call returns.
//
// Where the rows come from is a PkSource (below): the packed column blob of the three calls above (BlobSource), or a
// wire segment (WireSource, cc_apply_wire_host_packed), whose chunk is its entry bytes, its offsets and its piece of the
// aux blob (index / time), decoded by k_wire_decode after the offsets check on the device; a wire chunk may end the
// call (a manager entry: the rows before it are applied; a row that fails to decode or an offsets violation: the
// chunk is not applied).
//
// What the sinks change:
//
//   results  wide    two wide result sets (k & 1), each copied out straight into the caller's rows [lo, hi) while the
//                    next chunk is applied; set s is prefilled again only after its copy-out of chunk k - 2.
//                    Timeline: 8 stamps per chunk (H2D, decode, apply, D2H).
//            blob    one wide set, which never leaves HBM: the encoder (rp_encode) writes the chunk's directory entries
//                    and data areas into one of two stagings (k & 1) once that staging's copy-out of chunk k - 2 is
//                    done.  Chunk k's areas are placed from the blob offset where chunk k - 1's ended, which the host
//                    knows after chunk k - 1's cc_sync.  The copy-out sends the directory entries and the data bytes
//                    used, and only those, to their places in the caller's blob; the host writes the header last.
//                    Timeline: 10 stamps per chunk (H2D, decode, apply, encode, D2H).
//   events   none    nothing published (a publishing op fails the chunk); a checkpoint only on an engine with maps.
//            host    the chunk's events go to staging columns and from there, after the chunk's checks, to the caller's
//                    columns behind the events so far (hw_events / hw_events_back); pos is shifted to batch rows on
//                    the host.
//            device  the chunk's events are appended to engine-owned device columns behind those of the chunks before,
//                    the count comes back in a pinned word with the chunk's checks, and pos is shifted by a kernel once
//                    the chunk is kept.  The blob is encoded once, after the last chunk, and leaves in one D2H: its
//                    directory's length, and with it the offset of every data area, is known only with the last
//                    chunk's count (the result blob knows its row count up front).
namespace {

enum PkResults { kResWide, kResBlob };
enum PkEvents { kEvNone, kEvHost, kEvDevice };

// where a call's results and events go; the fields of the sinks not in use stay null
struct PkSink {
  PkResults results;
  PkEvents events;
  // kResWide: the caller's rows
  const cc_results* hout;
  // kResBlob: the caller's blob, with room for cc_respack_bound(n) bytes, and where its size goes
  uint8_t* res;
  uint64_t* res_bytes;
  // kEvHost: the caller's columns and count
  const cc_events* hev;
  // kEvDevice: the caller's blob, with room for cc_evpack_bound(ev_capacity) bytes, where its size goes, and where the
  // events published go (the failing chunk's included, as kEvHost's count)
  void* ev_blob;
  uint64_t ev_capacity;
  uint64_t* ev_bytes;
  uint64_t* ev_count;
  // CC_PACKED_TIMELINE: the stamps of the last call of this kind, and its chunks whose stamps are all recorded (each
  // kind of call keeps its own, so its timeline call reports the last call of its kind)
  std::vector<hipEvent_t>* stamp;
  uint64_t* chunks;
};

void ev_advance(cc_events* v, uint64_t used) {
  v->pos += used, v->target += used, v->code += used, v->src += used, v->tag += used, v->payload += used;
  v->capacity -= used;
}

int more_stamps(std::vector<hipEvent_t>* v, uint64_t want) {
  while (v->size() < want) {
    hipEvent_t ev;
    HIPCHECK(hipEventCreate(&ev));
    v->push_back(ev);
  }
  return CC_OK;
}

// the rows of a chunk: whole blocks within the caller's chunk_rows (0: 16 Mi), max_batch and one extended sub-batch (an
// engine smaller than a block takes a block: a batch larger than max_batch then fails as it does in cc_apply_batch)
uint64_t pk_chunk_rows(const cc_engine* e, const cc_packed_opts* opts) {
  const uint64_t kB = CC_PACK_BLOCK_ROWS;
  uint64_t chunk = opts && opts->chunk_rows ? opts->chunk_rows : (16ull << 20);
  chunk = std::min<uint64_t>(chunk, 1ull << 40);
  chunk = (chunk + kB - 1) / kB * kB;
  const uint64_t cap_rows = std::max<uint64_t>(std::min(e->cfg.max_batch, e->sub_ext) / kB * kB, kB);
  return std::min(chunk, cap_rows);
}

// Where a call's rows come from.  The pipeline asks a source for its cuts (whole blocks), has it put chunk k's input in
// flight on the copy-in stream, and later, on the engine stream, has it leave chunk k's wide columns in the kHwCol
// staging and say how many of the chunk's rows may be applied.
struct PkSource {
  // set by pk_run: record stamp `which` of chunk k on a stream (a no-op without CC_PACKED_TIMELINE)
  std::function<hipError_t(uint64_t, uint64_t, hipStream_t)> stamp;
  virtual ~PkSource() = default;
  virtual uint64_t chunks() const = 0;
  virtual uint64_t cut(uint64_t k) const = 0;  // the first row of chunk k; cut(chunks()) = n
  virtual uint32_t present() const = 0;        // the wide columns it leaves
  // chunk k's input on its way (stamps 0 and 1 around it, pk_landed[k & 1] behind it)
  virtual int send(uint64_t k) = 0;
  // The engine stream has waited for pk_landed[k & 1].  col: the staging columns of the chunk's rows.  *apply: rows
  // [cut(k), cut(k) + *apply) are to be applied; *end: the call ends with this chunk, returning *end_rc (which, when
  // not CC_OK, comes with *apply = 0: a chunk that fails in the source is not applied).
  virtual int unpack(uint64_t k, void* const* col, uint64_t* apply, bool* end, int* end_rc) = 0;
};

// A checked cc_pack blob sent piecewise: the piece of the blocks of rows [lo, hi) is their directory entries, then
// their data areas (contiguous, because offsets ascend with the block number), in one of two piece buffers.
struct BlobPieces {
  cc_engine* e;
  const uint8_t* blob;
  const cc_pack_header* hd;
  const cc_pack_block* dir;
  void* piece[2] = {};
  uint64_t piece_base[2] = {}, piece_dir[2] = {};
  BlobPieces(cc_engine* e_, const void* h_blob)
      : e(e_), blob((const uint8_t*)h_blob), hd((const cc_pack_header*)h_blob),
        dir((const cc_pack_block*)((const uint8_t*)h_blob + sizeof(cc_pack_header))) {}
  int send(uint64_t k, uint64_t row_lo, uint64_t row_hi) {
    const uint64_t kB = CC_PACK_BLOCK_ROWS;
    const uint64_t b0 = row_lo / kB, b1 = std::min(hd->blocks, (row_hi + kB - 1) / kB);
    const uint64_t lo = dir[b0].offset, hi = dir[b1 - 1].offset + dir[b1 - 1].bytes, db = (b1 - b0) * sizeof(cc_pack_block);
    void* p = nullptr;
    TRY(hw(e, kHwBlob0 + (int)(k & 1), db + (hi - lo), &p));
    HIPCHECK(hipMemcpyAsync(p, dir + b0, db, hipMemcpyHostToDevice, e->pk_in));
    if (hi > lo) HIPCHECK(hipMemcpyAsync((uint8_t*)p + db, blob + lo, hi - lo, hipMemcpyHostToDevice, e->pk_in));
    piece[k & 1] = p, piece_base[k & 1] = lo, piece_dir[k & 1] = db;
    return CC_OK;
  }
  int unpack(uint64_t k, uint64_t rows, void* const* col, uint32_t present) {
    const int s = (int)(k & 1);
    if (launch_unpack(unpack_args(piece[s], (const uint8_t*)piece[s] + piece_dir[s], piece_base[s], col, present),
                      (uint32_t)((rows + CC_PACK_BLOCK_ROWS - 1) / CC_PACK_BLOCK_ROWS), e->own_stream))
      return set_err(CC_ERR_HIP, "unpack launch", hipGetLastError());
    return CC_OK;
  }
};

// rows [0, n) of a checked blob (n > 0, its columns `present`) in chunks of `chunk` rows
struct BlobSource : PkSource {
  BlobPieces pieces;
  uint64_t n, chunk;
  uint32_t cols;
  BlobSource(cc_engine* e, const void* h_blob, uint64_t n_, uint32_t present_, uint64_t chunk_)
      : pieces(e, h_blob), n(n_), chunk(chunk_), cols(present_) {}
  uint64_t chunks() const override { return (n + chunk - 1) / chunk; }
  uint64_t cut(uint64_t k) const override { return std::min(n, k * chunk); }
  uint32_t present() const override { return cols; }
  int send(uint64_t k) override {
    cc_engine* e = pieces.e;
    HIPCHECK(stamp(k, 0, e->pk_in));
    TRY(pieces.send(k, cut(k), cut(k + 1)));
    HIPCHECK(stamp(k, 1, e->pk_in));
    HIPCHECK(hipEventRecord(e->pk_landed[k & 1], e->pk_in));
    return CC_OK;
  }
  int unpack(uint64_t k, void* const* col, uint64_t* apply, bool* end, int* end_rc) override {
    *apply = cut(k + 1) - cut(k), *end = false, *end_rc = CC_OK;
    return pieces.unpack(k, *apply, col, cols);
  }
};

// A wire segment (cc_apply_wire_host_packed): the entries' bytes and offsets decoded on the GPU (wire_gpu.hip
// wire_chunk_decode), index / time from the packed aux blob.  The cuts are the planner's (wire.cpp wire_plan_chunks):
// whole blocks, at most the pipeline's chunk rows, shortened until a chunk's entry bytes are at most kWireChunkBytes
// (1 GiB; a single block may exceed it).  Chunk k's staging (k & 1) holds its offsets, then (16-byte aligned) its bytes.
enum WsSlot : int { kHwWire0 = kEpSlots, kHwWire1, kWsSlots };
static_assert(kWsSlots <= 32, "cc_engine::hw_buf");

struct WireSource : PkSource {
  cc_engine* e;
  const cc_wire_codec* codec;
  cc_wire_interner* in;
  const cc_wire_segment* seg;
  BlobPieces aux;
  uint32_t aux_present;
  std::vector<WireChunk> plan;
  void* stage[2] = {};
  cc_wire_control* ctl;
  uint64_t* bad_row;
  WireSource(cc_engine* e_, const cc_wire_codec* codec_, cc_wire_interner* in_, const cc_wire_segment* seg_,
             uint32_t aux_present_, uint64_t chunk, cc_wire_control* ctl_, uint64_t* bad_row_)
      : e(e_), codec(codec_), in(in_), seg(seg_), aux(e_, seg_->aux_blob), aux_present(aux_present_), ctl(ctl_),
        bad_row(bad_row_) {
    wire_plan_chunks(seg->offsets, seg->n, seg->buf_len, chunk, kWireChunkBytes, &plan);
  }
  uint64_t chunks() const override { return plan.size(); }
  uint64_t cut(uint64_t k) const override { return k < plan.size() ? plan[k].lo : seg->n; }
  uint32_t present() const override { return aux_present | 0x1FC; }
  static uint64_t off_bytes(uint64_t rows) { return (8 * (rows + 1) + 15) & ~15ull; }
  int send(uint64_t k) override {
    const WireChunk& c = plan[k];
    const uint64_t* off = seg->offsets + c.lo;
    const uint64_t span = off[c.send] - off[0];  // (the ends hold, or the planner's scan passed rows [lo, lo + send))
    void* p = nullptr;
    TRY(hw(e, kHwWire0 + (int)(k & 1), off_bytes(c.send) + ((span + 15) & ~15ull) + 16, &p));
    stage[k & 1] = p;
    HIPCHECK(stamp(k, 0, e->pk_in));
    HIPCHECK(hipMemcpyAsync(p, off, 8 * (c.send + 1), hipMemcpyHostToDevice, e->pk_in));
    if (span) HIPCHECK(hipMemcpyAsync((uint8_t*)p + off_bytes(c.send), seg->buf + off[0], span, hipMemcpyHostToDevice, e->pk_in));
    TRY(aux.send(k, c.lo, c.hi));
    HIPCHECK(stamp(k, 1, e->pk_in));
    HIPCHECK(hipEventRecord(e->pk_landed[k & 1], e->pk_in));
    return CC_OK;
  }
  int unpack(uint64_t k, void* const* col, uint64_t* apply, bool* end, int* end_rc) override {
    const WireChunk& c = plan[k];
    TRY(aux.unpack(k, c.hi - c.lo, col, aux_present));
    const cc_batch_out cols{nullptr, nullptr, (uint32_t*)col[2], (uint8_t*)col[3], (uint8_t*)col[4],
                            (uint64_t*)col[5], (uint64_t*)col[6], (uint64_t*)col[7], (uint64_t*)col[8]};
    WireChunkIn w{codec, in, seg->buf, seg->buf_len, seg->offsets, c, stage[k & 1],
                  (uint8_t*)stage[k & 1] + off_bytes(c.send), &cols};
    return wire_chunk_decode(e, w, e->own_stream, apply, end, end_rc, ctl, bad_row);
  }
};

// rows [0, n) of a source (n > 0) applied chunk by chunk
int pk_run(cc_engine* e, PkSource& src, uint64_t n, const cc_packed_opts* opts, const PkSink& o, uint64_t* h_rows_done) {
  const bool res_blob = o.results == kResBlob, ev_host = o.events == kEvHost, ev_dev = o.events == kEvDevice;
  e->last_err_bits = 0;
  hipStream_t st = e->own_stream;
  if (st != e->last_stream) HIPCHECK(hipStreamSynchronize(e->last_stream));
  e->last_stream = st;
  TRY(pk_init(e));
  if (ev_dev) TRY(ep_pin(e));

  const uint64_t kB = CC_PACK_BLOCK_ROWS;
  const uint64_t nchunks = src.chunks();
  const uint32_t present = src.present();
  const bool ck = e->map_bits != 0 || o.events != kEvNone;  // as the parts of cc_apply_batch_host_prefix
  if (ck) TRY(ckpt_reserve(e));
  const bool stamps = opts && (opts->flags & CC_PACKED_TIMELINE);
  const uint64_t per = res_blob ? 10 : 8;  // stamps per chunk; the copy-out's are the last two
  if (stamps) {
    TRY(more_stamps(o.stamp, per * nchunks));
    if (ev_dev) TRY(more_stamps(&e->ep_call_stamp, 4));
  }
  auto stamp = [&](uint64_t k, uint64_t which, hipStream_t s) -> hipError_t {
    return stamps ? hipEventRecord((*o.stamp)[per * k + which], s) : hipSuccess;
  };
  src.stamp = stamp;
  cc_events acc{};  // kEvDevice: the call's events, in HBM
  if (ev_dev) TRY(ep_columns(e, o.ev_capacity, &acc));
  const uint64_t ev_cap = ev_host ? o.hev->capacity : o.ev_capacity;
  auto send = [&](uint64_t k) { return src.send(k); };
  // the result blob keeps the room of all n rows' directory entries; the data areas follow, chunk after chunk
  const uint64_t res_data0 = sizeof(cc_pack_header) + rp_blocks(n) * sizeof(cc_respack_block);
  uint64_t res_rows = 0, res_data = 0;  // rows whose results are on their way out, and their data bytes
  uint64_t ev_n = 0;                    // events of the chunks so far (the failing chunk's included)
  uint64_t ev_kept = 0;                 // events of the chunks fully applied: the event blob's
  // every stream drained before the call returns: a copy in flight reads the caller's blob or writes its results.  The
  // host writes the result blob's header last; the event blob is encoded and sent here
  auto leave = [&](int rc) {
    (void)hipStreamSynchronize(e->pk_in);
    (void)hipStreamSynchronize(e->pk_out);
    if (ev_host) *o.hev->count = ev_n;
    if (ev_dev) *o.ev_count = ev_n;
    if (res_blob) {
      *o.res_bytes = res_rows ? res_data0 + res_data : sizeof(cc_pack_header);
      blob_header(kResultBlob, o.res, res_rows, *o.res_bytes);
    }
    if (!ev_dev) return rc;
    const char* const why = rc ? cc_last_error() : nullptr;
    const std::string kept = why ? why : "";
    const int re = ep_encode(e, &acc, ev_kept, o.ev_blob, st, o.ev_bytes, stamps ? e->ep_call_stamp.data() : nullptr);
    if (re) {  // (the header-only blob the entry point wrote stands)
      *o.ev_bytes = sizeof(cc_pack_header);
      if (rc) (void)set_err(rc, kept.c_str());
    }
    return rc ? rc : re;
  };
  int rc = send(0);
  if (rc) return leave(rc);
  for (uint64_t k = 0; k < nchunks; ++k) {
    const uint64_t lo = src.cut(k), rows = src.cut(k + 1) - lo;
    const int s = (int)(k & 1);
    if (k + 1 < nchunks && (rc = send(k + 1))) return leave(rc);
    // decode: the wide columns of rows [lo, lo + rows)
    void* dcol[9] = {};
    for (int c = 0; c < 9; ++c)
      if (((present >> c) & 1) && (rc = hw(e, kHwCol + c, kPkEsz[c] * rows, &dcol[c]))) return leave(rc);
    const bool set1 = !res_blob && s;  // (only the wide sink has a second wide set)
    void *d_status, *d_value;
    if ((rc = hw(e, set1 ? kHwStatus1 : kHwStatus, rows, &d_status)) ||
        (rc = hw(e, set1 ? kHwValue1 : kHwValue, 8 * rows, &d_value)))
      return leave(rc);
    hipError_t x = hipStreamWaitEvent(st, e->pk_landed[s], 0);
    if (x == hipSuccess) x = stamp(k, 2, st);
    if (x != hipSuccess) return leave(set_err(CC_ERR_HIP, "packed apply: wait for the piece", x));
    // m: the rows of the chunk to apply (all of them, unless the source ends the call inside this chunk)
    uint64_t m = 0;
    bool src_end = false;
    int src_rc = CC_OK;
    if ((rc = src.unpack(k, dcol, &m, &src_end, &src_rc))) {
      (void)hipStreamSynchronize(st);
      return leave(rc);
    }
    if (src_end && (src_rc || m == 0)) return leave(src_rc);
    const uint64_t hi = lo + m;
    x = stamp(k, 3, st);
    // sentinels as in apply_host.  Wide: result set s is prefilled again once its copy-out of chunk k - 2 is done.  Blob:
    // chunk k - 1's encode has read the one set on this stream
    if (x == hipSuccess && !res_blob && k >= 2) x = hipStreamWaitEvent(st, e->pk_drained[s], 0);
    if (x == hipSuccess) x = hipMemsetAsync(d_status, 0xFF, m, st);
    if (x == hipSuccess) x = hipMemsetAsync(d_value, 0xA5, 8 * m, st);
    // the chunk's events are appended behind the events so far, in the device columns or in the host stream
    const uint64_t used = std::min(ev_n, ev_cap);
    uint64_t cnt = 0;
    cc_events v{}, dev{};
    if (ev_dev) {
      dev = acc;
      ev_advance(&dev, used);
      if (x == hipSuccess) x = hipMemsetAsync(dev.count, 0, sizeof(uint64_t), st);
    }
    if (x != hipSuccess) return leave(set_err(CC_ERR_HIP, "packed apply: result prefill", x));
    if (ev_host) {
      v = *o.hev;
      ev_advance(&v, used);
      v.count = &cnt;
      if ((rc = hw_events(e, &v, &dev))) return leave(rc);
    }
    if (ck && (rc = ckpt_save(e))) return leave(rc);
    const cc_batch d{(const uint64_t*)dcol[0], (const uint64_t*)dcol[1], (const uint32_t*)dcol[2],
                     (const uint8_t*)dcol[3],  (const uint8_t*)dcol[4],  (const uint64_t*)dcol[5],
                     (const uint64_t*)dcol[6], (const uint64_t*)dcol[7], (const uint64_t*)dcol[8]};
    const cc_results r{(uint8_t*)d_status, (uint64_t*)d_value};
    (void)stamp(k, 4, st);
    e->last_err_bits = 0;
    rc = cc_apply_batch(e, &d, m, &r, o.events != kEvNone ? &dev : nullptr, st);
    if (rc) {
      (void)hipStreamSynchronize(st);
      return leave(rc);
    }
    (void)stamp(k, 5, st);
    uint8_t* stage = nullptr;
    if (res_blob) {  // encode into staging s once its copy-out of chunk k - 2 is done; the total comes back with the checks
      if (k >= 2 && (x = hipStreamWaitEvent(st, e->pk_drained[s], 0)) != hipSuccess)
        return leave(set_err(CC_ERR_HIP, "packed apply: wait for the result staging", x));
      (void)stamp(k, 6, st);
      if ((rc = rp_encode(e, kHwRes0 + s, d_status, d_value, m, res_data0 + res_data, st, &stage))) {
        (void)hipStreamSynchronize(st);
        return leave(rc);
      }
      (void)stamp(k, 7, st);
    }
    // (the device columns' count of the chunk comes back with its checks too)
    if (ev_dev && (x = hipMemcpyAsync(e->ep_pin, dev.count, sizeof(uint64_t), hipMemcpyDeviceToHost, st)) != hipSuccess) {
      (void)hipStreamSynchronize(st);
      return leave(set_err(CC_ERR_HIP, "packed apply: event count read-back", x));
    }
    const int rs = cc_sync(e);  // device-side checks (capacity, unsupported ops, time order); the stream is drained
    int re = CC_OK;
    if (ev_host) {
      re = hw_events_back(e, &v, &dev);
      for (uint64_t i = 0; lo && i < std::min(cnt, v.capacity); ++i) v.pos[i] += (uint32_t)lo;
    } else if (ev_dev) {
      cnt = e->ep_pin[0];
      if (cnt > dev.capacity) {
        e->last_err_bits |= kErrEvents;  // (a full event stream, like a full max_events arena)
        re = set_err(CC_ERR_CAPACITY, "more events than the host event stream holds");
      }
    }
    ev_n += cnt;
    rc = rs ? rs : re;
    bool rolled_back = false;
    if (rc == CC_ERR_CAPACITY && ck) {  // a full event stream or map table region, and nothing else: not applied
      const uint32_t bits = e->last_err_bits;
      if (bits && !(bits & ~(kErrCapacity | kErrEvents))) {
        const int rr = ckpt_restore(e);
        if (rr) return leave(rr);
        e->last_err_bits = bits;
        rolled_back = true;
      }
    }
    if (!rolled_back) {  // (a failing chunk that stays applied returns its rows, as cc_apply_batch_host does)
      uint64_t total = 0;
      if (res_blob) {  // the directory entries to their place, the data bytes used behind those of the chunks before
        const uint64_t db = rp_blocks(m) * sizeof(cc_respack_block);
        total = *e->rp_pin;
        if (total > 9 * m + 32)
          return leave(set_err(CC_ERR_STATE, "internal check: the result blob encoder wrote past its bound"));
        x = stamp(k, per - 2, e->pk_out);
        if (x == hipSuccess)
          x = hipMemcpyAsync(o.res + sizeof(cc_pack_header) + (lo / kB) * sizeof(cc_respack_block), stage + kRpHead, db,
                             hipMemcpyDeviceToHost, e->pk_out);
        if (x == hipSuccess && total)
          x = hipMemcpyAsync(o.res + res_data0 + res_data, stage + kRpHead + db, total, hipMemcpyDeviceToHost, e->pk_out);
      } else {
        x = stamp(k, per - 2, e->pk_out);
        if (x == hipSuccess) x = hipMemcpyAsync(o.hout->status + lo, d_status, m, hipMemcpyDeviceToHost, e->pk_out);
        if (x == hipSuccess) x = hipMemcpyAsync(o.hout->value + lo, d_value, 8 * m, hipMemcpyDeviceToHost, e->pk_out);
      }
      if (x == hipSuccess) x = stamp(k, per - 1, e->pk_out);
      if (x == hipSuccess) x = hipEventRecord(e->pk_drained[s], e->pk_out);
      if (x != hipSuccess)
        return leave(set_err(CC_ERR_HIP, res_blob ? "packed apply: result blob copy-out" : "packed apply: result copy-out", x));
      res_rows = hi, res_data += total;
    }
    if (rc) return leave(rc);
    // the chunk is kept: its events in the device columns stay, their rows as batch positions
    if (ev_dev && lo && cnt && launch_ev_shift(dev.pos, cnt, (uint32_t)lo, st))
      return leave(set_err(CC_ERR_HIP, "event row shift launch", hipGetLastError()));
    ev_kept = ev_n;
    if (h_rows_done) *h_rows_done = hi;
    *o.chunks = stamps ? k + 1 : 0;
    if (src_end) break;  // (the source's stop: a manager entry; the rows before it are applied)
  }
  return leave(CC_OK);
}

// the two checks of the caller's result blob buffer that both result-blob calls make (other checks lie between them)
int res_blob_ok(const void* h_res_blob, const uint64_t* res_bytes) {
  if (!h_res_blob || !res_bytes) return set_err(CC_ERR_INVALID, "result blob: null argument");
  if ((uintptr_t)h_res_blob & 15) return set_err(CC_ERR_INVALID, "result blob: the blob must be 16-byte aligned");
  return CC_OK;
}

int res_blob_room(uint64_t n, uint64_t res_cap, uint64_t* res_bytes) {
  uint64_t bound = 0;
  TRY(cc_respack_bound(n, &bound));
  if (res_cap < bound) {
    *res_bytes = bound;
    return set_err(CC_ERR_CAPACITY, "result blob: the blob buffer is smaller than cc_respack_bound (*res_bytes = the bound)");
  }
  return CC_OK;
}

}  // namespace

extern "C" int cc_apply_batch_host_packed(cc_engine* e, const void* h_blob, uint64_t bytes, const cc_results* hout,
                                          const cc_events* hev, const cc_packed_opts* opts, uint64_t* h_rows_done) {
  if (h_rows_done) *h_rows_done = 0;
  if (!e || !hout) return set_err(CC_ERR_INVALID, "null argument");
  if (opts && (opts->flags & ~(uint32_t)CC_PACKED_TIMELINE)) return set_err(CC_ERR_INVALID, "packed apply: unknown flag");
  uint64_t n = 0;
  uint32_t present = 0;
  TRY(cc_pack_check(h_blob, bytes, &n, &present));  // (before anything is copied or launched)
  TRY(host_events_ok(hev));
  if (n && (!hout->status || !hout->value)) return set_err(CC_ERR_INVALID, "null argument");
  HIPCHECK(hipSetDevice(e->device));
  e->pk_chunks = 0;
  if (n == 0) {
    if (hev) *hev->count = 0;
    return CC_OK;
  }
  if ((present & kPkNeed) != kPkNeed)
    return set_err(CC_ERR_INVALID, "inst/op/flags/a/b columns and status/value outputs are required");
  PkSink o{};
  o.results = kResWide, o.hout = hout;
  o.events = hev ? kEvHost : kEvNone, o.hev = hev;
  o.stamp = &e->pk_stamp, o.chunks = &e->pk_chunks;
  BlobSource src(e, h_blob, n, present, pk_chunk_rows(e, opts));
  return pk_run(e, src, n, opts, o, h_rows_done);
}

extern "C" int cc_apply_batch_host_packed_results(cc_engine* e, const void* h_blob, uint64_t bytes, void* h_res_blob,
                                                  uint64_t res_cap, uint64_t* res_bytes, const cc_events* hev,
                                                  const cc_packed_opts* opts, uint64_t* h_rows_done) {
  if (h_rows_done) *h_rows_done = 0;
  if (!e) return set_err(CC_ERR_INVALID, "result blob: null argument");
  TRY(res_blob_ok(h_res_blob, res_bytes));
  if (opts && (opts->flags & ~(uint32_t)CC_PACKED_TIMELINE)) return set_err(CC_ERR_INVALID, "packed apply: unknown flag");
  uint64_t n = 0;
  uint32_t present = 0;
  TRY(cc_pack_check(h_blob, bytes, &n, &present));  // (before anything is copied or launched)
  TRY(host_events_ok(hev));
  TRY(res_blob_room(n, res_cap, res_bytes));
  if (n && (present & kPkNeed) != kPkNeed)
    return set_err(CC_ERR_INVALID, "inst/op/flags/a/b columns and status/value outputs are required");
  // from here on every return leaves a valid blob of the rows copied out so far
  blob_header(kResultBlob, h_res_blob, 0, sizeof(cc_pack_header));
  *res_bytes = sizeof(cc_pack_header);
  HIPCHECK(hipSetDevice(e->device));
  e->rp_chunks = 0;
  if (n == 0) {
    if (hev) *hev->count = 0;
    return CC_OK;
  }
  PkSink o{};
  o.results = kResBlob, o.res = (uint8_t*)h_res_blob, o.res_bytes = res_bytes;
  o.events = hev ? kEvHost : kEvNone, o.hev = hev;
  o.stamp = &e->rp_stamp, o.chunks = &e->rp_chunks;
  BlobSource src(e, h_blob, n, present, pk_chunk_rows(e, opts));
  return pk_run(e, src, n, opts, o, h_rows_done);
}

extern "C" int cc_apply_batch_host_packed_events(cc_engine* e, const void* h_blob, uint64_t bytes, void* h_res_blob,
                                                 uint64_t res_cap, uint64_t* res_bytes, void* h_ev_blob,
                                                 uint64_t ev_capacity, uint64_t ev_cap_bytes, uint64_t* ev_bytes,
                                                 uint64_t* ev_count, const cc_packed_opts* opts, uint64_t* h_rows_done) {
  if (h_rows_done) *h_rows_done = 0;
  if (!e) return set_err(CC_ERR_INVALID, "result blob: null argument");
  TRY(res_blob_ok(h_res_blob, res_bytes));
  if (!h_ev_blob || !ev_bytes || !ev_count) return set_err(CC_ERR_INVALID, "event blob: null argument");
  if ((uintptr_t)h_ev_blob & 15) return set_err(CC_ERR_INVALID, "event blob: the blob must be 16-byte aligned");
  if (opts && (opts->flags & ~(uint32_t)CC_PACKED_TIMELINE)) return set_err(CC_ERR_INVALID, "packed apply: unknown flag");
  uint64_t n = 0;
  uint32_t present = 0;
  TRY(cc_pack_check(h_blob, bytes, &n, &present));  // (before anything is copied or launched)
  TRY(res_blob_room(n, res_cap, res_bytes));
  uint64_t bound = 0;
  TRY(cc_evpack_bound(ev_capacity, &bound));
  if (ev_cap_bytes < bound) {
    *ev_bytes = bound;
    return set_err(CC_ERR_CAPACITY, "event blob: the blob buffer is smaller than cc_evpack_bound (*ev_bytes = the bound)");
  }
  if (n && (present & kPkNeed) != kPkNeed)
    return set_err(CC_ERR_INVALID, "inst/op/flags/a/b columns and status/value outputs are required");
  // from here on every return leaves a valid result blob of the rows copied out so far and a valid event blob
  blob_header(kResultBlob, h_res_blob, 0, sizeof(cc_pack_header));
  *res_bytes = sizeof(cc_pack_header);
  blob_header(kEventBlob, h_ev_blob, 0, sizeof(cc_pack_header));
  *ev_bytes = sizeof(cc_pack_header);
  *ev_count = 0;
  HIPCHECK(hipSetDevice(e->device));
  e->ep_chunks = 0;
  if (n == 0) return CC_OK;
  PkSink o{};
  o.results = kResBlob, o.res = (uint8_t*)h_res_blob, o.res_bytes = res_bytes;
  o.events = kEvDevice, o.ev_blob = h_ev_blob, o.ev_capacity = ev_capacity, o.ev_bytes = ev_bytes, o.ev_count = ev_count;
  o.stamp = &e->ep_stamp, o.chunks = &e->ep_chunks;
  BlobSource src(e, h_blob, n, present, pk_chunk_rows(e, opts));
  return pk_run(e, src, n, opts, o, h_rows_done);
}

// The log segment itself through the pipeline: a wire segment as the source, the result blob and (optionally) the
// event blob as the sinks.
extern "C" int cc_apply_wire_host_packed(cc_engine* e, const cc_wire_codec* codec, cc_wire_interner* in,
                                         const cc_wire_segment* seg, void* h_res_blob, uint64_t res_cap,
                                         uint64_t* res_bytes, void* h_ev_blob, uint64_t ev_capacity, uint64_t ev_cap_bytes,
                                         uint64_t* ev_bytes, uint64_t* ev_count, const cc_packed_opts* opts,
                                         uint64_t* h_rows_done, cc_wire_control* ctl, uint64_t* bad_row) {
  if (h_rows_done) *h_rows_done = 0;
  if (!e) return set_err(CC_ERR_INVALID, "result blob: null argument");
  TRY(res_blob_ok(h_res_blob, res_bytes));
  if (!in || !seg || !h_rows_done || !ctl || (seg->n && (!seg->buf || !seg->offsets || !seg->aux_blob)))
    return set_err(CC_ERR_INVALID, "wire decode: null argument");
  if (h_ev_blob) {
    if (!ev_bytes || !ev_count) return set_err(CC_ERR_INVALID, "event blob: null argument");
    if ((uintptr_t)h_ev_blob & 15) return set_err(CC_ERR_INVALID, "event blob: the blob must be 16-byte aligned");
  }
  if (opts && (opts->flags & ~(uint32_t)CC_PACKED_TIMELINE)) return set_err(CC_ERR_INVALID, "packed apply: unknown flag");
  const uint64_t n = seg->n;
  uint32_t present = 0;
  if (n) {  // index (and time) of the n rows, in the packed format: checked before anything is copied or launched
    uint64_t an = 0;
    TRY(cc_pack_check(seg->aux_blob, seg->aux_bytes, &an, &present));
    if (an != n) return set_err(CC_ERR_INVALID, "wire segment: the aux blob's row count differs from the segment's");
    if (!(present & 1)) return set_err(CC_ERR_INVALID, "wire segment: the aux blob lacks the index column");
    if (present & ~3u) return set_err(CC_ERR_INVALID, "wire segment: the aux blob holds a column other than index / time");
  }
  TRY(res_blob_room(n, res_cap, res_bytes));
  if (h_ev_blob) {
    uint64_t bound = 0;
    TRY(cc_evpack_bound(ev_capacity, &bound));
    if (ev_cap_bytes < bound) {
      *ev_bytes = bound;
      return set_err(CC_ERR_CAPACITY, "event blob: the blob buffer is smaller than cc_evpack_bound (*ev_bytes = the bound)");
    }
  }
  if (codec && (codec->utf8_len_bytes < 1 || codec->utf8_len_bytes > 8))  // (wire_args' check, before anything is copied)
    return set_err(CC_ERR_INVALID, "wire codec: utf8_len_bytes");
  // from here on every return leaves a valid result blob of the rows copied out so far and a valid event blob
  blob_header(kResultBlob, h_res_blob, 0, sizeof(cc_pack_header));
  *res_bytes = sizeof(cc_pack_header);
  if (h_ev_blob) {
    blob_header(kEventBlob, h_ev_blob, 0, sizeof(cc_pack_header));
    *ev_bytes = sizeof(cc_pack_header);
    *ev_count = 0;
  }
  HIPCHECK(hipSetDevice(e->device));
  e->rp_chunks = 0;
  if (n == 0) return CC_OK;
  PkSink o{};
  o.results = kResBlob, o.res = (uint8_t*)h_res_blob, o.res_bytes = res_bytes;
  o.events = h_ev_blob ? kEvDevice : kEvNone;
  o.ev_blob = h_ev_blob, o.ev_capacity = ev_capacity, o.ev_bytes = ev_bytes, o.ev_count = ev_count;
  o.stamp = &e->rp_stamp, o.chunks = &e->rp_chunks;  // (a result-blob call: the result-blob calls' stamps)
  uint64_t scratch_bad = 0;
  WireSource src(e, codec, in, seg, present, pk_chunk_rows(e, opts), ctl, bad_row ? bad_row : &scratch_bad);
  return pk_run(e, src, n, opts, o, h_rows_done);
}

extern "C" int cc_wire_packed_timeline(cc_engine* e, uint64_t cap, uint64_t* chunks, float* h_ms) {
  return cc_packed_results_timeline(e, cap, chunks, h_ms);  // (one stamp store for the engine's result-blob calls)
}

extern "C" int cc_packed_timeline(cc_engine* e, uint64_t cap, uint64_t* chunks, float* h_ms) {
  if (!e || !chunks || (cap && !h_ms)) return set_err(CC_ERR_INVALID, "null argument");
  HIPCHECK(hipSetDevice(e->device));
  *chunks = e->pk_chunks;
  for (uint64_t k = 0; k < std::min(cap, e->pk_chunks); ++k)
    for (int j = 0; j < 4; ++j)
      HIPCHECK(hipEventElapsedTime(h_ms + 4 * k + j, e->pk_stamp[8 * k + 2 * j], e->pk_stamp[8 * k + 2 * j + 1]));
  return CC_OK;
}

extern "C" int cc_packed_results_timeline(cc_engine* e, uint64_t cap, uint64_t* chunks, float* h_ms) {
  if (!e || !chunks || (cap && !h_ms)) return set_err(CC_ERR_INVALID, "null argument");
  HIPCHECK(hipSetDevice(e->device));
  *chunks = e->rp_chunks;
  for (uint64_t k = 0; k < std::min(cap, e->rp_chunks); ++k)
    for (int j = 0; j < 5; ++j)
      HIPCHECK(hipEventElapsedTime(h_ms + 5 * k + j, e->rp_stamp[10 * k + 2 * j], e->rp_stamp[10 * k + 2 * j + 1]));
  return CC_OK;
}

extern "C" int cc_packed_events_timeline(cc_engine* e, uint64_t cap, uint64_t* chunks, float* h_ms) {
  if (!e || !chunks || (cap && !h_ms)) return set_err(CC_ERR_INVALID, "null argument");
  HIPCHECK(hipSetDevice(e->device));
  *chunks = e->ep_chunks;
  float call_ms[2] = {0, 0};
  if (e->ep_chunks)
    for (int j = 0; j < 2; ++j)
      HIPCHECK(hipEventElapsedTime(call_ms + j, e->ep_call_stamp[2 * j], e->ep_call_stamp[2 * j + 1]));
  for (uint64_t k = 0; k < std::min(cap, e->ep_chunks); ++k) {
    for (int j = 0; j < 5; ++j)
      HIPCHECK(hipEventElapsedTime(h_ms + 7 * k + j, e->ep_stamp[10 * k + 2 * j], e->ep_stamp[10 * k + 2 * j + 1]));
    h_ms[7 * k + 5] = call_ms[0], h_ms[7 * k + 6] = call_ms[1];
  }
  return CC_OK;
}

extern "C" int cc_sessions_close_host(cc_engine* e, const uint64_t* h_clients, uint64_t count, const cc_events* h_events,
                                      uint64_t* h_closed) {
  if (!e) return set_err(CC_ERR_INVALID, "null engine");
  HIPCHECK(hipSetDevice(e->device));
  cc_events dev{};
  int rc = hw_events(e, h_events, &dev);
  if (rc) return rc;
  rc = cc_sessions_close(e, h_clients, count, h_events ? &dev : nullptr, e->own_stream, h_closed);
  const int re = hw_events_back(e, h_events, &dev);
  return rc ? rc : re;
}

extern "C" int cc_sessions_expire_host(cc_engine* e, const uint64_t* h_bitmap, uint64_t sessions, const cc_events* h_events,
                                       uint64_t* h_closed) {
  if (!e || (sessions && !h_bitmap)) return set_err(CC_ERR_INVALID, "null argument");
  std::vector<uint64_t> clients;  // ascending client session ids, as cc_sessions_expire orders them
  for (uint64_t wi = 0; wi < (sessions + 63) / 64; ++wi)
    for (uint64_t b = h_bitmap[wi]; b; b &= b - 1) {
      const uint64_t sid = wi * 64 + (uint64_t)__builtin_ctzll(b);
      if (sid < sessions) clients.push_back(sid);
    }
  return cc_sessions_close_host(e, clients.data(), clients.size(), h_events, h_closed);
}

extern "C" int cc_advance_time_events_host(cc_engine* e, uint64_t now, const cc_events* h_events) {
  if (!e) return set_err(CC_ERR_INVALID, "null engine");
  HIPCHECK(hipSetDevice(e->device));
  cc_events dev{};
  int rc = hw_events(e, h_events, &dev);
  if (rc) return rc;
  rc = cc_advance_time_events(e, now, h_events ? &dev : nullptr);
  const int re = hw_events_back(e, h_events, &dev);
  return rc ? rc : re;
}

extern "C" int cc_retained_bitmap_host(cc_engine* e, uint64_t first, uint64_t count, uint64_t* h_bitmap, uint64_t* h_count) {
  if (!e || (count && !h_bitmap)) return set_err(CC_ERR_INVALID, "null argument");
  if (count == 0) {
    if (h_count) *h_count = 0;
    return CC_OK;
  }
  HIPCHECK(hipSetDevice(e->device));
  const uint64_t words = (count + 63) / 64;
  void* d = nullptr;
  int rc = hw(e, kHwBitmap, 8 * words, &d);
  if (rc) return rc;
  if ((rc = cc_retained_bitmap(e, first, count, (uint64_t*)d, h_count))) return rc;
  HIPCHECK(hipMemcpy(h_bitmap, d, 8 * words, hipMemcpyDeviceToHost));
  return CC_OK;
}

// ---- packed blobs both ways on the device (pack_enc.hip, unpack_res.hip) ------------------------------------------------
// For a host that holds a log in HBM and splits it there (cc_split_batch_device): a share leaves as a batch blob
// (cc_pack_from_device), and the ranks' result and event blobs come back as device columns (cc_respack_to_device,
// cc_evpack_to_device) for cc_merge_results_device / cc_merge_events_device.  The encoder's staging is
// {total word (16 B) | directory entries | data areas}, as the result encoder's; the decoders stage the blob where
// cc_unpack_to_device does (kHwBlob0: the engine is synchronised between two such calls anyway).
namespace {

enum ShSlot : int { kHwShare = kWsSlots, kShSlots };
static_assert(kShSlots <= 32, "cc_engine::hw_buf");

// a validated result or event blob copied into the engine's staging on `st`; *d = the device copy
int blob_to_staging(cc_engine* e, const void* h_blob, const cc_pack_header* hd, hipStream_t st, const uint8_t** d) {
  void* p = nullptr;
  TRY(hw(e, kHwBlob0, hd->bytes, &p));
  HIPCHECK(hipMemcpyAsync(p, h_blob, hd->bytes, hipMemcpyHostToDevice, st));
  *d = (const uint8_t*)p;
  return CC_OK;
}

}  // namespace

extern "C" int cc_pack_from_device(cc_engine* e, const cc_batch* d_cols, uint64_t n, void* h_blob, uint64_t cap,
                                   uint64_t* bytes, void* stream) {
  if (!e || !d_cols || !bytes || (cap && !h_blob)) return set_err(CC_ERR_INVALID, "pack from device: null argument");
  if ((uintptr_t)h_blob & 15) return set_err(CC_ERR_INVALID, "pack from device: the blob must be 16-byte aligned");
  const void* const col[9] = {d_cols->index, d_cols->time, d_cols->inst, d_cols->op, d_cols->flags,
                              d_cols->key,   d_cols->a,    d_cols->b,    d_cols->aux};
  uint32_t present = 0;
  for (int c = 0; c < 9; ++c) {
    if ((uintptr_t)col[c] & 15)
      return set_err(CC_ERR_INVALID, "pack from device: a present column's device pointer is not 16-byte aligned");
    if (col[c]) present |= 1u << c;
  }
  uint64_t bound = 0;
  TRY(cc_pack_bound(n, present, &bound));
  if (cap < bound) {
    *bytes = bound;
    return set_err(CC_ERR_CAPACITY, "pack from device: the blob buffer is smaller than cc_pack_bound (*bytes = the bound)");
  }
  cc_pack_header hd{};
  hd.magic = (uint32_t)CC_PACK_MAGIC;
  hd.version = CC_PACK_VERSION;
  hd.n = n;
  hd.blocks = rp_blocks(n);
  hd.bytes = sizeof hd;
  hd.present = present;
  hd.block_rows = CC_PACK_BLOCK_ROWS;
  if (n) {
    if (hd.blocks > 0x7FFFFFFFull) return set_err(CC_ERR_CAPACITY, "pack from device: more than 2^31 blocks");
    HIPCHECK(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)stream;
    if (!e->rp_pin) HIPCHECK(hipHostMalloc((void**)&e->rp_pin, 16, hipHostMallocDefault));
    const uint64_t db = hd.blocks * sizeof(cc_pack_block);
    const uint64_t room = bound - sizeof hd - db;  // every present column raw; the tail block's paddings
    void* p = nullptr;
    TRY(hw(e, kHwShare, kRpHead + db + room, &p));
    PackEncArgs a{};
    for (int c = 0; c < 9; ++c) a.col[c] = col[c];
    a.present = present, a.n = n;
    a.dir = (cc_pack_block*)((uint8_t*)p + kRpHead);
    a.data = (uint8_t*)p + kRpHead + db;
    a.data_base = sizeof hd + db;
    a.total = (unsigned long long*)p;
    if (launch_pack_enc(a, st)) return set_err(CC_ERR_HIP, "batch blob encode launch", hipGetLastError());
    HIPCHECK(hipMemcpyAsync(e->rp_pin, p, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    const uint64_t total = *e->rp_pin;
    if (total > room) return set_err(CC_ERR_STATE, "internal check: the batch blob encoder wrote past its bound");
    // directory and data are adjacent in the staging as they are in the blob: one copy
    HIPCHECK(hipMemcpyAsync((uint8_t*)h_blob + sizeof hd, (uint8_t*)p + kRpHead, db + total, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    hd.bytes += db + total;
  }
  std::memcpy(h_blob, &hd, sizeof hd);
  *bytes = hd.bytes;
  return CC_OK;
}

extern "C" int cc_respack_to_device(cc_engine* e, const void* h_blob, uint64_t bytes, const cc_results* d_out, void* stream) {
  if (!e || !d_out) return set_err(CC_ERR_INVALID, "result blob to device: null argument");
  uint64_t n = 0;
  TRY(cc_respack_check(h_blob, bytes, &n));  // (a malformed blob never reaches the GPU)
  if (n == 0) return CC_OK;
  if (!d_out->status || !d_out->value || (((uintptr_t)d_out->status | (uintptr_t)d_out->value) & 15))
    return set_err(CC_ERR_INVALID, "result blob to device: status and value device pointers must be non-null and 16-byte aligned");
  const cc_pack_header* hd = (const cc_pack_header*)h_blob;
  if (hd->blocks > 0x7FFFFFFFull) return set_err(CC_ERR_CAPACITY, "result blob to device: more than 2^31 blocks");
  HIPCHECK(hipSetDevice(e->device));
  hipStream_t st = (hipStream_t)stream;
  const uint8_t* d = nullptr;
  TRY(blob_to_staging(e, h_blob, hd, st, &d));
  ResUnpackArgs a{};
  a.dir = (const cc_respack_block*)(d + sizeof *hd), a.data = d, a.data_base = 0;
  a.status = d_out->status, a.value = d_out->value;
  if (launch_res_unpack(a, (uint32_t)hd->blocks, st)) return set_err(CC_ERR_HIP, "result blob decode launch", hipGetLastError());
  return CC_OK;
}

extern "C" int cc_evpack_to_device(cc_engine* e, const void* h_blob, uint64_t bytes, const cc_events* d_out, void* stream) {
  if (!e || !d_out || !d_out->count) return set_err(CC_ERR_INVALID, "event blob to device: null argument");
  uint64_t n = 0;
  TRY(cc_evpack_check(h_blob, bytes, &n));  // (a malformed blob never reaches the GPU)
  if (d_out->capacity < n) return set_err(CC_ERR_CAPACITY, "event blob to device: more events than d_out->capacity");
  HIPCHECK(hipSetDevice(e->device));
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {
    HIPCHECK(hipMemsetAsync(d_out->count, 0, sizeof(uint64_t), st));
    return CC_OK;
  }
  if (!d_out->pos || !d_out->target || !d_out->code || !d_out->src || !d_out->tag || !d_out->payload ||
      (((uintptr_t)d_out->pos | (uintptr_t)d_out->target | (uintptr_t)d_out->code | (uintptr_t)d_out->src |
        (uintptr_t)d_out->tag | (uintptr_t)d_out->payload) & 15))
    return set_err(CC_ERR_INVALID, "event blob to device: the six device columns must be non-null and 16-byte aligned");
  const cc_pack_header* hd = (const cc_pack_header*)h_blob;
  if (hd->blocks > 0x7FFFFFFFull) return set_err(CC_ERR_CAPACITY, "event blob to device: more than 2^31 blocks");
  const uint8_t* d = nullptr;
  TRY(blob_to_staging(e, h_blob, hd, st, &d));
  EvUnpackArgs a{};
  a.dir = (const cc_evpack_block*)(d + sizeof *hd), a.data = d, a.data_base = 0;
  a.pos = d_out->pos, a.target = d_out->target, a.code = d_out->code, a.src = d_out->src, a.tag = d_out->tag;
  a.payload = d_out->payload, a.count = d_out->count, a.n = n;
  if (launch_ev_unpack(a, (uint32_t)hd->blocks, st)) return set_err(CC_ERR_HIP, "event blob decode launch", hipGetLastError());
  return CC_OK;
}

// ---- plain device memory (for the stateless device calls and hosts that keep columns resident) ---------------
extern "C" int cc_device_alloc(int device, uint64_t bytes, void** d_out) {
  if (!d_out) return set_err(CC_ERR_INVALID, "null argument");
  *d_out = nullptr;
  HIPCHECK(hipSetDevice(device));
  HIPCHECK(hipMalloc(d_out, std::max<uint64_t>(bytes, 1)));
  return CC_OK;
}

extern "C" int cc_device_free(void* d_ptr) {
  if (d_ptr) HIPCHECK(hipFree(d_ptr));
  return CC_OK;
}

extern "C" int cc_memcpy(void* dst, const void* src, uint64_t bytes, int kind, void* stream) {
  if (bytes == 0) return CC_OK;
  if (!dst || !src) return set_err(CC_ERR_INVALID, "null argument");
  const hipMemcpyKind k = kind == CC_MEMCPY_H2D ? hipMemcpyHostToDevice
                          : kind == CC_MEMCPY_D2H ? hipMemcpyDeviceToHost
                          : kind == CC_MEMCPY_D2D ? hipMemcpyDeviceToDevice
                                                  : hipMemcpyDefault;
  if (kind < CC_MEMCPY_H2D || kind > CC_MEMCPY_D2D) return set_err(CC_ERR_INVALID, "memcpy kind");
  HIPCHECK(hipMemcpyAsync(dst, src, bytes, k, (hipStream_t)stream));
  HIPCHECK(hipStreamSynchronize((hipStream_t)stream));
  return CC_OK;
}

extern "C" int cc_memset(void* d_ptr, int byte, uint64_t bytes, void* stream) {
  if (bytes == 0) return CC_OK;
  if (!d_ptr) return set_err(CC_ERR_INVALID, "null argument");
  HIPCHECK(hipMemsetAsync(d_ptr, byte, bytes, (hipStream_t)stream));
  HIPCHECK(hipStreamSynchronize((hipStream_t)stream));
  return CC_OK;
}
