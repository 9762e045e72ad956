// apply_batch.hip — cc_apply_batch (include/copycat_apply.h): the batched apply driver, as a sequence of named phases
// (list the barrier and in-stream rows; per sub-batch: partition.hip -> apply_*.hip -> answers; barrier rows and group
// timers between the sub-batches), and the map event buffers those phases share with cc_advance_time (ttl_flush).
// Host code only: every kernel is launched through the launch_* entry point of the unit that defines it.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <tuple>
#include <vector>

#include "engine_state.h"
#include "value_group.h"

using namespace cc;

// One form for every launch of the apply path: a failed launch is reported under `what`; with CC_DEBUG_SYNC=1
// (diagnostics) the stream is then drained, so that a kernel's failure is blamed on its own launch.
static const bool g_dbg_sync = getenv("CC_DEBUG_SYNC") != nullptr;
static int launched(int failed, const char* what, hipStream_t st) {
  if (failed) return set_err(CC_ERR_HIP, what, hipGetLastError());
  const hipError_t x = g_dbg_sync ? hipStreamSynchronize(st) : hipSuccess;
  return x == hipSuccess ? CC_OK : set_err(CC_ERR_HIP, (std::string("CC_DEBUG_SYNC after ") + what).c_str(), x);
}
#define DBG_SYNC(what) TRY(launched(0, what, st))  // after a launch that maps its own return codes
#define LAUNCH(call, what) TRY(launched(call, what, st))

// ---- the map event buffers (map_small.hip) and the overlapped small-map replay ----

// The map event buffers, sorted by hipcub: one event per map commit of a sub-batch at most; in TTL mode also one per
// expiry (at most one per commit that sees its key's timer fired, plus one per table entry).
static uint64_t small_cap_needed(const cc_engine* e) {
  return e->ttl_live ? 2 * e->sub_batch + e->map_entries : e->sub_batch;
}
static int alloc_sm_set(const cc_engine* e, cc_engine::SmSet& s, uint64_t cap, const char* what) {
  uint64_t got = 0;
  return regrow({BUF(s.key, 8 * cap), BUF(s.key2, 8 * cap), BUF(s.val, 4 * cap), BUF(s.val2, 4 * cap),
                 BUF(s.pay, sizeof(EvPay) * cap), BUF(s.cseg, 4ull * (e->cfg.max_resources + 2))}, got, cap, what);
}
static int launch_pending_replay(cc_engine* e, hipStream_t st);
static int wait_replay(cc_engine* e, int k, hipStream_t st);
static void free_sm_alt(cc_engine* e) {
  // (inside a batch: a replay not yet launched runs now, and every replay's exit marks fold into the snapshot on the
  // engine stream -- e->last_stream -- before the buffers go)
  if (e->last_stream) {
    (void)launch_pending_replay(e, e->last_stream);
    for (int k = 0; k < 2; ++k) (void)wait_replay(e, k, e->last_stream);
    (void)hipStreamSynchronize(e->last_stream);
  }
  if (e->side_st) (void)hipStreamSynchronize(e->side_st);
  e->rep_pending[0] = e->rep_pending[1] = false;
  e->sm_alt.release();
  e->sm_alt_on = false;
}
static int ensure_small(cc_engine* e) {
  const uint64_t cap = small_cap_needed(e);
  if (e->sm.key && e->sm_cap >= cap) return CC_OK;
  if (cap > 0xFFFFFFFFull) return set_err(CC_ERR_CAPACITY, "map event buffer beyond 2^32 entries");
  // grown (TTL mode): the counters keep their buffer, the events are rebuilt per sub-batch
  if (e->sm.key) free_sm_alt(e);  // (the side stream's replay is done with either set)
  const size_t tb = std::max<size_t>(small_sort_temp_bytes((uint32_t)cap), 256);
  TRY(alloc_sm_set(e, e->sm, cap, "hipMalloc map events"));
  TRY(alloc_once(e->d_sm_seg, 4ull * (e->cfg.max_resources + 1)));
  TRY(regrow({BUF(e->d_sm_temp, tb)}, e->sm_temp_bytes, tb, "hipMalloc map events"));
  e->sm_cap = cap;
  return CC_OK;
}
// the second event-buffer set and the side stream of the overlapped small-map replay (engine_state.h SmSet)
static int ensure_sm_alt(cc_engine* e) {
  if (e->sm_alt_on) return CC_OK;
  hipError_t x = hipSuccess;
  if (!e->side_st) x = hipStreamCreateWithFlags(&e->side_st, hipStreamNonBlocking);
  for (hipEvent_t* ev : {&e->ev_prep, &e->ev_rep[0], &e->ev_rep[1]})
    if (x == hipSuccess && !*ev) x = hipEventCreateWithFlags(ev, hipEventDisableTiming);
  if (x != hipSuccess) return set_err(CC_ERR_HIP, "hipMalloc map events (second set)", x);
  TRY(alloc_sm_set(e, e->sm_alt, e->sm_cap, "hipMalloc map events (second set)"));
  e->sm_alt_on = true;
  return CC_OK;
}
// the deferred replay on the side stream, after what the engine stream has queued so far
static int launch_pending_replay(cc_engine* e, hipStream_t st) {
  if (!e->pend) return CC_OK;
  e->pend = false;
  HIPCHECK(hipEventRecord(e->ev_prep, st));
  HIPCHECK(hipStreamWaitEvent(e->side_st, e->ev_prep, 0));
  if (launch_small_replay_kernel(e->pend_sa, e->side_st)) return set_err(CC_ERR_HIP, "small-map replay launch", hipGetLastError());
  HIPCHECK(hipEventRecord(e->ev_rep[e->pend_set], e->side_st));
  e->rep_pending[e->pend_set] = true;
  return CC_OK;
}
// the engine stream waits for the side-stream replay of event-buffer set k, then folds its exit marks into the
// d_msmall snapshot (common.h, the small-map window invariant: the only place a replay's result reaches the flags)
static int wait_replay(cc_engine* e, int k, hipStream_t st) {
  if (!e->rep_pending[k]) return CC_OK;
  HIPCHECK(hipStreamWaitEvent(st, e->ev_rep[k], 0));
  e->rep_pending[k] = false;
  uint8_t* const left = e->d_msm_left + (size_t)k * e->cfg.max_resources;
  return launched(launch_small_fold(left, e->d_msmall, e->cfg.max_resources, st), "small-map fold launch", st);
}
// the engine stream waits for the side stream's replays (before barrier rows, timers, and the batch's end)
static int join_replay(cc_engine* e, hipStream_t st) {
  TRY(launch_pending_replay(e, st));
  for (int k = 0; k < 2; ++k) TRY(wait_replay(e, k, st));
  return CC_OK;
}

// the current event buffers into an argument struct that names them ev_key / ev_val / ev_pay.  Read after
// ensure_small and the sub-batch's set swap, which both change them.
template <class A>
static void set_events(const cc_engine* e, A& a) {
  a.ev_key = e->sm.key;
  a.ev_val = e->sm.val;
  a.ev_pay = e->sm.pay;
}
// the replay's arguments on the engine stream (its exit marks in set 2, folded right after it)
static SmallArgs small_args(const cc_engine* e) {
  SmallArgs sa{};
  set_events(e, sa);
  sa.ev_key2 = e->sm.key2;
  sa.ev_val2 = e->sm.val2;
  sa.cap = (uint32_t)e->sm_cap;
  sa.temp = e->d_sm_temp;
  sa.temp_bytes = e->sm_temp_bytes;
  sa.ctl = e->d_sm_ctl;
  sa.seg = e->d_sm_seg;
  sa.nseg = e->d_sm_seg + e->cfg.max_resources;
  sa.state = e->d_msm;
  sa.big = e->d_mbig;
  sa.msmall = e->d_msmall;
  sa.left = e->d_msm_left + 2ull * e->cfg.max_resources;
  sa.err = e->d_err;
  sa.mpcap = e->d_mpcap;
  sa.max_resources = e->cfg.max_resources;
  sa.lvl_at = e->d_lvl_at;
  return sa;
}

// TTL mode: the map events appended so far (commits, expiries) -> every map's size and capacity, the small maps' key
// sets (map_small.hip: sort, runs, k_small_replay + k_ttl_replay), then the counters for the next round.
static int ttl_replay(cc_engine* e, hipStream_t st, const uint64_t* index = nullptr, uint64_t lo = 0,
                      const cc_results* out = nullptr) {
  uint32_t ctl[2] = {0, 0};
  HIPCHECK(hipMemcpyAsync(ctl, e->d_sm_ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  SmallArgs sa = small_args(e);
  sa.msize = e->d_msize;
  sa.index = index;  // (null for the expiry-only flushes: they grow no table)
  sa.lo = lo;
  sa.out_status = out ? out->status : nullptr;  // (the sub-batch's size / isEmpty rows among the events)
  sa.out_value = out ? out->value : nullptr;
  TRY(join_replay(e, st));  // (an overlapped replay of an earlier sub-batch: the models it writes)
  const int rs = launch_small_replay(sa, ctl[0], st, st);
  if (rs) return rs == -1 ? set_err(CC_ERR_HIP, "TTL map events launch", hipGetLastError())
                          : set_err(CC_ERR_STATE, "TTL map events exceed their buffer");
  DBG_SYNC("TTL map events launch");
  return launched(launch_small_finish(sa, st), "map event counters", st);
}

static TtlEmit ttl_emit_args(const cc_engine* e, const uint64_t* time, uint64_t n, uint64_t lo, uint64_t bl, uint64_t bh,
                             uint64_t adv) {
  TtlEmit t{};
  t.time = time;
  t.n = n;
  t.lo = lo;
  t.bl = bl;
  t.bh = bh;
  t.adv = adv;
  t.deferred = (e->cfg.flags & CC_CFG_TIMERS_DEFERRED) ? 1u : 0u;
  t.hh_key = e->d_hh_key;
  t.hh_val = e->d_hh_val;
  t.hh_n = e->hh_n;
  set_events(e, t);
  t.ev_cap = (uint32_t)e->sm_cap;
  t.ctl = e->d_sm_ctl;
  return t;
}

// TTL mode: the expiries of the boundaries [bl, bh] that no sub-batch owned (before a barrier row, at the batch end),
// or every timer due by `adv` (cc_advance_time), as size events.
int cc::ttl_flush(cc_engine* e, const uint64_t* time, uint64_t n, uint64_t bl, uint64_t bh, uint64_t adv, hipStream_t st) {
  TRY(ensure_small(e));
  const TtlEmit te = ttl_emit_args(e, time, n, bl, bl, bh, adv);
  LAUNCH(launch_ttl_scan(te, e->d_clock, e->d_tbl_word, e->d_tbl_key, e->d_tbl_dl, e->map_entries, e->d_err, st),
         "TTL scan launch");
  return ttl_replay(e, st);
}

// the cleared maps' size scan (map_clear.hip): one element per map event, sized with the event buffer
static int ensure_clr_scan(cc_engine* e) {
  if (e->d_clr_scan && e->clr_scan_cap >= e->sm_cap) return CC_OK;
  const size_t tb = std::max<size_t>(clr_scan_temp_bytes((uint32_t)e->sm_cap), 256);
  TRY(regrow({BUF(e->d_clr_scan, clr_scan_bytes_per_event() * e->sm_cap), BUF(e->d_clr_stemp, tb)}, e->clr_scan_cap,
             (size_t)e->sm_cap, "hipMalloc clear size scan"));
  e->clr_stemp_bytes = tb;
  return CC_OK;
}

// ---- the batch's row lists ----

// the in-stream lists, each regrown as a whole (first use: 2^20 rows; then what a scan counted)
static int grow_szq(cc_engine* e, uint32_t cap) {
  return regrow({BUF(e->d_szq, sizeof(uint32_t) * cap)}, e->szq_cap, cap, "hipMalloc size / isEmpty row list");
}
static int grow_cvq(cc_engine* e, uint32_t cap) {
  return regrow({BUF(e->d_cvq, sizeof(uint32_t) * cap), BUF(e->d_isc, sizeof(uint32_t) * cap)}, e->cvq_cap, cap,
                "hipMalloc containsValue row lists");
}
static int grow_clrq(cc_engine* e, uint32_t cap) {
  const size_t tb = std::max<size_t>(clr_sort_temp_bytes(cap), 256);
  TRY(regrow({BUF(e->d_clrq, sizeof(uint32_t) * cap), BUF(e->d_clr_keys, sizeof(uint64_t) * cap),
              BUF(e->d_clr_keys2, sizeof(uint64_t) * cap), BUF(e->d_clr_temp, tb)},
             e->clrq_cap, cap, "hipMalloc clear row lists"));
  e->clr_temp_bytes = tb;
  return CC_OK;
}

// containsValue in the stream (map_cv.hip): the batch's in-stream rows sorted (device) and copied to the host, which
// cuts each sub-batch's slice of them.
constexpr uint32_t kCvMaxRows = 1u << 21;  // in-stream containsValue rows per sub-batch (a denser run shortens it)
static int cv_rows(cc_engine* e, uint32_t n2, hipStream_t st) {
  e->isc_rows.clear();
  if (n2 == 0) return CC_OK;
  const size_t need = std::max<size_t>(cv_rows_temp_bytes(e->cvq_cap), 256);
  if (!e->d_isc2 || need > e->cv_rtemp_bytes)
    TRY(regrow({BUF(e->d_isc2, sizeof(uint32_t) * e->cvq_cap), BUF(e->d_cv_rtemp, need)}, e->cv_rtemp_bytes, need,
               "hipMalloc containsValue row sort"));
  LAUNCH(cv_sort_rows(e->d_isc, e->d_isc2, n2, e->d_cv_rtemp, e->cv_rtemp_bytes, st), "containsValue row sort");
  e->isc_rows.resize(n2);
  HIPCHECK(hipMemcpyAsync(e->isc_rows.data(), e->d_isc2, sizeof(uint32_t) * n2, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  return CC_OK;
}
// clears in the stream (map_clear.hip): the batch's list sorted by (map, row) with per-map offsets on the device; the
// host keeps the rows of any map cleared 128 times or more (a sub-batch holds at most 127 clears of one map)
static int clr_rows(cc_engine* e, uint32_t n, const cc_batch* c, hipStream_t st) {
  e->clr_n = n;
  e->clr_heavy.clear();
  if (n == 0) return CC_OK;
  ClrBatchArgs cb{};
  cb.rows = e->d_clrq;
  cb.n = n;
  cb.inst = c->inst;
  cb.inst_res = e->d_inst_res;
  cb.keys = e->d_clr_keys;
  cb.keys2 = e->d_clr_keys2;
  cb.off = e->d_clr_off;
  cb.R = e->cfg.max_resources;
  cb.temp = e->d_clr_temp;
  cb.temp_bytes = e->clr_temp_bytes;
  LAUNCH(launch_clr_batch(cb, st), "clear list launch");
  if (n >= 128) {
    std::vector<uint64_t> keys(n);
    HIPCHECK(hipMemcpyAsync(keys.data(), e->d_clr_keys2, sizeof(uint64_t) * n, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    for (uint32_t a = 0; a < n;) {
      uint32_t b = a;
      while (b < n && (keys[b] >> 32) == (keys[a] >> 32)) ++b;
      if (b - a >= 128) {
        std::vector<uint32_t> rows(b - a);
        for (uint32_t q = a; q < b; ++q) rows[q - a] = (uint32_t)keys[q];
        e->clr_heavy.push_back(std::move(rows));
      }
      a = b;
    }
  }
  return CC_OK;
}

// the operand set (sized for kCvMaxRows operands) and the event buffers (two events per commit, one per query)
constexpr uint32_t kCvBloomMaxBits = 25;  // the operand filter: ~16 bits per operand, 2^16 .. 2^25 bits
static int ensure_cv(cc_engine* e) {
  if (e->d_cvset) return CC_OK;
  const uint32_t sc = 2 * kCvMaxRows;
  const uint64_t ec = 2ull * e->sub_batch + kCvMaxRows;
  if (ec > 0xFFFFFFFFull) return set_err(CC_ERR_CAPACITY, "containsValue event buffer beyond 2^32 entries");
  const size_t tb = std::max<size_t>(cv_sort_temp_bytes((uint32_t)ec), 256);
  TRY(regrow({BUF(e->d_cvset, sizeof(CvEnt) * sc), BUF(e->d_cvcnt, sizeof(uint32_t) * sc),
              BUF(e->d_cvseg, sizeof(uint32_t) * (sc + 1)), BUF(e->d_cvev_key, 8 * ec), BUF(e->d_cvev_key2, 8 * ec),
              BUF(e->d_cvev_val, 4 * ec), BUF(e->d_cvev_val2, 4 * ec), BUF(e->d_cvev_ctl, sizeof(uint32_t) * 2),
              BUF(e->d_cvtemp, tb), BUF(e->d_cvbloom, (1ull << kCvBloomMaxBits) / 8)},
             e->cvset_cap, sc, "hipMalloc containsValue buffers"));
  e->cvev_cap = (uint32_t)ec;
  e->cvtemp_bytes = tb;
  return CC_OK;
}

// ---- one cc_apply_batch call ----

// what one listing pass counted
struct Listed {
  uint32_t nb = 0, ttl_seen = 0, qn = 0, cvn[2] = {0, 0}, cln = 0;
};

// One sub-batch [lo, hi): the contexts its launches share, filled in stages, and what its steps tell later ones.
struct Sub {
  uint64_t lo = 0, hi = 0;
  uint32_t tiles = 0;
  size_t cv_b = 0;  // its in-stream containsValue rows: isc_rows[cv_b, cv_b + cv_n)
  uint32_t cv_n = 0;
  bool clr_on = false;  // clears in the stream in this batch (map_clear.hip)
  bool v3 = false;      // value-only engines: value_path.hip
  bool vg = false;      // [lo, hi) is a group staged in the engine's group arrays (value_group.h): the partition
  uint64_t vg_seg = 0;  // covers all of it, sub_value and unpermute its segment vg_seg
  ClrSubArgs ca{};
  ClrCtx cctx{};
  CvSubArgs cva{};
  HotArgs ha{};
  SizeArgs sz{};  // this sub-batch's size / isEmpty rows (map_small.hip)
  TtlEmit te{};
  bool sized = false;  // the event pipeline ran (its counters are reset after the answers)
  uint32_t sized_events = 0;
  bool ttl_pending = false;  // TTL mode: the sub-batch's event replay, after the unpermute
  uint32_t cv_E = 0;         // in-stream containsValue events (final once the map apply kernels ran)
  bool cv_known = false;     // (read with the map events' count: one host round trip per sub-batch, not two)
  bool unpermuted = false;   // launched early, beside the host's counter readback
};

// the next thing in log order: a barrier row, or a group timer firing (timers first at the same boundary)
enum { kEnd = 0, kBarrier = 1, kTimer = 2 };
struct Next {
  int action;
  uint64_t hi;  // the rows before it are applied first
  size_t tk;    // kTimer: the timer
};

// One call: its arguments, what the phases hand on, and the phases in the order cc_apply_batch runs them.
struct Batch {
  cc_engine* e;
  const cc_batch* c;
  uint64_t n;
  const cc_results* out;
  const cc_events* ev;
  void* stream;  // as the caller passed it (the two-halves recursion passes it on)
  hipStream_t st = nullptr;
  uint64_t clock_before = 0;  // the engine clock before this batch (TTL mode and barrier rows need it on the host)
  bool deferred = false;      // CC_CFG_TIMERS_DEFERRED
  std::vector<uint64_t> sched_dl, sched_fb;  // per barrier (schedule rows): the timer's deadline, its firing boundary
  uint64_t cur = 0;     // rows before it are applied
  size_t bi = 0;        // the next barrier row
  uint64_t own_lo = 0;  // TTL mode: the first timer-firing boundary no sub-batch has owned yet (common.h TtlEmit)

  int validate(), scan_rows(bool inline_size, bool inline_ttl, Listed& l), list_rows(uint32_t& nb), apply_halves();
  int gather_bar_rows(uint32_t nb), fire_bounds(), detect_hot_keys();
  HotArgs hot_args(uint64_t lo, uint64_t hi) const;  // what the hot-key detect and bind share
  Next next_action() const;
  int cut_sub(uint64_t lo, uint64_t seg_hi, Sub& s), apply_sub(Sub& s);
  bool group_staged(uint64_t rows);             // value-only: the group staging holds (a group of) this stretch
  int apply_group(uint64_t lo, uint64_t& hi);   // value-only: one group from lo, cut before hi
  int sub_clear_epochs(Sub& s), sub_hot_bind(Sub& s), sub_partition(Sub& s), sub_value(Sub& s), sub_cv_prepare(Sub& s);
  int sub_map(Sub& s), sub_ttl_tail(Sub& s), sub_size_tail(Sub& s), sub_small_replay(Sub& s, uint32_t events);
  int sub_coord(Sub& s), unpermute(Sub& s), sub_answers(Sub& s), sub_events(Sub& s);
  template <class A> void set_results(A& a) const;
  template <class A> void set_staged(const Sub& s, A& a) const;
  MapSizeArgs map_size_args(const Sub& s) const;
  SizeArgs size_args(const Sub& s) const;
  int fire_group_timer(const Next& nx), apply_bar_row(uint64_t row), finish();
  int bar_group_schedule(const BarRow& br, size_t bk, uint32_t res, uint64_t row);
  int bar_whole_map(const BarRow& br, uint32_t res, uint64_t row);
};

// the argument checks, the stream hand-over, the control plane's queued registry writes
int Batch::validate() {
  if (n > e->cfg.max_batch) return set_err(CC_ERR_CAPACITY, "batch larger than max_batch");
  if (!c->inst || !c->op || !c->flags || !c->a || !c->b || !out->status || !out->value)
    return set_err(CC_ERR_INVALID, "inst/op/flags/a/b columns and status/value outputs are required");
  HIPCHECK(hipSetDevice(e->device));
  st = stream ? (hipStream_t)stream : e->own_stream;
  if (st != e->last_stream) HIPCHECK(hipStreamSynchronize(e->last_stream));
  if (e->dev_dirty()) TRY(quiesce(e));  // registry writes queued by the control plane since the last device work
  e->last_stream = st;
  if ((((uintptr_t)out->status) & 3) || (((uintptr_t)out->value) & 15) || (((uintptr_t)c->inst) & 15))
    return set_err(CC_ERR_INVALID, "inst and value must be 16-byte aligned, status 4-byte aligned");
  if (e->map_bits && !c->key) return set_err(CC_ERR_INVALID, "an engine with maps needs the key column");
  if (e->map_bits && !c->index)  // (log order of map events and the entries' claims: the tree-bin test, map_wide.hip)
    return set_err(CC_ERR_INVALID, "an engine with maps needs the index column");
  if (e->d_val_live && !c->index) return set_err(CC_ERR_INVALID, "CC_CFG_VALUE_RETAINED needs the index column");
  if (ev && (!ev->pos || !ev->target || !ev->code || !ev->src || !ev->tag || !ev->payload || !ev->count))
    return set_err(CC_ERR_INVALID, "event stream columns and count are required");
  deferred = (e->cfg.flags & CC_CFG_TIMERS_DEFERRED) != 0;
  e->bars.clear();
  e->szq_n = 0;
  e->isc_rows.clear();
  e->clr_n = 0;
  e->clr_heavy.clear();
  return CC_OK;
}

// the lists a listing pass fills, on first need
static int ensure_lists(cc_engine* e, bool inline_size, bool inline_ttl) {
  if ((inline_size || inline_ttl) && !e->d_szq) TRY(grow_szq(e, 1u << 20));
  if (inline_size || inline_ttl) TRY(alloc_once(e->d_szq_n, sizeof(uint32_t)));
  if (!inline_size) return CC_OK;
  if (!e->d_cvq) TRY(grow_cvq(e, 1u << 20));  // containsValue candidates (map_cv.hip)
  TRY(alloc_once(e->d_cvq_n, sizeof(uint32_t) * 2));
  TRY(alloc_once(e->d_mfirst, sizeof(uint32_t) * e->cfg.max_resources));
  TRY(alloc_once(e->d_maynull, e->cfg.max_resources));
  if (!e->d_clrq) TRY(grow_clrq(e, 1u << 20));  // clears in the stream (map_clear.hip)
  TRY(alloc_once(e->d_clrq_n, sizeof(uint32_t)));
  TRY(alloc_once(e->d_clr_off, sizeof(uint32_t) * (e->cfg.max_resources + 1)));
  TRY(alloc_once(e->d_clr_base, sizeof(uint32_t) * e->cfg.max_resources));
  return alloc_once(e->d_clr_eend, e->cfg.max_resources);
}

// one listing pass: the barrier scan, the containsValue classification, and every counter in one round trip
int Batch::scan_rows(bool inline_size, bool inline_ttl, Listed& l) {
  const bool sizes = inline_size || inline_ttl;
  if (e->szq_flagged) {
    LAUNCH(launch_mflag_clear(e->d_msmall, e->cfg.max_resources, st), "map flags");
    e->szq_flagged = false;
  }
  HIPCHECK(hipMemsetAsync(e->d_ttl_seen, 0, sizeof(uint32_t), st));
  LAUNCH(launch_map_barriers(c->inst, c->op, c->aux, n, e->d_inst_res, e->d_res_type, e->cfg.max_instances, e->d_bar,
                             e->d_bar_n, kBarCap, e->d_ttl_seen, sizes ? e->d_szq : nullptr,
                             sizes ? e->d_szq_n : nullptr, e->szq_cap, e->d_msmall, inline_size ? e->d_cvq : nullptr,
                             inline_size ? e->d_cvq_n : nullptr, e->cvq_cap, inline_size ? e->d_mfirst : nullptr,
                             e->cfg.max_resources, inline_size ? e->d_clrq : nullptr,
                             inline_size ? e->d_clrq_n : nullptr, e->clrq_cap, st),
         "map barrier scan launch");
  if (inline_size) {  // containsValue candidates: in the stream, or barriers (map_cv.hip)
    CvBatchArgs cb{};
    cb.inst = c->inst;
    cb.op = c->op;
    cb.flags = c->flags;
    cb.n = n;
    cb.inst_res = e->d_inst_res;
    cb.max_inst = e->cfg.max_instances;
    cb.mflag = e->d_msmall;
    cb.tbl_word = e->d_tbl_word;
    cb.entries = e->map_entries;
    cb.cvq = e->d_cvq;
    cb.cvq_n = e->d_cvq_n;
    cb.cvq_cap = e->cvq_cap;
    cb.mfirst = e->d_mfirst;
    cb.maynull = e->d_maynull;
    cb.R = e->cfg.max_resources;
    cb.bar = e->d_bar;
    cb.bar_n = e->d_bar_n;
    cb.bar_cap = kBarCap;
    cb.isc = e->d_isc;
    cb.isc_n = e->d_cvq_n + 1;
    LAUNCH(launch_cv_batch(cb, st), "containsValue classify launch");
  }
  // (one round trip: every counter into the pinned words, then one synchronize)
  uint64_t* const pin = e->h_pin;
  uint32_t* const p32 = reinterpret_cast<uint32_t*>(pin + 1);
  HIPCHECK(hipMemcpyAsync(pin, e->d_clock, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIPCHECK(hipMemcpyAsync(p32 + 0, e->d_bar_n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHECK(hipMemcpyAsync(p32 + 1, e->d_ttl_seen, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (sizes) HIPCHECK(hipMemcpyAsync(p32 + 2, e->d_szq_n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (inline_size) HIPCHECK(hipMemcpyAsync(p32 + 3, e->d_cvq_n, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (inline_size) HIPCHECK(hipMemcpyAsync(p32 + 5, e->d_clrq_n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (e->map_bits) {  // the batch's first and last log index (map event positions, below)
    HIPCHECK(hipMemcpyAsync(pin + 4, c->index, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(pin + 5, c->index + n - 1, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  }
  HIPCHECK(hipStreamSynchronize(st));
  // Map events are keyed by their position (log index - the sub-batch's first, 32 bits: common.h kEvPosBits).
  // A batch whose whole index range fits needs no cut; else each sub-batch ends before its first row 2^32 past
  // its start (k_span_cut, one round trip per sub-batch, only then)
  if (e->map_bits) e->span_cut = n && pin[5] - pin[4] >= (1ull << kEvPosBits);
  clock_before = pin[0];
  l = Listed{};
  l.nb = p32[0];
  l.ttl_seen = p32[1];
  if (sizes) l.qn = p32[2];
  if (inline_size) l.cvn[0] = p32[3], l.cvn[1] = p32[4], l.cln = p32[5];
  return CC_OK;
}

// Whole-map ops are barriers (map_wide.hip): find them, and the rows answered in the stream.
// Outside TTL mode the size / isEmpty, clear / removeValue and Delete rows of maps, sets and multimaps and a map's
// containsValue rows are answered in the stream (listed, their slots flagged); in TTL mode size / isEmpty rows are
// (the event replay answers them), the others are barriers.  A batch that turns TTL mode on (or lists more than a
// list holds) is scanned again with TTL mode's lists (or larger ones).
int Batch::list_rows(uint32_t& nb) {
  bool inline_size = e->map_bits && !e->ttl_live;
  bool inline_ttl = e->map_bits && e->ttl_live;
  Listed l;
  for (int pass = 0;; ++pass) {
    TRY(ensure_lists(e, inline_size, inline_ttl));
    TRY(scan_rows(inline_size, inline_ttl, l));
    if (!inline_size && !inline_ttl) break;
    e->szq_flagged = l.qn > 0 || l.cvn[0] > 0 || l.cln > 0;
    if (inline_size && (l.ttl_seen || pass > 2)) {  // this batch turns TTL mode on: containsValue and clear become
      inline_size = false;                          // barriers again, size / isEmpty stay in the stream
      inline_ttl = pass <= 2;
      continue;
    }
    // a larger list, then the same scan again
    if (l.qn > e->szq_cap) { TRY(grow_szq(e, l.qn)); continue; }
    if (l.cln > e->clrq_cap) { TRY(grow_clrq(e, l.cln)); continue; }
    if (l.cvn[0] > e->cvq_cap) { TRY(grow_cvq(e, l.cvn[0])); continue; }
    e->szq_n = l.qn;
    if (inline_ttl) break;  // (TTL mode lists size / isEmpty rows only)
    TRY(cv_rows(e, l.cvn[1], st));          // the in-stream rows, sorted, on the host too
    TRY(clr_rows(e, l.cln, c, st));  // the in-stream clears: sorted by (map, row), offsets
    break;
  }
  if (l.ttl_seen && !e->ttl_live) {  // TTL mode for good: sizes and capacities from commit + expiry events
    e->ttl_live = true;
    e->small_live = false;  // (every map's events are replayed in TTL mode, the small ones' key sets included)
  }
  nb = l.nb;
  // The leak log (commits dropped without clean()) is drained before every batch of an engine that can add to it:
  // every multimap put, every bus unregister, and with value events every re-listen (AtomicValueState.listen :41-49) may land
  // there, at most one entry per row, so the drained log gets room for n more; a coordination engine without value events
  // adds entries only in the close fan-out (cc_sessions_close sizes the log for that itself) but is drained here
  // too, so nothing accumulates across batches toward the log's end.
  if (e->has_mmaps || e->coord_on) {
    TRY(drain_leaks(e));
    // (a bus row drops at most its own or the commit it replaces, and a leave the leaver's registrations besides:
    // entries the buses held before the batch, or rows of the batch that dropped nothing of their own)
    const uint64_t held = std::min<uint64_t>(n, e->bus_slots) * e->coord_cap;
    if (e->has_mmaps || e->bus_slots || (e->cfg.flags & CC_CFG_VALUE_EVENTS)) TRY(ensure_leak(e, n + held));
  }
  return CC_OK;
}

// More barrier rows than one listing holds: the batch runs as two consecutive batches (a batch boundary is a point
// of the log like any other: timers due by its clock have fired there in both timer orders, A8).  With an event
// stream the second half's events are appended after the first's, their rows moved by h.
int Batch::apply_halves() {
  if (n < 2) return set_err(CC_ERR_CAPACITY, "more whole-map ops and group schedules in one row than kBarCap");
  const uint64_t h = n / 2;
  auto shift = [h](const auto* p) { return p ? p + h : p; };
  const cc_batch c2{shift(c->index), shift(c->time), shift(c->inst), shift(c->op), shift(c->flags), shift(c->key),
                    shift(c->a), shift(c->b), shift(c->aux)};
  const cc_results o2{out->status + h, out->value + h};
  int rc = cc_apply_batch(e, c, h, out, ev, stream);
  if (rc || !ev || !e->coord_on) return rc ? rc : cc_apply_batch(e, &c2, n - h, &o2, ev, stream);
  uint64_t n1 = 0, n2 = 0;
  HIPCHECK(hipMemcpyAsync(&n1, ev->count, sizeof n1, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  if (n1 > ev->capacity) return set_err(CC_ERR_CAPACITY, "event stream capacity exceeded");
  TRY(alloc_once(e->d_half_count, sizeof(uint64_t)));
  cc_events ev2 = *ev;
  ev2.pos += n1, ev2.target += n1, ev2.code += n1, ev2.src += n1, ev2.tag += n1, ev2.payload += n1;
  ev2.capacity -= n1;
  ev2.count = e->d_half_count;
  TRY(cc_apply_batch(e, &c2, n - h, &o2, &ev2, stream));
  HIPCHECK(hipMemcpyAsync(&n2, e->d_half_count, sizeof n2, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  LAUNCH(launch_ev_shift(ev2.pos, std::min(n2, ev2.capacity), (uint32_t)h, st), "event row shift launch");
  const uint64_t total = n1 + n2;
  HIPCHECK(hipMemcpyAsync(ev->count, &total, sizeof total, hipMemcpyHostToDevice, st));
  HIPCHECK(hipStreamSynchronize(st));  // (total is a host local)
  return CC_OK;
}

// the barrier rows in log order, then their columns in one gather (one copy back, not one per field)
int Batch::gather_bar_rows(uint32_t nb) {
  e->bars.resize(nb);
  HIPCHECK(hipMemcpy(e->bars.data(), e->d_bar, sizeof(uint32_t) * nb, hipMemcpyDeviceToHost));
  std::sort(e->bars.begin(), e->bars.end());
  if (nb > e->bar_rows_cap)
    TRY(regrow({BUF(e->d_bar_rows, sizeof(BarRow) * nb)}, e->bar_rows_cap, nb, "hipMalloc barrier rows"));
  HIPCHECK(hipMemcpyAsync(e->d_bar, e->bars.data(), sizeof(uint32_t) * nb, hipMemcpyHostToDevice, st));
  LAUNCH(launch_bar_fields(e->d_bar, nb, c->inst, c->op, c->flags, c->a, c->key, c->aux, c->index, c->time,
                           e->d_bar_rows, st),
         "barrier rows gather launch");
  e->bar_rows.resize(nb);
  HIPCHECK(hipMemcpyAsync(e->bar_rows.data(), e->d_bar_rows, sizeof(BarRow) * nb, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  return CC_OK;
}

// Group timers: where each pending one fires in this batch, and where the timer of each schedule row of the batch
// would (the clock at row r is max(clock_before, time[r])): the first row r >= from whose clock reaches the deadline
// -> the boundary the timer fires at (manager mode: after row r; module mode: before it, A8), or ~0 when no row of
// this batch reaches it.  One device search for all of them (k_fire_bounds).
int Batch::fire_bounds() {
  if (e->coord_on || e->ttl_live) {  // events of this batch start at 0; the log clock must not go backwards inside it
    if (e->coord_on) HIPCHECK(hipMemsetAsync(e->d_ev_total, 0, sizeof(unsigned long long), st));
    // (without barrier rows every row goes through k_part_ext, which checks it against the row before it)
    if (!e->bars.empty()) LAUNCH(launch_time_check(c->time, n, e->d_clock, e->d_err, st), "time check");
  }
  sched_dl.assign(e->bars.size(), 0);
  sched_fb.assign(e->bars.size(), ~0ull);
  std::vector<uint64_t> dl, from;
  std::vector<uint32_t> who;  // < gtimers.size(): a pending timer; else gtimers.size() + barrier index
  for (size_t q = 0; q < e->gtimers.size(); ++q) {
    dl.push_back(e->gtimers[q].deadline);
    from.push_back(0);
    who.push_back((uint32_t)q);
  }
  for (size_t k = 0; k < e->bars.size(); ++k) {
    const BarRow& br = e->bar_rows[k];
    if (br.op != CC_OP_GROUP_SCHEDULE) continue;
    const uint64_t delay = c->aux ? br.aux : 0;
    const uint64_t clock = c->time ? std::max(br.t_row, clock_before) : clock_before;
    sched_dl[k] = clock + ((int64_t)delay > 0 ? delay : 0);  // schedule :86-103
    dl.push_back(sched_dl[k]);
    from.push_back(deferred ? e->bars[k] : (uint64_t)e->bars[k] + 1);
    who.push_back((uint32_t)(e->gtimers.size() + k));
  }
  const uint32_t m = (uint32_t)dl.size();
  if (!m) return CC_OK;
  if (m > e->fb_cap) TRY(regrow({BUF(e->d_fb, sizeof(uint64_t) * 3 * m)}, e->fb_cap, m, "hipMalloc timer bounds"));
  std::vector<uint64_t> res(m);
  HIPCHECK(hipMemcpyAsync(e->d_fb, dl.data(), 8ull * m, hipMemcpyHostToDevice, st));
  HIPCHECK(hipMemcpyAsync(e->d_fb + m, from.data(), 8ull * m, hipMemcpyHostToDevice, st));
  LAUNCH(launch_fire_bounds(c->time, n, clock_before, e->d_fb, e->d_fb + m, m, deferred, e->d_fb + 2 * m, st),
         "timer bounds launch");
  HIPCHECK(hipMemcpyAsync(res.data(), e->d_fb + 2 * m, 8ull * m, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  for (uint32_t i = 0; i < m; ++i) {
    if (who[i] < e->gtimers.size()) e->gtimers[who[i]].fire_b = res[i];
    else sched_fb[who[i] - e->gtimers.size()] = res[i];
  }
  return CC_OK;
}

// the batch's hot map keys (apply_map_hot.hip): counted once, bound per sub-batch
HotArgs Batch::hot_args(uint64_t lo, uint64_t hi) const {
  HotArgs ha{};
  ha.inst = c->inst;
  ha.flags = c->flags;
  ha.key = c->key;
  ha.lo = lo;
  ha.hi = hi;
  ha.inst_res = e->d_inst_res;
  ha.res_type = e->d_res_type;
  ha.max_inst = e->cfg.max_instances;
  ha.hot_samp = e->d_hot_samp;
  ha.hot_cand = e->d_hot_cand;
  ha.hot_cand_n = e->d_hot_cand_n;
  return ha;
}
int Batch::detect_hot_keys() {
  return launched(launch_map_hot_detect(hot_args(0, n), st), "hot-key detect launch", st);
}

Next Batch::next_action() const {
  const uint64_t bar_b = bi < e->bars.size() ? (uint64_t)e->bars[bi] : ~0ull;
  size_t tk = e->gtimers.size();
  for (size_t q = 0; q < e->gtimers.size(); ++q) {
    const auto& g = e->gtimers[q];
    if (g.fire_b == ~0ull || g.fire_b < cur) continue;
    if (tk == e->gtimers.size()) { tk = q; continue; }
    const auto& o = e->gtimers[tk];
    if (std::make_tuple(g.fire_b, g.deadline, g.id) < std::make_tuple(o.fire_b, o.deadline, o.id)) tk = q;
  }
  const uint64_t tim_b = tk < e->gtimers.size() ? e->gtimers[tk].fire_b : ~0ull;
  if (tim_b != ~0ull && tim_b <= bar_b) return Next{kTimer, tim_b, tk};
  return bar_b != ~0ull ? Next{kBarrier, bar_b, tk} : Next{kEnd, n, tk};
}

// ---- one sub-batch ----

// the sub-batch starting at lo: the other event-buffer set, then its end, cut before seg_hi by a map's 128th clear,
// by kCvMaxRows in-stream containsValue rows and by the index span
int Batch::cut_sub(uint64_t lo, uint64_t seg_hi, Sub& s) {
  uint64_t& hi = s.hi = std::min(seg_hi, lo + (e->ext ? e->sub_ext : e->sub_batch));
  if (e->sm_alt_on && !e->ttl_live) {  // the other event-buffer set, once its replay is done (engine_state.h SmSet)
    std::swap(e->sm, e->sm_alt);
    e->sm_cur ^= 1;
    TRY(wait_replay(e, e->sm_cur, st));  // (its replay's exit marks fold into the snapshot here)
  }
  for (const auto& hv : e->clr_heavy) {  // at most 127 in-stream clears of one map per sub-batch (map_clear.hip)
    const size_t q = (size_t)(std::lower_bound(hv.begin(), hv.end(), (uint32_t)lo) - hv.begin());
    if (q + 127 < hv.size() && hv[q + 127] < hi) hi = hv[q + 127];
  }
  // this sub-batch's in-stream containsValue rows (at most kCvMaxRows: a denser run ends the sub-batch earlier)
  auto cv_at = [this](uint64_t row) {
    return (size_t)(std::lower_bound(e->isc_rows.begin(), e->isc_rows.end(), (uint32_t)row) - e->isc_rows.begin());
  };
  size_t cv_b = 0, cv_e = 0;
  if (!e->isc_rows.empty()) {
    cv_b = cv_at(lo);
    cv_e = cv_at(hi);
    if (cv_e - cv_b > kCvMaxRows) {
      cv_e = cv_b + kCvMaxRows;
      hi = e->isc_rows[cv_e];
    }
  }
  if (e->span_cut && !e->ttl_live) {  // (TTL mode positions events by row, 2 (row - lo) + 1: always within 32 bits)
    HIPCHECK(hipMemsetAsync(e->d_span_cut, 0xFF, sizeof(uint64_t), st));
    LAUNCH(launch_span_cut(c->index, lo, hi, e->d_span_cut, st), "span cut launch");
    HIPCHECK(hipMemcpyAsync(e->h_pin + 6, e->d_span_cut, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    if (e->h_pin[6] > lo && e->h_pin[6] < hi) hi = e->h_pin[6];
    if (!e->isc_rows.empty()) cv_e = cv_at(hi);  // (the in-stream containsValue rows of the shortened sub-batch)
  }
  s.lo = lo;
  s.tiles = (uint32_t)((hi - lo + kTile - 1) / kTile);
  s.cv_b = cv_b;
  s.cv_n = (uint32_t)(cv_e - cv_b);
  s.clr_on = e->clr_n > 0;
  s.v3 = !e->ext;
  return CC_OK;
}

// clears in the stream: the sub-batch's clear epochs per map (map_clear.hip), and the context every map kernel reads
int Batch::sub_clear_epochs(Sub& s) {
  ClrSubArgs& ca = s.ca;
  TRY(ensure_small(e));  // (the cleared maps' sizes ride the map event buffer)
  ca.keys = e->d_clr_keys2;
  ca.n = e->clr_n;
  ca.off = e->d_clr_off;
  ca.R = e->cfg.max_resources;
  ca.lo = s.lo;
  ca.hi = s.hi;
  ca.base = e->d_clr_base;
  ca.eend = e->d_clr_eend;
  ca.mflag = e->d_msmall;
  ca.err = e->d_err;
  ca.index = c->index;
  set_events(e, ca);
  ca.ev_cap = (uint32_t)e->sm_cap;
  ca.ev_ctl = e->d_sm_ctl;
  ca.cgen = e->d_mw_cgen;
  // the epoch buckets: at most 1024 per map and ~64 MB in all
  uint32_t nbmax = 16;
  while (nbmax < 1024 && (uint64_t)(2 * nbmax) * e->cfg.max_resources <= (64ull << 20)) nbmax <<= 1;
  uint32_t sh = 0;
  while (((s.hi - s.lo + (1ull << sh) - 1) >> sh) > nbmax) ++sh;
  ca.bshift = sh;
  ca.nb = (uint32_t)((s.hi - s.lo + (1ull << sh) - 1) >> sh);
  const size_t need = (size_t)nbmax * e->cfg.max_resources;
  if (e->clr_btab_bytes < need) TRY(regrow({BUF(e->d_clr_btab, need)}, e->clr_btab_bytes, need, "hipMalloc clear epochs"));
  ca.btab = e->d_clr_btab;
  LAUNCH(launch_clr_sub(ca, st), "clear epochs launch");
  s.cctx = ClrCtx{e->d_msmall, e->d_clr_keys2, e->d_clr_off, e->d_clr_base, e->d_clr_eend, s.lo, e->d_tbl_ep,
                  e->d_clr_btab, ca.nb, ca.bshift};
  return CC_OK;
}

// what every apply kernel reads: the partition's tile table and bucket counts, the staged results
template <class A>
void Batch::set_results(A& a) const {
  a.ttab = e->d_ttab;
  a.sb = e->sb_total();
  a.sb_val = e->sb;
  a.rst_status = e->d_rst_status;
  a.rst_value = e->d_rst_value;
  a.err = e->d_err;
  a.mark = marker_of(e);
}
// what the hot-key kernels and the map apply both read: the sub-batch's staged map records, the table, the results
template <class A>
void Batch::set_staged(const Sub& s, A& a) const {
  set_results(a);
  a.lo = s.lo;
  a.mrec = e->d_mrec;
  a.cb = c->b;
  a.tiles = s.tiles;
  a.map_bits = e->map_bits;
  a.tbl_key = e->d_tbl_key;
  a.tbl_word = e->d_tbl_word;
  a.tbl_val = e->d_tbl_val;
  a.tbl_ci = e->d_tbl_ci;
  a.tbl_ins = e->d_tbl_ins;
  a.tbl_claim = e->d_tbl_claim;
  a.idx0 = c->index ? c->index + s.lo : nullptr;
}

// hot map keys of this sub-batch (routed to their own buckets by the partition); TTL mode has none: every key goes
// through its region (timers are walked in order)
int Batch::sub_hot_bind(Sub& s) {
  if (e->ttl_live) {
    HIPCHECK(hipMemsetAsync(e->d_hot_n, 0, sizeof(uint32_t), st));
    return CC_OK;
  }
  HotArgs& ha = s.ha = hot_args(s.lo, s.hi);
  set_staged(s, ha);
  ha.hot = e->d_hot;
  ha.hot_n = e->d_hot_n;
  ha.hot_rpre = e->d_hot_rpre;
  ha.hot_rstart = e->d_hot_rstart;
  ha.hot_len = e->d_hot_len;
  ha.hot_cond = e->d_hot_cond;
  ha.hot_agg = e->d_hot_agg;
  ha.hot_s0 = e->d_hot_s0;
  ha.hot_meta = e->d_hot_meta;
  ha.hot_msz = e->d_hot_msz;
  ha.msmall = nullptr;  // (every map's keys are hot-routed)
  if (e->small_live || e->szq_n || s.clr_on) {  // small / size-queried / cleared maps' hot commits: map events
    TRY(ensure_small(e));
    if (!c->index) return set_err(CC_ERR_INVALID, "an engine with maps needs the index column (log order)");
    ha.hc.clr = s.cctx;  // (cleared maps: commit epochs, map_clear.hip)
    ha.hc.mflag = e->d_msmall;
    ha.hc.hh_key = e->d_hh_key;
    ha.hc.hh_val = e->d_hh_val;
    ha.hc.hh_n = e->hh_n;
    ha.hc.xr = e->d_mrec;
    ha.hc.lo = s.lo;
    set_events(e, ha.hc);
    ha.hc.ev_cap = (uint32_t)e->sm_cap;
    ha.hc.ev_ctl = e->d_sm_ctl;
    ha.hc.idx0p = c->index + s.lo;
    ha.hc.tbl_ep = e->d_tbl_ep;
  }
  static const bool no_hot = diag_env("CC_NO_HOT");  // diagnostics: every key through its region
  if (no_hot) HIPCHECK(hipMemsetAsync(e->d_hot_n, 0, sizeof(uint32_t), st));
  else LAUNCH(launch_map_hot_bind(ha, st), "hot-key bind launch");
  return CC_OK;
}

// the partition; directly after it the previous sub-batch's small-map replay (engine_state.h pend_sa)
int Batch::sub_partition(Sub& s) {
  PartArgs pa{};
  pa.inst = c->inst;
  pa.op = c->op;
  pa.flags = c->flags;
  pa.a = c->a;
  pa.b = c->b;
  pa.key = c->key;
  pa.index = c->index;
  pa.aux = (e->coord_on || e->ttl_live) ? c->aux : nullptr;  // maps read ttl only in TTL mode (the scan saw none)
  pa.time = c->time;
  pa.clock_base = e->d_clock;
  pa.ext_flags = ((e->cfg.flags & CC_CFG_VALUE_EVENTS) ? kExtValue : 0u) | (deferred ? kExtDeferred : 0u) |
                 ((e->coord_on || e->ttl_live) && e->bars.empty() ? kExtTimeCheck : 0u);
  pa.err = e->d_err;
  pa.ext = e->ext;
  pa.lo = s.lo;
  pa.hi = s.hi;
  pa.inst_res = e->d_inst_res;
  pa.inst_id = e->coord_on ? e->d_inst_id : nullptr;
  pa.res_type = e->d_res_type;
  pa.sb_kind = e->d_sb_kind;
  pa.max_inst = e->cfg.max_instances;
  pa.sb = e->sb_total();
  pa.sb_val = e->sb;
  pa.sbq_base = e->quarter ? e->sbq_base() : 0u;
  pa.map_bits = e->map_bits;
  pa.hot = e->d_hot;
  pa.hot_n = e->d_hot_n;
  pa.st_meta = e->d_st_meta;
  pa.st_ab = e->d_st_ab;
  pa.xrec = e->d_xrec;
  pa.mrec = e->d_mrec;
  pa.hot_meta = e->d_hot_meta;
  pa.clr = s.cctx;  // (each map commit's clear epoch into its meta word)
  pa.cpos = e->d_cpos;
  pa.ttab = e->d_ttab;
  pa.dummy = e->sub_batch;
  if (s.vg) {  // the whole group in one launch: tile-local records, cpos and ttab rows in the group arrays
    pa.st_ab = reinterpret_cast<u64x2*>(e->d_vg_rec);
    pa.cpos = e->d_vg_cpos;
    pa.ttab = e->d_vg_ttab;
    pa.dummy = e->vg_rows;
  }
  pa.v3 = s.v3;
  pa.mark = marker_of(e);
  if (launch_partition(pa, st)) {
    const hipError_t x = hipGetLastError();
    if (x == hipSuccess) return set_err(CC_ERR_CAPACITY, "the partition's LDS cannot hold this engine's buckets");
    return set_err(CC_ERR_HIP, "partition launch", x);
  }
  DBG_SYNC("partition launch");
  TRY(launch_pending_replay(e, st));  // (the previous sub-batch's small-map replay, beside this one's work)
  if (e->map_bits && e->ttl_live) LAUNCH(launch_map_rows(e->d_cpos, s.lo, s.hi, e->d_map_row, st), "map rows launch");
  return CC_OK;
}

int Batch::sub_value(Sub& s) {
  ValueArgs va{};
  set_results(va);
  va.st_meta = e->d_st_meta;
  va.st_ab = e->d_st_ab;
  va.tiles = s.v3 ? (uint32_t)((s.hi - s.lo + kV3Tile - 1) / kV3Tile) : s.tiles;
  va.v3 = s.v3;
  va.rst_word = e->d_rst_word;
  va.ca = c->a;
  va.cb = c->b;
  va.lo = s.lo;
  va.sb_kind = e->d_sb_kind;
  va.val_meta = e->d_val_meta;
  va.val_v = e->d_val_v;
  va.dummy = e->sub_batch;
  if (s.vg) {
    // Segment vg_seg of the group: the group arrays from the segment's first tile on, its first row, and the dummy
    // position counted from that tile.  Rows and staging move together: an escaped record finds its operands at row
    // lo + its tile's first position (value_path.hip v3_decode_escaped), both counted from the segment's start.
    VgSegment g;
    const int rc = vg_segment(s.hi - s.lo, e->sub_batch, e->vg_rows, s.vg_seg, g);
    if (rc) return set_err(rc, "value group: a segment outside its staging");
    const uint64_t p0 = g.tile0 * kV3Tile;
    va.st_ab = reinterpret_cast<u64x2*>(e->d_vg_rec + p0);
    va.rst_word = e->d_vg_word + p0;
    va.rst_value = e->d_vg_value + p0;
    va.ttab = e->d_vg_ttab + g.tile0 * (va.sb + 1);
    va.tiles = (uint32_t)g.tiles;
    va.lo = s.lo + g.row0;
    va.dummy = g.dummy;
  }
  return launched(launch_apply_value(va, st), "apply launch", st);
}

// in-stream containsValue: operand set, initial counts, query events (map_cv.hip)
int Batch::sub_cv_prepare(Sub& s) {
  CvSubArgs& cva = s.cva;
  TRY(ensure_cv(e));
  uint32_t sc = 1024;
  while (sc < 2 * s.cv_n) sc <<= 1;
  cva.cv.mflag = e->d_msmall;
  cva.cv.set = e->d_cvset;
  cva.cv.mask = sc - 1;
  cva.cv.bloom = e->d_cvbloom;
  cva.cv.bbits = 16;
  while (cva.cv.bbits < kCvBloomMaxBits && (1ull << cva.cv.bbits) < 16ull * s.cv_n) ++cva.cv.bbits;
  cva.cv.ev_key = e->d_cvev_key;
  cva.cv.ev_val = e->d_cvev_val;
  cva.cv.cap = e->cvev_cap;
  cva.cv.ctl = e->d_cvev_ctl;
  cva.cv.idx0p = c->index + s.lo;
  cva.set = e->d_cvset;
  cva.cnt = e->d_cvcnt;
  cva.isc = e->d_isc2 + s.cv_b;
  cva.isc_n = s.cv_n;
  cva.lo = s.lo;
  cva.inst = c->inst;
  cva.flags = c->flags;
  cva.a = c->a;
  cva.index = c->index;
  cva.inst_res = e->d_inst_res;
  cva.tbl_word = e->d_tbl_word;
  cva.tbl_val = e->d_tbl_val;
  cva.entries = e->map_entries;
  cva.err = e->d_err;
  cva.key2 = e->d_cvev_key2;
  cva.val2 = e->d_cvev_val2;
  cva.seg = e->d_cvseg;
  cva.nseg = e->d_cvseg + e->cvset_cap;
  cva.coll = e->d_cvseg;          // (free until the answers' runs: the prepare's collision list)
  cva.coll_n = e->d_cvev_ctl + 1;
  cva.temp = e->d_cvtemp;
  cva.temp_bytes = e->cvtemp_bytes;
  cva.out_status = out->status;
  cva.out_value = out->value;
  LAUNCH(launch_cv_prepare(cva, st), "containsValue prepare launch");
  s.ha.cv = cva.cv;
  return CC_OK;
}

// the hot-key apply (outside TTL mode) and the map apply; TTL mode: this sub-batch owns the timer-firing boundaries
// [own_lo, hi] (common.h TtlEmit)
int Batch::sub_map(Sub& s) {
  if (!e->ttl_live) LAUNCH(launch_map_hot_apply(s.ha, st), "hot-key apply launch");
  MapArgs ma{};
  ma.cv = s.cva.cv;
  ma.clr = s.cctx;
  set_staged(s, ma);
  ma.dropped = e->d_mw_drop;
  ma.cgen = e->d_mw_cgen;
  ma.cset = e->d_cset;
  ma.cset_mask = e->cset_mask;
  ma.cset_full = e->d_cset_full;
  ma.ttl = e->ttl_live;
  ma.tbl_dl = e->d_tbl_dl;
  ma.map_row = e->d_map_row;
  ma.time = c->time;
  ma.aux = c->aux;
  ma.clock_base = e->d_clock;
  ma.deferred = deferred;
  ma.rst_msz = e->d_rst_msz;
  if (e->ttl_live) {
    TRY(ensure_small(e));
    s.te = ttl_emit_args(e, c->time, n, s.lo, own_lo, s.hi, 0);
    ma.ttl_emit = s.te;
  }
  LAUNCH(launch_apply_map(ma, st), "map apply launch");
  if (s.clr_on) LAUNCH(launch_clr_gen(s.ca, st), "clear generation launch");
  return CC_OK;
}

// what both modes' map size launches share; the event fields only once the event buffers are settled
MapSizeArgs Batch::map_size_args(const Sub& s) const {
  MapSizeArgs za{};
  za.ttab = e->d_ttab;
  za.cpos = e->d_cpos;
  za.tiles = s.tiles;
  za.rows = s.hi - s.lo;
  za.sb = e->sb_total();
  za.k0 = e->sb;
  za.k1 = e->sbq_base();
  za.sb_hot = e->sb + (1u << e->map_bits);
  za.rst_msz = e->d_rst_msz;
  za.hot = e->d_hot;
  za.hot_n = e->d_hot_n;  // (0: no hot keys in TTL mode)
  za.hot_len = e->d_hot_len;
  za.hot_rpre = e->d_hot_rpre;
  za.hot_msz = e->d_hot_msz;
  za.res_type = e->d_res_type;
  za.max_resources = e->cfg.max_resources;
  za.tcnt = e->d_msz_tcnt;
  za.msize = e->d_msize;
  za.mpcap = e->d_mpcap;
  za.list = e->d_msz_list;
  za.list_n = e->d_msz_list_n;
  za.err = e->d_err;
  za.lvl_at = e->d_lvl_at;
  za.index = c->index;
  za.lo = s.lo;
  return za;
}
static void map_size_events(const cc_engine* e, MapSizeArgs& za) {
  za.mrec = e->d_mrec;
  za.hh_key = e->d_hh_key;
  za.hh_val = e->d_hh_val;
  za.hh_n = e->hh_n;
  set_events(e, za);
  za.ev_cap = (uint32_t)e->sm_cap;
  za.sm_ctl = e->d_sm_ctl;
}
// this sub-batch's size / isEmpty rows, joining the map events
SizeArgs Batch::size_args(const Sub& s) const {
  SizeArgs sz{};
  sz.szq = e->d_szq;
  sz.szq_n = e->szq_n;
  sz.lo = s.lo;
  sz.hi = s.hi;
  sz.inst = c->inst;
  sz.op = c->op;
  sz.index = c->index;
  sz.inst_res = e->d_inst_res;
  sz.res_type = e->d_res_type;
  set_events(e, sz);
  sz.cap = (uint32_t)e->sm_cap;
  sz.ctl = e->d_sm_ctl;
  sz.err = e->d_err;
  return sz;
}

// TTL mode: exact sizes and capacities from the sub-batch's commits and expiries as events; the size / isEmpty rows
// join them at their rows' positions
int Batch::sub_ttl_tail(Sub& s) {
  LAUNCH(launch_ttl_scan(s.te, e->d_clock, e->d_tbl_word, e->d_tbl_key, e->d_tbl_dl, e->map_entries, e->d_err, st),
         "TTL scan launch");
  MapSizeArgs za = map_size_args(s);
  map_size_events(e, za);
  za.map_row = e->d_map_row;
  LAUNCH(launch_map_size(za, st), "map size launch");
  own_lo = s.hi + 1;
  if (e->szq_n) {
    s.sz = size_args(s);
    s.sz.ttl = true;
    LAUNCH(launch_size_emit(s.sz, st), "size query launch");
  }
  s.ttl_pending = true;  // (the replay answers them: after the unpermute's placeholders)
  return CC_OK;
}

// the replay of the sub-batch's map events (sort, runs, the small maps' models): on the engine stream, or deferred
// to the side stream, where it overlaps the next sub-batch (engine_state.h SmSet), launched once that sub-batch's
// partition is queued (launch_pending_replay)
int Batch::sub_small_replay(Sub& s, uint32_t events) {
  SmallArgs sa = small_args(e);
  sa.cseg = e->sm.cseg;
  sa.idx0 = c->index + s.lo;
  static const bool no_side = diag_env("CC_NO_SIDE_REPLAY");  // diagnostics: the replay on the engine stream
  if (events && !no_side) {
    TRY(ensure_sm_alt(e));
    sa.defer = true;
    sa.left = e->d_msm_left + (size_t)e->sm_cur * e->cfg.max_resources;  // (folded by wait_replay)
  }
  const int rs = launch_small_replay(sa, events, st, st);
  if (sa.defer && !rs) {
    e->pend_sa = sa;
    e->pend = true;
    e->pend_set = e->sm_cur;
  }
  if (rs) return rs == -1 ? set_err(CC_ERR_HIP, "small-map replay launch", hipGetLastError())
                          : set_err(CC_ERR_STATE, "small-map events exceed their buffer");
  DBG_SYNC("small-map replay launch");
  return CC_OK;
}

// outside TTL mode: exact map sizes and HashMap capacities (containsValue's iteration order); the small /
// size-queried / cleared maps' insertions and removals as events, counted in the sub-batch's one host round trip
int Batch::sub_size_tail(Sub& s) {
  const bool events = e->small_live || e->szq_n || s.clr_on;
  MapSizeArgs za = map_size_args(s);
  if (events) {
    TRY(ensure_small(e));
    if (!c->index) return set_err(CC_ERR_INVALID, "an engine with maps needs the index column (log order)");
    map_size_events(e, za);
    za.msmall = e->d_msmall;
    za.idx0 = c->index + s.lo;
  }
  LAUNCH(launch_map_size(za, st), "map size launch");
  if (e->szq_n) {
    s.sz = size_args(s);
    s.sz.sorted_key = e->sm.key2;
    s.sz.sorted_val = e->sm.val2;
    s.sz.seg = e->d_sm_seg;
    s.sz.nseg = e->d_sm_seg + e->cfg.max_resources;
    s.sz.msize = e->d_msize;
    s.sz.out_status = out->status;
    s.sz.out_value = out->value;
    LAUNCH(launch_size_emit(s.sz, st), "size query launch");
  }
  if (s.clr_on) LAUNCH(launch_clr_events(s.ca, st), "clear events launch");
  if (!events) return CC_OK;
  uint32_t* const p32 = reinterpret_cast<uint32_t*>(e->h_pin);  // (pinned: one round trip for both)
  HIPCHECK(hipMemcpyAsync(p32, e->d_sm_ctl, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (s.cv_n) HIPCHECK(hipMemcpyAsync(p32 + 2, e->d_cvev_ctl, sizeof s.cv_E, hipMemcpyDeviceToHost, st));
  if (!e->coord_on) {  // (the coordination apply, launched later, writes staged results: then no early unpermute)
    if (!e->ev_rb) HIPCHECK(hipEventCreateWithFlags(&e->ev_rb, hipEventDisableTiming));
    HIPCHECK(hipEventRecord(e->ev_rb, st));
    TRY(unpermute(s));  // (on the GPU while the host waits for the counters)
    HIPCHECK(hipEventSynchronize(e->ev_rb));
  } else {
    HIPCHECK(hipStreamSynchronize(st));
  }
  const uint32_t ctl[2] = {p32[0], p32[1]};
  if (s.cv_n) memcpy(&s.cv_E, p32 + 2, sizeof s.cv_E);
  s.cv_known = s.cv_n != 0;
  e->stat_events += ctl[0];
  TRY(sub_small_replay(s, ctl[0]));
  if (e->small_live && ctl[0] == 0 && ctl[1] == 0) e->small_live = false;  // (ctl[1]: maps small after the last replay)
  s.sized = true;
  s.sized_events = ctl[0];
  return CC_OK;
}

int Batch::sub_coord(Sub& s) {
  HIPCHECK(hipMemsetAsync(e->d_ev_cnt, 0, sizeof(uint16_t) * (s.hi - s.lo), st));
  HIPCHECK(hipMemsetAsync(e->d_arena_n, 0, sizeof(unsigned long long), st));
  CoordArgs ca{};
  set_results(ca);
  ca.xrec = e->d_xrec;
  ca.tiles = s.tiles;
  ca.sbq_base = e->quarter ? e->sbq_base() : 0u;
  ca.sb_kind = e->d_sb_kind;
  ca.res_type = e->d_res_type;
  ca.inst_id = e->d_inst_id;
  ca.coord = e->d_coord;
  ca.coord_cap = e->coord_cap;
  ca.val_meta = e->d_val_meta;
  ca.val_v = e->d_val_v;
  ca.ev_cnt = e->d_ev_cnt;
  ca.arena = e->d_arena;
  ca.arena_n = e->d_arena_n;
  ca.arena_cap = e->arena_cap;
  ca.leak = e->d_leak;
  ca.leak_n = e->d_leak_n;
  ca.leak_cap = e->leak_cap;
  ca.fx = e->d_fan;
  ca.bus = e->bus_slots != 0;
  if (!e->has_topics) return launched(launch_apply_coord(ca, st), "coordination apply launch", st);
  // TopicState.publish, MessageBusState register / unregister / leave: the walk leaves fan records, k_topic_fanout
  // expands them into the arena
  HIPCHECK(hipMemsetAsync(e->d_fan, 0, offsetof(FanCtx, cap), st));
  TRY(launched(launch_apply_coord(ca, st), "coordination apply launch", st));
  FanoutArgs fa{};
  fa.fx = e->d_fan;
  fa.arena = e->d_arena;
  fa.arena_n = e->d_arena_n;
  fa.arena_cap = e->arena_cap;
  fa.err = e->d_err;
  fa.mark = marker_of(e);
  return launched(launch_topic_fanout(fa, st), "topic fan-out launch", st);
}

// the sub-batch's results back to log order (every staged result is written by then)
int Batch::unpermute(Sub& s) {
  UnpermuteArgs ua{};
  ua.cpos = e->d_cpos;
  ua.ttab = e->d_ttab;
  ua.sb = e->sb_total();
  ua.lo = s.lo;
  ua.hi = s.hi;
  ua.rst_status = e->d_rst_status;
  ua.rst_value = e->d_rst_value;
  ua.out_status = out->status;
  ua.out_value = out->value;
  ua.dummy_status = e->d_rst_status + e->sub_batch;
  ua.dummy_value = e->d_rst_value + e->sub_batch;
  ua.v3 = s.v3;
  ua.words = e->d_rst_word;
  if (s.vg) {
    // Segment vg_seg of the group, right behind its apply, whose result words are then still in the last-level cache
    // (one unpermute over a whole 100M-row group read them from HBM and took 0.07 ms per step longer than the
    // launches it saved: DESIGN 4.3).  The status dummy rows stay the per-sub-batch array's.
    VgSegment g;
    const int rc = vg_segment(s.hi - s.lo, e->sub_batch, e->vg_rows, s.vg_seg, g);
    if (rc) return set_err(rc, "value group: a segment outside its staging");
    const uint64_t p0 = g.tile0 * kV3Tile;
    ua.lo = s.lo + g.row0;
    ua.hi = ua.lo + g.rows;
    ua.cpos = e->d_vg_cpos + p0;
    ua.rst_value = e->d_vg_value + p0;
    ua.dummy_value = e->d_vg_value + e->vg_rows;
    ua.words = e->d_vg_word + p0;
  }
  ua.mark = marker_of(e);
  s.unpermuted = true;
  return launched(launch_unpermute(ua, st), "unpermute launch", st);
}

// the answers written over the unpermute's placeholders: in-stream containsValue (map_cv.hip), TTL mode's replay,
// size / isEmpty rows and the cleared maps' (map_small.hip, map_clear.hip); then the next sub-batch's counters
int Batch::sub_answers(Sub& s) {
  if (s.cv_n) {
    if (!s.cv_known) {
      HIPCHECK(hipMemcpyAsync(e->h_pin, e->d_cvev_ctl, sizeof s.cv_E, hipMemcpyDeviceToHost, st));
      HIPCHECK(hipStreamSynchronize(st));
      memcpy(&s.cv_E, e->h_pin, sizeof s.cv_E);
    }
    const int rc = launch_cv_answer(s.cva, s.cv_E, st);
    if (rc) return rc == -2 ? set_err(CC_ERR_CAPACITY, "containsValue events exceed their buffer")
                            : set_err(CC_ERR_HIP, "containsValue answer launch", hipGetLastError());
    DBG_SYNC("containsValue answer launch");
  }
  // TTL mode: sizes, capacities, small maps' key sets, and the size / isEmpty rows' answers
  if (s.ttl_pending) TRY(ttl_replay(e, st, c->index, s.lo, out));
  if (!s.sized) return CC_OK;
  if (e->szq_n && s.sized_events) LAUNCH(launch_size_answer(s.sz, st), "size answer launch");
  if (s.clr_on && s.sized_events) {  // the cleared maps' sizes, capacities and size / isEmpty rows (map_clear.hip)
    ClrReplayArgs cr{};
    cr.key = e->sm.key2;
    cr.val = e->sm.val2;
    cr.pay = e->sm.pay;
    cr.mflag = e->d_msmall;
    cr.msize = e->d_msize;
    cr.mpcap = e->d_mpcap;
    cr.lvl_at = e->d_lvl_at;
    cr.idx0 = c->index + s.lo;
    cr.out_status = out->status;
    cr.out_value = out->value;
    TRY(ensure_clr_scan(e));
    cr.scan = e->d_clr_scan;
    cr.temp = e->d_clr_stemp;
    cr.temp_bytes = e->clr_stemp_bytes;
    LAUNCH(launch_clr_replay(cr, s.sized_events, st), "clear replay launch");
  }
  SmallArgs sf{};
  sf.ctl = e->d_sm_ctl;
  sf.msmall = e->d_msmall;
  sf.max_resources = e->cfg.max_resources;
  return launched(launch_small_finish(sf, st), "small-map counters", st);
}

// the sub-batch's coordination events into the caller's event stream, in log order (events.hip)
int Batch::sub_events(Sub& s) {
  EventArgs ea{};
  ea.cpos = e->d_cpos;
  ea.lo = s.lo;
  ea.hi = s.hi;
  ea.tiles = s.tiles;
  ea.ev_cnt = e->d_ev_cnt;
  ea.row_of = e->d_row_of;
  ea.ev_loc = e->d_ev_loc;
  ea.tile_sum = e->d_tile_sum;
  ea.tile_off = e->d_tile_off;
  ea.ev_total = e->d_ev_total;
  ea.arena = e->d_arena;
  ea.arena_n = e->d_arena_n;
  ea.arena_cap = e->arena_cap;
  ea.perm = e->d_ev_perm;
  ea.bucket = e->d_ev_bucket;  // the tile-bucketed order pass (CC_EV_V1=1: the gather pass)
  ea.ccnt = e->d_ev_ccnt;
  if (ev) {
    ea.out_cap = ev->capacity;
    ea.out_pos = ev->pos;
    ea.out_target = ev->target;
    ea.out_code = ev->code;
    ea.out_src = ev->src;
    ea.out_tag = ev->tag;
    ea.out_payload = ev->payload;
  }
  ea.err = e->d_err;
  ea.mark = marker_of(e);
  return launched(launch_events(ea, st), "events launch", st);
}

// one sub-batch, cut by cut_sub: its steps in stream order
int Batch::apply_sub(Sub& s) {
  if (s.clr_on) TRY(sub_clear_epochs(s));
  s.cva.clr = s.cctx;
  ++e->stat_subbatches;
  e->stat_isc += s.cv_n;
  if (e->map_bits) TRY(sub_hot_bind(s));
  TRY(sub_partition(s));
  if (e->has_values || !e->ext) TRY(sub_value(s));
  if (s.cv_n) TRY(sub_cv_prepare(s));
  if (e->map_bits) {
    TRY(sub_map(s));
    TRY(e->ttl_live ? sub_ttl_tail(s) : sub_size_tail(s));
  }
  if (e->coord_on) TRY(sub_coord(s));
  if (!s.unpermuted) TRY(unpermute(s));
  TRY(sub_answers(s));
  if (e->coord_on) TRY(sub_events(s));
  return CC_OK;
}

// ---- a value-only engine's group (value_group.h) ----

// The group staging for a stretch of `rows` rows: allocated by the first stretch longer than a sub-batch, for
// min(rows, max_batch, the group's limit) in whole tiles; grown by a longer one; kept until destroy.  false: the
// per-sub-batch path takes the stretch (one segment, CC_VALUE_GROUP_TILES=0, or the allocation failed).
bool Batch::group_staged(uint64_t rows) {
  VgPlan p;
  if (e->ext || rows <= e->sub_batch || !vg_plan(rows, e->sub_batch, e->cfg.max_batch, e->vg_knob, p) || !p.group_rows)
    return false;
  if (p.staging_rows <= e->vg_rows) return true;
  if (p.staging_rows >= e->vg_refused) return false;
  const uint64_t rows_al = p.staging_rows, pad = 4 * kPT;
  const int rc = regrow({BUF(e->d_vg_rec, sizeof(uint64_t) * (rows_al + pad)), BUF(e->d_vg_cpos, sizeof(uint16_t) * rows_al),
                         BUF(e->d_vg_ttab, sizeof(uint16_t) * (rows_al / kV3Tile) * (e->sb_total() + 1)),
                         BUF(e->d_vg_word, sizeof(uint32_t) * (rows_al + pad)),
                         BUF(e->d_vg_value, sizeof(uint64_t) * (rows_al + pad))},
                        e->vg_rows, rows_al, "hipMalloc value group staging");
  if (rc) {  // (not an error of the call: the launches below check hipGetLastError, so the failure is taken off it)
    (void)hipGetLastError();
    e->vg_refused = rows_al;
    return false;
  }
  return true;
}

// One group from lo: the partition over all of it in one launch, then the apply and the unpermute segment by segment
// in log order (the walker state goes from one apply launch to the next through val_meta / val_v).
int Batch::apply_group(uint64_t lo, uint64_t& hi) {
  // what else cuts a sub-batch (cut_sub: a map's 128th clear, containsValue rows, the index span, the event-buffer
  // swap) needs maps; a value-only engine has none
  if (e->ext || e->map_bits || e->coord_on || e->ttl_live || e->span_cut || e->sm_alt_on || e->clr_n ||
      !e->clr_heavy.empty() || !e->isc_rows.empty())
    return set_err(CC_ERR_STATE, "value group on an engine whose sub-batches have other cuts");
  VgPlan p;
  if (!vg_plan(hi - lo, e->sub_batch, e->cfg.max_batch, e->vg_knob, p) || !p.group_rows)
    return set_err(CC_ERR_STATE, "value group without a plan");
  hi = std::min(hi, lo + std::min(p.group_rows, e->vg_rows));
  Sub g;
  g.lo = lo;
  g.hi = hi;
  g.tiles = (uint32_t)((hi - lo + kTile - 1) / kTile);
  g.v3 = g.vg = true;
  TRY(sub_partition(g));
  const uint64_t segs = vg_segments(hi - lo, e->sub_batch);
  for (g.vg_seg = 0; g.vg_seg < segs; ++g.vg_seg) {
    ++e->stat_subbatches;
    TRY(sub_value(g));
    TRY(unpermute(g));
  }
  return CC_OK;
}

// ---- between the sub-batches ----

// a group timer fires at the boundary nx.hi (MembershipGroupState.java:92-98)
int Batch::fire_group_timer(const Next& nx) {
  const cc_engine::GroupTimer gt = e->gtimers[nx.tk];
  e->gtimers.erase(e->gtimers.begin() + (ptrdiff_t)nx.tk);
  const uint32_t pos = (uint32_t)(deferred ? nx.hi - 1 : nx.hi);
  LAUNCH(launch_group_fire(e->d_coord, e->coord_cap, gt.slot, gt.member, gt.tag, gt.payload, pos, e->d_ev_total, ev,
                           e->d_err, st),
         "group timer launch");
  cur = nx.hi;
  return CC_OK;
}

// a group schedule row :86-103 (member = key, callback = a, delay = aux): the timer it arms, if the member exists
int Batch::bar_group_schedule(const BarRow& br, size_t bk, uint32_t res, uint64_t row) {
  const uint64_t member = br.key;
  LAUNCH(launch_group_schedule(e->d_coord, e->coord_cap, res, member, row, out->status, out->value, e->d_ttl_seen, st),
         "group schedule launch");
  uint32_t found = 0;
  HIPCHECK(hipMemcpyAsync(&found, e->d_ttl_seen, sizeof found, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  if (!found) return CC_OK;
  cc_engine::GroupTimer gt{};
  gt.deadline = sched_dl[bk];
  gt.id = ++e->gtimer_seq;
  gt.member = member;
  gt.tag = CC_FLAG_TAG_A(br.flags);
  gt.payload = gt.tag == CC_TAG_NULL ? 0 : br.a;
  gt.slot = res;
  gt.idx = br.idx;
  gt.fire_b = sched_fb[bk];
  e->gtimers.push_back(gt);
  return CC_OK;
}

// a whole-map op (map_wide.hip) of a map, set or multimap
int Batch::bar_whole_map(const BarRow& br, uint32_t res, uint64_t row) {
  MapWideArgs mw{};
  mw.slot = res;
  mw.op = e->res_type[res] == CC_RES_SET        ? set_as_map_op(br.op)
          : e->res_type[res] == CC_RES_MULTIMAP ? mmap_as_map_op(br.op, CC_FLAG_TAG_A(br.flags))
                                                : br.op;
  mw.atag = CC_FLAG_TAG_A(br.flags);
  mw.apay = br.a;
  mw.row = row;
  mw.tbl_word = e->d_tbl_word;
  mw.tbl_key = e->d_tbl_key;
  mw.tbl_val = e->d_tbl_val;
  mw.tbl_ins = e->d_tbl_ins;
  mw.tbl_claim = e->d_tbl_claim;
  mw.lvl_at = e->d_lvl_at;
  if (e->ttl_live) {  // the clock at which the reference last fired timers before this row (A8)
    uint64_t t0 = clock_before, t1 = clock_before;
    if (c->time) {
      t1 = std::max(br.t_row, clock_before);
      if (row > 0) t0 = std::max(br.t_prev, clock_before);
    }
    mw.tbl_dl = e->d_tbl_dl;
    mw.fire_clock = deferred ? t0 : t1;
  }
  mw.entries = e->map_entries;
  mw.peak_lo = e->d_mw_peak;
  mw.dropped = e->d_mw_drop;
  mw.cgen = e->d_mw_cgen;
  mw.cset = e->d_cset;
  mw.cset_n = e->cset_mask + 1;
  mw.cset_full = e->d_cset_full;
  mw.map_bits = e->map_bits;
  mw.msize = e->d_msize;  // exact in both modes (TTL mode: commit + expiry events, map_small.hip)
  mw.mpcap = e->d_mpcap;
  mw.ctl = e->d_mw_ctl;
  mw.small = e->res_type[res] == CC_RES_MAP ? e->d_msm : nullptr;
  mw.big = e->d_mbig;
  mw.hh_key = e->d_hh_key;
  mw.hh_val = e->d_hh_val;
  mw.hh_n = e->hh_n;
  mw.out_status = out->status;
  mw.out_value = out->value;
  mw.err = e->d_err;
  LAUNCH(launch_map_wide(mw, st), "whole-map op launch");
  if (e->res_type[res] == CC_RES_MAP && (mw.op == CC_OP_MAP_CLEAR || mw.op == CC_OP_DELETE))
    LAUNCH(launch_big_clear(e->d_mbig, e->d_msm, res, st) || launch_small_clear(e->d_msm, res, st),
           "small-map clear launch");
  return CC_OK;
}

// the barrier row `row`, against the state as it stands after the rows before it
int Batch::apply_bar_row(uint64_t row) {
  ++e->stat_barriers;
  const BarRow& br = e->bar_rows[bi];
  const size_t bk = bi;
  cur = row + 1;
  ++bi;
  if (e->map_bits && e->ttl_live) {  // the timers that fire up to this row's boundary, as size events (TtlEmit)
    if (own_lo <= row) TRY(ttl_flush(e, c->time, n, own_lo, row, 0, st));
    own_lo = row + 1;
  }
  // (k_map_barriers listed the row through the device registry; the host mirror must agree before its slot
  // indexes any per-resource array)
  uint32_t res = 0;
  if (row >= n || br.inst >= e->cfg.max_instances || (res = e->inst_res[br.inst]) >= e->cfg.max_resources ||
      !(is_keyed(e->res_type[res]) || e->res_type[res] == CC_RES_GROUP))
    return set_err(CC_ERR_STATE, "barrier row does not resolve to a map / set / multimap / group on the host registry");
  return e->res_type[res] == CC_RES_GROUP ? bar_group_schedule(br, bk, res, row) : bar_whole_map(br, res, row);
}

// the batch's end: set / multimap results, retained value commits, the event count, the clock, the applied watermark
int Batch::finish() {
  if (e->has_sets || e->has_mmaps) {
    KeyedResultArgs ka{c->inst, c->op, c->flags, c->index, n, e->d_inst_res, e->d_res_type, e->cfg.max_instances,
                       out->status, out->value, e->d_leak, e->d_leak_n, e->leak_cap, e->d_err};
    LAUNCH(launch_keyed_results(ka, st), "set / multimap results launch");
  }
  // Retained value commits (live.hip): after every value op of the batch has applied.  The post-pass attributes
  // each row through the END-of-batch inst_res / res_type / val_meta: correct because the registry cannot change
  // inside a cc_apply_batch call (resource create/delete, instance open/close are host calls that quiesce the
  // stream between batches; no op applied on the device rebinds an instance or retypes a slot).
  if (e->d_val_live)
    LAUNCH(launch_value_live(c->inst, c->op, out->status, out->value, c->index, n, e->d_inst_res, e->d_res_type,
                             e->cfg.max_instances, e->d_val_meta, e->cfg.max_resources, e->d_val_wrow, e->d_val_live, st),
           "retained value launch");
  if (e->coord_on && ev)
    HIPCHECK(hipMemcpyAsync(ev->count, e->d_ev_total, sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
  // the log clock (timers: lock timeouts, map TTL)
  if (e->coord_on || e->map_bits) LAUNCH(launch_clock_advance(c->time, n, 0, e->d_clock, st), "clock");
  if (c->index) {  // the applied watermark = index of the batch's last entry
    HIPCHECK(hipMemcpyAsync(e->d_last_index, c->index + (n - 1), sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    e->applied_pending = true;
  }
  return CC_OK;
}

extern "C" int cc_apply_batch(cc_engine* e, const cc_batch* c, uint64_t n, const cc_results* out, const cc_events* ev,
                              void* stream) {
  if (!e || !c || !out) return set_err(CC_ERR_INVALID, "null argument");
  e->last_end = nullptr;  // (profiling markers: no begin marker is shared across calls)
  if (n == 0) return CC_OK;
  Batch b{e, c, n, out, ev, stream};
  TRY(b.validate());
  if (e->map_bits || e->coord_on) {
    uint32_t nb = 0;
    TRY(b.list_rows(nb));
    if (nb > kBarCap) return b.apply_halves();
    if (nb) TRY(b.gather_bar_rows(nb));
  }
  TRY(b.fire_bounds());
  if (e->map_bits && !e->ttl_live) TRY(b.detect_hot_keys());
  for (;;) {
    const Next nx = b.next_action();
    for (uint64_t lo = b.cur; lo < nx.hi;) {
      if (b.group_staged(nx.hi - lo)) {  // value-only, more than one segment: one partition and one unpermute
        uint64_t hi = nx.hi;
        TRY(b.apply_group(lo, hi));
        lo = hi;
        continue;
      }
      Sub s;
      TRY(b.cut_sub(lo, nx.hi, s));
      TRY(b.apply_sub(s));
      lo = s.hi;
    }
    TRY(join_replay(e, b.st));  // (barrier rows, timers and the caller read the small maps' models)
    if (nx.action == kTimer) {
      TRY(b.fire_group_timer(nx));
    } else if (nx.action == kBarrier) {
      TRY(b.apply_bar_row(nx.hi));
    } else {
      // TTL mode: the boundaries after the last sub-batch (manager mode: row n)
      if (e->map_bits && e->ttl_live && b.own_lo <= n) TRY(ttl_flush(e, c->time, n, b.own_lo, n, 0, b.st));
      break;
    }
  }
  return b.finish();
}
