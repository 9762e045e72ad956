// route.cpp — an event stream grouped by owning client session (DESIGN §6 "The route").  Host code only; the
// reference that route_gpu.hip's device call is compared with, and the baseline of scripts/route_rate.py.
//
// An event row names its receiver as an instance slot; session_of_inst maps the slot to the host's dense ordinal of the
// client session that owns it.  cc_route_events is a stable least-significant-digit radix ordering of
// (session ordinal, event number) on `threads` workers, then one gather:
//   0. every event is checked (target inside the table, the table entry inside the sessions) and gets its key;
//   1. per round of kHostBits bits of the key: every worker counts the digits of its slice, an exclusive prefix over
//      (digit, worker) gives every worker its place for every digit, and the worker moves its slice's
//      (key, event number) pairs there in slice order: stable by construction;
//   2. the heads (where the sorted key changes) are counted per slice and compacted into the directory;
//   3. the rows are gathered through the final permutation.
// Nothing is stored to an output before step 0 has passed for the whole stream and the directory's capacity is known to
// suffice.  No table is sized by n_sessions.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

#include "route.h"

namespace {

constexpr uint32_t kHostBits = 11;  // the host's own digit: 2048 counters per worker stay in its L1
constexpr uint32_t kHostDigits = 1u << kHostBits;

template <class F>
void parallel(uint32_t threads, F f) {
  if (threads == 1) {
    f(0u);
    return;
  }
  std::vector<std::thread> th;
  th.reserve(threads);
  for (uint32_t t = 0; t < threads; ++t) th.emplace_back(f, t);
  for (auto& x : th) x.join();
}

void note(std::atomic<uint64_t>& err, uint64_t key) {
  uint64_t cur = err.load(std::memory_order_relaxed);
  while (key < cur && !err.compare_exchange_weak(cur, key, std::memory_order_relaxed)) {
  }
}

}  // namespace

namespace cc {

int route_fail(const char* who, uint64_t key) {
  static const char* const what[2] = {"target is not below n_inst", "session_of_inst[target] is not below n_sessions"};
  char msg[160];
  snprintf(msg, sizeof msg, "%s: event %llu: %s", who, (unsigned long long)(key >> 1), what[key & 1]);
  return set_err(CC_ERR_INVALID, msg);
}

int route_check_args(const char* who, const cc_events* in, uint64_t n, const uint32_t* session_of_inst,
                     const uint64_t* id_of_inst, uint32_t n_inst, uint32_t n_sessions, const cc_events* out,
                     const uint64_t* out_instance, const cc_route_dir* dir, const uint64_t* n_active) {
  auto fail = [&](int code, const char* what) {
    char msg[160];
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return set_err(code, msg);
  };
  if (n >= (1ull << 32)) return fail(CC_ERR_INVALID, "n_events must be below 2^32");
  if (!in || !out || !dir || !n_active) return fail(CC_ERR_INVALID, "null argument");
  if (!dir->start || !dir->count || (dir->capacity && !dir->session)) return fail(CC_ERR_INVALID, "null directory array");
  if ((n_inst && !session_of_inst)) return fail(CC_ERR_INVALID, "null session_of_inst");
  if ((id_of_inst == nullptr) != (out_instance == nullptr))
    return fail(CC_ERR_INVALID, "id_of_inst and out_instance must be both NULL or both set");
  auto a4 = [](const void* p) { return ((uintptr_t)p & 3) != 0; };
  auto a8 = [](const void* p) { return ((uintptr_t)p & 7) != 0; };
  if (a4(in->pos) || a4(in->target) || a8(in->payload) || a4(out->pos) || a4(out->target) || a8(out->payload) ||
      a8(out->count) || a4(session_of_inst) || a8(id_of_inst) || a8(out_instance) || a4(dir->session) || a4(dir->start) ||
      a8(dir->count))
    return fail(CC_ERR_INVALID, "a column lacks its natural alignment");
  if (n) {
    if (!in->pos || !in->target || !in->code || !in->src || !in->tag || !in->payload)
      return fail(CC_ERR_INVALID, "null input column");
    if (!out->pos || !out->target || !out->code || !out->src || !out->tag || !out->payload)
      return fail(CC_ERR_INVALID, "null output column");
    if (n_sessions == 0) return fail(CC_ERR_INVALID, "n_sessions is 0 with events to route");
  }
  if (out->capacity < n) return fail(CC_ERR_CAPACITY, "the output stream is too small");
  return CC_OK;
}

}  // namespace cc

extern "C" int cc_route_events(const cc_events* in, uint64_t n, const uint32_t* session_of_inst, const uint64_t* id_of_inst,
                               uint32_t n_inst, uint32_t n_sessions, uint32_t threads, const cc_events* out,
                               uint64_t* out_instance, const cc_route_dir* dir, uint64_t* n_active) {
  using cc::set_err;
  if (const int rc = cc::route_check_args("route events", in, n, session_of_inst, id_of_inst, n_inst, n_sessions, out,
                                          out_instance, dir, n_active))
    return rc;
  if (n == 0) {
    *n_active = 0;
    return CC_OK;
  }
  uint32_t T = threads ? threads : std::max(1u, std::thread::hardware_concurrency());
  T = (uint32_t)std::min<uint64_t>(std::min<uint32_t>(T, 256), std::max<uint64_t>(1, n / 16384));  // 16 Ki events each
  auto lo = [&](uint32_t t) { return n * t / T; };
  std::vector<uint32_t> key[2], perm[2];
  for (int k = 0; k < 2; ++k) key[k].resize(n), perm[k].resize(n);
  // 0. every event: the checks, the key and the identity permutation
  std::atomic<uint64_t> err{cc::kRouteNoErr};
  parallel(T, [&](uint32_t t) {
    for (uint64_t j = lo(t); j < lo(t + 1); ++j) {
      const uint32_t x = in->target[j];
      uint32_t s = 0;
      if (x >= n_inst || (s = session_of_inst[x]) >= n_sessions) {
        note(err, cc::route_key(j, x >= n_inst ? cc::kRouteTarget : cc::kRouteSession));
        break;  // (a later event of this slice has a larger key)
      }
      key[0][j] = s, perm[0][j] = (uint32_t)j;
    }
  });
  if (err.load() != cc::kRouteNoErr) return cc::route_fail("route events", err.load());
  // 1. the rounds
  uint32_t bits = 0;
  for (uint32_t x = n_sessions - 1; x; x >>= 1) ++bits;
  int cur = 0;
  std::vector<uint64_t> hist((size_t)T * kHostDigits);
  for (uint32_t shift = 0; shift < bits; shift += kHostBits, cur ^= 1) {
    const uint32_t* ki = key[cur].data();
    const uint32_t* pi = perm[cur].data();
    uint32_t* ko = key[cur ^ 1].data();
    uint32_t* po = perm[cur ^ 1].data();
    parallel(T, [&](uint32_t t) {
      uint64_t* h = hist.data() + (size_t)t * kHostDigits;
      std::fill(h, h + kHostDigits, 0);
      for (uint64_t j = lo(t); j < lo(t + 1); ++j) ++h[(ki[j] >> shift) & (kHostDigits - 1)];
    });
    uint64_t run = 0;
    for (uint32_t d = 0; d < kHostDigits; ++d)
      for (uint32_t t = 0; t < T; ++t) {
        uint64_t& h = hist[(size_t)t * kHostDigits + d];
        const uint64_t c = h;
        h = run;
        run += c;
      }
    parallel(T, [&](uint32_t t) {
      uint64_t* h = hist.data() + (size_t)t * kHostDigits;
      for (uint64_t j = lo(t); j < lo(t + 1); ++j) {
        const uint64_t d = h[(ki[j] >> shift) & (kHostDigits - 1)]++;
        ko[d] = ki[j], po[d] = pi[j];
      }
    });
  }
  const uint32_t* k = key[cur].data();
  const uint32_t* p = perm[cur].data();
  // 2. the directory: heads per slice, their prefix, then the stores
  std::vector<uint64_t> heads(T + 1, 0);
  parallel(T, [&](uint32_t t) {
    uint64_t c = 0;
    for (uint64_t j = lo(t); j < lo(t + 1); ++j) c += j == 0 || k[j] != k[j - 1];
    heads[t] = c;
  });
  uint64_t active = 0;
  for (uint32_t t = 0; t <= T; ++t) {
    const uint64_t c = heads[t];
    heads[t] = active;
    active += c;
  }
  *n_active = active;
  if (active > dir->capacity) return set_err(CC_ERR_CAPACITY, "route events: the directory is too small");
  parallel(T, [&](uint32_t t) {
    uint64_t at = heads[t];
    for (uint64_t j = lo(t); j < lo(t + 1); ++j)
      if (j == 0 || k[j] != k[j - 1]) dir->session[at] = k[j], dir->start[at] = (uint32_t)j, ++at;
  });
  dir->start[active] = (uint32_t)n;
  *dir->count = active;
  // 3. the rows
  parallel(T, [&](uint32_t t) {
    for (uint64_t j = lo(t); j < lo(t + 1); ++j) {
      const uint32_t s = p[j];
      const uint32_t x = in->target[s];
      out->pos[j] = in->pos[s];
      out->target[j] = x;
      out->code[j] = in->code[s];
      out->src[j] = in->src[s];
      out->tag[j] = in->tag[s];
      out->payload[j] = in->payload[s];
      if (out_instance) out_instance[j] = id_of_inst[x];
    }
  });
  if (out->count) *out->count = n;
  return CC_OK;
}
