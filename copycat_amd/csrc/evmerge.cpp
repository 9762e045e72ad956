// evmerge.cpp — the per-rank event streams of a sharded log back into log order (DESIGN §6 "The event merge").
// Host code only; the reference that evmerge_gpu.hip's device call is compared with.
//
// Each rank's engine publishes its events with pos = a row of that rank's share; rows[r] (the split's row ids) maps it
// back to a log row.  A log row belongs to one rank and a rank's events are ordered by pos, so the merged stream is,
// log row by log row, the owning rank's run of events for that row.  cc_merge_events is a multi-threaded
// count-then-copy over blocks of kBlock consecutive log rows:
//   0. every event is checked (pos non-decreasing and inside the rank's share, its log row inside the log);
//   1. per block, every rank's events of the block are found by two binary searches (rows[r], then pos), the block's
//      rows get their first event and their event count (a row claimed by two runs is refused), the block its total;
//   2. exclusive prefix over the blocks: where each block's events start in the output;
//   3. per block, the rows' counts become offsets and every rank's events of the block are copied to
//      block start + row offset + (event - the row's first event): reads are sequential per rank, the writes stay inside
//      the block's output range.
// Nothing is stored to the output before steps 0 and 1 have passed for the whole log.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

#include "engine_state.h"
#include "evmerge.h"

namespace {

constexpr uint32_t kBlock = 8192;  // log rows per block: 64 KiB of per-row tables per thread
constexpr uint64_t kNoErr = ~0ull;

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

struct Part {
  const uint32_t *pos, *target;
  const uint8_t *code, *src, *tag;
  const uint64_t *payload, *rows;
  uint64_t count, row_count;
};

// rank r's events whose log row lies in [b0, b1): [ea, eb)
inline void block_range(const Part& p, uint64_t b0, uint64_t b1, uint64_t& ea, uint64_t& eb) {
  ea = eb = 0;
  if (!p.count) return;
  const uint64_t ra = (uint64_t)(std::lower_bound(p.rows, p.rows + p.row_count, b0) - p.rows);
  const uint64_t rb = (uint64_t)(std::lower_bound(p.rows, p.rows + p.row_count, b1) - p.rows);
  ea = (uint64_t)(std::lower_bound(p.pos, p.pos + p.count, ra, [](uint32_t x, uint64_t v) { return x < v; }) - p.pos);
  eb = (uint64_t)(std::lower_bound(p.pos, p.pos + p.count, rb, [](uint32_t x, uint64_t v) { return x < v; }) - p.pos);
  if (eb < ea) eb = ea;  // (a `rows` that is not increasing: refused by the caller's total)
}

// The block's per-row tables: first[i] = the first event of log row b0 + i in its rank's stream, cnt[i] = its events.
// Returns the block's events, or kNoErr when a row is claimed by two runs or an event's row lies outside the block.
uint64_t block_tables(const std::vector<Part>& parts, uint64_t b0, uint64_t b1, uint32_t* first, uint32_t* cnt,
                      std::atomic<uint64_t>& err) {
  std::fill(cnt, cnt + (b1 - b0), 0u);
  uint64_t total = 0;
  for (uint32_t r = 0; r < parts.size(); ++r) {
    const Part& p = parts[r];
    uint64_t ea, eb;
    block_range(p, b0, b1, ea, eb);
    for (uint64_t j = ea; j < eb; ++j) {
      const uint64_t row = p.rows[p.pos[j]];
      const bool head = j == ea || p.pos[j] != p.pos[j - 1];
      if (row < b0 || row >= b1 || (head && cnt[row - b0])) {
        note(err, cc::evmerge_key(r, j, cc::kEvmClaimed));
        return kNoErr;
      }
      if (head) first[row - b0] = (uint32_t)j;
      ++cnt[row - b0];
    }
    total += eb - ea;
  }
  return total;
}

}  // namespace

namespace cc {

int evmerge_fail(const char* who, uint64_t key) {
  static const char* const what[4] = {"pos is not below the rank's row count", "pos decreases",
                                      "rows[rank][pos] is not below n",
                                      "its log row is claimed by two runs of events (rows is not the split's)"};
  char msg[160];
  snprintf(msg, sizeof msg, "%s: rank %u, event %llu: %s", who, (unsigned)(key >> 34),
           (unsigned long long)((key >> 2) & 0xFFFFFFFFull), what[key & 3]);
  return set_err(CC_ERR_INVALID, msg);
}

}  // namespace cc

extern "C" int cc_merge_events(const cc_events* parts, const uint64_t* const* rows, const uint64_t* row_counts, uint64_t n,
                               uint32_t world, uint32_t threads, const cc_events* out, uint64_t* total) {
  using cc::set_err;
  if (world == 0 || world > 256) return set_err(CC_ERR_INVALID, "merge events: world must be in [1, 256]");
  if (n >= (1ull << 32)) return set_err(CC_ERR_INVALID, "merge events: n must be below 2^32 (pos is 32 bits wide)");
  if (!parts || !rows || !row_counts || !out || !total) return set_err(CC_ERR_INVALID, "merge events: null argument");
  if (n == 0) {
    *total = 0;
    if (out->count) *out->count = 0;
    return CC_OK;
  }
  std::vector<Part> P(world);
  uint64_t sum = 0;
  bool over = false;
  for (uint32_t r = 0; r < world; ++r) {
    const cc_events& e = parts[r];
    const uint64_t c = e.count ? *e.count : 0;
    P[r] = Part{e.pos, e.target, e.code, e.src, e.tag, e.payload, rows[r], c, row_counts[r]};
    if (row_counts[r] > n) return set_err(CC_ERR_INVALID, "merge events: a rank's row count exceeds n");
    over |= c > e.capacity;
    sum += c;
  }
  *total = sum;
  if (over) return set_err(CC_ERR_CAPACITY, "merge events: a part holds more events than its capacity (that rank's apply overflowed)");
  for (uint32_t r = 0; r < world; ++r) {
    const Part& p = P[r];
    if (p.count >= (1ull << 32)) return set_err(CC_ERR_INVALID, "merge events: a part's count must be below 2^32");
    if (p.count && (!p.pos || !p.target || !p.code || !p.src || !p.tag || !p.payload || !p.rows))
      return set_err(CC_ERR_INVALID, "merge events: null column in a part that holds events");
  }
  if (sum >= (1ull << 32)) return set_err(CC_ERR_INVALID, "merge events: the total must be below 2^32");
  uint32_t T = threads ? threads : std::max(1u, std::thread::hardware_concurrency());
  T = std::min<uint32_t>(T, 256);
  const uint64_t blocks = (n + kBlock - 1) / kBlock;
  T = (uint32_t)std::min<uint64_t>(T, std::max<uint64_t>(1, std::max(blocks, sum / (2 * kBlock))));  // a block or 16 Ki events each
  std::atomic<uint64_t> err{kNoErr};
  // 0. every event, in T slices per rank
  parallel(T, [&](uint32_t t) {
    for (uint32_t r = 0; r < world; ++r) {
      const Part& p = P[r];
      const uint64_t lo = p.count * t / T, hi = p.count * (t + 1) / T;
      for (uint64_t j = lo; j < hi; ++j) {
        const uint32_t x = p.pos[j];
        uint32_t kind;
        if (x >= p.row_count) kind = cc::kEvmPosRange;
        else if (j && p.pos[j - 1] > x) kind = cc::kEvmPosOrder;
        else if (p.rows[x] >= n) kind = cc::kEvmRowRange;
        else continue;
        note(err, cc::evmerge_key(r, j, kind));
        break;  // (a later event of this slice has a larger key)
      }
    }
  });
  if (err.load() != kNoErr) return cc::evmerge_fail("merge events", err.load());
  // 1. the blocks' event counts
  std::vector<uint64_t> bsum(blocks + 1, 0);
  parallel(T, [&](uint32_t t) {
    std::vector<uint32_t> first(kBlock), cnt(kBlock);
    for (uint64_t b = blocks * t / T; b < blocks * (t + 1) / T; ++b) {
      const uint64_t b0 = b * kBlock, b1 = std::min<uint64_t>(n, b0 + kBlock);
      const uint64_t s = block_tables(P, b0, b1, first.data(), cnt.data(), err);
      if (s == kNoErr) return;
      bsum[b] = s;
    }
  });
  if (err.load() != kNoErr) return cc::evmerge_fail("merge events", err.load());
  // 2. exclusive prefix
  uint64_t run = 0;
  for (uint64_t b = 0; b <= blocks; ++b) {
    const uint64_t s = bsum[b];
    bsum[b] = run;
    run += s;
  }
  if (run != sum) return set_err(CC_ERR_INVALID, "merge events: the rows' runs do not add up to the events (rows is not increasing)");
  if (sum > out->capacity) return set_err(CC_ERR_CAPACITY, "merge events: the output stream is too small");
  if (sum && (!out->pos || !out->target || !out->code || !out->src || !out->tag || !out->payload))
    return set_err(CC_ERR_INVALID, "merge events: null output column");
  // 3. copy
  parallel(T, [&](uint32_t t) {
    std::vector<uint32_t> first(kBlock), off(kBlock);
    for (uint64_t b = blocks * t / T; b < blocks * (t + 1) / T; ++b) {
      if (bsum[b + 1] == bsum[b]) continue;
      const uint64_t b0 = b * kBlock, b1 = std::min<uint64_t>(n, b0 + kBlock);
      block_tables(P, b0, b1, first.data(), off.data(), err);
      uint32_t s = 0;
      for (uint64_t i = 0; i < b1 - b0; ++i) {
        const uint32_t c = off[i];
        off[i] = s;
        s += c;
      }
      for (uint32_t r = 0; r < world; ++r) {
        const Part& p = P[r];
        uint64_t ea, eb;
        block_range(p, b0, b1, ea, eb);
        for (uint64_t j = ea; j < eb; ++j) {
          const uint64_t row = p.rows[p.pos[j]];
          const uint64_t d = bsum[b] + off[row - b0] + (j - first[row - b0]);
          out->pos[d] = (uint32_t)row;
          out->target[d] = p.target[j];
          out->code[d] = p.code[j];
          out->src[d] = p.src[j];
          out->tag[d] = p.tag[j];
          out->payload[d] = p.payload[j];
        }
      }
    }
  });
  if (out->count) *out->count = sum;
  return CC_OK;
}
