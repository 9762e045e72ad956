// wire_chunk_fuzz.cpp — host-only check of the chunk planner of cc_apply_wire_host_packed (copycat_amd/csrc/wire.cpp
// wire_plan_chunks), built with -fsanitize=address,undefined by tests/test_wire_chunks.py (test infrastructure; never
// part of the product library).
//
// Over seeded random offset arrays (well-formed ones with entries of very different sizes, and ones with a decreasing
// offset, an offset past the buffer, or garbage), random chunk sizes and byte caps, the plan must satisfy:
//   1. every cut is a multiple of CC_PACK_BLOCK_ROWS rows, except the segment's end;
//   2. the chunks cover [0, n) once and in order, none empty, none longer than the chunk size;
//   3. the bytes a chunk copies, offsets[lo + send] - offsets[lo], are at most the cap unless the chunk is one block;
//   4. `ok` is the end-offset check, a chunk with no violation inside passes it, and what a chunk copies lies inside
//      the buffer: with ok, all of [offsets[lo], offsets[hi]); without, the rows before the first violation a full
//      scan finds, which is `send`.
// Every offsets array is an exact-size heap allocation, so the sanitizer sees any read past offsets[n].
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "engine_state.h"

namespace cc {
int set_err(int code, const char*, hipError_t) { return code; }  // the engine's cc_last_error store is not linked
}  // namespace cc
extern "C" int cc_handle_hashes(cc_engine*, const uint64_t*, const int32_t*, uint64_t) { return CC_OK; }

namespace {
uint64_t g_rng = 0x13198A2E03707344ull;
uint64_t rnd() {  // splitmix64
  uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

uint64_t full_scan(const uint64_t* off, uint64_t rows, uint64_t buf_len) {  // written again here, on purpose
  uint64_t i = 0;
  while (i < rows && off[i + 1] >= off[i] && off[i + 1] <= buf_len) ++i;
  return i;
}

#define REQUIRE(c)                                                                                         \
  do {                                                                                                     \
    if (!(c)) {                                                                                            \
      fprintf(stderr, "case %llu: %s (n %llu chunk %llu cap %llu buf_len %llu, chunk [%llu, %llu) send %llu ok %d)\n", \
              (unsigned long long)it, #c, (unsigned long long)n, (unsigned long long)chunk_rows,           \
              (unsigned long long)cap, (unsigned long long)buf_len, (unsigned long long)c_.lo,             \
              (unsigned long long)c_.hi, (unsigned long long)c_.send, (int)c_.ok);                         \
      return 1;                                                                                            \
    }                                                                                                      \
  } while (0)
}  // namespace

int main(int argc, char** argv) {
  const uint64_t cases = argc > 1 ? strtoull(argv[1], nullptr, 10) : 2000;
  const uint64_t kB = CC_PACK_BLOCK_ROWS;
  uint64_t bad_cases = 0, capped = 0, single_over = 0, chunks_total = 0, not_ok = 0;
  for (uint64_t it = 0; it < cases; ++it) {
    const uint64_t n = 1 + rnd() % (it % 8 == 0 ? 40 * kB : 6 * kB);
    uint64_t* off = (uint64_t*)malloc(8 * (n + 1));
    // a well-formed array: mostly small entries, sometimes runs of large ones and single huge ones
    off[0] = rnd() % 64;
    const uint32_t shape = (uint32_t)(rnd() % 4);
    for (uint64_t i = 0; i < n; ++i) {
      uint64_t len = 20 + rnd() % 50;
      if (shape == 1 && (i / 512) % 3 == 0) len = 2000 + rnd() % 4000;
      if (shape == 2 && rnd() % 3000 == 0) len = 1ull << (20 + rnd() % 14);
      if (shape == 3) len = rnd() % 3 ? 0 : 34;
      off[i + 1] = off[i] + len;
    }
    uint64_t buf_len = off[n] + rnd() % 16;
    // the violations
    const uint32_t kind = (uint32_t)(rnd() % 6);
    const uint64_t at = 1 + rnd() % n;  // an offset other than the first
    if (kind == 1) off[at] = off[at - 1] - 1 - rnd() % 8;                   // decreasing (may wrap below zero)
    if (kind == 2) off[at] = buf_len + 1 + rnd() % 1000;                     // past the end
    if (kind == 3) off[at / kB * kB] = rnd();                                // garbage at a block boundary
    if (kind == 4) for (int j = 0; j < 5; ++j) off[rnd() % (n + 1)] = rnd() >> (rnd() % 60);
    if (kind == 5) buf_len = off[n] ? off[n] - 1 - rnd() % off[n] : 0;       // the buffer is shorter than the offsets say
    const uint64_t chunk_rows = kB * (1 + rnd() % 8);
    const uint64_t cap = rnd() % 4 == 0 ? 1ull << 30 : 4096 + rnd() % (400 * 1024);
    std::vector<cc::WireChunk> plan;
    cc::wire_plan_chunks(off, n, buf_len, chunk_rows, cap, &plan);
    uint64_t pos = 0;
    const bool clean = full_scan(off, n, buf_len) == n;
    if (!clean) ++bad_cases;
    cc::WireChunk c_{};
    REQUIRE(!plan.empty());
    for (const cc::WireChunk& c : plan) {
      c_ = c;
      ++chunks_total;
      REQUIRE(c.lo == pos && c.hi > c.lo && c.hi <= n);        // 2
      REQUIRE(c.hi - c.lo <= chunk_rows);
      REQUIRE(c.lo % kB == 0 && (c.hi % kB == 0 || c.hi == n));  // 1
      const uint64_t rows = c.hi - c.lo;
      const bool ends = off[c.lo] <= off[c.hi] && off[c.hi] <= buf_len;
      const uint64_t first_bad = full_scan(off + c.lo, rows, buf_len);
      REQUIRE(c.ok == ends);                                   // 4
      if (first_bad == rows) REQUIRE(c.ok);
      REQUIRE(c.send <= rows);
      if (c.ok) {
        REQUIRE(c.send == rows);
      } else {
        ++not_ok;
        REQUIRE(c.send == first_bad && c.send < rows);
      }
      // the copy stays inside the buffer (no row to send: no byte is copied, wherever offsets[lo] points)
      if (c.send) REQUIRE(off[c.lo] <= off[c.lo + c.send] && off[c.lo + c.send] <= buf_len);
      const uint64_t span = off[c.lo + c.send] - off[c.lo];
      if (c.send && span > cap) {                                        // 3
        REQUIRE(rows <= kB);
        ++single_over;
      }
      if (rows < chunk_rows && c.hi != n) ++capped;
      pos = c.hi;
    }
    REQUIRE(pos == n);
    free(off);
  }
  printf("cases=%llu bad_cases=%llu chunks=%llu capped=%llu single_over=%llu not_ok=%llu\n", (unsigned long long)cases,
         (unsigned long long)bad_cases, (unsigned long long)chunks_total, (unsigned long long)capped,
         (unsigned long long)single_over, (unsigned long long)not_ok);
  return 0;
}
