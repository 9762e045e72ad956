// respack_fuzz.cpp — copycat_amd/csrc/respack.cpp under AddressSanitizer + UndefinedBehaviorSanitizer (host only; see
// tests/test_respack_asan.py).
//
//   1. random result columns (every width the encoder can choose, values around zero, 0 .. 3 blocks) are packed into an
//      exact-size buffer, validated, decoded into exact-size columns and compared byte for byte;
//   2. `iterations` mutated blobs (byte flips, boundary values in directory fields, truncations, directory entries
//      spliced from another block or blob) go to cc_respack_check and cc_respack_unpack, each from an exact-size heap
//      copy, the output columns sized exactly by the n the validator reports: an accepted blob that reads outside its
//      bytes or writes outside n rows is a sanitizer report.  Every input must come back CC_OK or CC_ERR_INVALID.
//
// usage: respack_fuzz [iterations = 100000] [seed = 1]
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/copycat_apply.h"

namespace cc {
int pack_err(int code, const char*) { return code; }  // the engine's cc_last_error store is not linked
}

namespace {

uint64_t g_state = 1;
uint64_t rnd() {  // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
uint64_t below(uint64_t n) { return n ? rnd() % n : 0; }

[[noreturn]] void die(const char* what) {
  std::fprintf(stderr, "respack_fuzz: %s\n", what);
  std::exit(2);
}

void* exact(size_t bytes) {  // 16-byte aligned, not one byte longer (a zero-size request still gets a pointer)
  void* p = nullptr;
  if (posix_memalign(&p, 16, bytes ? bytes : 1)) die("out of memory");
  return p;
}

struct Rows {
  uint8_t* status;
  uint64_t* value;
  explicit Rows(uint64_t n) : status((uint8_t*)exact(n)), value((uint64_t*)exact(8 * n)) {}
  ~Rows() {
    std::free(status);
    std::free(value);
  }
  Rows(const Rows&) = delete;
  cc_results res() const { return cc_results{status, value}; }
};

// one block in a random style: statuses constant or random; values constant or a span of 1 / 2 / 4 / 8 bytes from a
// random base, which may sit just below zero (the signed base)
void fill(Rows& r, uint64_t lo, uint64_t hi) {
  const int style = (int)below(5);
  const uint64_t span = style == 0 ? 0 : style == 1 ? 0xFF : style == 2 ? 0xFFFF : style == 3 ? 0xFFFFFFFFull : ~0ull;
  uint64_t base = rnd();
  if (below(3) == 0) base = (uint64_t)0 - below(span / 2 + 2);
  const bool flat = below(2) == 0;
  const uint8_t st = (uint8_t)rnd();
  for (uint64_t i = lo; i < hi; ++i) {
    r.value[i] = base + (span == ~0ull ? rnd() : below(span + 1));
    r.status[i] = flat ? st : (uint8_t)rnd();
  }
}

struct Blob {
  uint8_t* p = nullptr;
  uint64_t bytes = 0;
};

Blob pack_random(uint64_t n, uint32_t threads) {
  Rows c(n);
  for (uint64_t lo = 0; lo < n; lo += CC_PACK_BLOCK_ROWS) fill(c, lo, lo + CC_PACK_BLOCK_ROWS < n ? lo + CC_PACK_BLOCK_ROWS : n);
  const cc_results in = c.res();
  uint64_t need = 0, bound = 0, got = 0;
  if (cc_respack_bound(n, &bound) != CC_OK) die("cc_respack_bound failed");
  if (cc_respack_pack(&in, n, nullptr, 0, threads, &need) != CC_ERR_CAPACITY) die("a zero capacity was not refused");
  if (need > bound) die("the blob is larger than cc_respack_bound");
  Blob b{(uint8_t*)exact(need), need};
  if (need > 64) {  // one byte short: refused, and not a byte written (an exact-size buffer: a write is a report)
    Blob s{(uint8_t*)exact(need - 1), need - 1};
    std::memset(s.p, 0xEE, (size_t)s.bytes);
    if (cc_respack_pack(&in, n, s.p, s.bytes, threads, &got) != CC_ERR_CAPACITY || got != need) die("a short capacity was not refused");
    for (uint64_t i = 0; i < s.bytes; ++i)
      if (s.p[i] != 0xEE) die("a refused encode wrote into the buffer");
    std::free(s.p);
  }
  if (cc_respack_pack(&in, n, b.p, need, threads, &got) != CC_OK || got != need) die("cc_respack_pack failed at the exact size");
  uint64_t n2 = ~0ull;
  if (cc_respack_check(b.p, b.bytes, &n2) != CC_OK || n2 != n) die("a fresh blob does not validate");
  Rows d(n);
  const cc_results out = d.res();
  if (cc_respack_unpack(b.p, b.bytes, &out, threads) != CC_OK) die("a fresh blob does not decode");
  if (n && (std::memcmp(c.status, d.status, n) || std::memcmp(c.value, d.value, 8 * n))) die("round trip differs");
  return b;
}

void put(uint8_t* p, uint64_t v, int bytes) { std::memcpy(p, &v, (size_t)bytes); }

uint64_t boundary() {
  static const uint64_t k[] = {0, 1, 2, 3, 4, 8, 9, 15, 16, 17, 255, 256, 4095, 4096, 4097, 65535, 65536,
                               0x7FFFFFFFull, 0x80000000ull, 0xFFFFFFFFull, 0x100000000ull, ~0ull, ~0ull - 15, 1ull << 63};
  return k[below(sizeof k / sizeof k[0])];
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t iterations = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 100000;
  g_state = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1;
  // the seeds: mostly one small block (cheap to copy and decode 100,000 times), a few with a tail and 2 - 3 blocks
  std::vector<Blob> seeds;
  const uint64_t sizes[] = {0, 1, 2, 15, 16, 17, 33, 100, 255, 300, 4095, 4096, 4097, 2 * 4096 + 77};
  uint64_t packed = 0;
  for (int rep = 0; rep < 6; ++rep)
    for (uint64_t n : sizes) {
      seeds.push_back(pack_random(n, 1 + (uint32_t)below(4)));
      ++packed;
    }
  std::vector<size_t> cheap, dear;
  for (size_t i = 0; i < seeds.size(); ++i) (seeds[i].bytes <= 4096 ? cheap : dear).push_back(i);

  uint64_t ok = 0, invalid = 0;
  for (uint64_t it = 0; it < iterations; ++it) {
    const Blob& s = below(50) == 0 && !dear.empty() ? seeds[dear[below(dear.size())]] : seeds[cheap[below(cheap.size())]];
    uint64_t bytes = s.bytes;
    const int kind = (int)below(8);
    if (kind == 0) bytes = below(s.bytes + 1);                                      // truncation
    if (kind == 1 && s.bytes > 64) bytes = 64 + below(s.bytes - 64 + 1) / 16 * 16;  // ... at a 16-byte boundary
    uint8_t* m = (uint8_t*)exact(bytes);
    std::memcpy(m, s.p, (size_t)bytes);
    cc_pack_header h{};
    if (bytes >= sizeof h) std::memcpy(&h, m, sizeof h);
    const uint64_t dir_bytes = bytes >= sizeof h ? (h.blocks <= 4 ? h.blocks : 4) * sizeof(cc_respack_block) : 0;
    const uint64_t meta = bytes < sizeof h + dir_bytes ? bytes : sizeof h + dir_bytes;  // header + directory
    if (kind == 1 && bytes >= sizeof h) put(m + offsetof(cc_pack_header, bytes), bytes, 8);  // (a consistent total)
    if (kind == 2 || kind == 3)  // byte flips, mostly in the header and the directory
      for (uint64_t f = 1 + below(4); f-- && bytes;) {
        const uint64_t at = below(4) && meta ? below(meta) : below(bytes);
        m[at] ^= (uint8_t)(1u << below(8));
      }
    if (kind == 4 && meta)  // a random byte
      m[below(meta)] = (uint8_t)rnd();
    if ((kind == 5 || kind == 6) && meta >= 8) {  // a boundary value in an aligned field of the header / directory
      const int w = 1 << below(4);
      const uint64_t at = below(meta - (uint64_t)w + 1) / (uint64_t)w * (uint64_t)w;
      put(m + at, boundary() + (below(2) ? 0 : below(3) - 1), w);
    }
    if (kind == 7 && dir_bytes) {  // a directory entry (or one column's entry) of another block or blob
      const Blob& o = seeds[below(seeds.size())];
      cc_pack_header oh;
      std::memcpy(&oh, o.p, sizeof oh);
      if (oh.blocks && sizeof h + dir_bytes <= bytes) {
        const uint64_t from = sizeof oh + below(oh.blocks) * sizeof(cc_respack_block);
        const uint64_t to = sizeof h + below(dir_bytes / sizeof(cc_respack_block)) * sizeof(cc_respack_block);
        if (below(2)) {
          std::memcpy(m + to, o.p + from, sizeof(cc_respack_block));
        } else {
          const uint64_t c = 16 + 16 * below(2), c2 = 16 + 16 * below(2);
          std::memcpy(m + to + c, o.p + from + c2, sizeof(cc_pack_col));
        }
      }
    }
    uint64_t n = 0;
    const int rc = cc_respack_check(m, bytes, &n);
    if (rc == CC_OK) {
      ++ok;
      Rows d(n);
      const cc_results out = d.res();
      if (cc_respack_unpack(m, bytes, &out, 1 + (uint32_t)below(3)) != CC_OK) die("an accepted blob does not decode");
    } else if (rc == CC_ERR_INVALID) {
      ++invalid;
      Rows d(16);
      const cc_results out = d.res();
      if (cc_respack_unpack(m, bytes, &out, 1) != CC_ERR_INVALID) die("the decoder took a blob the validator refused");
    } else {
      die("cc_respack_check returned neither CC_OK nor CC_ERR_INVALID");
    }
    std::free(m);
  }
  for (Blob& b : seeds) std::free(b.p);
  std::printf("packed %llu result sets; checked %llu mutated blobs: %llu accepted, %llu refused\n", (unsigned long long)packed,
              (unsigned long long)iterations, (unsigned long long)ok, (unsigned long long)invalid);
  return ok + invalid == iterations ? 0 : 1;
}
