// pack_fuzz.cpp — copycat_amd/csrc/pack.cpp under AddressSanitizer + UndefinedBehaviorSanitizer (host only; see
// tests/test_pack_asan.py).
//
//   1. random batches (every width the encoder can choose, REL_A, absent columns, 0 .. 3 blocks) are packed into an
//      exact-size buffer, validated, decoded into exact-size columns and compared byte for byte;
//   2. `iterations` mutated blobs (byte flips, boundary values in directory fields, truncations, directory entries
//      spliced from another block or blob) go to cc_pack_check and cc_unpack_batch, each from an exact-size heap
//      copy, the output columns sized exactly by the n the validator reports: an accepted blob that reads outside
//      its bytes or writes outside n rows is a sanitizer report.  Every input must come back CC_OK or CC_ERR_INVALID.
//
// usage: pack_fuzz [iterations = 100000] [seed = 1]
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
  std::fprintf(stderr, "pack_fuzz: %s\n", what);
  std::exit(2);
}

void* exact(size_t bytes) {  // 16-byte aligned, not one byte longer (a zero-size request still gets a pointer)
  void* p = nullptr;
  if (posix_memalign(&p, 16, bytes ? bytes : 1)) die("out of memory");
  return p;
}

constexpr size_t kEsz[9] = {8, 8, 4, 1, 1, 8, 8, 8, 8};

struct Columns {
  void* col[9] = {};
  uint64_t n = 0;
  Columns(uint64_t rows, uint32_t present) : n(rows) {
    for (int c = 0; c < 9; ++c)
      if ((present >> c) & 1) col[c] = exact(rows * kEsz[c]);
  }
  ~Columns() {
    for (void* p : col) std::free(p);
  }
  Columns(const Columns&) = delete;
  cc_batch in() const {
    return cc_batch{(const uint64_t*)col[0], (const uint64_t*)col[1], (const uint32_t*)col[2],
                    (const uint8_t*)col[3],  (const uint8_t*)col[4],  (const uint64_t*)col[5],
                    (const uint64_t*)col[6], (const uint64_t*)col[7], (const uint64_t*)col[8]};
  }
  cc_batch_out out() const {
    return cc_batch_out{(uint64_t*)col[0], (uint64_t*)col[1], (uint32_t*)col[2], (uint8_t*)col[3], (uint8_t*)col[4],
                        (uint64_t*)col[5], (uint64_t*)col[6], (uint64_t*)col[7], (uint64_t*)col[8]};
  }
};

// one column of one block in a random style: constant, a span of 1 / 2 / 4 / 8 bytes from a random base (which may sit
// just below zero: the signed base), or b = a + a small signed step
void fill(Columns& c, int k, uint64_t lo, uint64_t hi) {
  const int style = (int)below(7);
  const uint64_t span = style == 0 ? 0 : style == 1 ? 0xFF : style == 2 ? 0xFFFF : style == 3 ? 0xFFFFFFFFull : ~0ull;
  uint64_t base = rnd();
  if (below(3) == 0) base = (uint64_t)0 - below(span / 2 + 2);
  const uint64_t step = style == 5 ? 0x7F : 0x7FFF;
  for (uint64_t i = lo; i < hi; ++i) {
    uint64_t v = base + (span == ~0ull ? rnd() : below(span + 1));
    if (style >= 5 && k == 7 && c.col[6]) v = ((const uint64_t*)c.col[6])[i] + below(2 * step + 2) - step - 1;
    if (kEsz[k] == 8) ((uint64_t*)c.col[k])[i] = v;
    else if (kEsz[k] == 4) ((uint32_t*)c.col[k])[i] = (uint32_t)v;
    else ((uint8_t*)c.col[k])[i] = (uint8_t)v;
  }
}

struct Blob {
  uint8_t* p = nullptr;
  uint64_t bytes = 0;
};

Blob pack_random(uint64_t n, uint32_t present, uint32_t threads) {
  Columns c(n, present);
  for (uint64_t lo = 0; lo < n; lo += CC_PACK_BLOCK_ROWS)
    for (int k = 0; k < 9; ++k)
      if (c.col[k]) fill(c, k, lo, lo + CC_PACK_BLOCK_ROWS < n ? lo + CC_PACK_BLOCK_ROWS : n);
  const cc_batch in = c.in();
  uint64_t need = 0, bound = 0, got = 0;
  if (cc_pack_bound(n, present, &bound) != CC_OK) die("cc_pack_bound failed");
  if (cc_pack_batch(&in, n, nullptr, 0, threads, &need) != CC_ERR_CAPACITY) die("a zero capacity was not refused");
  if (need > bound) die("the blob is larger than cc_pack_bound");
  Blob b{(uint8_t*)exact(need), need};
  if (need > 64) {  // one byte short: refused, and not a byte written (an exact-size buffer: a write is a report)
    Blob s{(uint8_t*)exact(need - 1), need - 1};
    std::memset(s.p, 0xEE, (size_t)s.bytes);
    if (cc_pack_batch(&in, n, s.p, s.bytes, threads, &got) != CC_ERR_CAPACITY || got != need) die("a short capacity was not refused");
    for (uint64_t i = 0; i < s.bytes; ++i)
      if (s.p[i] != 0xEE) die("a refused encode wrote into the buffer");
    std::free(s.p);
  }
  if (cc_pack_batch(&in, n, b.p, need, threads, &got) != CC_OK || got != need) die("cc_pack_batch failed at the exact size");
  uint64_t n2 = ~0ull;
  uint32_t p2 = ~0u;
  if (cc_pack_check(b.p, b.bytes, &n2, &p2) != CC_OK || n2 != n) die("a fresh blob does not validate");
  // (a zero-row batch's columns may all be absent: the encoder sees the pointers it is given)
  Columns d(n, p2);
  const cc_batch_out out = d.out();
  if (cc_unpack_batch(b.p, b.bytes, &out, threads) != CC_OK) die("a fresh blob does not decode");
  for (int k = 0; k < 9; ++k)
    if (c.col[k] && n && (!d.col[k] || std::memcmp(c.col[k], d.col[k], n * kEsz[k]))) die("round trip differs");
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
      uint32_t present = rep == 0 ? 0x1FF : (uint32_t)below(512);
      if (rep == 1) present = 0xDC | 1;  // a value batch: index, inst, op, flags, a, b
      seeds.push_back(pack_random(n, present, 1 + (uint32_t)below(4)));
      ++packed;
    }
  std::vector<size_t> cheap, dear;
  for (size_t i = 0; i < seeds.size(); ++i) (seeds[i].bytes <= 16384 ? cheap : dear).push_back(i);

  uint64_t ok = 0, invalid = 0;
  for (uint64_t it = 0; it < iterations; ++it) {
    const Blob& s = below(50) == 0 && !dear.empty() ? seeds[dear[below(dear.size())]] : seeds[cheap[below(cheap.size())]];
    uint64_t bytes = s.bytes;
    const int kind = (int)below(8);
    if (kind == 0) bytes = below(s.bytes + 1);                                   // truncation
    if (kind == 1 && s.bytes > 64) bytes = 64 + below(s.bytes - 64 + 1) / 16 * 16;  // ... at a 16-byte boundary
    uint8_t* m = (uint8_t*)exact(bytes);
    std::memcpy(m, s.p, (size_t)bytes);
    cc_pack_header h{};
    if (bytes >= sizeof h) std::memcpy(&h, m, sizeof h);
    const uint64_t dir_bytes = bytes >= sizeof h ? (h.blocks <= 4 ? h.blocks : 4) * sizeof(cc_pack_block) : 0;
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
        const uint64_t from = sizeof oh + below(oh.blocks) * sizeof(cc_pack_block);
        const uint64_t to = sizeof h + below(dir_bytes / sizeof(cc_pack_block)) * sizeof(cc_pack_block);
        if (below(2)) {
          std::memcpy(m + to, o.p + from, sizeof(cc_pack_block));
        } else {
          const uint64_t c = 16 + 16 * below(9), c2 = 16 + 16 * below(9);
          std::memcpy(m + to + c, o.p + from + c2, sizeof(cc_pack_col));
        }
      }
    }
    uint64_t n = 0;
    uint32_t present = 0;
    const int rc = cc_pack_check(m, bytes, &n, &present);
    if (rc == CC_OK) {
      ++ok;
      Columns d(n, present);
      const cc_batch_out out = d.out();
      if (cc_unpack_batch(m, bytes, &out, 1 + (uint32_t)below(3)) != CC_OK) die("an accepted blob does not decode");
    } else if (rc == CC_ERR_INVALID) {
      ++invalid;
      Columns d(16, 0x1FF);
      const cc_batch_out out = d.out();
      if (cc_unpack_batch(m, bytes, &out, 1) != CC_ERR_INVALID) die("the decoder took a blob the validator refused");
    } else {
      die("cc_pack_check returned neither CC_OK nor CC_ERR_INVALID");
    }
    std::free(m);
  }
  for (Blob& b : seeds) std::free(b.p);
  std::printf("packed %llu batches; checked %llu mutated blobs: %llu accepted, %llu refused\n", (unsigned long long)packed,
              (unsigned long long)iterations, (unsigned long long)ok, (unsigned long long)invalid);
  return ok + invalid == iterations ? 0 : 1;
}
