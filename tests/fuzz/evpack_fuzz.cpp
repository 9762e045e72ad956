// evpack_fuzz.cpp — copycat_amd/csrc/evpack.cpp under AddressSanitizer + UndefinedBehaviorSanitizer (host only; see
// tests/test_evpack_asan.py).
//
//   1. random event columns (every width the encoder can choose, fan-outs that take a payload table, payloads around
//      zero, 0 .. 3 blocks) are packed into an exact-size buffer, validated, decoded into exact-size columns and
//      compared byte for byte;
//   2. `iterations` mutated blobs (byte flips, boundary values in directory fields, truncations, directory entries
//      spliced from another block or blob, a table's entry count or the pos bytes under a table changed) go to
//      cc_evpack_check and cc_evpack_unpack, each from an exact-size heap copy, the output columns sized exactly by the
//      n the validator reports: an accepted blob that reads outside its bytes or writes outside n rows is a sanitizer
//      report.  Every input must come back CC_OK or CC_ERR_INVALID.
//
// usage: evpack_fuzz [iterations = 100000] [seed = 1]
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
  std::fprintf(stderr, "evpack_fuzz: %s\n", what);
  std::exit(2);
}

void* exact(size_t bytes) {  // 16-byte aligned, not one byte longer (a zero-size request still gets a pointer)
  void* p = nullptr;
  if (posix_memalign(&p, 16, bytes ? bytes : 1)) die("out of memory");
  return p;
}

struct Rows {
  uint64_t n;
  uint32_t *pos, *target;
  uint8_t *code, *src, *tag;
  uint64_t* payload;
  uint64_t count = ~0ull;
  explicit Rows(uint64_t n_)
      : n(n_), pos((uint32_t*)exact(4 * n_)), target((uint32_t*)exact(4 * n_)), code((uint8_t*)exact(n_)),
        src((uint8_t*)exact(n_)), tag((uint8_t*)exact(n_)), payload((uint64_t*)exact(8 * n_)) {}
  ~Rows() {
    std::free(pos), std::free(target), std::free(code), std::free(src), std::free(tag), std::free(payload);
  }
  Rows(const Rows&) = delete;
  cc_events ev() { return cc_events{pos, target, code, src, tag, payload, n, &count}; }
  bool same(const Rows& o) const {
    return !n || (!std::memcmp(pos, o.pos, 4 * n) && !std::memcmp(target, o.target, 4 * n) && !std::memcmp(code, o.code, n) &&
                  !std::memcmp(src, o.src, n) && !std::memcmp(tag, o.tag, n) && !std::memcmp(payload, o.payload, 8 * n));
  }
};

uint64_t span_of(int style) {
  return style == 0 ? 0 : style == 1 ? 0xFF : style == 2 ? 0xFFFF : style == 3 ? 0xFFFFFFFFull : ~0ull;
}

// one block in a random style: pos a fan-out (runs of equal rows with one payload each), sorted, random or constant;
// targets and payloads constant or a span of 1 / 2 / 4 / 8 bytes from a random base, which may sit just below zero
void fill(Rows& r, uint64_t lo, uint64_t hi) {
  const int pstyle = (int)below(4);
  const uint64_t per = 1 + below(below(2) ? 4 : 200);
  const uint64_t vspan = span_of((int)below(5)), tspan = span_of((int)below(4));
  uint64_t vbase = rnd();
  if (below(3) == 0) vbase = (uint64_t)0 - below(vspan / 2 + 2);
  const uint32_t tbase = (uint32_t)rnd(), pbase = (uint32_t)below(1u << 30);
  const bool flat = below(2) == 0;
  const uint8_t byte = (uint8_t)rnd();
  uint64_t run_payload = 0;
  uint32_t p = pbase;
  for (uint64_t i = lo; i < hi; ++i) {
    const uint64_t v = vbase + (vspan == ~0ull ? rnd() : below(vspan + 1));
    if (pstyle == 0) {
      if ((i - lo) % per == 0) run_payload = v, p += (uint32_t)(i == lo ? 0 : 1 + below(3));
      r.pos[i] = p, r.payload[i] = run_payload;
    } else {
      if (pstyle == 1) p += (uint32_t)below(20);
      r.pos[i] = pstyle == 1 ? p : pstyle == 2 ? (uint32_t)rnd() : 0xFFFFFFFFu;
      r.payload[i] = v;
    }
    r.target[i] = tbase + (uint32_t)below(tspan + 1);
    r.code[i] = flat ? byte : (uint8_t)rnd();
    r.src[i] = below(4) ? byte : (uint8_t)rnd();
    r.tag[i] = flat ? (uint8_t)(byte + 1) : (uint8_t)rnd();
  }
}

struct Blob {
  uint8_t* p = nullptr;
  uint64_t bytes = 0;
};

uint64_t g_tables = 0;  // blocks of the seeds whose payload went as a table

Blob pack_random(uint64_t n, uint32_t threads) {
  Rows c(n);
  for (uint64_t lo = 0; lo < n; lo += CC_PACK_BLOCK_ROWS) fill(c, lo, lo + CC_PACK_BLOCK_ROWS < n ? lo + CC_PACK_BLOCK_ROWS : n);
  cc_events in = c.ev();
  in.capacity = 0, in.count = nullptr;  // (the encoder takes the column pointers only)
  uint64_t need = 0, bound = 0, got = 0;
  if (cc_evpack_bound(n, &bound) != CC_OK) die("cc_evpack_bound failed");
  if (cc_evpack_pack(&in, n, nullptr, 0, threads, &need) != CC_ERR_CAPACITY) die("a zero capacity was not refused");
  if (need > bound) die("the blob is larger than cc_evpack_bound");
  Blob b{(uint8_t*)exact(need), need};
  if (need > 64) {  // one byte short: refused, and not a byte written (an exact-size buffer: a write is a report)
    Blob s{(uint8_t*)exact(need - 1), need - 1};
    std::memset(s.p, 0xEE, (size_t)s.bytes);
    if (cc_evpack_pack(&in, n, s.p, s.bytes, threads, &got) != CC_ERR_CAPACITY || got != need) die("a short capacity was not refused");
    for (uint64_t i = 0; i < s.bytes; ++i)
      if (s.p[i] != 0xEE) die("a refused encode wrote into the buffer");
    std::free(s.p);
  }
  if (cc_evpack_pack(&in, n, b.p, need, threads, &got) != CC_OK || got != need) die("cc_evpack_pack failed at the exact size");
  uint64_t n2 = ~0ull;
  if (cc_evpack_check(b.p, b.bytes, &n2) != CC_OK || n2 != n) die("a fresh blob does not validate");
  Rows d(n);
  const cc_events out = d.ev();
  if (cc_evpack_unpack(b.p, b.bytes, &out, threads) != CC_OK) die("a fresh blob does not decode");
  if (d.count != n) die("the decoder did not write the count");
  if (!c.same(d)) die("round trip differs");
  for (uint64_t k = 0; k * CC_PACK_BLOCK_ROWS < n; ++k) {
    cc_evpack_block e;
    std::memcpy(&e, b.p + sizeof(cc_pack_header) + k * sizeof e, sizeof e);
    g_tables += e.col[5].mode == CC_PK_BY_POS;
  }
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
  for (int rep = 0; rep < 8; ++rep)
    for (uint64_t n : sizes) {
      seeds.push_back(pack_random(n, 1 + (uint32_t)below(4)));
      ++packed;
    }
  if (!g_tables) die("no seed took a payload table");
  std::vector<size_t> cheap, dear;
  for (size_t i = 0; i < seeds.size(); ++i) (seeds[i].bytes <= 8192 ? cheap : dear).push_back(i);

  uint64_t ok = 0, invalid = 0;
  for (uint64_t it = 0; it < iterations; ++it) {
    const Blob& s = below(50) == 0 && !dear.empty() ? seeds[dear[below(dear.size())]] : seeds[cheap[below(cheap.size())]];
    uint64_t bytes = s.bytes;
    const int kind = (int)below(10);
    if (kind == 0) bytes = below(s.bytes + 1);                                      // truncation
    if (kind == 1 && s.bytes > 64) bytes = 64 + below(s.bytes - 64 + 1) / 16 * 16;  // ... at a 16-byte boundary
    uint8_t* m = (uint8_t*)exact(bytes);
    std::memcpy(m, s.p, (size_t)bytes);
    cc_pack_header h{};
    if (bytes >= sizeof h) std::memcpy(&h, m, sizeof h);
    const uint64_t dir_bytes = bytes >= sizeof h ? (h.blocks <= 4 ? h.blocks : 4) * sizeof(cc_evpack_block) : 0;
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
        const uint64_t from = sizeof oh + below(oh.blocks) * sizeof(cc_evpack_block);
        const uint64_t to = sizeof h + below(dir_bytes / sizeof(cc_evpack_block)) * sizeof(cc_evpack_block);
        if (below(2)) {
          std::memcpy(m + to, o.p + from, sizeof(cc_evpack_block));
        } else {
          const uint64_t c = 16 + 16 * below(6), c2 = 16 + 16 * below(6);
          std::memcpy(m + to + c, o.p + from + c2, sizeof(cc_pack_col));
        }
      }
    }
    if ((kind == 8 || kind == 9) && dir_bytes && sizeof h + dir_bytes <= bytes) {  // the table mode and what it leans on
      uint8_t* const e = m + sizeof h + below(dir_bytes / sizeof(cc_evpack_block)) * sizeof(cc_evpack_block);
      cc_evpack_block b;
      std::memcpy(&b, e, sizeof b);
      const int what = (int)below(5);
      if (what == 0) e[16 + 16 * below(6)] = CC_PK_BY_POS;                                  // the mode, on any column
      if (what == 1) put(e + 16 + 16 * 5 + 2, below(2) ? boundary() : below(b.col[5].reserved16 + 2), 2);  // the entries
      if (what == 2) e[16 + 1] = (uint8_t)(1u << below(4));                                 // the pos width under it
      if (what == 3) e[16 + 16 * 5] = CC_PK_BY_POS, put(e + 16 + 16 * 5 + 2, 1 + below(4096), 2);
      if (what == 4 && b.offset + b.col[0].offset < bytes) {  // a pos offset's byte under a table
        const uint64_t lo = b.offset + b.col[0].offset, len = (uint64_t)b.rows * b.col[0].width;
        if (len && lo + len <= bytes) m[lo + below(len)] = (uint8_t)(below(2) ? 0xFF : rnd());
      }
    }
    uint64_t n = 0;
    const int rc = cc_evpack_check(m, bytes, &n);
    if (rc == CC_OK) {
      ++ok;
      Rows d(n);
      const cc_events out = d.ev();
      if (cc_evpack_unpack(m, bytes, &out, 1 + (uint32_t)below(3)) != CC_OK) die("an accepted blob does not decode");
    } else if (rc == CC_ERR_INVALID) {
      ++invalid;
      Rows d(16);
      const cc_events out = d.ev();
      if (cc_evpack_unpack(m, bytes, &out, 1) != CC_ERR_INVALID) die("the decoder took a blob the validator refused");
    } else {
      die("cc_evpack_check returned neither CC_OK nor CC_ERR_INVALID");
    }
    std::free(m);
  }
  for (Blob& b : seeds) std::free(b.p);
  std::printf("packed %llu event streams (%llu blocks with a payload table); checked %llu mutated blobs: %llu accepted, %llu refused\n",
              (unsigned long long)packed, (unsigned long long)g_tables, (unsigned long long)iterations, (unsigned long long)ok,
              (unsigned long long)invalid);
  return ok + invalid == iterations ? 0 : 1;
}
