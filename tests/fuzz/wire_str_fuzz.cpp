// wire_str_fuzz.cpp — host-only check of the parser with a String dictionary (copycat_amd/csrc/wire_plain.h wire_parse
// over a DictView) against the host decoder (wire.cpp decode_one), built with -fsanitize=address,undefined by
// tests/test_wire_strings.py (test infrastructure; never part of the product library).  The dictionary is the host
// mirror (wire.cpp wire_dict_sync), whose image is what the device copies, read through the same DictView::find.
//
// Properties.  Conservative, on every input: the parser either escapes, or returns exactly decode_one's columns with
// CC_OK and the interner's count does not move.  Complete, on the fixture and on unmutated generated entries: when
// every String of an entry is interned, at most CC_WIRE_STR_MAX bytes long and (as a key) has its key bit, the entry
// must be resolved.  Coverage: at least a quarter of the unmutated generated entries are such entries and carry a
// String (a condition on the generator below, checked here).  Growth: interning from 0 to 5,000 Strings in steps,
// after every step each interned String resolves to its handle and an un-interned one misses.
// Built a second time with -DCC_WIRE_DICT_WEAK_HASH (the hash cut to 4 bits) every property must hold unchanged: nearly
// every probe then meets cells of equal hash and other bytes, so only the byte compare tells them apart.
// Each entry is parsed from a heap copy of exactly its bytes, so the sanitizer sees any overread.
//
// Two interners hold the same Strings in the same order: `in`, which the dictionary mirrors and nothing else touches,
// and `ref`, which decode_one interns into (an escaped entry's unknown Strings land there, past the common prefix, so
// the handles of the known ones agree).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "engine_state.h"
#include "wire_plain.h"

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
uint64_t n_resolved = 0, n_resolved_str = 0, n_escape = 0;
uint32_t g_sch[cc::kSchemaIds];
cc_wire_interner *g_in = nullptr, *g_ref = nullptr;
cc::WireDict g_dict;
std::map<uint64_t, int32_t> g_hh;  // the handles whose key bit is set
constexpr uint64_t kFirst = 1;

uint64_t count_of(cc_wire_interner* in) { return cc::wire_interner_info(in).count; }

// -> 1 resolved, 0 escape, -1 the property is broken; *strs = the Strings the parser resolved
int check(const cc_wire_codec& c, const std::vector<uint8_t>& bytes, unsigned* strs = nullptr) {
  uint8_t* buf = (uint8_t*)malloc(bytes.empty() ? 1 : bytes.size());  // exact size: one byte past it is an ASan report
  if (!bytes.empty()) memcpy(buf, bytes.data(), bytes.size());
  cc::PlainRow r{};
  const bool got = cc::wire_parse(cc::HostBytes{buf}, (uint32_t)bytes.size(), c, g_sch, g_dict.view(kFirst), r);
  uint8_t op = 0, flags = 0, kind = 0;
  uint64_t key = 0, a = 0, b = 0, aux = 0, iid = 0;
  cc_wire_out out{};
  out.iid = &iid, out.op = &op, out.flags = &flags, out.key = &key, out.a = &a, out.b = &b, out.aux = &aux, out.kind = &kind;
  const uint64_t before = count_of(g_ref);
  const int rc = cc::wire_decode_one(nullptr, c, g_ref, buf, buf + bytes.size(), 0, 0, &out);
  free(buf);
  if (strs) *strs = r.strs;
  if (!got) {
    ++n_escape;
    return 0;
  }
  ++n_resolved;
  if (r.strs) ++n_resolved_str;
  if (rc != CC_OK || kind != 0 || iid != r.iid || op != r.op || flags != r.flags || key != r.key || a != r.a || b != r.b ||
      aux != r.aux || count_of(g_ref) != before) {
    fprintf(stderr, "resolved row differs from decode_one (rc %d, interner %llu -> %llu, %zu bytes):", rc,
            (unsigned long long)before, (unsigned long long)count_of(g_ref), bytes.size());
    for (uint8_t x : bytes) fprintf(stderr, " %02x", x);
    fprintf(stderr, "\n");
    return -1;
  }
  return 1;
}

// ---- the String pool of the generator ----
enum Cls { KEYED, PLAIN_INTERNED, UNKNOWN, LONG_INTERNED };
struct PoolStr {
  std::string s;
  Cls cls;
};
std::vector<PoolStr> g_pool;
std::vector<size_t> g_by_cls[4];

void intern_both(const std::string& s, bool keyed) {
  uint64_t h0 = 0, h1 = 0;
  cc_wire_intern(g_in, (const uint8_t*)s.data(), s.size(), &h0);
  cc_wire_intern(g_ref, (const uint8_t*)s.data(), s.size(), &h1);
  if (h0 != h1) abort();
  if (keyed) g_hh[h0] = 0;
}

void build_pool() {
  // one long run of bytes with NULs and bytes >= 0x80: the pool holds its prefixes (prefixes of each other), copies
  // that differ only in the last byte, and random Strings of every length 0 .. CC_WIRE_STR_MAX + 1
  std::string base(CC_WIRE_STR_MAX + 40, '\0');
  for (auto& ch : base) ch = (char)(rnd() % 5 == 0 ? 0 : rnd() % 3 == 0 ? 0x80 + rnd() % 128 : 'a' + rnd() % 26);
  auto add = [&](const std::string& s) {
    for (const PoolStr& p : g_pool)
      if (p.s == s) return;
    Cls cls = s.size() > CC_WIRE_STR_MAX ? (rnd() & 1 ? LONG_INTERNED : UNKNOWN)
                                         : (rnd() % 10 < 7 ? KEYED : rnd() % 3 ? PLAIN_INTERNED : UNKNOWN);
    g_pool.push_back(PoolStr{s, cls});
  };
  for (uint32_t n : {0u, 1u, 2u, 3u, 4u, 7u, 8u, 9u, 15u, 16u, 17u, 23u, 24u, 25u, 63u, 64u, 65u, (uint32_t)CC_WIRE_STR_MAX - 1,
                     (uint32_t)CC_WIRE_STR_MAX, (uint32_t)CC_WIRE_STR_MAX + 1, (uint32_t)CC_WIRE_STR_MAX + 9}) {
    add(base.substr(0, n));
    if (n) {
      std::string t = base.substr(0, n);
      t[n - 1] = (char)(t[n - 1] ^ 0x01);
      add(t);
    }
  }
  for (uint32_t n = 0; n <= CC_WIRE_STR_MAX + 1; ++n) {
    std::string t(n, '\0');
    for (auto& ch : t) ch = (char)(rnd() % 7 == 0 ? 0 : rnd() % 4 == 0 ? 0x80 + rnd() % 128 : '0' + rnd() % 40);
    add(t);
  }
  for (size_t i = 0; i < g_pool.size(); ++i) {
    const PoolStr& p = g_pool[i];
    if (p.cls != UNKNOWN) intern_both(p.s, p.cls == KEYED);
    g_by_cls[p.cls].push_back(i);
  }
}

// an entry written under codec c: identifier widths at random (at least wide enough for the signed id)
void put_uint(std::vector<uint8_t>& o, const cc_wire_codec& c, uint64_t v, int n) {
  for (int i = 0; i < n; ++i) o.push_back((uint8_t)(v >> (8 * (c.big_endian ? n - 1 - i : i))));
}
void put_id(std::vector<uint8_t>& o, const cc_wire_codec& c, int64_t id) {
  int w = 1;
  while (w < 4 && (id < -(1ll << (8 * w - 1)) || id >= (1ll << (8 * w - 1)))) ++w;
  w += (int)(rnd() % (uint64_t)(5 - w));
  o.push_back((uint8_t)w);
  put_uint(o, c, (uint64_t)id, w);
}
struct Gen {           // what the generator knows of the entry it wrote
  bool sure = true;    // every part is one the parser with this dictionary must resolve
  unsigned strs = 0;   // non-null Strings written
};
// a String field; key: it is the entry's key
void put_string(std::vector<uint8_t>& o, const cc_wire_codec& c, bool key, Gen& g) {
  put_id(o, c, c.id_string);
  if (c.utf8_presence_byte) {
    const bool null = rnd() % 16 == 0;
    o.push_back(null ? 0 : (uint8_t)(1 + rnd() % 2));
    if (null) {
      if (key) g.sure = false;  // (a null key fails on the host; an optional one is allowed, but stay on the safe side)
      return;
    }
  }
  const unsigned pick = (unsigned)(rnd() % 20);
  const Cls cls = pick < 17 ? (key || rnd() % 4 ? KEYED : PLAIN_INTERNED) : pick == 17 ? (key ? PLAIN_INTERNED : UNKNOWN)
                : pick == 18 ? UNKNOWN : LONG_INTERNED;
  const PoolStr& p = g_pool[g_by_cls[cls][rnd() % g_by_cls[cls].size()]];
  const bool fits = c.utf8_len_bytes >= 2 || p.s.size() < 256;  // (a 1-byte length cannot carry 256 and more)
  const std::string s = fits ? p.s : p.s.substr(0, 255);
  if (!fits || cls == UNKNOWN || cls == LONG_INTERNED || (key && cls != KEYED)) g.sure = false;
  put_uint(o, c, s.size(), c.utf8_len_bytes);
  o.insert(o.end(), s.begin(), s.end());
  ++g.strs;
}
void put_value(std::vector<uint8_t>& o, const cc_wire_codec& c, bool key, Gen& g) {
  const unsigned k = (unsigned)(rnd() % 20);
  if (k < 12) return put_string(o, c, key, g);
  switch (k) {
    case 12: o.push_back(0), g.sure = g.sure && !key; break;
    case 13: case 14: put_id(o, c, c.id_long), put_uint(o, c, rnd() & 1 ? rnd() : (uint64_t)(int64_t)(rnd() % 5 - 2), 8); break;
    case 15: case 16: put_id(o, c, c.id_int), put_uint(o, c, rnd(), 4); break;
    case 17: case 18: put_id(o, c, c.id_bool), o.push_back((uint8_t)(rnd() % 3)); break;
    default: put_id(o, c, (int64_t)(rnd() % 300)), g.sure = false; break;  // some other registered type (or, by chance, one of ours)
  }
}
std::vector<uint8_t> gen(const cc_wire_codec& c, Gen& g) {
  std::vector<uint8_t> o;
  const bool top_ok = rnd() % 24 != 0, op_ok = rnd() % 24 != 0;
  put_id(o, c, top_ok ? 30 + (int64_t)(rnd() & 1) : (int64_t)(rnd() % 40));
  put_uint(o, c, rnd(), 8);
  const cc::Schema* s = nullptr;
  for (int tries = 0; tries < 8; ++tries) {  // mostly operations that carry a writeObject field
    s = &cc::kSchema[rnd() % (sizeof cc::kSchema / sizeof cc::kSchema[0])];
    bool carries = false;
    for (int k = 0; k < cc::kSchemaFields && s->f[k] != cc::F_END; ++k)
      carries = carries || (s->f[k] != cc::F_AUX && s->f[k] != cc::F_LKEY);
    if (carries) break;
  }
  put_id(o, c, op_ok ? (int64_t)s->op : (int64_t)(rnd() % 300));
  if (!top_ok || !op_ok) g.sure = false;
  for (int k = 0; k < cc::kSchemaFields && s->f[k] != cc::F_END; ++k) {
    if (s->f[k] == cc::F_AUX || s->f[k] == cc::F_LKEY) put_uint(o, c, rnd(), 8);
    else put_value(o, c, s->f[k] == cc::F_KEY || s->f[k] == cc::F_KEY_OPT, g);
  }
  // the four ids must tell the types apart for the generator's knowledge to hold
  const int32_t ids[4] = {c.id_bool, c.id_int, c.id_long, c.id_string};
  for (int i = 0; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j)
      if (ids[i] == ids[j]) g.sure = false;
  return o;
}

// interning 0 -> 5,000 Strings in steps: a dictionary of its own
int growth() {
  cc_wire_interner* in = nullptr;
  if (cc_wire_interner_create(7, &in) != CC_OK) return 2;
  cc::WireDict d;
  std::map<uint64_t, int32_t> hh;
  std::vector<std::string> strs;
  auto name = [](uint64_t i) {
    std::string s = "key-" + std::to_string(i * 2654435761ull % 1000003);
    if (i % 5 == 0) s += std::string(i % 97, (char)('a' + i % 26));  // (mixed lengths, up to 100 and more)
    if (i % 11 == 0) s.push_back('\0');
    return s;
  };
  uint64_t cells_before = 0, doublings = 0;
  for (uint64_t target : {0ull, 1ull, 2ull, 31ull, 32ull, 33ull, 100ull, 1000ull, 1024ull, 2500ull, 5000ull}) {
    while (strs.size() < target) {
      strs.push_back(name(strs.size()));
      uint64_t h = 0;
      cc_wire_intern(in, (const uint8_t*)strs.back().data(), strs.back().size(), &h);
      if (h != 7 + strs.size() - 1) return 1;  // (the names are distinct)
      if (strs.size() % 3 == 0) hh[h] = 0;
    }
    cc::wire_dict_sync(d, in, hh, false);
    if (d.cells.size() != cells_before) ++doublings, cells_before = d.cells.size();
    if (d.strings != strs.size() || 2 * d.strings > d.cells.size() || (d.cells.size() & (d.cells.size() - 1))) {
      fprintf(stderr, "growth: %llu strings in %zu cells\n", (unsigned long long)d.strings, d.cells.size());
      return 1;
    }
    const cc::DictView v = d.view(7);
    for (uint64_t i = 0; i <= strs.size(); ++i) {  // i == size: the next name, not interned yet
      const std::string s = i < strs.size() ? strs[i] : name(i);
      uint8_t* buf = (uint8_t*)malloc(s.empty() ? 1 : s.size());
      if (!s.empty()) memcpy(buf, s.data(), s.size());
      uint32_t rank = ~0u;
      bool reg = false;
      const bool hit = v.find(cc::HostBytes{buf}, 0, (uint32_t)s.size(), rank, reg);
      free(buf);
      const bool want = i < strs.size();
      if (hit != want || (hit && (rank != i || reg != ((i + 1) % 3 == 0)))) {
        fprintf(stderr, "growth: at %llu of %zu: hit %d rank %u key bit %d\n", (unsigned long long)i, strs.size(), hit, rank, reg);
        return 1;
      }
    }
  }
  cc_wire_interner_destroy(in);
  if (doublings < 5 || cells_before != 16384) {
    fprintf(stderr, "growth: the table doubled only %llu times\n", (unsigned long long)doublings);
    return 1;
  }
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 5) {
    fprintf(stderr, "usage: wire_str_fuzz FIXTURE.bin OFFSETS.txt STRINGS.bin ITERATIONS\n");
    return 2;
  }
  auto slurp = [](const char* path, std::vector<uint8_t>& out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    for (int ch; (ch = fgetc(f)) != EOF;) out.push_back((uint8_t)ch);
    fclose(f);
    return true;
  };
  std::vector<uint8_t> blob, sblob;
  if (!slurp(argv[1], blob) || !slurp(argv[3], sblob)) return 2;
  std::vector<uint64_t> off;
  FILE* g = fopen(argv[2], "r");
  if (!g) return 2;
  for (unsigned long long x; fscanf(g, "%llu", &x) == 1;) off.push_back(x);
  fclose(g);
  const long iters = atol(argv[4]);
  cc::schema_words(g_sch);
  if (cc_wire_interner_create(kFirst, &g_in) != CC_OK || cc_wire_interner_create(kFirst, &g_ref) != CC_OK) return 2;
  cc_wire_codec def;
  cc_wire_codec_default(&def);

  // the fixture's Strings (STRINGS.bin: a 4-byte little-endian length, then the bytes, for each), all with a key bit
  for (size_t at = 0; at + 4 <= sblob.size();) {
    uint32_t n = 0;
    memcpy(&n, sblob.data() + at, 4);
    intern_both(std::string((const char*)sblob.data() + at + 4, n), true);
    at += 4 + n;
  }
  build_pool();
  cc::wire_dict_sync(g_dict, g_in, g_hh, false);
  if (g_dict.strings + g_dict.long_strings != count_of(g_in) || g_dict.long_strings == 0) return 2;

  std::vector<std::vector<uint8_t>> ents;
  for (size_t i = 0; i + 1 < off.size(); ++i) ents.emplace_back(blob.begin() + off[i], blob.begin() + off[i + 1]);
  uint64_t fixture_resolved = 0, fixture_str = 0;
  for (auto& e : ents) {
    unsigned strs = 0;
    const int r = check(def, e, &strs);
    if (r < 0) return 1;
    fixture_resolved += (uint64_t)r;
    fixture_str += r > 0 && strs;
  }
  for (auto& e : ents)  // every truncation of every entry
    for (size_t n = 0; n < e.size(); ++n)
      if (check(def, std::vector<uint8_t>(e.begin(), e.begin() + n)) < 0) return 1;
  uint64_t plain_gen = 0, sure = 0, sure_str = 0, mutated_resolved = 0;
  for (long it = 0; it < iters; ++it) {
    cc_wire_codec c = def;
    if (rnd() % 4) {  // random codec parameters
      c.big_endian = rnd() & 1;
      c.utf8_presence_byte = rnd() & 1;
      c.utf8_len_bytes = 1 + (uint8_t)(rnd() % 8);
      int32_t* ids[4] = {&c.id_bool, &c.id_int, &c.id_long, &c.id_string};
      for (int32_t* id : ids)
        if (rnd() & 1) *id = rnd() % 3 == 0 ? (int32_t)rnd() : (int32_t)(rnd() % 300) - 20;  // (may coincide)
    }
    Gen gi;
    const bool generated = rnd() % 4 != 0;
    std::vector<uint8_t> x = generated ? gen(c, gi) : ents[rnd() % ents.size()];
    const unsigned how = (unsigned)(rnd() % 9);
    switch (how) {
      case 0: {  // byte flips
        const int k = 1 + (int)(rnd() % 4);
        for (int j = 0; j < k && !x.empty(); ++j) x[rnd() % x.size()] ^= (uint8_t)(1 + rnd() % 255);
        break;
      }
      case 1: {  // splice: a prefix of one entry + a suffix of another
        Gen other;
        const auto y = rnd() & 1 ? gen(c, other) : ents[rnd() % ents.size()];
        x.resize(x.empty() ? 0 : rnd() % x.size());
        const size_t from = y.empty() ? 0 : rnd() % y.size();
        x.insert(x.end(), y.begin() + from, y.end());
        break;
      }
      case 2: {  // truncation or trailing bytes
        if (rnd() & 1) x.resize(x.empty() ? 0 : rnd() % x.size());
        else for (int j = 1 + (int)(rnd() % 9); j > 0; --j) x.push_back((uint8_t)rnd());
        break;
      }
      case 3: {  // garbage
        x.resize(rnd() % 80);
        for (auto& b : x) b = (uint8_t)rnd();
        break;
      }
      case 4: {  // 0xFF runs (a length field among them)
        if (!x.empty()) {
          const size_t at = rnd() % x.size();
          for (size_t j = at; j < x.size() && j < at + 8; ++j) x[j] = 0xFF;
        }
        break;
      }
      default: break;  // as generated
    }
    unsigned strs = 0;
    const int r = check(c, x, &strs);
    if (r < 0) return 1;
    if (how < 5) {
      mutated_resolved += (uint64_t)r;
    } else if (generated) {
      ++plain_gen;
      if (gi.sure) {
        ++sure;
        if (gi.strs) ++sure_str;
        if (r != 1 || strs != gi.strs) {
          fprintf(stderr, "an entry whose Strings the dictionary holds was not resolved (%u of %u Strings, %zu bytes):", strs,
                  gi.strs, x.size());
          for (uint8_t b : x) fprintf(stderr, " %02x", b);
          fprintf(stderr, "\n");
          return 1;
        }
      }
    }
  }
  if (4 * sure_str < plain_gen) {
    fprintf(stderr, "the generator falls short: %llu of %llu unmutated generated entries are resolvable and carry a String\n",
            (unsigned long long)sure_str, (unsigned long long)plain_gen);
    return 1;
  }
  if (count_of(g_in) != g_dict.cell_of.size()) return 1;  // (nothing but the set-up interned into the mirrored interner)
  if (growth()) return 1;
  cc_wire_interner_destroy(g_in);
  cc_wire_interner_destroy(g_ref);
  printf("wire_str_fuzz: fixture_resolved=%llu fixture_with_string=%llu resolved=%llu resolved_with_string=%llu escaped=%llu "
         "mutated_resolved=%llu unmutated_generated=%llu sure=%llu sure_with_string=%llu dict_strings=%llu dict_long=%llu "
         "growth=ok\n",
         (unsigned long long)fixture_resolved, (unsigned long long)fixture_str, (unsigned long long)n_resolved,
         (unsigned long long)n_resolved_str, (unsigned long long)n_escape, (unsigned long long)mutated_resolved,
         (unsigned long long)plain_gen, (unsigned long long)sure, (unsigned long long)sure_str,
         (unsigned long long)g_dict.strings, (unsigned long long)g_dict.long_strings);
  return 0;
}
