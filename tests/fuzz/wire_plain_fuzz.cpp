// wire_plain_fuzz.cpp — host-only check of the parser the GPU wire decoder runs (copycat_amd/csrc/wire_plain.h
// wire_plain_parse) against the host decoder (wire.cpp decode_one), built with -fsanitize=address,undefined by
// tests/test_wire_plain.py (test infrastructure; never part of the product library).
//
// The classifier must be conservative: for every input it either escapes or returns exactly the columns decode_one
// returns with CC_OK.  Inputs: the committed fixture (tests/golden/wire_fixture.*), every truncation of every fixture
// entry, and seeded mutations under random codec parameters (byte order, the ids of Long / Integer / Boolean / String,
// identifier widths 1-4) of fixture entries and of entries generated under that codec.  Each entry is parsed from a
// heap copy of exactly its bytes, so the sanitizer sees any overread.  Prints the count of fixture rows that came back
// plain (the test compares it with the fixture's JSON) and the totals.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "engine_state.h"
#include "wire_plain.h"

namespace cc {
int set_err(int code, const char*, hipError_t) { return code; }  // the engine's cc_last_error store is not linked
}  // namespace cc
extern "C" int cc_handle_hashes(cc_engine*, const uint64_t*, const int32_t*, uint64_t) { return CC_OK; }

namespace {
uint64_t g_rng = 0x243F6A8885A308D3ull;
uint64_t rnd() {  // splitmix64
  uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
uint64_t n_plain = 0, n_escape = 0, n_escape_ok = 0;
uint32_t g_sch[cc::kSchemaIds];

// -> 1 plain, 0 escape, -1 the property is broken
int check(cc_wire_interner* in, const cc_wire_codec& c, const std::vector<uint8_t>& bytes) {
  uint8_t* buf = (uint8_t*)malloc(bytes.empty() ? 1 : bytes.size());  // exact size: one byte past it is an ASan report
  if (!bytes.empty()) memcpy(buf, bytes.data(), bytes.size());
  cc::PlainRow r{};
  const bool plain = cc::wire_plain_parse(cc::HostBytes{buf}, (uint32_t)bytes.size(), c, g_sch, r);
  uint8_t op = 0, flags = 0, kind = 0;
  uint64_t key = 0, a = 0, b = 0, aux = 0, iid = 0;
  cc_wire_out out{};
  out.iid = &iid, out.op = &op, out.flags = &flags, out.key = &key, out.a = &a, out.b = &b, out.aux = &aux, out.kind = &kind;
  const int rc = cc::wire_decode_one(nullptr, c, in, buf, buf + bytes.size(), 0, 0, &out);
  free(buf);
  if (!plain) {
    ++n_escape;
    if (rc == CC_OK) ++n_escape_ok;
    return 0;
  }
  ++n_plain;
  if (rc != CC_OK || kind != 0 || iid != r.iid || op != r.op || flags != r.flags || key != r.key || a != r.a || b != r.b ||
      aux != r.aux) {
    fprintf(stderr, "plain row differs from decode_one (rc %d, %zu bytes):", rc, bytes.size());
    for (uint8_t x : bytes) fprintf(stderr, " %02x", x);
    fprintf(stderr, "\n");
    return -1;
  }
  return 1;
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
void put_value(std::vector<uint8_t>& o, const cc_wire_codec& c) {
  switch (rnd() % 6) {
    case 0: o.push_back(0); break;
    case 1: put_id(o, c, c.id_long), put_uint(o, c, rnd() & 1 ? rnd() : (uint64_t)(int64_t)(rnd() % 5 - 2), 8); break;
    case 2: put_id(o, c, c.id_int), put_uint(o, c, rnd(), 4); break;
    case 3: put_id(o, c, c.id_bool), o.push_back((uint8_t)(rnd() % 3)); break;
    case 4: {  // a String
      put_id(o, c, c.id_string);
      const bool null = c.utf8_presence_byte && rnd() % 4 == 0;
      if (c.utf8_presence_byte) o.push_back(null ? 0 : 1);
      if (!null) {
        const int n = (int)(rnd() % 6);
        put_uint(o, c, (uint64_t)n, c.utf8_len_bytes);
        for (int i = 0; i < n; ++i) o.push_back((uint8_t)('a' + rnd() % 26));
      }
      break;
    }
    default: put_id(o, c, (int64_t)(rnd() % 300)); break;  // some other registered type
  }
}
std::vector<uint8_t> gen(const cc_wire_codec& c) {
  std::vector<uint8_t> o;
  put_id(o, c, rnd() % 16 ? 30 + (int64_t)(rnd() & 1) : (int64_t)(rnd() % 40));
  put_uint(o, c, rnd(), 8);
  const cc::Schema& s = cc::kSchema[rnd() % (sizeof cc::kSchema / sizeof cc::kSchema[0])];
  put_id(o, c, rnd() % 16 ? (int64_t)s.op : (int64_t)(rnd() % 300));
  for (int k = 0; k < cc::kSchemaFields && s.f[k] != cc::F_END; ++k) {
    if (s.f[k] == cc::F_AUX || s.f[k] == cc::F_LKEY) put_uint(o, c, rnd(), 8);
    else put_value(o, c);
  }
  return o;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: wire_plain_fuzz FIXTURE.bin OFFSETS.txt ITERATIONS\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> blob;
  for (int ch; (ch = fgetc(f)) != EOF;) blob.push_back((uint8_t)ch);
  fclose(f);
  std::vector<uint64_t> off;
  FILE* g = fopen(argv[2], "r");
  if (!g) return 2;
  for (unsigned long long x; fscanf(g, "%llu", &x) == 1;) off.push_back(x);
  fclose(g);
  const long iters = atol(argv[3]);
  cc::schema_words(g_sch);
  cc_wire_interner* in = nullptr;
  if (cc_wire_interner_create(1, &in) != CC_OK) return 2;
  cc_wire_codec def;
  cc_wire_codec_default(&def);

  std::vector<std::vector<uint8_t>> ents;
  for (size_t i = 0; i + 1 < off.size(); ++i) ents.emplace_back(blob.begin() + off[i], blob.begin() + off[i + 1]);
  uint64_t fixture_plain = 0;
  for (auto& e : ents) {
    const int r = check(in, def, e);
    if (r < 0) return 1;
    fixture_plain += (uint64_t)r;
  }
  for (auto& e : ents)  // every truncation of every entry
    for (size_t n = 0; n < e.size(); ++n)
      if (check(in, def, std::vector<uint8_t>(e.begin(), e.begin() + n)) < 0) return 1;
  uint64_t gen_plain = 0;
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
    std::vector<uint8_t> x = rnd() & 1 ? gen(c) : ents[rnd() % ents.size()];
    switch (rnd() % 6) {
      case 0: {  // byte flips
        const int k = 1 + (int)(rnd() % 4);
        for (int j = 0; j < k && !x.empty(); ++j) x[rnd() % x.size()] ^= (uint8_t)(1 + rnd() % 255);
        break;
      }
      case 1: {  // splice: a prefix of one entry + a suffix of another
        const auto y = rnd() & 1 ? gen(c) : ents[rnd() % ents.size()];
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
      case 4: {  // 0xFF runs
        if (!x.empty()) {
          const size_t at = rnd() % x.size();
          for (size_t j = at; j < x.size() && j < at + 8; ++j) x[j] = 0xFF;
        }
        break;
      }
      default: break;  // as generated
    }
    const int r = check(in, c, x);
    if (r < 0) return 1;
    gen_plain += (uint64_t)r;
  }
  cc_wire_interner_destroy(in);
  printf("wire_plain_fuzz: fixture_plain=%llu plain=%llu escaped=%llu (of which the host decodes %llu) mutated_plain=%llu\n",
         (unsigned long long)fixture_plain, (unsigned long long)n_plain, (unsigned long long)n_escape,
         (unsigned long long)n_escape_ok, (unsigned long long)gen_plain);
  return 0;
}
