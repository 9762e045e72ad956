// wire_plain.h — the part of the Catalyst wire format that needs no host state, for host and device.
//
// wire.cpp's decoder and wire_gpu.hip's k_wire_decode share what is here: the one field-order table (kSchema) and one
// parser of a single InstanceCommand / InstanceQuery entry of known length (wire_plain_parse).  The parser reads the
// entry through a byte accessor (the host plain memory, the device its LDS window) and either yields a PLAIN row or
// says ESCAPE.  A row is plain when the top id is 30 / 31, the inner id is in the schema, every writeObject field is
// null / Long / Integer / Boolean under the codec passed in, a required key is not null and the fields end exactly at
// the entry's end.  Everything else escapes to wire.cpp's decode_one: a String (the interner), a class-name
// identifier, an unknown id, truncation, trailing bytes, a manager entry (the registry).  The classifier is
// conservative: whenever it says plain, decode_one returns CC_OK with the same columns (tests/fuzz/wire_plain_fuzz.cpp
// holds it to that under AddressSanitizer).
//
// The String dictionary.  An engine may hold a device copy of an interner's Strings (cc_wire_dict_attach).  The parser
// form that takes a dictionary (wire_parse<Bytes, DictView>) then also yields entries whose Strings are all known: a
// String of at most CC_WIRE_STR_MAX bytes that the dictionary holds gives tag HANDLE and value first_handle + rank; as
// a key it also needs the cell's "hash registered" bit.  The dictionary is an open-addressing table of DictCell (at
// most half full, power-of-two cells, linear probing) over a byte pool in which every String starts 8-byte aligned
// and is zero-padded to a multiple of 8 bytes.  dict_hash is the one definition of the hash; DictView::find the one
// definition of the probe, for the host mirror (wire.cpp) and the kernel.  A hit is a hit only after the length and
// every byte compare equal, so a resolved String is exactly the interner's (tests/fuzz/wire_str_fuzz.cpp runs both
// with the hash cut to 4 bits).
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/copycat_apply.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CC_WIRE_HD __host__ __device__
#else
#define CC_WIRE_HD
#endif

namespace cc {

// Catalyst Serializer identifier bytes: the width of the type id that follows (null has none)
enum : uint8_t { kIdNull = 0x00, kIdInt8 = 0x01, kIdInt16 = 0x02, kIdInt24 = 0x03, kIdInt32 = 0x04, kIdClass = 0x05 };

// operand slots of one op, in wire order
enum Field : uint8_t {
  F_END = 0,
  F_KEY,      // serializer.writeObject(key): a non-null key -> key column + key tag
  F_KEY_OPT,  // same, may be null (MultiMapCommands.Size() without a key): key 0
  F_A,        // serializer.writeObject(value) -> operand a
  F_B,        // serializer.writeObject(...) -> operand b
  F_AUX,      // buffer.writeLong(ttl / timeout / delay) -> aux
  F_LKEY,     // buffer.writeLong(member) -> key column, key tag LONG
};

constexpr int kSchemaFields = 5;
struct Schema {
  uint8_t op;
  Field f[kSchemaFields];
};

// Field order per @SerializeWith id, from the writeObject chains of the reference's command classes.
constexpr Schema kSchema[] = {
    // AtomicValueCommands.java: Get/Listen/Unlisten write nothing (:82,:249,:263); Set/GetAndSet write only the
    // value (:126,:228 — they override ValueCommand.writeObject, so ttl never travels, A2); CompareAndSet
    // expect, update (:182-184)
    {CC_OP_VALUE_GET, {F_END}},
    {CC_OP_VALUE_SET, {F_A, F_END}},
    {CC_OP_VALUE_CAS, {F_A, F_B, F_END}},
    {CC_OP_VALUE_GETANDSET, {F_A, F_END}},
    {CC_OP_VALUE_LISTEN, {F_END}},
    {CC_OP_VALUE_UNLISTEN, {F_END}},
    // MapCommands.java: KeyQuery/KeyCommand key (:88,:119-121); ContainsValue value (:166-168); KeyValueCommand
    // key, value (:200-202); TtlCommand key, value, ttl (:241-243); GetOrDefault key, default (:331-333);
    // ReplaceIfPresent key, value, ttl, replace (:421-423); IsEmpty/Size/Clear nothing
    {CC_OP_MAP_CONTAINSKEY, {F_KEY, F_END}},
    {CC_OP_MAP_CONTAINSVALUE, {F_A, F_END}},
    {CC_OP_MAP_PUT, {F_KEY, F_A, F_AUX, F_END}},
    {CC_OP_MAP_PUTIFABSENT, {F_KEY, F_A, F_AUX, F_END}},
    {CC_OP_MAP_GET, {F_KEY, F_END}},
    {CC_OP_MAP_GETORDEFAULT, {F_KEY, F_A, F_END}},
    {CC_OP_MAP_REMOVE, {F_KEY, F_END}},
    {CC_OP_MAP_REMOVEIFPRESENT, {F_KEY, F_A, F_END}},
    {CC_OP_MAP_REPLACE, {F_KEY, F_A, F_AUX, F_END}},
    {CC_OP_MAP_REPLACEIFPRESENT, {F_KEY, F_A, F_AUX, F_B, F_END}},
    {CC_OP_MAP_ISEMPTY, {F_END}},
    {CC_OP_MAP_SIZE, {F_END}},
    {CC_OP_MAP_CLEAR, {F_END}},
    // MultiMapCommands.java: KeyQuery key (:121-123); EntryQuery key, value (:190-192); ValueQuery value
    // (:154-156); TtlCommand key, value, ttl (:308-310); EntryCommand key, value (:267-269); RemoveValue value
    // (:399-400); Size is a KeyQuery whose key may be null (:420-430)
    {CC_OP_MMAP_CONTAINSKEY, {F_KEY, F_END}},
    {CC_OP_MMAP_CONTAINSENTRY, {F_KEY, F_A, F_END}},
    {CC_OP_MMAP_CONTAINSVALUE, {F_A, F_END}},
    {CC_OP_MMAP_PUT, {F_KEY, F_A, F_AUX, F_END}},
    {CC_OP_MMAP_GET, {F_KEY, F_END}},
    {CC_OP_MMAP_REMOVE, {F_KEY, F_A, F_END}},
    {CC_OP_MMAP_REMOVEVALUE, {F_A, F_END}},
    {CC_OP_MMAP_ISEMPTY, {F_END}},
    {CC_OP_MMAP_SIZE, {F_KEY_OPT, F_END}},
    {CC_OP_MMAP_CLEAR, {F_END}},
    // QueueCommands.java: ValueCommand / ValueQuery value (:87-88,:118-120); the rest nothing
    {CC_OP_QUEUE_CONTAINS, {F_A, F_END}},
    {CC_OP_QUEUE_ADD, {F_A, F_END}},
    {CC_OP_QUEUE_OFFER, {F_A, F_END}},
    {CC_OP_QUEUE_PEEK, {F_END}},
    {CC_OP_QUEUE_POLL, {F_END}},
    {CC_OP_QUEUE_ELEMENT, {F_END}},
    {CC_OP_QUEUE_REMOVE, {F_A, F_END}},
    {CC_OP_QUEUE_SIZE, {F_END}},
    {CC_OP_QUEUE_ISEMPTY, {F_END}},
    {CC_OP_QUEUE_CLEAR, {F_END}},
    // SetCommands.java: the element travels as the key column (ValueCommand / ValueQuery value :87-88,:118-120);
    // Add = TtlCommand element, ttl (:172-174)
    {CC_OP_SET_CONTAINS, {F_KEY, F_END}},
    {CC_OP_SET_ADD, {F_KEY, F_AUX, F_END}},
    {CC_OP_SET_REMOVE, {F_KEY, F_END}},
    {CC_OP_SET_SIZE, {F_END}},
    {CC_OP_SET_ISEMPTY, {F_END}},
    {CC_OP_SET_CLEAR, {F_END}},
    // LeaderElectionCommands.java: nothing (:50,:69)
    {CC_OP_ELECT_LISTEN, {F_END}},
    {CC_OP_ELECT_UNLISTEN, {F_END}},
    {CC_OP_ELECT_ISLEADER, {F_END}},
    // LockCommands.java: Lock timeout (:80-81); Unlock nothing
    {CC_OP_LOCK_LOCK, {F_AUX, F_END}},
    {CC_OP_LOCK_UNLOCK, {F_END}},
    // MembershipGroupCommands.java: Join/Leave nothing; Schedule member, delay, callback (:124-126); Execute
    // member, callback (:172-174)
    {CC_OP_GROUP_JOIN, {F_END}},
    {CC_OP_GROUP_LEAVE, {F_END}},
    {CC_OP_GROUP_SCHEDULE, {F_LKEY, F_AUX, F_A, F_END}},
    {CC_OP_GROUP_EXECUTE, {F_LKEY, F_A, F_END}},
    // TopicCommands.java: Listen / Unlisten nothing; Publish message (:100-108)
    {CC_OP_TOPIC_LISTEN, {F_END}},
    {CC_OP_TOPIC_UNLISTEN, {F_END}},
    {CC_OP_TOPIC_PUBLISH, {F_A, F_END}},
};

// The schema by inner id, one word per id, as the parser reads it (the host decoder too): bit 31 = a known operation,
// field k in bits [3k, 3k + 3).  The table is built from kSchema where it is used: by wire.cpp for the host, and
// uploaded once per engine for the device (wire_gpu.hip), which keeps it in LDS.
constexpr uint32_t kSchemaIds = 256;
constexpr uint32_t kSchemaKnown = 1u << 31;
constexpr uint32_t schema_word(const Schema& s) {
  uint32_t w = kSchemaKnown;
  for (int k = 0; k < kSchemaFields && s.f[k] != F_END; ++k) w |= (uint32_t)s.f[k] << (3 * k);
  return w;
}
inline void schema_words(uint32_t* out /*[kSchemaIds]*/) {
  for (uint32_t i = 0; i < kSchemaIds; ++i) out[i] = 0;
  for (const Schema& s : kSchema) out[s.op] = schema_word(s);
}

// The longest entry that can be plain: both identifiers 4 bytes wide, every writeObject field a Long behind a 4-byte id.
constexpr uint32_t kWireIdMax = 1 + 4;           // identifier byte + id
constexpr uint32_t kWireValueMax = kWireIdMax + 8;  // a boxed Long
constexpr uint32_t field_max(Field f) { return f == F_END ? 0u : (f == F_AUX || f == F_LKEY) ? 8u : kWireValueMax; }
constexpr uint32_t schema_max(const Schema& s) {
  uint32_t n = 0;
  for (int k = 0; k < kSchemaFields && s.f[k] != F_END; ++k) n += field_max(s.f[k]);
  return n;
}
constexpr uint32_t wire_plain_max() {
  uint32_t m = 0;
  for (const Schema& s : kSchema) m = schema_max(s) > m ? schema_max(s) : m;
  return kWireIdMax + 8 + kWireIdMax + m;  // top id, instance id, inner id, fields
}
constexpr uint32_t kWirePlainMax = wire_plain_max();
static_assert(kWirePlainMax == 65, "the longest plain entry: 18 header bytes + MAP_REPLACEIFPRESENT's 13 + 13 + 8 + 13");

struct PlainRow {
  uint64_t iid, key, a, b, aux;
  uint8_t op, flags;
  uint8_t strs;  // Strings resolved through the dictionary
};

// A byte accessor over host memory.  le64 / le32 assemble bytes [i, i + 8) / [i, i + 4) little-endian; the parser
// calls them only inside the entry.
struct HostBytes {
  const uint8_t* p;
  CC_WIRE_HD uint32_t u8(uint32_t i) const { return p[i]; }
  CC_WIRE_HD uint64_t le64(uint32_t i) const {
    uint64_t v = 0;
    for (int k = 7; k >= 0; --k) v = (v << 8) | p[i + k];
    return v;
  }
  CC_WIRE_HD uint32_t le32(uint32_t i) const {
    uint32_t v = 0;
    for (int k = 3; k >= 0; --k) v = (v << 8) | p[i + k];
    return v;
  }
  // bytes [i, i + n), n in 1..7, little-endian (reads no byte past them)
  CC_WIRE_HD uint64_t lepart(uint32_t i, uint32_t n) const {
    uint64_t v = 0;
    for (uint32_t k = n; k-- > 0;) v = (v << 8) | p[i + k];
    return v;
  }
};

CC_WIRE_HD inline uint64_t wire_bswap64(uint64_t v) { return __builtin_bswap64(v); }
CC_WIRE_HD inline uint32_t wire_bswap32(uint32_t v) { return __builtin_bswap32(v); }

// ---- the String dictionary ---------------------------------------------------------------------------------------
// One cell, 32 bytes, 32-byte aligned (one gather never straddles a cache line); the first 16 bytes decide nearly
// every probe.
struct alignas(32) DictCell {
  uint64_t hash;   // dict_hash of the bytes
  uint32_t len;    // UTF-8 bytes, <= CC_WIRE_STR_MAX
  uint32_t flags;  // kDictUsed | kDictKeyReg
  uint64_t off;    // of the String in the pool, a multiple of 8
  uint32_t rank;   // handle - first_handle
  uint32_t pad;
};
static_assert(sizeof(DictCell) == 32, "DictCell");
enum : uint32_t { kDictUsed = 1u, kDictKeyReg = 2u };  // KeyReg: the handle's String.hashCode is registered on the engine

// The hash of `n` bytes at `pos` behind the accessor: 8 bytes a step, the tail through lepart.
// -DCC_WIRE_DICT_WEAK_HASH cuts it to 4 bits (a test build: nearly every probe then meets equal-hash cells).
template <class Bytes>
CC_WIRE_HD inline uint64_t dict_hash(const Bytes& s, uint32_t pos, uint32_t n) {
  uint64_t h = 0x9E3779B97F4A7C15ull ^ ((uint64_t)n * 0xFF51AFD7ED558CCDull);
  uint32_t i = 0;
  for (; i + 8 <= n; i += 8) {
    h = (h ^ s.le64(pos + i)) * 0xFF51AFD7ED558CCDull;
    h ^= h >> 32;
  }
  if (i < n) {
    h = (h ^ s.lepart(pos + i, n - i)) * 0xFF51AFD7ED558CCDull;
    h ^= h >> 32;
  }
  h *= 0xC4CEB9FE1A85EC53ull;
  h ^= h >> 29;
#ifdef CC_WIRE_DICT_WEAK_HASH
  h &= 15u;
#endif
  return h;
}

// The table as the parser reads it: the host mirror's vectors, or their device copies.
struct DictView {
  static constexpr bool kEnabled = true;
  const DictCell* cells;  // [mask + 1]
  const uint64_t* pool;   // the byte pool as 8-byte words
  uint32_t mask;
  uint64_t first;         // the interner's first handle
  // the cell of bytes [pos, pos + n) behind `s` -> true, its rank and key bit
  template <class Bytes>
  CC_WIRE_HD bool find(const Bytes& s, uint32_t pos, uint32_t n, uint32_t& rank, bool& key_reg) const {
    const uint64_t h = dict_hash(s, pos, n);
    uint32_t at = (uint32_t)h & mask;
    for (uint32_t probe = 0; probe <= mask; ++probe, at = (at + 1) & mask) {  // (at most half full: an empty cell ends it)
      const DictCell& c = cells[at];
      const uint32_t fl = c.flags;
      if (!(fl & kDictUsed)) return false;
      if (c.hash != h || c.len != n) continue;
      const uint64_t* q = pool + (c.off >> 3);
      bool same = true;
      uint32_t i = 0;
      for (; same && i + 8 <= n; i += 8) same = q[i >> 3] == s.le64(pos + i);
      if (same && i < n) same = q[i >> 3] == s.lepart(pos + i, n - i);  // (the pool's padding is zero)
      if (same) {
        rank = c.rank;
        key_reg = (fl & kDictKeyReg) != 0;
        return true;
      }
    }
    return false;
  }
};
struct NoDict {  // the parser without a dictionary: a String escapes
  static constexpr bool kEnabled = false;
};

// The longest entry the parser with a dictionary yields: as wire_plain_max, every writeObject field a String of
// CC_WIRE_STR_MAX bytes behind a 4-byte id, a presence byte and an 8-byte length.
constexpr uint32_t kWireStrValueMax = kWireIdMax + 1 + 8 + CC_WIRE_STR_MAX;
constexpr uint32_t field_str_max(Field f) { return f == F_END ? 0u : (f == F_AUX || f == F_LKEY) ? 8u : kWireStrValueMax; }
constexpr uint32_t wire_str_max() {
  uint32_t m = 0;
  for (const Schema& s : kSchema) {
    uint32_t n = 0;
    for (int k = 0; k < kSchemaFields && s.f[k] != F_END; ++k) n += field_str_max(s.f[k]);
    m = n > m ? n : m;
  }
  return kWireIdMax + 8 + kWireIdMax + m;
}
constexpr uint32_t kWireStrEntryMax = wire_str_max();
static_assert(kWireStrEntryMax == 18 + 3 * kWireStrValueMax + 8, "the longest entry: MAP_REPLACEIFPRESENT's three Strings");

// One entry of `len` bytes behind `s` under codec `c`, with the schema words `sch` -> true: plain, `r` filled with the
// host decoder's canonical values (Integer sign-extended, Boolean any nonzero byte -> 1, a null optional key -> key 0
// and key tag 0, F_LKEY -> key tag LONG).  false: escape (r is unspecified).
// wire_parse is the parser; `d` is NoDict (a String escapes: wire_plain_parse) or a DictView.  With a dictionary a
// String is read as wire.cpp's read_utf8 reads it: the optional presence byte (0: tag NULL, value 0), the length
// (utf8_len_bytes in the codec's byte order), the bytes.  It yields tag HANDLE and first + rank when the dictionary
// holds it; a String key (key tag 3) also needs the cell's key bit.  A length above CC_WIRE_STR_MAX or past the entry,
// an unknown String and a key without the bit escape.  The parser never interns and never registers.
template <class Bytes, class Dict>
CC_WIRE_HD inline bool wire_parse(const Bytes& s, uint32_t len, const cc_wire_codec& c, const uint32_t* sch, const Dict& d,
                                  PlainRow& r) {
  if (len > (Dict::kEnabled ? kWireStrEntryMax : kWirePlainMax)) return false;
  const bool be = c.big_endian != 0;
  uint32_t pos = 0;
  // identifier + id (ids are signed, 1-4 bytes in the codec's byte order)
  auto read_id = [&](int64_t& id) -> bool {
    if (pos >= len) return false;
    const uint32_t w = s.u8(pos);
    if (w < kIdInt8 || w > kIdInt32 || len - pos - 1 < w) return false;
    uint64_t raw = 0;
    for (uint32_t i = 0; i < w; ++i) raw |= (uint64_t)s.u8(pos + 1 + i) << (8 * (be ? w - 1 - i : i));
    id = (int64_t)(raw << (64 - 8 * w)) >> (64 - 8 * w);
    pos += 1 + w;
    return true;
  };
  auto read_u64 = [&](uint64_t& v) -> bool {
    if (len - pos < 8) return false;
    v = s.le64(pos);
    if (be) v = wire_bswap64(v);
    pos += 8;
    return true;
  };
  r.strs = 0;
  bool key_reg = true;  // (of the value read last)
  // serializer.writeObject(value) of a null / Long / Integer / Boolean, and with a dictionary a known String
  auto read_value = [&](uint32_t& tag, uint64_t& v) -> bool {
    key_reg = true;
    if (pos >= len) return false;
    if (s.u8(pos) == kIdNull) {
      tag = CC_TAG_NULL, v = 0, pos += 1;
      return true;
    }
    int64_t id = 0;
    if (!read_id(id)) return false;
    if (id == c.id_long) {
      tag = CC_TAG_LONG;
      return read_u64(v);
    }
    if (id == c.id_int) {
      if (len - pos < 4) return false;
      uint32_t x = s.le32(pos);
      if (be) x = wire_bswap32(x);
      tag = CC_TAG_INT, v = (uint64_t)(int64_t)(int32_t)x, pos += 4;
      return true;
    }
    if (id == c.id_bool) {
      if (len - pos < 1) return false;
      tag = CC_TAG_BOOL, v = s.u8(pos) ? 1 : 0, pos += 1;
      return true;
    }
    if constexpr (Dict::kEnabled) {
      if (id == c.id_string) {
        if (c.utf8_presence_byte) {
          if (pos >= len) return false;
          if (!s.u8(pos++)) {
            tag = CC_TAG_NULL, v = 0;
            return true;
          }
        }
        const uint32_t lw = c.utf8_len_bytes;
        if (len - pos < lw) return false;
        uint64_t n = lw == 8 ? s.le64(pos) : s.lepart(pos, lw);
        if (be) n = wire_bswap64(n) >> (64 - 8 * lw);
        pos += lw;
        if (n > CC_WIRE_STR_MAX || len - pos < n) return false;
        uint32_t rank = 0;
        if (!d.find(s, pos, (uint32_t)n, rank, key_reg)) return false;
        tag = CC_TAG_HANDLE, v = d.first + rank, pos += (uint32_t)n;
        ++r.strs;
        return true;
      }
    }
    return false;  // a String without a dictionary, or a type with no canonical tag
  };
  int64_t top = 0, id = 0;
  if (!read_id(top) || (top != 30 && top != 31)) return false;
  if (!read_u64(r.iid)) return false;
  if (!read_id(id) || id < 0 || id >= (int64_t)kSchemaIds) return false;
  const uint32_t w = sch[id];
  if (!(w & kSchemaKnown)) return false;
  r.op = (uint8_t)id;
  r.key = r.a = r.b = r.aux = 0;
  uint32_t ta = CC_TAG_NULL, tb = CC_TAG_NULL, kt = 0;
  for (int k = 0; k < kSchemaFields; ++k) {
    const uint32_t f = (w >> (3 * k)) & 7u;
    if (f == F_END) break;
    uint32_t tag = 0;
    uint64_t v = 0;
    if (f == F_KEY || f == F_KEY_OPT) {
      if (!read_value(tag, v)) return false;
      if (tag == CC_TAG_NULL) {
        if (f == F_KEY) return false;
      } else {
        if (tag == CC_TAG_HANDLE && !key_reg) return false;  // the host registers the hash, then the bit is set
        kt = tag == CC_TAG_LONG ? 0u : tag == CC_TAG_INT ? 1u : tag == CC_TAG_BOOL ? 2u : 3u;
        r.key = v;
      }
    } else if (f == F_A) {
      if (!read_value(ta, r.a)) return false;
    } else if (f == F_B) {
      if (!read_value(tb, r.b)) return false;
    } else if (f == F_AUX) {
      if (!read_u64(r.aux)) return false;
    } else {  // F_LKEY
      if (!read_u64(r.key)) return false;
      kt = 0;
    }
  }
  if (pos != len) return false;
  r.flags = CC_FLAGS(ta, tb, kt);
  return true;
}

template <class Bytes>
CC_WIRE_HD inline bool wire_plain_parse(const Bytes& s, uint32_t len, const cc_wire_codec& c, const uint32_t* sch,
                                        PlainRow& r) {
  return wire_parse(s, len, c, sch, NoDict{}, r);
}

}  // namespace cc
