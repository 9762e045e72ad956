// value_path.hip — the value-only engine pipeline (the c2 headline): k_part_v4 -> k_apply_value_v3 -> k_unpermute.
//
// A stable group-by of the sub-batch by super-bucket (256 AtomicValueState slots), one walk per slot in log order,
// then the results back to log order, shaped for HBM bytes and CU occupancy:
//
//  * one 8-byte staging record per commit: the meta (slot, op class, the two value tags) and the operands packed as
//    small two's complement numbers (the CAS update as a difference from the expected value); a commit whose
//    operands do not fit keeps its row in the tile instead and the apply reads them from the batch's a / b columns;
//  * 8192-commit tiles, each ranked whole in one persistent 1024-thread workgroup per CU and written out of an LDS
//    image in full lines; the apply walks each slot in registers while loader waves stage the next chunk.
//
// Reference semantics are AtomicValueState's (atomic/src/main/java/io/atomix/atomic/state/AtomicValueState.java):
// get :77-83, set :114-118, compareAndSet :123-133, getAndSet :138-144, delete :146-157; dispatch and unknown
// sessions ResourceManager.operateResource :56-72 (UNKNOWN_SESSION rows are answered by the unpermute).
#include <type_traits>

#include "common.h"
#include "engine_internal.h"

namespace cc {

#ifdef CC_PHASE_TIMING  // diagnostics build: phase clocks of k_part_v4 (g_ph_v3p) and k_apply_value_v3 (g_ph_v3a)
__device__ unsigned long long g_ph_v3p[kPhases], g_ph_v3a[kPhases];
int phase_read_v3(int kernel, uint64_t* out) {
  unsigned long long z[kPhases] = {};
  const void* sym = kernel == K_PART_TILE ? HIP_SYMBOL(g_ph_v3p) : HIP_SYMBOL(g_ph_v3a);
  if (hipMemcpyFromSymbol(out, sym, sizeof z) != hipSuccess || hipMemcpyToSymbol(sym, z, sizeof z) != hipSuccess)
    return CC_ERR_HIP;
  return CC_OK;
}
#endif


// ---- the 8-byte value record -------------------------------------------------------------------------------
// w = meta (18 bits) | payload (46 bits) << 18
//   meta: slot-in-super-bucket 0..7 | class 8..10 | compare tag 11..13 | new tag 14..16 | escaped 17
//   payload, set / getAndSet: the canonical new value as a 46-bit two's complement number (sign-extended back);
//            CAS: the canonical expected value as a 32-bit two's complement number | (update - expected) as a 14-bit
//            one << 32;
//            escaped (an operand that does not fit): the commit's row in its 8192-commit tile; the apply reads the
//            operands from the batch's a / b columns there (exact for every input; only the bytes moved differ).
// A DistributedAtomicLong CAS loop (DistributedAtomicLong.java:117-146) expects a value the resource holds and updates
// it by a small delta, so its records never escape while the values stay within +-2^31; the 16-byte record of round 3
// (full expected value + 33-bit delta) moved 8 more bytes per commit through the partition's writes and the apply's
// reads.
enum : uint32_t { kC3Get = 0, kC3Set = 1, kC3Cas = 2, kC3Gas = 3, kC3Del = 4, kC3Lis = 5, kC3Unk = 6 };
constexpr int kV3ExpBits = 32, kV3DeltaBits = 14, kV3SetBits = 46;
static_assert(kV3ExpBits + kV3DeltaBits == kV3SetBits && 18 + kV3SetBits == 64, "the record's payload field");
static_assert(kV3Tile <= (1 << 13), "the record's row field");

__device__ inline bool v3_fits(uint64_t x, int bits) {  // x == sign-extension of its low `bits` bits
  return (uint64_t)(((int64_t)(x << (64 - bits))) >> (64 - bits)) == x;
}

// (An escaped record's row, < 8192, is ORed in where the partition places the record: v3_set_row.)
__device__ inline uint64_t v3_encode(uint32_t op, uint32_t flags, uint64_t a, uint64_t b, uint32_t slot) {
  const uint32_t ta = CC_FLAG_TAG_A(flags), tb = CC_FLAG_TAG_B(flags);
  const uint64_t pa = ta ? a : 0, pb = tb ? b : 0;  // canonical NULL payload
  uint32_t cls = kC3Unk, ct = 0, nt = 0, esc = 0;
  uint64_t pl = 0;
  if (op == CC_OP_VALUE_GET) {
    cls = kC3Get;
  } else if (op == CC_OP_VALUE_SET || op == CC_OP_VALUE_GETANDSET) {
    cls = op == CC_OP_VALUE_SET ? kC3Set : kC3Gas;
    nt = ta;
    esc = v3_fits(pa, kV3SetBits) ? 0u : 1u;
    pl = pa;
  } else if (op == CC_OP_VALUE_CAS) {
    cls = kC3Cas;
    ct = ta;
    nt = tb;
    const uint64_t d = pb - pa;
    esc = v3_fits(pa, kV3ExpBits) && v3_fits(d, kV3DeltaBits) ? 0u : 1u;
    pl = (pa & 0xFFFFFFFFull) | (d << kV3ExpBits);
  } else if (op == CC_OP_DELETE) {
    cls = kC3Del;
  } else if (op == CC_OP_VALUE_LISTEN || op == CC_OP_VALUE_UNLISTEN) {
    cls = kC3Lis;
  }
  pl = esc ? 0ull : pl;
  return (uint64_t)(slot | (cls << 8) | (ct << 11) | (nt << 14) | (esc << 17)) | (pl << 18);
}
__device__ inline uint32_t v3_slot(uint64_t r) { return (uint32_t)r & 0xFFu; }
__device__ inline uint64_t v3_set_row(uint64_t r, uint32_t row) {
  return ((r >> 17) & 1u) ? (r | ((uint64_t)row << 18)) : r;
}

// The record -> the walk's form: a meta word, the canonical compare value x and the canonical new value y (cf.
// common.h value_encode; the bits are laid out for this file's walk alone, which is its slot, so none is carried):
//   bits 0..7   the status byte of an op that does not return the current value (CAS: OK|BOOL, unknown: UNKNOWN_OP)
//   bit 8 W     the op writes y unconditionally: set, getAndSet -- and delete, which writes "no value"
//   bit 9 C     compareAndSet;  bit 10 R  the op returns the current value: get, getAndSet
//   bit 11 L    listen / unlisten: events, not applied here (flagged)
//   bits 12..14 the compare tag
//   bits 16..31 the slot's meta word after a write (vmeta): the new tag | has-current << 8; 0 for a delete
// The class's part comes from two byte tables indexed by a shift: byte `cls` of kV3OpLo is the status byte, of
// kV3OpHi the W C R L bits (0..3) and has-current after a write (4).
constexpr uint32_t kM3W = 1u << 8, kM3C = 1u << 9, kM3R = 1u << 10, kM3L = 1u << 11;
__host__ __device__ constexpr uint32_t v3_class_bits(uint32_t cls) {  // status | W C R L << 8 | has-current << 12
  return cls == kC3Get   ? kM3R
         : cls == kC3Set ? (kM3W | 0x1000u)
         : cls == kC3Cas ? (kM3C | 0x1000u | CC_STATUS(CC_ST_OK, CC_TAG_BOOL))
         : cls == kC3Gas ? (kM3W | kM3R | 0x1000u)
         : cls == kC3Del ? kM3W
         : cls == kC3Lis ? kM3L
                         : CC_STATUS(CC_ST_UNKNOWN_OP, CC_TAG_NULL);  // kC3Unk, and 7 (never encoded)
}
__host__ __device__ constexpr uint64_t v3_class_table(int shift) {
  uint64_t tb = 0;
  for (uint32_t c = 0; c < 8; ++c) tb |= (uint64_t)((v3_class_bits(c) >> shift) & 0xFFu) << (8 * c);
  return tb;
}
constexpr uint64_t kV3OpLo = v3_class_table(0), kV3OpHi = v3_class_table(8);

// A record whose operands are in it (not escaped).  x is the 32-bit expected value for every class: the walk reads x
// only under C.  y is the 46-bit payload, or expected + delta for a CAS; classes without a payload (delete among
// them) carry 0, and a delete's new tag is 0.
__device__ inline void v3_decode(uint64_t r, uint32_t& m, uint64_t& x, uint64_t& y) {
  const uint32_t lo = (uint32_t)r;
  const uint32_t sh = (lo >> 5) & 0x38u;  // 8 * class
  const uint32_t kh = (uint32_t)(kV3OpHi >> sh) & 0x1Fu;
  // kh * 0x100100 = kh << 8 | kh << 20: W C R L to bits 8..11, has-current to bit 24
  m = ((uint32_t)(kV3OpLo >> sh) & 0xFFu) | ((kh * 0x100100u) & 0x01000F00u) |
      ((lo << 1) & (7u << 12)) | ((lo << 2) & (7u << 16));  // compare tag 11..13 -> 12..14, new tag 14..16 -> 16..18
  const uint64_t e = (uint64_t)(int64_t)(int32_t)(uint32_t)(r >> 18);
  x = e;
  y = ((lo >> 8) & 7u) == kC3Cas ? e + (uint64_t)((int64_t)r >> (64 - kV3DeltaBits)) : (uint64_t)((int64_t)r >> 18);
}
// An escaped record (rare): the operands from the batch columns.  tile_row0 = the batch row of the record's tile
// start.
__device__ inline void v3_decode_escaped(uint64_t r, const uint64_t* __restrict__ ca, const uint64_t* __restrict__ cb,
                                         uint64_t tile_row0, uint64_t& x, uint64_t& y) {
  const uint32_t lo = (uint32_t)r;
  const uint32_t cls = (lo >> 8) & 7u, ct = (lo >> 11) & 7u, nt = (lo >> 14) & 7u;
  const bool cas = cls == kC3Cas, wr = cls == kC3Set || cls == kC3Gas;
  const uint64_t row = tile_row0 + ((r >> 18) & (kV3Tile - 1));
  x = cas && ct ? ca[row] : 0;
  y = cas ? (nt ? cb[row] : 0) : (wr && nt ? ca[row] : 0);
}

// ---- the packed result ----------------------------------------------------------------------------------------
// The apply writes one 4-byte word per result into an array of its own (rst_word, indexed by staging position like
// the records):
//   bits 0..23   the payload as a 24-bit two's complement number (sign-extended back by the unpermute); 0 if escaped
//   bits 24..30  the status, 7 bits: code | tag << 4 (tags <= 6)
//   bit 31       escaped: the payload is outside [-2^23, 2^23) and is written whole to rst_value at the same staging
//                position, where the unpermute reads it
// The word follows the record's idea (32-bit expected value, 14-bit delta): a CAS answers a boolean, a get /
// getAndSet of a DistributedAtomicLong a small counter, so a 56-bit payload laid over the 8-byte record moved 4 bytes
// per commit twice (the apply's write, the unpermute's read) that almost never carried anything.  (9 B per commit in
// two arrays before round 3: a status byte array whose lines were written in ~32-byte pieces by different workgroups,
// and the value array.)
constexpr int kV3ResBits = 24;
__device__ inline bool v3_res_fits(uint64_t v) {  // v == sign-extension of its low 24 bits
  return (uint64_t)(int64_t)((int32_t)((uint32_t)v << (32 - kV3ResBits)) >> (32 - kV3ResBits)) == v;
}
__device__ inline uint32_t v3_pack_result(uint32_t status, uint64_t v, bool esc) {
  return (esc ? (1u << 31) : ((uint32_t)v & ((1u << kV3ResBits) - 1))) | ((status & 0x7Fu) << kV3ResBits);
}
__device__ inline uint64_t v3_result_payload(uint32_t wd) {
  return (uint64_t)(int64_t)((int32_t)(wd << (32 - kV3ResBits)) >> (32 - kV3ResBits));
}
// Element i of a staging array through a 32-bit byte offset (uniform base + zero-extended offset: no 64-bit shift
// and add per access).  Staging positions, the dummy rows' among them, stay below 2^29 (launch_apply_value_v3).
template <class T>
__device__ inline T* v3_at(T* base, uint32_t i) {
  using B = std::conditional_t<std::is_const<T>::value, const char, char>;
  return reinterpret_cast<T*>(reinterpret_cast<B*>(base) + (uint32_t)(i * (uint32_t)sizeof(T)));
}

// ---- k_part_v4: one persistent 1024-thread workgroup per CU, one pass per 8192-commit tile --------------------
// Same output as the round-3 k_part_v3 (the tile's records grouped by super-bucket in log order, its ttab row and cpos), but
// the whole tile is ranked at once and placed into a 128 KiB LDS image of the tile's staging region, which is then
// written out contiguously: every 128-byte line of the staging area is written whole by one instruction (k_part_v3
// wrote each run piece per 2048-commit chunk, and lines shared by two pieces reached HBM as partial writes: 22.6 B
// written per commit for 18).  Thread (w, j, l) holds commit w*512 + j*64 + l of the tile in registers (the
// tile's rows are wave-contiguous, so per-wave lane-ordered counters give a stable rank).
// The tile loop keeps the next tile's loads in flight through the tile's compute.  At the top of a tile, once its
// columns have landed, the gathers of inst_res are issued and every row is encoded into its 8-byte record (slot 0,
// the row set if escaped: nothing in the record needs the rank), which frees the raw column registers while the
// gathers are still out; the next tile's columns are then loaded in two slices, one right there and one while wave 0
// scans.  The placement only ORs the slot into the record.  The columns are loaded 16 bytes a lane (14 load
// instructions a thread and tile, 28 as 4- and 8-byte loads: the tile's read time follows the number of load
// instructions a CU has to get through, not their bytes) and change to the rank layout through 4 KB of LDS per wave.
// Registers: 128 VGPRs, no scratch (16 of records beside the 44 of the raw next tile, so resource and rank share a
// register); LDS 148,488 B, one workgroup per CU as before.
// LDS hazards: each wave zeroes its own counter row at the top of a tile (its previous readers -- wave 0's scan and
// the wave's own placement -- finished before the previous tile's B3); img / kst are rewritten only after the next
// tile's B1 / B2, which every thread reaches after its own write-out reads; stg[w] is wave w's alone (a wave's LDS
// accesses execute in order).
constexpr int kP4T = 1024;
constexpr int kP4W = kP4T / kWave;    // 16 waves
constexpr int kP4J = kV3Tile / kP4T;  // 8 commits per thread
static_assert(kP4J == 8, "k_part_v4 keeps 8 commits per thread in registers");

template <int KP, int KSB>
__global__ __launch_bounds__(kP4T) void k_part_v4(const uint32_t* __restrict__ inst, const uint8_t* __restrict__ op,
                                                const uint8_t* __restrict__ flags, const uint64_t* __restrict__ ca,
                                                const uint64_t* __restrict__ cb, uint64_t lo, uint64_t hi,
                                                const uint32_t* __restrict__ inst_res, uint32_t max_inst, uint32_t sb,
                                                uint32_t tiles, uint64_t* __restrict__ st_rec, uint16_t* __restrict__ cpos,
                                                uint16_t* __restrict__ ttab) {
  __shared__ uint64_t img[kV3Tile];          // the tile's records in staging order
  __shared__ uint32_t wc[kP4W][kMaxSb / 2];  // per-wave counters (packed u16 pairs) -> per-wave exclusive prefixes
  __shared__ uint16_t kst[kMaxSb + 1];       // tile-local run starts (+ live count)
  __shared__ uint64_t stg[kP4W][kWave * kP4J];  // per wave: one column of its 512 rows, from load layout to row layout
  const uint32_t t = threadIdx.x, w = t >> 6, l = t & 63;
  const uint32_t hw = (sb + 1) / 2;
  uint32_t T = blockIdx.x;
  if (T >= tiles) return;
  PH_DECL
  // of2[j / 2] >> 16 * (j % 2) = op | flags << 8 of row j (two rows per register).  With 4-byte aligned op / flags
  // columns (`wide`, a property of the launch) they arrive as 4-row words (lane l of wave w holds rows
  // w*512 + i*256 + 4l .. +3), one load instruction per 256 rows instead of one per 64 (the 16 byte loads per
  // thread were issue-bound in the address unit: 19.4 -> 15.1 us per tile without them), and are spread to the rank
  // layout (row w*512 + j*64 + l) by lane shuffles at the top of the tile; unaligned columns load bytes.  The tile
  // loop is compiled once for each form: a branch around loads inside the loop would make the counted waits behind
  // it wait for the loads of both arms.
  const bool opfl_al = ((((uintptr_t)op) | ((uintptr_t)flags) | (uintptr_t)lo) & 3u) == 0;
  const uint32_t q0 = w * (kWave * kP4J) + l;  // row of j = 0; row of j = q0 + 64 j
  // r[j]: the row's resource (< 2^17) | its rank among its wave's rows of the same super-bucket (< 512) << 17 from
  // the rank on; kNoRes = no resource
  constexpr uint32_t kResBits = 17;
  static_assert(kMaxSb << KSB <= 1 << kResBits && kWave * kP4J <= 1 << (31 - kResBits), "k_part_v4 packs resource and rank");
  // The next tile's loads go out in two slices: the instance column, op / flags and the first kS1 of the four
  // operand loads right after the encode, the rest between B1 and B2.
  constexpr int kS1 = 2, kOpLoads = kP4J / 2;
  auto tile_loop = [&](auto wide_c) {
    constexpr bool wide = decltype(wide_c)::value;
    // ofr: a wide tile's op / flags words ({op 0, op 1, flags 0, flags 1}) until `unpack`; of2 from there on, and
    // for byte loads from the start
    // riw / aw / bw: the instance and operand columns as loaded, 16 bytes a lane: lane l of wave w holds rows
    // w*512 + 256 i + 4l .. +3 of inst in riw[i] and rows w*512 + 128 m + 2l, +1 of a / b in aw[m] / bw[m].  A CU
    // gets through its load instructions at a rate that does not depend on their width, so the
    // columns come in as few instructions as their layout allows (14 a thread and tile instead of 28) and are turned to the rank layout (row
    // w*512 + 64 j + l) through the wave's own 4 KB of `stg` at the top of the tile.
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    u32x4 riw[2], aw[kP4J / 2], bw[kP4J / 2];
    uint32_t ofr[kP4J / 2];
    auto rowq = [&](int j) -> uint32_t { return q0 + (uint32_t)j * kWave; };
    // row j is below n (q0 + 64 j < n, n <= 8192) with j on the scalar side: no per-row register
    auto row_below = [&](int j, uint32_t n) -> bool { return (int)q0 < (int)n - j * kWave; };
    // A tile's loads, in the order they are needed back (loads return in issue order): the instance column (the
    // gathers wait for it alone), op / flags, then the operand loads m0 .. m1-1.  Buffer loads: one descriptor per
    // column and tile (base = the tile's first row, size = its live rows; block-uniform), the thread's row as a
    // 32-bit offset and j in the instruction's immediate, so a load takes no address registers, no clamp and no
    // branch: a row past the batch end reads as 0 (ignored), and past the last tile the size is 0 and nothing is
    // read.  (An aligned op / flags word that holds a live row is read whole, so its size is rounded up to 4; a
    // 16-byte load is range-checked dword by dword, so the live rows of one that straddles the batch end arrive.)
    uint64_t lt0 = 0;
    uint32_t lnr = 0;
    auto rsrc = [&](const void* col, uint32_t esz, uint32_t rows) {
      return __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(static_cast<const uint8_t*>(col)) + lt0 * esz, 0,
                                               (int)(rows * esz), 0x00020000);
    };
    // (the thread's row as the tile loop sees it afresh: offsets computed ahead of the loop would each hold a
    // register through it instead of folding into the instructions' immediates)
    auto row0 = [&]() -> uint32_t {
      uint32_t q = q0;
      asm volatile("" : "+v"(q));
      return q;
    };
    constexpr int kNt = 2;  // the nontemporal cache policy bit of a buffer load
    auto load_head = [&](uint32_t TT) {
      const bool live = TT < tiles;
      lt0 = live ? lo + (uint64_t)TT * kV3Tile : lo;
      lnr = live ? (uint32_t)(hi - lt0 < (uint64_t)kV3Tile ? hi - lt0 : (uint64_t)kV3Tile) : 0u;
      const auto di = rsrc(inst, 4, lnr);
      const uint32_t q = row0();
      const uint32_t qw = q + 3u * (q & 63u);  // w * 512 + 4 l
#pragma unroll
      for (int i = 0; i < 2; ++i) riw[i] = __builtin_amdgcn_raw_buffer_load_b128(di, 4 * qw + i * (16 * kWave), 0, kNt);
#ifdef CC_DIAG_NO_OPFL  // diagnostics build only: op / flags not loaded (wrong results; the byte loads' issue cost)
#pragma unroll
      for (int j = 0; j < kP4J / 2; ++j) ofr[j] = 0x11321132u;
#else
      if constexpr (wide) {
        const auto dop = rsrc(op, 1, (lnr + 3u) & ~3u), dfl = rsrc(flags, 1, (lnr + 3u) & ~3u);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const uint32_t ic = qw + (uint32_t)i * (4 * kWave);  // w * 512 + 4 l + 256 i
          ofr[i] = __builtin_amdgcn_raw_buffer_load_b32(dop, ic, 0, kNt);
          ofr[2 + i] = __builtin_amdgcn_raw_buffer_load_b32(dfl, ic, 0, kNt);
        }
      } else {
        const auto dop = rsrc(op, 1, lnr), dfl = rsrc(flags, 1, lnr);
#pragma unroll
        for (int j = 0; j < kP4J; ++j) {
          const uint32_t v = (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(dop, q + j * kWave, 0, kNt) |
                             ((uint32_t)__builtin_amdgcn_raw_buffer_load_b8(dfl, q + j * kWave, 0, kNt) << 8);
          ofr[j / 2] = j % 2 ? (ofr[j / 2] | (v << 16)) : v;
        }
      }
#endif
    };
    auto load_ab = [&](int m0, int m1) {  // the operand loads m0 .. m1-1 of the four
      const auto da = rsrc(ca, 8, lnr), db = rsrc(cb, 8, lnr);
      const uint32_t q = row0();
      const uint32_t q2 = q + (q & 63u);  // w * 512 + 2 l
#pragma unroll
      for (int m = m0; m < m1; ++m) {
        aw[m] = __builtin_amdgcn_raw_buffer_load_b128(da, 8 * q2 + m * (16 * kWave), 0, kNt);
        bw[m] = __builtin_amdgcn_raw_buffer_load_b128(db, 8 * q2 + m * (16 * kWave), 0, kNt);
      }
    };
    // One column of the wave's 512 rows through its part of `stg`: written as loaded, read in the rank layout.  The
    // wave's LDS accesses execute in order; the fences keep the compiler from moving a read over a write.
    auto stg_fence = [&]() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront", "local"); };
    // (at the top of a tile: the words landed with the instance column the gathers there wait for)
    auto unpack = [&]() {
#ifndef CC_DIAG_NO_OPFL
      if constexpr (wide) {
        uint32_t o2[kP4J / 2];
#pragma unroll
        for (int j = 0; j < kP4J; ++j) {
          const int src = (j % 4) * 16 + (int)(l >> 2);
          const uint32_t sh = 8u * (l & 3u);
          const uint32_t o = ((uint32_t)__shfl((int)ofr[j / 4], src, kWave) >> sh) & 0xFFu;
          const uint32_t f = ((uint32_t)__shfl((int)ofr[2 + j / 4], src, kWave) >> sh) & 0xFFu;
          o2[j / 2] = j % 2 ? (o2[j / 2] | ((o | (f << 8)) << 16)) : (o | (f << 8));
        }
#pragma unroll
        for (int j = 0; j < kP4J / 2; ++j) ofr[j] = o2[j];
      }
#endif
    };
    load_head(T);
    load_ab(0, kOpLoads);
    for (;;) {
      const uint64_t tile0 = lo + (uint64_t)T * kV3Tile;
      const uint32_t tbase = T * kV3Tile;
      const uint32_t nrow = (uint32_t)(hi - tile0 < (uint64_t)kV3Tile ? hi - tile0 : (uint64_t)kV3Tile);
      const uint32_t Tn = T + gridDim.x;
      for (uint32_t k = l; k < hw; k += kWave) wc[w][k] = 0;
      uint32_t r[kP4J], okm = 0;
      uint64_t rec[kP4J];
      {
        u32x4* s4 = reinterpret_cast<u32x4*>(stg[w]);
        const uint32_t* s1 = reinterpret_cast<const uint32_t*>(stg[w]);
        s4[l] = riw[0];
        s4[kWave + l] = riw[1];
        stg_fence();
#pragma unroll
        for (int j = 0; j < kP4J; ++j) {  // instance -> resource (unconditional gathers; the select comes at the rank)
          const uint32_t ri = s1[j * kWave + l];
          const bool ok = row_below(j, nrow) && ri < max_inst;
          r[j] = inst_res[ok ? ri : 0u];
          okm |= ok ? 1u << j : 0u;
        }
        stg_fence();
      }
      unpack();
      uint64_t av[kP4J], bv[kP4J];
      {
        u32x4* s4 = reinterpret_cast<u32x4*>(stg[w]);
#pragma unroll
        for (int m = 0; m < kP4J / 2; ++m) s4[m * kWave + l] = aw[m];
        stg_fence();
#pragma unroll
        for (int j = 0; j < kP4J; ++j) av[j] = stg[w][j * kWave + l];
        stg_fence();
#pragma unroll
        for (int m = 0; m < kP4J / 2; ++m) s4[m * kWave + l] = bw[m];
        stg_fence();
#pragma unroll
        for (int j = 0; j < kP4J; ++j) bv[j] = stg[w][j * kWave + l];
        stg_fence();
      }
      // (while the gathers fly) every row's record with slot 0, its row set if escaped: nothing in it needs the rank
#pragma unroll
      for (int j = 0; j < kP4J; ++j) {
        const uint32_t ofj = ofr[j / 2] >> (16 * (j % 2));
        rec[j] = v3_set_row(v3_encode(ofj & 0xFFu, (ofj >> 8) & 0xFFu, av[j], bv[j], 0), rowq(j));
        asm volatile("" : "+v"(rec[j]));  // the finished word, here: its parts must not stay live beside the next tile
      }
      // the raw registers are free: the next tile's loads fly through the rest of this tile
      load_head(Tn);
      load_ab(0, kS1);
#pragma unroll
      for (int j = 0; j < kP4J; ++j) {
        const uint32_t g = (okm >> j) & 1u ? r[j] : kNoRes;
        const uint32_t k = g >> KSB, sh = 16 * (k & 1);
        r[j] = g != kNoRes ? g | (((atomicAdd(&wc[w][k >> 1], 1u << sh) >> sh) & 0xFFFFu) << kResBits) : kNoRes;
      }
      PH(0);
      lds_barrier();  // B1: counters complete
      PH(1);
      if (w == 0) {   // per super-bucket: exclusive prefix over the waves (in place), totals, tile-local run starts
        uint32_t tot[KP];
#pragma unroll
        for (int e = 0; e < KP; e += 2) {
          const uint32_t pr = (l * KP + e) / 2;
          uint32_t acc = 0;
          if (pr < hw) {
#pragma unroll
            for (int q = 0; q < kP4W; ++q) {
              const uint32_t x = wc[q][pr];
              wc[q][pr] = acc;
              acc += x;
            }
          }
          tot[e] = acc & 0xFFFFu;
          tot[e + 1] = acc >> 16;
        }
        uint32_t mine = 0;
#pragma unroll
        for (int e = 0; e < KP; ++e) mine += tot[e];
        uint32_t inc = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const uint32_t y = __shfl_up(inc, d, 64);
          if (l >= (uint32_t)d) inc += y;
        }
        uint32_t run = inc - mine;
        uint16_t* row = ttab + (uint64_t)T * (sb + 1);
#pragma unroll
        for (int e = 0; e < KP; ++e) {
          const uint32_t k = l * KP + e;
          if (k < sb) {
            kst[k] = (uint16_t)run;
            row[k] = (uint16_t)run;
          }
          run += tot[e];
        }
        if (l == 63) {
          kst[sb] = (uint16_t)inc;
          row[sb] = (uint16_t)inc;
        }
      }
      load_ab(kS1, kOpLoads);  // the second slice: waves 1-15 issue it while wave 0 scans, wave 0 after its scan
      PH(2);
      lds_barrier();  // B2: prefixes and run starts
      PH(3);
#pragma unroll
      for (int j = 0; j < kP4J; ++j) {
        uint32_t cp = 0xFFFFu;
        if (r[j] != kNoRes) {
          const uint32_t k = (r[j] & ((1u << kResBits) - 1)) >> KSB, sh = 16 * (k & 1);
          const uint32_t sp = kst[k] + ((wc[w][k >> 1] >> sh) & 0xFFFFu) + (r[j] >> kResBits);
          img[sp] = rec[j] | (r[j] & ((1u << KSB) - 1));
          cp = sp;
        }
        if (row_below(j, nrow)) cpos[tbase + rowq(j)] = (uint16_t)cp;
      }
      PH(4);
      lds_barrier();             // B3: the image is complete
      PH(5);
      // whole tile region, unconditionally (a fixed store count; rows past the live count are never read), 16 B a lane
#pragma unroll
      for (int m = 0; m < kP4J / 2; ++m)
        reinterpret_cast<uint4*>(st_rec + tbase)[t + m * kP4T] = reinterpret_cast<const uint4*>(img)[t + m * kP4T];
      PH(6);
      if (Tn >= tiles) break;
      T = Tn;
    }
  };
  if (opfl_al) tile_loop(std::true_type{});
  else tile_loop(std::false_type{});
#ifdef CC_PHASE_TIMING
  PH_FLUSH(g_ph_v3p);
#endif
}

// ---- k_apply_value_v3: walker / loader waves (apply_value.hip k_apply_value_ws) over 8-byte records ------------
// One 1024-thread workgroup per super-bucket: waves 0-3 walk (thread t = slot t, AtomicValueState in registers),
// waves 4-15 load, decode, rank and place the next chunk (3072 records) into the other LDS buffer and store the
// previous chunk's results.  The super-bucket's list is its run in every 8192-commit tile, in tile (= log) order.
//
// The loaders run one chunk further ahead than they place.  While the walkers walk chunk i, a loader wave
// (`loader_iter`) takes its results of chunk i-1 out of the other LDS buffer into registers, decodes its records of
// chunk i+1 (they were loaded during iteration i-1 and ranked at its end), issues the lookups and loads of chunk i+2
// into the freed record registers, packs and stores the results, places chunk i+1 at base + rank, and last -- the
// loads have had the store and the placement to arrive -- ranks chunk i+2 into its per-wave slot counters.  The
// workgroup barrier that ends the iteration then orders the twelve waves' counters before the scan: at the top of
// the next iteration ONE loader wave (a different one each chunk) turns them in place into placement bases (slot
// start + the counts of the waves before, k_part_v4's wave-0 scan) and the walkers' slot starts, and posts on the
// LDS counter `lbar`.  Nobody needs the bases before its placement, most of an iteration later, so the wait for the
// post falls through: no loader wave waits for another in the steady state, and rank and slot of a record (one
// packed register each) are the only ranking state that lives across the barrier.
//
// A record's staging position is c + (rstart - rpre) of its run: the wave holds a window of 64 runs (a lane each), pushes one flag per run boundary to the lane
// the boundary falls on (ds_permute) and counts the flags at or below each lane (ballot + mbcnt); a window with an
// empty run (two boundaries on one lane) or with more than 64 runs takes the per-wave search instead.
// The workgroups of one XCD (blockIdx b and b + 8 share one) take a contiguous range of super-buckets (`s` below),
// so the 128-byte lines two neighbouring super-buckets share at their run boundaries meet in one L2.
//
// LDS hazards (the chunk pipeline; cf. the k_apply_map chunk-0 race).  B(i) is the workgroup barrier that
// ends iteration i (the walk of chunk i); B(-2) and B(-1) are the prologue's two.  Loader iteration i places chunk
// i+1; the prologue's (between B(-2) and B(-1), no walk beside it) is iteration -1 and places chunk 0.
//   * buffer b = c & 1 is placed with chunk c during iteration c-1 and walked during iteration c; B(c-1) separates the
//     two.  The walkers' in-place results in it are read back by the loaders in iteration c+1, after B(c);
//   * those result reads (sab[b] at the top of `loader_iter`) must precede every wave's placement of chunk c+2 into
//     the same buffer in the same iteration.  Nothing else orders two loader waves there any more, so each wave
//     arrives on the LDS counter `rbar` once its results are in registers and waits for all twelve arrivals of the
//     iteration before its first placement.  The arrivals are the first thing after the barrier and the placement
//     comes after the decode, the lookups and the result store, so the wait falls through;
//   * wcnt (one buffer).  Row w is zeroed and ranked by wave w alone, at the end of iteration i-1 (chunk i+1), after
//     that wave's placement of chunk i has read the row's previous bases (one wave's LDS accesses stay in order);
//     read and rewritten by the scanning wave at the top of iteration i, after B(i-1); read by wave w's placement of
//     chunk i+1 after the post; zeroed again after that placement.  The scan of chunk i+2 comes after B(i);
//   * sstart[c & 1] is written by chunk c's scan at the top of iteration c-1, while the walkers read sstart[(c-1) & 1];
//     they read it at the top of iteration c, after B(c-1), and are done with chunk c-2's before B(c-2);
//   * the counters only grow and every wave counts the same targets in a register: rbar by twelve per loader
//     iteration (target 12, 24, ...: rd_n), lbar by one per chunk (the post of chunk c makes it c + 1).
//     Prologue: every loader wave loads and ranks chunk 0; B(-2); iteration -1: wave 0 scans chunk 0 and posts
//     (lbar = 1), all read dummy results, arrive (rbar = 12), load chunk 1, wait for rbar >= 12 and lbar >= 1 -- the
//     one place where the post is really waited for -- place chunk 0 and rank chunk 1; B(-1).
//     Steady state, iteration i = 0 .. nch-1: wave (i+1) % 12 scans chunk i+1 and posts (lbar = i + 2); all arrive
//     (rbar = 12 (i + 2)), wait for both, place chunk i+1, rank chunk i+2; B(i).  The posts are one barrier apart,
//     so lbar >= c + 1 means exactly "chunk c is scanned"; the scanning wave rotates with the chunk and wraps after
//     twelve.  The chunks past the end (nch and nch + 1) are loaded from the dummy words, ranked, scanned and
//     "placed" like any other with no live record, so no count depends on where the list ends.
//     Epilogue: after B(nch-1) the loaders store the last chunk's results; no counter is touched.  At the end
//     lbar = nch + 1 and rbar = 12 (nch + 1).
//     nch = 0: the prologue alone (lbar = 1, rbar = 12), no walk.  nch = 1: the prologue and iteration 0, whose
//     scan, placement and rank are of empty chunks.  nch = 2: chunk 1 is the last one placed with live records (in
//     iteration 0).  nch >= 3: every role above is live.  No wait depends on anything but the workgroup-uniform
//     iteration count, and every wait's arrivals precede a barrier the waiting wave has not reached yet;
//   * rb0 / rpre (the run table) are written once, before the first workgroup barrier, and never rebuilt.
constexpr int kWsPer = 4;
// NS slots per super-bucket: 256 (1024-thread workgroups: 4 walker + 12 loader waves, 3072-record chunks, one
// workgroup per CU) or 128 (512-thread workgroups: 2 walker + 6 loader waves, 1536-record chunks, 79 KB of LDS: two
// workgroups per CU, so one workgroup's per-chunk loader chain -- rank, arrival barrier, placement bases, placement
// -- overlaps the other's; with one workgroup per CU that chain, not the bytes, bounded the launch: 0.60 ms/step
// with contiguous loads and no walk at all, profiles/r03/diag1).
template <int NS>
struct V3A {
  static constexpr int WW = NS / kWave;               // walker waves
  static constexpr int LW = NS == 128 ? 6 : 12;       // loader waves
  static constexpr int T = (WW + LW) * kWave;         // workgroup threads
  static constexpr int W = T / kWave;
  static constexpr int CH = LW * kWave * kWsPer;      // records per chunk
  static constexpr int NP = NS / 2;                   // packed u16 counter pairs
  static constexpr int SPL = NS / kWave;              // slots per loader lane in the placement bases
  static constexpr int TPT = (kV3MaxTiles + T - 1) / T;  // run-table tiles per thread
  static constexpr int MINW = NS == 128 ? 4 : 1;      // waves per SIMD asked of the register allocator
};

__device__ inline uint32_t v3_value_walk(uint32_t m, uint64_t x, uint64_t y, uint32_t& ms, uint64_t& v, uint64_t& rv) {
  const uint32_t tag = ms & 0xFFu;
  // compareAndSet :124 (value == null && expect == null) || (value != null && value.equals(expect))
  const bool ceq = (m & kM3C) != 0 && ((m >> 12) & 7u) == tag && v == x;
  const bool is_r = (m & kM3R) != 0;
  const bool wr = (m & kM3W) != 0 || ceq;  // (a delete writes "no value": y = 0, meta 0)
  rv = is_r ? v : (ceq ? 1ull : 0ull);
  const uint32_t st = is_r ? (tag << 4) : (m & 0xFFu);
  ms = wr ? (m >> 16) : ms;
  v = wr ? y : v;
  return st;
}

// Largest r in [0, tiles) with rpre[r] <= c (two-round 64-ary search by the whole wave; tiles <= 4096).
__device__ inline uint32_t v3_find_run(const uint32_t* rpre, uint32_t tiles, uint32_t c) {
  const uint32_t l = __lane_id();
  const uint32_t step = (tiles + kWave - 1) / kWave;
  uint32_t cand = l * step;
  uint64_t b = __ballot(cand < tiles && rpre[cand] <= c);
  const uint32_t base = (uint32_t)(63 - __clzll((long long)b)) * step;
  cand = base + l;
  b = __ballot(l < step && cand < tiles && rpre[cand] <= c);
  return base + (uint32_t)(63 - __clzll((long long)b));
}

// The loaders' LDS counter: arrive (this wave's earlier LDS accesses are done), wait (the counter reached target).
__device__ inline void v3_loader_arrive(uint32_t* ctr) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  if (__lane_id() == 0) __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ inline void v3_loader_wait(uint32_t* ctr, uint32_t target) {
  while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < target) __builtin_amdgcn_s_sleep(1);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

template <int NS>
__global__ __launch_bounds__(V3A<NS>::T, V3A<NS>::MINW) void k_apply_value_v3(const uint64_t* __restrict__ st_rec,
                                                        uint32_t* __restrict__ rst_word,
                                                        const uint64_t* __restrict__ ca, const uint64_t* __restrict__ cb,
                                                        uint64_t lo, const uint16_t* __restrict__ ttab, uint32_t tiles,
                                                        uint32_t sb, uint32_t* __restrict__ val_meta,
                                                        uint64_t* __restrict__ val_v, uint64_t* __restrict__ rst_value,
                                                        uint64_t dummy,
                                                        uint32_t* __restrict__ err_out) {
  using P = V3A<NS>;
#ifdef CC_DIAG  // diagnostics build only (-DCC_DIAG=1: no walk, 2: contiguous positions -- wrong results by design; 4: internal checks only, common.h kErrSmallFlag)
  constexpr uint32_t diag = CC_DIAG;
#else
  constexpr uint32_t diag = 0;
#endif
  constexpr int kWsLW = P::LW, kWsCh = P::CH, kAVW = P::W, kVSlots3 = NS, kVPairs3 = P::NP;
  constexpr uint32_t kL0 = P::WW * kWave;       // first loader thread
  __shared__ u64x2 sab[2][kWsCh];               // chunk buffers sorted by slot; results in place {value, status}
  __shared__ uint32_t sm[2][kWsCh];             //   meta words
  // per-loader-wave slot counts (packed u16 pairs); after the chunk's scan, in place: the sorted position of the
  // wave's first record of each slot (a chunk holds 3072 records at most, so positions fit the u16 halves too)
  __shared__ uint32_t wcnt[kWsLW][kVPairs3];
  __shared__ uint32_t sstart[2][kVSlots3 + 1];  // slot run starts of each buffer (+ total)
  __shared__ uint16_t rb0[kV3MaxTiles];         // start of this super-bucket's run inside tile r
  __shared__ uint32_t rpre[kV3MaxTiles + 1];    // records of this super-bucket before tile r
  __shared__ uint32_t wsum[kAVW];
  __shared__ uint32_t lbar, rbar;               // the loaders' counters: chunks posted, result-read arrivals
  auto rstart = [&](uint32_t r) -> uint32_t { return r * kV3Tile + rb0[r]; };  // staging position of run r

  // Workgroups b and b + 8 share an XCD (observed dispatch; speed only, any placement gives the same results):
  // workgroup 8y + x takes super-bucket x*q + min(x, r) + y (q = grid / 8, r = grid % 8), a bijection for any grid
  // that gives the workgroups of one XCD a contiguous range of super-buckets.
  const uint32_t gx_ = blockIdx.x & 7u, gq_ = gridDim.x >> 3, gr_ = gridDim.x & 7u;
  const uint32_t s = gx_ * gq_ + (gx_ < gr_ ? gx_ : gr_) + (blockIdx.x >> 3);
  const uint32_t t = threadIdx.x, w = t >> 6, l = t & 63;
  const bool walker = t < kL0;
  const uint32_t lw = walker ? 0u : w - P::WW;
  uint32_t ms = 0;
  uint64_t sv = 0;
  if (walker) {
    ms = val_meta[(uint64_t)s * kVSlots3 + t];
    sv = val_v[(uint64_t)s * kVSlots3 + t];
  }
  if (t == 0) lbar = rbar = 0;  // (wcnt: every loader wave zeroes its row before it ranks)
  {  // the super-bucket's list = its run in every tile, in tile order; thread t owns tiles TPT*t .. TPT*t + TPT-1
    uint32_t len[P::TPT], lsum = 0;
#pragma unroll
    for (int q = 0; q < P::TPT; ++q) {
      const uint32_t tt = P::TPT * t + q;
      len[q] = 0;
      if (tt < tiles) {
        const uint16_t* row = ttab + (uint64_t)tt * (sb + 1);
        const uint32_t b0 = row[s], b1 = row[s + 1];
        rb0[tt] = (uint16_t)b0;
        len[q] = b1 - b0;
      }
      lsum += len[q];
    }
    uint32_t inc = lsum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t y = __shfl_up(inc, d, 64);
      if (l >= (uint32_t)d) inc += y;
    }
    if (l == 63) wsum[w] = inc;
    lds_barrier();
    uint32_t pre = inc - lsum, all = 0;
    for (uint32_t q = 0; q < (uint32_t)kAVW; ++q) {
      const uint32_t x = wsum[q];
      if (q < w) pre += x;
      all += x;
    }
#pragma unroll
    for (int q = 0; q < P::TPT; ++q) {
      if (P::TPT * t + q < tiles) rpre[P::TPT * t + q] = pre;
      pre += len[q];
    }
    if (t == 0) rpre[tiles] = all;
    lds_barrier();
  }
  const uint32_t cnt = rpre[tiles];
  const uint32_t nch = (cnt + kWsCh - 1) / kWsCh;
  uint32_t err = 0, macc = 0;  // macc: OR of the meta words this thread walked
#ifdef CC_PHASE_TIMING
  // thread 0 (walker): 0 walk, 1 wait; thread 256 (loader): 2 result store, 3 clear + rank (with the wait for the
  // loads), 4 counter waits + workgroup barriers, 5 placement bases, 6 result reads + decode + place, 7 load issue
  uint64_t wph_last = wall_clock64(), wph[kPhases] = {0, 0, 0, 0, 0, 0, 0, 0};
  auto WPH = [&](int k) {
    if (t == 0 || t == kL0) {
      const uint64_t n_ = wall_clock64();
      wph[k] += n_ - wph_last;
      wph_last = n_;
    }
  };
#else
  auto WPH = [&](int) {};
#endif

  // loader registers: the chunk to place next (rr, g; loaded and ranked one iteration ahead), the sorted / staging
  // positions of the chunk being walked (pp, gp) and of the chunk before it (qp, gq: its results are stored during
  // the walk)
#define CC_J4(X) X(0) X(1) X(2) X(3)
  // A record past the end of the list has the staging position dpos, one of the dummy words behind the staging area
  // (its loads and result stores stay unconditional): a position is live iff it is below dpos0.
  const uint32_t dpos0 = (uint32_t)dummy, dpos = dpos0 + t;
#define CC_DECL(J) uint32_t g##J = dpos, pp##J = 0, gp##J = dpos, qp##J = 0, gq##J = dpos; uint64_t rr##J = 0;
  CC_J4(CC_DECL)
#undef CC_DECL
  // record c0 + lw*256 + j*64 + l of the list (log order = (loader wave, j, lane)).
  // Staging position of list record c: the run r holding it gives c + (rstart[r] - rpre[r]).  One 64-ary search per
  // wave and chunk finds the wave's first run; lane k then holds the end wB and the offset wD of window run rrow + k.
  // Per 64-record group: the runs that end at or before the group's first record are counted with one ballot; every
  // run that ends inside the group (at record crow + d, 0 < d < 64) pushes a flag to lane d, and lane l's run is the
  // first one plus the flags on lanes 1..l.  (Lanes with nothing to push target lane 0, whose flag is not counted.
  // The window runs that matter are non-empty -- `win` -- so no two of them push to one lane.)
#define CC_LOAD1(J)                                                                               \
  {                                                                                               \
    const uint32_t crow = c0w + (J) * kWave, c = crow + l;                                        \
    uint32_t gpos = dpos;                                                                         \
    if (crow < cnt) { /* wave-uniform */                                                          \
      if (win) {                                                                                  \
        const uint32_t ri0 = (uint32_t)__popcll(__ballot(wB <= crow));                            \
        const uint32_t d_ = wB - crow;                                                            \
        const uint32_t fl_ = (uint32_t)__builtin_amdgcn_ds_permute((int)((d_ - 1u < kWave - 1u ? d_ : 0u) << 2), 1); \
        const uint64_t fm_ = __ballot(fl_ != 0) >> 1;                                             \
        const uint32_t ri = __builtin_amdgcn_mbcnt_hi((uint32_t)(fm_ >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)fm_, ri0)); \
        const uint32_t rd_ = (uint32_t)__shfl((int)wD, (int)ri, 64);                              \
        if (c < cnt) gpos = c + rd_;                                                              \
      } else {                                                                                    \
        uint32_t r = v3_find_run(rpre, tiles, crow);                                              \
        if (c < cnt) {                                                                            \
          while (rpre[r + 1] <= c) ++r;                                                           \
          gpos = rstart(r) + (c - rpre[r]);                                                       \
        }                                                                                         \
      }                                                                                           \
    }                                                                                             \
    if (diag & 2u) gpos = c < cnt ? c : dpos; /* diagnostics: contiguous positions (wrong results) */ \
    g##J = gpos;                                                                                  \
    rr##J = *v3_at(st_rec, gpos);                                                                 \
  }
#define CC_LOAD_CHUNK(C0)                                                                         \
  {                                                                                               \
    const uint32_t c0w = (C0) + lw * (kWave * kWsPer);                                            \
    uint32_t wB = 0xFFFFFFFFu, wD = 0;                                                            \
    bool win = false;                                                                             \
    if (c0w < cnt) {                                                                              \
      const uint32_t rrow = v3_find_run(rpre, tiles, c0w);                                        \
      const uint32_t kr = rrow + l;                                                               \
      const uint32_t wP = kr < tiles ? rpre[kr] : 0xFFFFFFFFu;                                    \
      wB = kr < tiles ? rpre[kr + 1] : 0xFFFFFFFFu;                                               \
      wD = kr < tiles ? rstart(kr) - wP : 0u;                                                     \
      const uint32_t lastc = c0w + kWave * kWsPer - 1 < cnt ? c0w + kWave * kWsPer - 1 : cnt - 1; \
      /* the window reaches past the wave's last record, and none of its runs up to there is empty */ \
      win = (uint32_t)__shfl((int)wB, 63, 64) > lastc && __ballot(wB == wP && wP <= lastc) == 0;  \
    }                                                                                             \
    CC_J4(CC_LOAD1)                                                                               \
  }
  uint32_t rd_n = 0;  // rbar after the previous loader iteration (twelve result-read arrivals each)
  // the registers' chunk as ranked at the end of the iteration before: rank (< 3072) | slot << 16
  uint32_t rs0 = 0, rs1 = 0, rs2 = 0, rs3 = 0;
  // the results of the chunk walked before (buffer b, positions qp / gq) into registers, ahead of the placement that
  // overwrites them; then into rst_word at the records' staging positions: one packed 4-byte word per result
  // (v3_pack_result), unconditional stores (rows past the end go to the dummy words).  A value that does not fit the
  // word's 24 bits also goes to rst_value: looked for once per wave and group, so the common path has no per-lane
  // branch.
#define CC_RES_READ(J) const u64x2 re##J = sab[b][qp##J];
#define CC_RES_WRITE(J)                                                             \
  {                                                                                 \
    const bool esc_ = !v3_res_fits(re##J.x) && gq##J < dpos0;                       \
    uint32_t wd_ = v3_pack_result((uint32_t)re##J.y, re##J.x, false);               \
    if (__ballot(esc_)) { /* wave-uniform, rare */                                  \
      if (esc_) {                                                                   \
        wd_ = v3_pack_result((uint32_t)re##J.y, re##J.x, true);                     \
        *v3_at(rst_value, gq##J) = re##J.x;                                         \
      }                                                                             \
    }                                                                               \
    *v3_at(rst_word, gq##J) = wd_;                                                  \
  }
  // Rank the registers' chunk into this wave's counter row (the last thing a loader wave does before a workgroup
  // barrier: the barrier, not a counter, orders the twelve rows before the scan that follows it).
  auto rank_chunk = [&]() {
    for (uint32_t k = l; k < (uint32_t)kVPairs3; k += kWave) wcnt[lw][k] = 0;
#define CC_RANK1(J)                                                                 \
    {                                                                               \
      const uint32_t sl_ = v3_slot(rr##J), sh_ = 16 * (sl_ & 1);                    \
      const uint32_t rk_ = g##J < dpos0 ? (atomicAdd(&wcnt[lw][sl_ >> 1], 1u << sh_) >> sh_) & 0xFFFFu : 0u; \
      rs##J = rk_ | (sl_ << 16);                                                    \
    }
    CC_J4(CC_RANK1)
#undef CC_RANK1
    WPH(3);
  };
  // One loader wave per chunk (c % 12, at the top of the iteration that places chunk c) turns the twelve rows into
  // chunk c's placement bases and the walkers' sstart[b] (b = c & 1), and posts: lbar = chunks posted.
  auto scan_chunk = [&](uint32_t b) {
    // lane l owns slots SPL*l .. SPL*l + SPL-1 (counter pairs PPL*l ..): the slots' totals over the waves, their
    // exclusive scan (the slot starts), then each wave's counter replaced by start + the counts of the waves before
    constexpr int PPL = P::SPL / 2;
    uint32_t acc[PPL], mine = 0;
#pragma unroll
    for (int e = 0; e < PPL; ++e) acc[e] = 0;
#pragma unroll
    for (int q = 0; q < kWsLW; ++q) {
#pragma unroll
      for (int e = 0; e < PPL; ++e) acc[e] += wcnt[q][PPL * l + e];
    }
#pragma unroll
    for (int e = 0; e < PPL; ++e) mine += (acc[e] & 0xFFFFu) + (acc[e] >> 16);
    uint32_t inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t y = __shfl_up(inc, d, 64);
      if (l >= (uint32_t)d) inc += y;
    }
    uint32_t run = inc - mine;
#pragma unroll
    for (int e = 0; e < PPL; ++e) {
      const uint32_t k = P::SPL * l + 2 * e;
      const uint32_t lo_ = run, hi_ = run + (acc[e] & 0xFFFFu);
      sstart[b][k] = lo_;  // the walkers' run starts of chunk c (read after the next workgroup barrier)
      sstart[b][k + 1] = hi_;
      run = hi_ + (acc[e] >> 16);
      acc[e] = lo_ | (hi_ << 16);
    }
    if (l == 63) sstart[b][kVSlots3] = inc;
#pragma unroll
    for (int q = 0; q < kWsLW; ++q) {
#pragma unroll
      for (int e = 0; e < PPL; ++e) {
        const uint32_t cv = wcnt[q][PPL * l + e];
        wcnt[q][PPL * l + e] = acc[e];
        acc[e] += cv;  // no carry between the halves: every sum is a position <= 3072
      }
    }
    WPH(5);
    v3_loader_arrive(&lbar);  // the post: chunk c's bases are in wcnt
  };
  // One loader iteration, beside the walk of chunk c-1: chunk c's scan (one wave), the results of chunk c-2 out of
  // buffer b = c & 1, the registers' chunk c (ranked before the last barrier, rs) decoded and placed into buffer b,
  // chunk c+1 loaded into the freed registers and ranked.
  auto loader_iter = [&](uint32_t c, uint32_t b) {
    if (lw == c % (uint32_t)kWsLW) scan_chunk(b);  // wave-uniform
    CC_J4(CC_RES_READ)
    v3_loader_arrive(&rbar);  // chunk c-2's results of this wave are in registers
#define CC_DEC1(J)                                                                  \
    const bool live##J = g##J < dpos0;                                              \
    uint32_t m##J;                                                                  \
    uint64_t x##J, y##J;                                                            \
    v3_decode(rr##J, m##J, x##J, y##J);                                             \
    if (__ballot(live##J && (((uint32_t)rr##J >> 17) & 1u))) { /* wave-uniform, rare: an escaped record */ \
      if (live##J && (((uint32_t)rr##J >> 17) & 1u))                                \
        v3_decode_escaped(rr##J, ca, cb, lo + (uint64_t)(g##J / kV3Tile) * kV3Tile, x##J, y##J); \
    }
    CC_J4(CC_DEC1)
#undef CC_DEC1
    WPH(6);
    // the records are decoded: their registers take chunk c+1 (lookups, then the loads; the result store and the
    // placement below run while the loads are in flight)
#define CC_KEEP1(J) const uint32_t gc##J = g##J;
    CC_J4(CC_KEEP1)
#undef CC_KEEP1
    CC_LOAD_CHUNK((c + 1) * (uint32_t)kWsCh)
    WPH(7);
    CC_J4(CC_RES_WRITE)
    WPH(2);
#define CC_SHIFT1(J) qp##J = pp##J; gq##J = gp##J; gp##J = gc##J;
    CC_J4(CC_SHIFT1)
#undef CC_SHIFT1
    rd_n += kWsLW;
    v3_loader_wait(&rbar, rd_n);      // every loader wave holds its results of chunk c-2: buffer b may be overwritten
    v3_loader_wait(&lbar, c + 1);     // chunk c's bases are posted (at the top of this iteration)
    WPH(4);
    const uint16_t* pb = reinterpret_cast<const uint16_t*>(&wcnt[lw][0]);  // u16 half k = slot k (little endian)
#define CC_PLACE1(J)                                                                \
    {                                                                               \
      pp##J = live##J ? pb[rs##J >> 16] + (rs##J & 0xFFFFu) : 0u;                   \
      if (live##J) {                                                                \
        sm[b][pp##J] = m##J;                                                        \
        sab[b][pp##J] = u64x2{x##J, y##J};                                          \
      }                                                                             \
    }
    CC_J4(CC_PLACE1)
#undef CC_PLACE1
    WPH(6);
    rank_chunk();  // chunk c+1 (waits for its loads)
  };

  if (!walker) {  // prologue: chunk 0 loaded and ranked; then one loader iteration without a walk
    CC_LOAD_CHUNK(0)
    rank_chunk();
  }
  lds_barrier();
  if (!walker) loader_iter(0, 0);  // chunk 0 scanned and placed, chunk 1 loaded and ranked
  lds_barrier();
  for (uint32_t i = 0; i < nch; ++i) {
    const uint32_t b = i & 1;
    if (walker) {
      const uint32_t start = sstart[b][t], run = (diag & 1u) ? 0u : sstart[b][t + 1] - start;
      if (run) {
        uint32_t mA[4], mB[4];
        u64x2 xA[4], xB[4];
        const uint32_t last = start + run - 1;
        auto fetch = [&](uint32_t k0, uint32_t (&mm)[4], u64x2 (&xx)[4]) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const uint32_t pq = min(start + k0 + q, last);
            mm[q] = sm[b][pq];
            xx[q] = sab[b][pq];
          }
        };
        auto walk4 = [&](uint32_t k0, const uint32_t (&mm)[4], const u64x2 (&xx)[4]) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if (k0 + q < run) {
              uint64_t rv;
              const uint32_t stt = v3_value_walk(mm[q], xx[q].x, xx[q].y, ms, sv, rv);
              macc |= mm[q];
              // the result over the record, one 16-byte LDS write: with 2 reads + 1 write per record, a group of 4
              // records' reads plus the previous group's writes stay within the 15 outstanding LDS operations a
              // wave can wait on precisely (two writes per record overflowed it and serialised the pipeline)
              sab[b][start + k0 + q] = u64x2{rv, (uint64_t)stt};
            }
          }
        };
        fetch(0, mA, xA);
        for (uint32_t k0 = 0; k0 < run; k0 += 8) {
          fetch(k0 + 4, mB, xB);
          walk4(k0, mA, xA);
          if (k0 + 4 >= run) break;
          fetch(k0 + 8, mA, xA);
          walk4(k0 + 4, mB, xB);
        }
      }
    } else {
      // chunk i-1's results (i = 0: the dummy rows), chunk i+1's scan and placement (past the end: no live records),
      // chunk i+2's loads and rank (past the end: empty)
      loader_iter(i + 1, b ^ 1);
    }
    if (walker) WPH(0);
    lds_barrier();  // buffer hand-over: b walked (results in place), b^1 placed
    WPH(walker ? 1 : 4);
  }
  if (!walker && nch) {  // the last chunk's results (qp / gq since its walk)
    const uint32_t b = (nch - 1) & 1;
    CC_J4(CC_RES_READ)
    CC_J4(CC_RES_WRITE)
  }
  if (macc & kM3L) err |= kErrUnsupported;  // a listen / unlisten record among the walked ones
#ifdef CC_PHASE_TIMING
  if (t == 0 || t == kL0)
    for (int q = 0; q < kPhases; ++q) atomicAdd(&g_ph_v3a[q], (unsigned long long)wph[q]);
#endif
#undef CC_RES_READ
#undef CC_RES_WRITE
#undef CC_LOAD_CHUNK
#undef CC_LOAD1
#undef CC_J4
  if (walker) {
    val_meta[(uint64_t)s * kVSlots3 + t] = ms;
    val_v[(uint64_t)s * kVSlots3 + t] = sv;
  }
  if (err) atomicOr(err_out, err);
}

// ---- k_unpermute_v3: the packed results back to log order ----------------------------------------------------
// partition.hip k_unpermute over packed 4-byte result words: per 8192-commit tile (persistent, two 512-thread
// workgroups per CU), the tile's staged words are read contiguously into a 32 KB LDS image (the next tile's are loaded
// into registers meanwhile: 4 sixteen-byte loads of words and 4 eight-byte loads of cpos per thread), then the
// results are gathered through cpos and written in log order.  Unknown-session rows (cpos 0xFFFF) get
// UNKNOWN_SESSION here (ResourceManager.java:60-69).  6 B read and 9 B written per commit.
//
// The stores are whole lines: a wave's cpos load covers 256 commits, four a lane; the lanes trade them (two shuffles
// per half) so that lane l writes commits 2l, 2l+1 of each half of 128 -- a value store of the wave is 1 KB contiguous
// and a status store one 128-byte line -- and the stores are nontemporal: the outputs are written once and no kernel
// of this pipeline reads them, so they need not stay in the caches the staging arrays are read from (a cache policy
// only: a later reader, the result encoder or a copy, sees them like any other store).  Measured on c2 (ms per
// step of this kernel, two runs each): four commits a lane (16-byte value stores at a 32-byte stride) 0.277-0.283;
// the same nontemporal 0.340 (half-written lines no longer meet in L2); whole lines 0.270; whole lines nontemporal
// 0.241.  Workgroups per CU, before the stores changed: two 0.276, three 0.280, four (64 VGPRs: 44 B of scratch)
// 0.333.
constexpr int kU3T = 512;
constexpr int kU3Wg = 2;  // workgroups per CU the grid is sized for
typedef unsigned long long ull2 __attribute__((ext_vector_type(2)));
template <int NT, int TL>
__global__ __launch_bounds__(NT) void k_unpermute_v3(const uint16_t* __restrict__ cpos, uint32_t tiles, uint64_t n,
                                                   const uint32_t* __restrict__ words, const uint64_t* __restrict__ esc_value,
                                                   uint8_t* __restrict__ out_status, uint64_t* __restrict__ out_value,
                                                   uint8_t* __restrict__ dummy_status, uint64_t* __restrict__ dummy_value) {
  constexpr int kUnVal = TL / (4 * NT);  // 16-byte four-word loads per thread per tile (4)
  constexpr int kUnPos = TL / (4 * NT);  // 4-commit cpos groups per thread per tile (4)
  static_assert(kUnVal == 4 && kUnPos == 4, "unpermute prefetch registers");
  __shared__ uint4 lw4[TL / 4];
  const uint32_t* lw = reinterpret_cast<const uint32_t*>(lw4);
  const uint32_t t = threadIdx.x, l = t & 63u;
  // prefetch registers as named scalars (an array would live in scratch and make every prefetch wait)
  uint4 v0, v1, v2, v3;
  uint2 p0, p1, p2, p3;
  auto load = [&](uint32_t TT) {
    const uint64_t i0 = (uint64_t)TT * TL;
    const uint4* sv = reinterpret_cast<const uint4*>(words + i0) + t;
    const uint2* sp = reinterpret_cast<const uint2*>(cpos + i0) + t;
    v0 = sv[0 * NT]; v1 = sv[1 * NT]; v2 = sv[2 * NT]; v3 = sv[3 * NT];
    p0 = sp[0 * NT]; p1 = sp[1 * NT]; p2 = sp[2 * NT]; p3 = sp[3 * NT];
  };
  uint32_t T = blockIdx.x;
  load(T < tiles ? T : tiles - 1);
  const uint8_t unk = CC_STATUS(CC_ST_UNKNOWN_SESSION, CC_TAG_NULL);
  uint64_t tail_i = ~0ull, tail_v = 0;
  uint32_t tail_sw = 0;
  for (; T < tiles; T += gridDim.x) {
    lds_barrier();  // the previous tile's scatter is done reading LDS
    lw4[t + 0 * NT] = v0; lw4[t + 1 * NT] = v1; lw4[t + 2 * NT] = v2; lw4[t + 3 * NT] = v3;
    const uint2 pp[kUnPos] = {p0, p1, p2, p3};
    lds_barrier();
    load(T + gridDim.x < tiles ? T + gridDim.x : tiles - 1);
    const uint64_t i0 = (uint64_t)T * TL;
#pragma unroll
    for (int k = 0; k < kUnPos; ++k) {
      // lane j holds the cpos of commits w0 + 4j .. 4j+3 (w0: the wave's first commit of this group); lane l takes
      // commits w0 + 128h + 2l, +1: one half of lane 32h + l/2's four
      const uint64_t w0 = i0 + 4 * (uint64_t)(t - l + k * NT);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int src = 32 * h + (int)(l >> 1);
        const uint32_t px = (uint32_t)__shfl((int)pp[k].x, src, 64), py = (uint32_t)__shfl((int)pp[k].y, src, 64);
        const uint32_t pr = (l & 1u) ? py : px;
        const uint32_t p[2] = {pr & 0xFFFF, pr >> 16};
        const uint64_t i = w0 + 128 * h + 2 * l;  // commits i, i+1
        uint32_t sw = 0;
        uint64_t v[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const bool ok = p[q] != 0xFFFF;
          const uint32_t wd = ok ? lw[p[q]] : 0;
          uint64_t x = v3_result_payload(wd);
          if (wd >> 31) x = esc_value[i0 + p[q]];  // escaped payload (rare)
          sw |= (uint32_t)(ok ? (wd >> kV3ResBits) & 0x7Fu : unk) << (8 * q);
          v[q] = x;
        }
        const bool in = i + 2 <= n;
        uint16_t* os = in ? reinterpret_cast<uint16_t*>(out_status) + i / 2 : reinterpret_cast<uint16_t*>(dummy_status) + t;
        ull2* ov = in ? reinterpret_cast<ull2*>(out_value) + i / 2 : reinterpret_cast<ull2*>(dummy_value) + t;
        __builtin_nontemporal_store((uint16_t)sw, os);
        __builtin_nontemporal_store(ull2{v[0], v[1]}, ov);
        if (!in && i < n) {  // the straddling pair (at most one in the grid): its first commit, written after the loop
          tail_sw = sw;
          tail_v = v[0];
          tail_i = i;
        }
      }
    }
  }
  if (tail_i != ~0ull) {  // commit n-1 of an odd n
    out_status[tail_i] = (uint8_t)tail_sw;
    out_value[tail_i] = tail_v;
  }
}

int launch_unpermute_v3(const UnpermuteArgs& a, const uint32_t* words, hipStream_t st) {
  const uint64_t n = a.hi - a.lo;
  const uint64_t t3 = (n + kV3Tile - 1) / kV3Tile;
  const uint32_t grid = (uint32_t)(t3 < (uint64_t)kU3Wg * kPersistGrid ? t3 : (uint64_t)kU3Wg * kPersistGrid);
  hipLaunchKernelGGL((k_unpermute_v3<kU3T, kV3Tile>), dim3(grid), dim3(kU3T), 0, st, a.cpos, (uint32_t)t3, n, words,
                     a.rst_value, a.out_status + a.lo, a.out_value + a.lo, a.dummy_status, a.dummy_value);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Slots per value super-bucket: 256.  (128-slot buckets -- two 512-thread apply workgroups per CU -- measured slower
// on c2: apply 0.91 -> 0.98, partition 0.88 -> 0.92 ms/step, profiles/r03/ab_ns128: the apply is bound by the loaders'
// instruction and LDS throughput, not by the latency a second workgroup would hide, and 16-record runs over-fetch.)
// Any tile count the staging holds (a.dummy: its positions): a sub-batch, or a value-only engine's whole group.  The
// kV3MaxTiles limit is the apply's run table's and is checked where it lives, launch_apply_value_v3.
int launch_part_v3(const PartArgs& a, uint32_t tiles, hipStream_t st) {
  if (a.sb > (uint32_t)kMaxSb || (uint64_t)tiles * kV3Tile > a.dummy) return -1;
  const uint32_t grid = tiles < (uint32_t)kPersistGrid ? tiles : (uint32_t)kPersistGrid;
  const uint32_t kp = (a.sb + kWave - 1) / kWave;  // super-buckets per lane of the scan wave
#define CC_LAUNCH4(KP)                                                                                                 \
  hipLaunchKernelGGL((k_part_v4<KP, 8>), dim3(grid), dim3(kP4T), 0, st, a.inst, a.op, a.flags, a.a, a.b, a.lo, a.hi,   \
                     a.inst_res, a.max_inst, a.sb, tiles, reinterpret_cast<uint64_t*>(a.st_ab), a.cpos, a.ttab)
  if (kp <= 2) CC_LAUNCH4(2);
  else if (kp <= 4) CC_LAUNCH4(4);
  else CC_LAUNCH4(8);
#undef CC_LAUNCH4
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_apply_value_v3(const ValueArgs& a, hipStream_t st) {
  // (the kernel keeps staging positions, the dummy words' among them, in 32 bits, and their byte offsets too: v3_at)
  if (a.tiles > (uint32_t)kV3MaxTiles || a.dummy + V3A<256>::T > (1ull << 29)) return -1;
  hipLaunchKernelGGL(k_apply_value_v3<256>, dim3(a.sb_val), dim3(V3A<256>::T), 0, st,
                     reinterpret_cast<const uint64_t*>(a.st_ab), a.rst_word, a.ca, a.cb, a.lo, a.ttab, a.tiles, a.sb, a.val_meta, a.val_v,
                     a.rst_value, a.dummy, a.err);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace cc
