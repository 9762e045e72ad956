// wire_gpu.hip — the Catalyst wire format decoded on the GPU: wire bytes in, the ordinary wide columns in HBM out
// (include/copycat_apply.h "the same decode on the GPU"; the format and the host decoder: wire.cpp, wire_plain.h).
//
// k_wire_decode: one workgroup of 256 lanes per tile of CC_WIRE_TILE_ROWS consecutive entries, taken as groups of 256
// entries, lane i the i-th entry of the group.
//   1. Staging.  An entry longer than the longest plain entry (kWirePlainMax, 65 bytes) escapes without a byte being
//      read.  The others' bytes go global -> LDS with 16-byte loads, lane i the i-th 16 bytes, through a fixed window
//      of kWin bytes that starts at the (16-byte-aligned) start of the first entry still to parse: kWin holds any 256
//      consecutive short entries, so a group of short entries is one window; a long String entry in the group ends a
//      window early, and the entries the window's end cuts are parsed from the next window, which starts at the first
//      of them.  Each window parses at least its first entry, so the loop ends.
//   2. Parse.  One lane parses one entry from LDS with the parser the host decoder is checked against
//      (wire_plain_parse).  Single bytes are byte reads; the 8-byte and 4-byte fields, unaligned and big-endian, are
//      three (two) aligned dword reads joined by v_alignbyte_b32 and one byte swap, not eight byte reads.
//   3. Instance lookup.  inst = the slot of the instance id in the engine's device hash table (open addressing,
//      linear probing, at most half full); an unknown id gives max_instances.
//   4. Output.  The group's rows go to LDS and leave as 16-byte stores, lane j the j-th 16 bytes of a column: two u64
//      rows, four u32 rows or sixteen u8 rows per lane (narrow stores cost several times a 16-byte store per byte:
//      unpack.hip).  The last partial 16 bytes of a column's tail are stored row by row.
//   5. Escapes.  A row that is not plain gets the host decoder's defaults (inst = max_instances, everything else 0)
//      and one bit in the escape bitmap: each wave stores the ballot of its 64 rows as one word, so the rows come out
//      in row order by construction; the count is one atomic add per wave that has any.
// The host (wire_to_device) decodes the escaped rows with wire.cpp's decode_one, in ascending row order, and
// k_wire_patch writes them over the columns.
// The kernel moves (entry bytes + 8 B offset + 38 B columns) per row once; its bar is the H2D of its own input.
// Measured (scripts/wire_rate.py, profiles/wire_gpu/rate.json: 16 Mi CompareAndSet entries of 34 bytes, MI355X): the
// kernel takes 0.77 ms (1.7 TB/s over those bytes), the H2D of the same input 12.5 ms.
//
// The String dictionary (cc_wire_dict_attach; layout, hash and probe: wire_plain.h).  k_wire_decode is a template:
// <false> is the kernel above, unchanged, and the only one an engine without a dictionary (or a call with another
// interner) launches; <true> runs the same parser over a DictView, so a String of at most CC_WIRE_STR_MAX bytes that
// the attached interner holds becomes a HANDLE in the lane that parses the entry: the lane hashes the bytes from its
// LDS window 8 at a time (LdsBytes::le64, the tail masked), reads the cell (32 bytes, one cache line) and compares the
// pool's words with the window's; two dependent global reads per String, hidden by the other waves of the SIMD.  The
// threshold of step 1 becomes kWireStrEntryMax (836 bytes: MAP_REPLACEIFPRESENT with three Strings), which fits a
// window twenty times over, so a window still holds any 256 consecutive plain entries and still parses its first
// entry.  An unknown or longer String, and a String key whose hash is not registered, escape as in step 5.  The host
// keeps the exact image (wire.cpp WireDict); wire_dict_update sends what changed before the decode: the pool's new
// words, and the changed cells as a list that k_dict_scatter writes, or the whole table after a doubling.
// Measured (scripts/wire_rate.py --strings, profiles/wire_gpu/rate_strings.json: 16 Mi Put entries of 53 bytes with a
// 16-byte String key, MI355X): with 1,024 keys (table and pool in L2) the
// kernel takes 1.67 ms, with 1 Mi keys (64 MiB table + 16 MiB pool: the Infinity Cache) 2.21 ms, the H2D of the
// same input 18.5 ms; the call takes 195 / 206 ms where the same engine unattached (every row escapes) takes
// 2298 / 14034 ms.  On an all-plain stream <true> is 7.1 % slower than <false> (rate_plain_ab.json: its occupancy).
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): k_wire_decode<false> 95 VGPRs, 106 SGPRs (174 SGPR
// spills, to VGPR lanes), no scratch, 29,504 B LDS, occupancy 5 waves / SIMD; k_wire_decode<true> 100 VGPRs, 106 SGPRs
// (197 SGPR spills, to VGPR lanes), no scratch, 29,504 B LDS, occupancy 4 waves / SIMD; k_wire_patch 30 VGPRs,
// k_dict_scatter 10 VGPRs, both no scratch, no LDS.
//
// The pipeline's chunk (cc_apply_wire_host_packed; host_path.hip WireSource, wire_chunk_decode below).  A chunk's
// offsets are not scanned by the host: k_wire_offsets_check finds the first row whose end offset falls below its start
// or lies past the chunk's staged span, k_wire_offsets_clamp rewrites the offsets after it, and only then k_wire_decode
// runs, unchanged.  Resources (as above): k_wire_offsets_check 20 VGPRs, 30 SGPRs, k_wire_offsets_clamp 6 VGPRs,
// 20 SGPRs; both no spills, no scratch, no LDS, occupancy 8 waves / SIMD.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "engine_state.h"
#include "wire_plain.h"

namespace cc {

namespace {

constexpr uint32_t kWireLanes = 256;
constexpr uint32_t kWaves = kWireLanes / 64;
constexpr uint32_t kWireTile = CC_WIRE_TILE_ROWS;
static_assert(kWireTile % kWireLanes == 0, "a tile is whole groups of 256 entries");
// the window: 256 short entries behind a start up to 15 bytes past a 16-byte boundary, in whole 16-byte loads; the
// LDS array has 16 bytes more, for the aligned dwords an 8-byte field's read may touch past the window
constexpr uint32_t kWin = (15 + kWireLanes * kWirePlainMax + 15) / 16 * 16;

// an entry in the LDS window, starting at byte `base` of it
struct LdsBytes {
  const uint8_t* win;
  uint32_t base;
  __device__ uint32_t u8(uint32_t i) const { return win[base + i]; }
  __device__ uint32_t le32(uint32_t i) const {
    const uint32_t at = base + i;
    const uint32_t* w = (const uint32_t*)(win + (at & ~3u));
    return __builtin_amdgcn_alignbyte(w[1], w[0], at & 3u);
  }
  __device__ uint64_t le64(uint32_t i) const {
    const uint32_t at = base + i;
    const uint32_t* w = (const uint32_t*)(win + (at & ~3u));
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
    return (uint64_t)__builtin_amdgcn_alignbyte(w1, w0, at & 3u) |
           ((uint64_t)__builtin_amdgcn_alignbyte(w2, w1, at & 3u) << 32);
  }
  // bytes [i, i + n), n in 1..7: the same three dwords (they lie inside the LDS array wherever the entry ends),
  // the bytes past n masked off
  __device__ uint64_t lepart(uint32_t i, uint32_t n) const { return le64(i) & (~0ull >> (64 - 8 * n)); }
};

__device__ inline uint32_t slot_of(const WireArgs& a, uint64_t id) {
  uint32_t h = (uint32_t)((id * 0x9E3779B97F4A7C15ull) >> 32) & a.tbl_mask;
  for (uint32_t probe = 0; probe <= a.tbl_mask; ++probe) {  // (the table is at most half full: an empty cell ends it)
    const uint32_t s = a.tbl_slot[h];
    if (s == ~0u) break;
    if (a.tbl_id[h] == id) return s;
    h = (h + 1) & a.tbl_mask;
  }
  return a.max_inst;
}

// rows [0, rows) of one column of the group: LDS -> global, 16 bytes per lane
template <class T>
__device__ inline void store_col(T* out, const T* lds, uint32_t rows) {
  constexpr uint32_t per = 16 / sizeof(T);
  for (uint32_t c = threadIdx.x; c * per < rows; c += kWireLanes) {
    if ((c + 1) * per <= rows) {
      *(uint4*)(out + c * per) = *(const uint4*)(lds + c * per);
    } else {
      for (uint32_t j = c * per; j < rows; ++j) out[j] = lds[j];
    }
  }
}

// the longest entry the parser with a dictionary yields fits a window by itself, so every window parses its first entry
static_assert(15 + kWireStrEntryMax <= kWin, "the longest device-parsable entry fits one window");

template <bool kDict>
__global__ __launch_bounds__(256) void k_wire_decode(WireArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t win[kWin + 16];
  __shared__ __attribute__((aligned(16))) uint64_t o64[5][kWireLanes];  // key, a, b, aux, iid
  __shared__ __attribute__((aligned(16))) uint32_t o32[kWireLanes];     // inst
  __shared__ __attribute__((aligned(16))) uint8_t o8[2][kWireLanes];    // op, flags
  __shared__ uint32_t s_sch[kSchemaIds];
  __shared__ uint64_t s_first[kWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  s_sch[tid] = a.schema[tid];
  static_assert(kSchemaIds == kWireLanes, "one schema word per lane");
  const uint64_t t0 = (uint64_t)blockIdx.x * kWireTile;
  const uint64_t base0 = a.off[0];
  uint32_t str_rows = 0;  // (kDict) this wave's decoded rows with a resolved String, over the tile
  for (uint32_t g = 0; g < kWireTile / kWireLanes; ++g) {
    const uint64_t g0 = t0 + (uint64_t)g * kWireLanes;
    if (g0 >= a.n) break;  // (the same in every lane)
    const uint32_t rows = (uint32_t)min((uint64_t)kWireLanes, a.n - g0);
    const bool valid = tid < rows;
    const uint64_t beg = valid ? a.off[g0 + tid] - base0 : 0, end = valid ? a.off[g0 + tid + 1] - base0 : 0;
    const uint64_t gend = a.off[g0 + rows] - base0;
    // still to parse; the longer ones escape unread
    bool pend = valid && end - beg <= (kDict ? kWireStrEntryMax : kWirePlainMax);
    bool plain = false;
    PlainRow r{};
    for (;;) {
      const uint64_t bal = __ballot(pend);
      const uint64_t first = __shfl((unsigned long long)beg, bal ? __ffsll((unsigned long long)bal) - 1 : 0);
      if (lane == 0) s_first[wave] = bal ? first : ~0ull;
      __syncthreads();  // (every lane is also done with the previous window)
      const uint64_t wb = min(min(s_first[0], s_first[1]), min(s_first[2], s_first[3]));
      if (wb == ~0ull) break;  // nothing left to parse in the group (the same in every lane)
      const uint64_t wbase = wb & ~15ull;
      const uint32_t lim = (uint32_t)min((uint64_t)kWin, ((gend + 15) & ~15ull) - wbase);
      for (uint32_t i = tid * 16; i < lim; i += kWireLanes * 16) *(uint4*)(win + i) = *(const uint4*)(a.bytes + wbase + i);
      __syncthreads();
      if (pend && end <= wbase + kWin) {
        pend = false;
        const LdsBytes ent{win, (uint32_t)(beg - wbase)};
        if constexpr (kDict) plain = wire_parse(ent, (uint32_t)(end - beg), a.codec, s_sch, a.dict, r);
        else plain = wire_plain_parse(ent, (uint32_t)(end - beg), a.codec, s_sch, r);
      }
    }
    o64[0][tid] = plain ? r.key : 0;
    o64[1][tid] = plain ? r.a : 0;
    o64[2][tid] = plain ? r.b : 0;
    o64[3][tid] = plain ? r.aux : 0;
    o64[4][tid] = plain ? r.iid : 0;
    o32[tid] = plain ? slot_of(a, r.iid) : a.max_inst;
    o8[0][tid] = plain ? r.op : 0;
    o8[1][tid] = plain ? r.flags : 0;
    const uint64_t esc = __ballot(valid && !plain);
    if (lane == 0 && g0 + wave * 64 < a.n) {
      a.esc[(g0 >> 6) + wave] = esc;
      if (esc) atomicAdd(a.esc_n, (unsigned long long)__popcll(esc));
    }
    if constexpr (kDict) str_rows += (uint32_t)__popcll(__ballot(plain && r.strs != 0));
    __syncthreads();
    store_col(a.key + g0, o64[0], rows);
    store_col(a.a + g0, o64[1], rows);
    store_col(a.b + g0, o64[2], rows);
    store_col(a.aux + g0, o64[3], rows);
    if (a.iid) store_col(a.iid + g0, o64[4], rows);
    store_col(a.inst + g0, o32, rows);
    store_col(a.op + g0, o8[0], rows);
    store_col(a.flags + g0, o8[1], rows);
    __syncthreads();  // (the next group writes the LDS columns again)
  }
  if constexpr (kDict) {  // one atomic per tile: every wave adding to the one counter serialises in L2
    if (lane == 0) s_first[wave] = str_rows;
    __syncthreads();
    const uint64_t sum = s_first[0] + s_first[1] + s_first[2] + s_first[3];
    if (tid == 0 && sum) atomicAdd(a.esc_n + 1, (unsigned long long)sum);
  }
}

// host-decoded rows over the columns: one lane per row (sparse rows: narrow stores)
__global__ __launch_bounds__(256) void k_wire_patch(WireArgs a, const WirePatch* rows, uint64_t m) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const WirePatch p = rows[i];
  if (p.row >= a.n) return;
  a.inst[p.row] = p.inst;
  a.op[p.row] = p.op;
  a.flags[p.row] = p.flags;
  a.key[p.row] = p.key;
  a.a[p.row] = p.a;
  a.b[p.row] = p.b;
  a.aux[p.row] = p.aux;
  if (a.iid) a.iid[p.row] = p.iid;
}

// changed dictionary cells over the device table: one lane per (cell index, cell) pair
struct DictPatch {
  uint32_t at, pad[7];
  DictCell cell;
};
static_assert(sizeof(DictPatch) == 64, "DictPatch");
__global__ __launch_bounds__(256) void k_dict_scatter(DictCell* cells, uint32_t mask, const DictPatch* list, uint64_t m) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const uint32_t at = list[i].at;
  if (at > mask) return;
  cells[at] = list[i].cell;
}

// The offsets of one pipeline chunk checked on the device (cc_apply_wire_host_packed): off[0 .. n] are the chunk's
// staged offsets, whose two ends the host checked (off[0] <= off[n] = span_end <= the buffer's length).  Lane t of a
// block takes offsets 2t and 2t + 1 in one 16-byte load and its right neighbour's first offset by a shuffle (the last
// lane of a wave reads it), so it judges rows 2t and 2t + 1; the first row i with off[i + 1] < off[i] or
// off[i + 1] > span_end is kept per lane (rows ascend with the grid stride), reduced over the wave, and one atomicMin
// per wave that found any goes to *bad (~0 before: no such row).
__global__ __launch_bounds__(256) void k_wire_offsets_check(const uint64_t* off, uint64_t n, uint64_t span_end,
                                                            unsigned long long* bad) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t stride = (uint64_t)gridDim.x * 256;
  unsigned long long first = ~0ull;
  for (uint64_t base = (uint64_t)blockIdx.x * 256; 2 * base < n; base += stride) {  // (the same in every lane of a block)
    const uint64_t p = base + threadIdx.x;
    uint64_t x = 0, y = 0;
    if (2 * p + 1 <= n) {
      const ulonglong2 v = *(const ulonglong2*)(off + 2 * p);
      x = v.x, y = v.y;
    } else if (2 * p <= n) {
      x = off[2 * p];
    }
    uint64_t z = __shfl_down((unsigned long long)x, 1);
    if (lane == 63 && 2 * p + 2 <= n) z = off[2 * p + 2];
    if (first != ~0ull) continue;
    if (2 * p < n && (y < x || y > span_end)) first = 2 * p;
    else if (2 * p + 1 < n && (z < y || z > span_end)) first = 2 * p + 1;
  }
  for (int d = 32; d; d >>= 1) {
    const unsigned long long o = __shfl_xor(first, d);
    first = o < first ? o : first;
  }
  if (lane == 0 && first != ~0ull) atomicMin(bad, first);
}

// Every offset after the row *bad rewritten to that row's start (*bad >= n: nothing to do).  The rows before it ascend
// inside [off[0], span_end], so afterwards off[0 .. n] is non-decreasing and ends inside the staged span, whatever the
// host passed.  k_wire_decode needs this: it forms its window addresses from the offsets alone (wbase from an entry's
// start, the window's length from the group's last offset) and does not bound them by the staged span itself.  The
// clamped entries are zero-length, escape, and the host discards their rows.
__global__ __launch_bounds__(256) void k_wire_offsets_clamp(uint64_t* off, uint64_t n, const unsigned long long* bad) {
  const uint64_t b = *bad;
  if (b >= n) return;
  const uint64_t v = off[b];  // (never written: only offsets after b are)
  for (uint64_t j = b + 1 + (uint64_t)blockIdx.x * 256 + threadIdx.x; j <= n; j += (uint64_t)gridDim.x * 256) off[j] = v;
}

enum WrSlot : int { kWrBytes = 0, kWrOff, kWrEsc, kWrTable, kWrSchema, kWrPatch };

// device buffer `slot` of the decoder with room for `bytes` (contents not kept; the calls are synchronous)
int wr(cc_engine* e, int slot, size_t bytes, void** out) {
  bytes = std::max<size_t>(bytes, 256);
  if (e->wr_cap[slot] < bytes) {
    const size_t cap = std::max(bytes, e->wr_cap[slot] * 3 / 2);
    if (e->wr_buf[slot]) (void)hipFree(e->wr_buf[slot]);
    e->wr_buf[slot] = nullptr;
    e->wr_cap[slot] = 0;
    const hipError_t x = hipMalloc(&e->wr_buf[slot], cap);
    if (x != hipSuccess) return set_err(CC_ERR_HIP, "hipMalloc (wire decoder staging)", x);
    e->wr_cap[slot] = cap;
  }
  *out = e->wr_buf[slot];
  return CC_OK;
}

// The device table instance id -> slot, rebuilt from the session registry when it has changed: the host builds the
// image (ids, then slots) and one H2D sends it.
int wire_table(cc_engine* e, hipStream_t st) {
  if (e->wr_gen == e->inst_gen && e->wr_buf[kWrTable]) return CC_OK;
  uint64_t cells = 64;
  while (cells < 2ull * e->cfg.max_instances) cells <<= 1;
  if (cells > (1ull << 31)) return set_err(CC_ERR_CAPACITY, "wire decode: instance table");
  const uint32_t mask = (uint32_t)(cells - 1);
  std::vector<uint64_t> img(cells + (cells + 1) / 2, 0);
  uint32_t* slots = (uint32_t*)(img.data() + cells);
  for (uint64_t i = 0; i < cells; ++i) slots[i] = ~0u;
  for (const auto& kv : e->inst_by_id) {
    uint32_t h = wire_tbl_hash(kv.first, mask);
    while (slots[h] != ~0u) h = (h + 1) & mask;
    img[h] = kv.first;
    slots[h] = kv.second;
  }
  void* d = nullptr;
  TRY(wr(e, kWrTable, img.size() * 8, &d));
  HIPCHECK(hipMemcpyAsync(d, img.data(), img.size() * 8, hipMemcpyHostToDevice, st));
  HIPCHECK(hipStreamSynchronize(st));  // (img leaves scope)
  e->wr_mask = mask;
  e->wr_gen = e->inst_gen;
  return CC_OK;
}

// a device buffer of the dictionary with room for `bytes`; keep: the first `keep` bytes survive a reallocation
int dict_buf(void** buf, size_t* cap_bytes, size_t bytes, size_t keep, hipStream_t st) {
  if (*cap_bytes >= bytes) return CC_OK;
  const size_t cap = std::max<size_t>(std::max<size_t>(bytes, *cap_bytes * 2), 4096);
  void* p = nullptr;
  const hipError_t x = hipMalloc(&p, cap);
  if (x != hipSuccess) return set_err(CC_ERR_HIP, "hipMalloc (wire dictionary)", x);
  if (*buf && keep) {
    if (hipMemcpyAsync(p, *buf, keep, hipMemcpyDeviceToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
      (void)hipFree(p);
      return set_err(CC_ERR_HIP, "wire dictionary: pool copy");
    }
  }
  if (*buf) (void)hipFree(*buf);
  *buf = p;
  *cap_bytes = cap;
  return CC_OK;
}

// Bring the attached dictionary up to date with its interner and the engine's registered hashes, the host mirror
// first, then the device copy: the new pool words, and either the changed cells (a list and k_dict_scatter) or,
// after a doubling, the whole table.  Synchronous on `st` when anything moved.
int wire_dict_update(cc_engine* e, const cc_wire_interner* in, hipStream_t st) {
  WireDictDev& w = *e->wdict;
  WireDict& d = w.host;
  const bool grown = wire_interner_info(in).count != d.cell_of.size(), remark = w.hh_gen != e->hh_gen;
  if (grown || remark) {
    w.last_sync_strings = wire_dict_sync(d, in, e->hh, remark);
    w.hh_gen = e->hh_gen;
  }
  if (!d.rebuilt && d.dirty.empty() && d.pool_sent == d.pool.size()) return CC_OK;
  size_t cap = w.pool_cap * 8;
  TRY(dict_buf(&w.d_pool, &cap, (d.pool.size() + 1) * 8, d.pool_sent * 8, st));
  w.pool_cap = cap / 8;
  if (d.pool.size() > d.pool_sent)
    HIPCHECK(hipMemcpyAsync((uint64_t*)w.d_pool + d.pool_sent, d.pool.data() + d.pool_sent, (d.pool.size() - d.pool_sent) * 8,
                            hipMemcpyHostToDevice, st));
  std::vector<DictPatch> list;
  if (d.rebuilt) {
    cap = w.cells_cap * sizeof(DictCell);
    TRY(dict_buf(&w.d_cells, &cap, d.cells.size() * sizeof(DictCell), 0, st));
    w.cells_cap = cap / sizeof(DictCell);
    HIPCHECK(hipMemcpyAsync(w.d_cells, d.cells.data(), d.cells.size() * sizeof(DictCell), hipMemcpyHostToDevice, st));
    ++w.full_uploads;
  } else if (!d.dirty.empty()) {
    list.resize(d.dirty.size());
    for (size_t i = 0; i < list.size(); ++i) list[i] = DictPatch{d.dirty[i], {}, d.cells[d.dirty[i]]};  // (a cell listed twice carries the same image twice)
    cap = w.list_cap * sizeof(DictPatch);
    TRY(dict_buf(&w.d_list, &cap, list.size() * sizeof(DictPatch), 0, st));
    w.list_cap = cap / sizeof(DictPatch);
    HIPCHECK(hipMemcpyAsync(w.d_list, list.data(), list.size() * sizeof(DictPatch), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_dict_scatter, dim3((uint32_t)((list.size() + 255) / 256)), dim3(256), 0, st, (DictCell*)w.d_cells,
                       (uint32_t)(d.cells.size() - 1), (const DictPatch*)w.d_list, (uint64_t)list.size());
    if (hipGetLastError() != hipSuccess) return set_err(CC_ERR_HIP, "wire dictionary scatter launch");
  }
  HIPCHECK(hipStreamSynchronize(st));  // (the staged list leaves scope; the mirror may change after the call)
  d.rebuilt = false;
  d.dirty.clear();
  d.pool_sent = d.pool.size();
  return CC_OK;
}

// the attached dictionary serves this call: the same interner object the attach saw
bool dict_serves(const cc_engine* e, const cc_wire_interner* in) {
  return e->wdict && e->wdict->in == in && e->wdict->serial == wire_interner_info(in).serial;
}

}  // namespace

int launch_wire_decode(const WireArgs& a, hipStream_t st) {
  if (a.n == 0) return 0;
  const uint64_t tiles = (a.n + kWireTile - 1) / kWireTile;
  if (tiles > 0x7FFFFFFFull) return -1;
  if (a.dict.cells) hipLaunchKernelGGL(k_wire_decode<true>, dim3((uint32_t)tiles), dim3(kWireLanes), 0, st, a);
  else hipLaunchKernelGGL(k_wire_decode<false>, dim3((uint32_t)tiles), dim3(kWireLanes), 0, st, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_wire_patch(const WireArgs& a, const WirePatch* rows, uint64_t m, hipStream_t st) {
  if (m == 0) return 0;
  hipLaunchKernelGGL(k_wire_patch, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, st, a, rows, m);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int wire_args(cc_engine* e, const cc_wire_codec* codec, const cc_batch_out* d_cols, uint64_t* d_iid, WireArgs* a) {
  void* const col[7] = {d_cols->inst, d_cols->op, d_cols->flags, d_cols->key, d_cols->a, d_cols->b, d_cols->aux};
  for (void* p : col)
    if (!p || ((uintptr_t)p & 15))
      return set_err(CC_ERR_INVALID, "wire decode: a device column is null or not 16-byte aligned");
  if ((uintptr_t)d_iid & 15) return set_err(CC_ERR_INVALID, "wire decode: d_iid is not 16-byte aligned");
  cc_wire_codec c;
  if (codec) c = *codec;
  else cc_wire_codec_default(&c);
  if (c.utf8_len_bytes < 1 || c.utf8_len_bytes > 8) return set_err(CC_ERR_INVALID, "wire codec: utf8_len_bytes");
  *a = WireArgs{};
  a->codec = c;
  a->max_inst = e->cfg.max_instances;
  a->inst = (uint32_t*)col[0], a->op = (uint8_t*)col[1], a->flags = (uint8_t*)col[2];
  a->key = (uint64_t*)col[3], a->a = (uint64_t*)col[4], a->b = (uint64_t*)col[5], a->aux = (uint64_t*)col[6];
  a->iid = d_iid;
  return CC_OK;
}

namespace {

// what a decode needs on the device besides its input: the schema words, the pinned words and the instance table
// (first use / when stale) -> a->schema and a->tbl_*
int wire_args_device(cc_engine* e, hipStream_t st, WireArgs* a) {
  void* d_sch;
  if (!e->wr_buf[kWrSchema]) {
    uint32_t sch[kSchemaIds];
    schema_words(sch);
    TRY(wr(e, kWrSchema, sizeof sch, &d_sch));
    HIPCHECK(hipMemcpy(d_sch, sch, sizeof sch, hipMemcpyHostToDevice));
  }
  d_sch = e->wr_buf[kWrSchema];
  if (!e->wr_pin) HIPCHECK(hipHostMalloc((void**)&e->wr_pin, 64, hipHostMallocDefault));
  TRY(wire_table(e, st));
  a->schema = (const uint32_t*)d_sch;
  a->tbl_id = (const uint64_t*)e->wr_buf[kWrTable];
  a->tbl_slot = (const uint32_t*)(a->tbl_id + (e->wr_mask + 1ull));
  a->tbl_mask = e->wr_mask;
  return CC_OK;
}

}  // namespace

int wire_args_dict(cc_engine* e, const cc_wire_interner* in, hipStream_t st, WireArgs* a) {
  a->dict = DictView{};
  if (!dict_serves(e, in)) return CC_OK;
  TRY(wire_dict_update(e, in, st));
  a->dict = DictView{(const DictCell*)e->wdict->d_cells, (const uint64_t*)e->wdict->d_pool,
                     (uint32_t)(e->wdict->host.cells.size() - 1), e->wdict->first};
  return CC_OK;
}

int wire_patch_rows(cc_engine* e, const WireArgs& a, const std::vector<WirePatch>& patch, hipStream_t st) {
  if (patch.empty()) return CC_OK;
  void* d_patch;
  TRY(wr(e, kWrPatch, patch.size() * sizeof(WirePatch), &d_patch));
  HIPCHECK(hipMemcpyAsync(d_patch, patch.data(), patch.size() * sizeof(WirePatch), hipMemcpyHostToDevice, st));
  if (launch_wire_patch(a, (const WirePatch*)d_patch, patch.size(), st))
    return set_err(CC_ERR_HIP, "wire patch launch", hipGetLastError());
  HIPCHECK(hipStreamSynchronize(st));
  return CC_OK;
}

int wire_keys_done(cc_engine* e, cc_wire_interner* in, const std::vector<uint64_t>& skeys) {
  const uint64_t hh_gen = e->hh_gen;
  TRY(wire_register_keys(e, in, skeys.data(), skeys.size()));
  if (dict_serves(e, in) && e->wdict->hh_gen == hh_gen) {  // the only change of hh since the sync: set those key bits
    wire_dict_mark_keys(e->wdict->host, e->wdict->first, skeys.data(), skeys.size());
    e->wdict->hh_gen = e->hh_gen;
  }
  return CC_OK;
}

int wire_to_device(cc_engine* e, const cc_wire_codec* codec, cc_wire_interner* in, const uint8_t* h_buf, uint64_t buf_len,
                   const uint64_t* h_offsets, uint64_t n, const cc_batch_out* d_cols, uint64_t* d_iid,
                   cc_wire_control* h_ctl, uint64_t ctl_cap, uint64_t* ctl_count, cc_wire_stats* stats, hipStream_t st,
                   uint64_t* bad_row, bool stop_at_ctl, uint64_t* stop_row) {
  if (!e || !in || !h_buf || !h_offsets || !d_cols || !ctl_count || (ctl_cap && !h_ctl))
    return set_err(CC_ERR_INVALID, "wire decode: null argument");
  WireArgs a{};
  TRY(wire_args(e, codec, d_cols, d_iid, &a));
  *ctl_count = 0;
  if (stop_row) *stop_row = n;
  if (stats) *stats = cc_wire_stats{n, 0, 0};
  if (n == 0) return CC_OK;
  HIPCHECK(hipSetDevice(e->device));
  // the rows before the first offsets violation go to the device (its row fails the call, unless a row before it does)
  const uint64_t m = wire_first_bad_offset(h_offsets, n, buf_len);
  a.n = m;
  std::vector<uint64_t> esc;  // the escape bitmap
  uint64_t esc_n = 0;
  if (m) {
    // staging: bytes [offsets[0], offsets[m]) at the start of a buffer padded to whole 16-byte loads, the offsets as
    // they are (the kernel subtracts offsets[0])
    const uint64_t span = h_offsets[m] - h_offsets[0];
    void *d_bytes, *d_off, *d_esc;
    TRY(wr(e, kWrBytes, ((span + 15) & ~15ull) + 16, &d_bytes));
    TRY(wr(e, kWrOff, 8 * (m + 1), &d_off));
    const uint64_t words = (m + 63) / 64;
    TRY(wr(e, kWrEsc, 16 + 8 * words, &d_esc));  // the count, then (16-byte aligned) the bitmap
    TRY(wire_args_device(e, st, &a));
    TRY(wire_args_dict(e, in, st, &a));
    for (hipEvent_t& ev : e->wr_ev)
      if (!ev) HIPCHECK(hipEventCreate(&ev));
    HIPCHECK(hipEventRecord(e->wr_ev[0], st));
    if (span) HIPCHECK(hipMemcpyAsync(d_bytes, h_buf + h_offsets[0], span, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(d_off, h_offsets, 8 * (m + 1), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemsetAsync(d_esc, 0, 16, st));
    a.bytes = (const uint8_t*)d_bytes;
    a.off = (const uint64_t*)d_off;
    a.esc_n = (unsigned long long*)d_esc;
    a.esc = (uint64_t*)d_esc + 2;
    HIPCHECK(hipEventRecord(e->wr_ev[1], st));
    if (launch_wire_decode(a, st)) return set_err(CC_ERR_HIP, "wire decode launch", hipGetLastError());
    HIPCHECK(hipEventRecord(e->wr_ev[2], st));
    HIPCHECK(hipMemcpyAsync(e->wr_pin, d_esc, 16, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    esc_n = e->wr_pin[0];
    if (a.dict.cells) e->wdict->last_str_rows = e->wr_pin[1];
    if (esc_n) {
      esc.resize(words);
      HIPCHECK(hipMemcpyAsync(esc.data(), a.esc, 8 * words, hipMemcpyDeviceToHost, st));
    }
    HIPCHECK(hipEventRecord(e->wr_ev[3], st));
    HIPCHECK(hipStreamSynchronize(st));
    e->wr_timed = true;
  }
  // the fallback: every escaped row through the host decoder, in ascending row order
  WireFallback f;
  f.patch.reserve(esc_n);
  wire_fallback(e, a.codec, in, h_buf, h_offsets, 0, stop_at_ctl, EscRows{esc.data(), esc.size()}, &f);
  TRY(wire_patch_rows(e, a, f.patch, st));
  if (stats) stats->host_rows = f.patch.size(), stats->device_rows = m - std::min<uint64_t>(m, esc_n);
  if (f.fail_rc) {  // (cc_last_error holds decode_one's "wire row N: ...")
    if (bad_row) *bad_row = f.fail_row;
    return f.fail_rc;
  }
  if (!f.stopped && m < n) {
    if (bad_row) *bad_row = m;
    return set_err(CC_ERR_INVALID, h_offsets[m + 1] < h_offsets[m] ? "wire decode: offsets decrease"
                                                                   : "wire decode: entry ends past the buffer");
  }
  if (stop_row) *stop_row = f.stopped ? f.stop : n;
  TRY(wire_keys_done(e, in, f.skeys));
  *ctl_count = f.ctl.size();
  if (f.ctl.size() > ctl_cap) return set_err(CC_ERR_CAPACITY, "wire decode: more manager entries than h_ctl holds");
  if (!f.ctl.empty()) memcpy(h_ctl, f.ctl.data(), f.ctl.size() * sizeof(cc_wire_control));
  return CC_OK;
}

// One chunk of cc_apply_wire_host_packed, as wire_to_device decodes a segment, with the offsets scan on the device:
// the dictionary sync, the offsets check and clamp, k_wire_decode, ONE read-back (escape count, dictionary counter and
// the first bad offset row together in the pinned words), then the host fallback in row order and the patch.  The
// dictionary sync before each chunk lets a String first seen in chunk k resolve on the device in chunk k + 1;
// exactness does not depend on it: an unresolved String escapes, and the host fallback gives it the same handle.
int wire_chunk_decode(cc_engine* e, const WireChunkIn& in, hipStream_t st, uint64_t* apply, bool* end, int* end_rc,
                      cc_wire_control* ctl, uint64_t* bad_row) {
  const WireChunk& c = in.c;
  const uint64_t rows = c.hi - c.lo, s = c.send;
  const uint64_t* off = in.h_offsets + c.lo;
  *apply = 0, *end = false, *end_rc = CC_OK;
  WireArgs a{};
  TRY(wire_args(e, in.codec, in.d_cols, nullptr, &a));
  a.n = s;
  std::vector<uint64_t> esc;
  uint64_t esc_n = 0, dev_bad = ~0ull;
  if (s) {
    void* d_esc;
    const uint64_t words = (s + 63) / 64;
    TRY(wr(e, kWrEsc, 32 + 8 * words, &d_esc));  // escape count, dictionary counter, first bad offset row; the bitmap
    TRY(wire_args_device(e, st, &a));
    TRY(wire_args_dict(e, in.in, st, &a));
    HIPCHECK(hipMemsetAsync(d_esc, 0, 16, st));
    HIPCHECK(hipMemsetAsync((uint8_t*)d_esc + 16, 0xFF, 16, st));
    a.bytes = (const uint8_t*)in.d_bytes;
    a.off = (const uint64_t*)in.d_off;
    a.esc_n = (unsigned long long*)d_esc;
    a.esc = (uint64_t*)d_esc + 4;
    unsigned long long* d_bad = (unsigned long long*)d_esc + 2;
    const uint32_t cb = (uint32_t)std::min<uint64_t>(1024, (s / 2 + 256) / 256);
    hipLaunchKernelGGL(k_wire_offsets_check, dim3(cb), dim3(256), 0, st, a.off, s, off[s], d_bad);
    hipLaunchKernelGGL(k_wire_offsets_clamp, dim3((uint32_t)std::min<uint64_t>(256, (s + 256) / 256)), dim3(256), 0, st,
                       (uint64_t*)in.d_off, s, (const unsigned long long*)d_bad);
    if (hipGetLastError() != hipSuccess) return set_err(CC_ERR_HIP, "wire offsets check launch");
    if (launch_wire_decode(a, st)) return set_err(CC_ERR_HIP, "wire decode launch", hipGetLastError());
    HIPCHECK(hipMemcpyAsync(e->wr_pin, d_esc, 32, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    esc_n = e->wr_pin[0];
    if (a.dict.cells) e->wdict->last_str_rows = e->wr_pin[1];
    dev_bad = e->wr_pin[2];
    if (esc_n) {
      esc.resize(words);
      HIPCHECK(hipMemcpyAsync(esc.data(), a.esc, 8 * words, hipMemcpyDeviceToHost, st));
      HIPCHECK(hipStreamSynchronize(st));
    }
  }
  // m: the first offsets violation of the chunk as wire_to_device finds it (rows: none).  The device's check is the
  // stricter one (an offset past the chunk's own end, though inside the buffer, is caught where it rises, the host's
  // where it falls again), so when it reports a row the host scans this one chunk itself, and the rows between the
  // two, which were not decoded on the device, go through the host decoder with the escaped ones.
  uint64_t m = c.ok ? rows : s, lim = s, extra = ~0ull;
  if (dev_bad < s) {
    m = wire_first_bad_offset(off, rows, in.buf_len);
    if (!c.ok || m < dev_bad || m >= rows)
      return set_err(CC_ERR_STATE, "internal check: the device offsets check disagrees with the host scan");
    lim = extra = dev_bad;
  }
  WireFallback f;
  EscRows er{esc.data(), esc.size()};
  bool esc_done = false;
  auto next = [&]() -> uint64_t {
    if (!esc_done) {
      const uint64_t r = er();
      if (r != ~0ull && r < lim) return r;
      esc_done = true;
    }
    return extra < m ? extra++ : ~0ull;
  };
  wire_fallback(e, a.codec, in.in, in.h_buf, off, c.lo, true, next, &f);
  TRY(wire_patch_rows(e, a, f.patch, st));
  if (f.fail_rc) {  // (cc_last_error holds decode_one's "wire row N: ...", N a segment row)
    *end = true, *end_rc = f.fail_rc, *bad_row = c.lo + f.fail_row;
    return CC_OK;
  }
  if (!f.stopped && m < rows) {
    *end = true, *bad_row = c.lo + m;
    *end_rc = set_err(CC_ERR_INVALID, off[m + 1] < off[m] ? "wire decode: offsets decrease"
                                                           : "wire decode: entry ends past the buffer");
    return CC_OK;
  }
  TRY(wire_keys_done(e, in.in, f.skeys));
  *apply = f.stopped ? f.stop : rows;
  if (f.stopped) *end = true, *ctl = f.ctl.back();
  return CC_OK;
}
}  // namespace cc

extern "C" int cc_wire_timeline(cc_engine* e, float* h_ms) {
  if (!e || !h_ms) return set_err(CC_ERR_INVALID, "null argument");
  if (!e->wr_timed) return set_err(CC_ERR_STATE, "wire timeline: no decode has run on this engine");
  for (int k = 0; k < 3; ++k) HIPCHECK(hipEventElapsedTime(&h_ms[k], e->wr_ev[k], e->wr_ev[k + 1]));
  return CC_OK;
}

extern "C" int cc_wire_dict_detach(cc_engine* e) {
  if (!e) return set_err(CC_ERR_INVALID, "null argument");
  if (!e->wdict) return CC_OK;
  (void)hipSetDevice(e->device);
  for (void* p : {e->wdict->d_cells, e->wdict->d_pool, e->wdict->d_list})
    if (p) (void)hipFree(p);
  delete e->wdict;
  e->wdict = nullptr;
  return CC_OK;
}

extern "C" int cc_wire_dict_attach(cc_engine* e, cc_wire_interner* in) {
  if (!e || !in) return set_err(CC_ERR_INVALID, "wire dictionary: null argument");
  HIPCHECK(hipSetDevice(e->device));
  (void)cc_wire_dict_detach(e);
  const WireInternerInfo info = wire_interner_info(in);
  e->wdict = new WireDictDev{};
  e->wdict->in = in, e->wdict->serial = info.serial, e->wdict->first = info.first;
  const int rc = wire_dict_update(e, in, nullptr);
  if (rc) (void)cc_wire_dict_detach(e);
  return rc;
}

extern "C" int cc_wire_dict_get_info(cc_engine* e, cc_wire_dict_info* out) {
  if (!e || !out) return set_err(CC_ERR_INVALID, "null argument");
  if (!e->wdict) return set_err(CC_ERR_STATE, "wire dictionary: none is attached to this engine");
  const WireDictDev& w = *e->wdict;
  *out = cc_wire_dict_info{w.host.strings,  w.host.long_strings, w.host.pool.size() * 8, w.host.cells.size(),
                           w.full_uploads, w.last_sync_strings,  w.last_str_rows};
  return CC_OK;
}

extern "C" int cc_wire_decode_to_device(cc_engine* e, const cc_wire_codec* codec, cc_wire_interner* in, const uint8_t* h_buf,
                                        uint64_t buf_len, const uint64_t* h_offsets, uint64_t n,
                                        const cc_batch_out* d_cols, uint64_t* d_iid, cc_wire_control* h_ctl,
                                        uint64_t ctl_cap, uint64_t* ctl_count, cc_wire_stats* stats, void* stream,
                                        uint64_t* bad_row) {
  return wire_to_device(e, codec, in, h_buf, buf_len, h_offsets, n, d_cols, d_iid, h_ctl, ctl_cap, ctl_count, stats,
                        (hipStream_t)stream, bad_row, false, nullptr);
}
