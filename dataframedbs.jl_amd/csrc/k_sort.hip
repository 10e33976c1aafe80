// k_sort.hip — K12: stable sortperm of the selected rows by one fixed-width column (by several: one key after another, k_sort_rekey below; by a String column:
// its 8-byte sub-keys one after another, k_sort_strkey below), and the gather that follows a row list (gfx950).
//
// Replaces sortperm(collect(col)) / partialsortperm / sort over Base.iterate(::DFColumn) (src/tables/column.jl:102-126): the reference collects the selected
// values one element at a time and sorts them on the host.
//
// Least-significant-digit radix sort of {key, row} pairs, 8 key bits per pass.  The key is the SELECT KEY of select_key.hpp (its unsigned order is isless),
// complemented within its bits for a descending sort; the row is the 0-based table row in 32 bits.  Pairs live as two arrays (keys: 8 bytes, rows: 4 bytes)
// in two halves that the passes ping-pong between.
//
// BUILD (k_sort_build): streams the column through the selection bitmap and the missing bitmap like k_select_hist — one wave per 1024-row tile, lane = row,
// 16 nontemporal loads in flight, tiles whose tile count is 0 skipped — and writes every KEPT row's pair at live_base[tile] + its rank among the tile's kept
// rows (popcounts of ballots), so the pairs start in table order.  Kept: selected, not missing, and (top-k cut) key <= cut.  Selected MISSING rows are not
// keyed at all — the bytes under a missing bit are never loaded —: their rows go, in table order, to a list of their own that the host lays behind (REV:
// before) the sorted rows.  The write phase also accumulates one 256-bin histogram per key byte in LDS (8 x 256 x 4 B = 8 KB for an 8-byte key), flushed
// with 64-bit integer atomicAdds of the non-zero bins; a wave whose kept lanes all hold one digit adds once with their popcount (an all-equal byte would
// otherwise serialise 64 adds on one LDS address).  The host skips the pass of every byte whose histogram has a single non-zero bin.  When the kept rows are
// not simply the selected ones (a nullable column, a cut) a count phase of the same kernel first leaves the kept and the missing rows per tile, which
// launch_scan_counts turns into live_base / miss_base.
//
// A PASS is three launches; no kernel ever waits on another workgroup (no look-back), so the result does not depend on scheduling:
//   k_sort_count    one workgroup per chunk of kSortChunk pairs: the chunk's 256-bin digit histogram in LDS -> counts[bin * nchunks + chunk]
//   (launch_scan_counts: one exclusive scan over the bin-major counts = where every (digit, chunk) run starts)
//   k_sort_scatter  re-reads the chunk; wave w owns pairs [w * 1024, (w + 1) * 1024) of it in 16 rounds of 64; a pair's rank inside the chunk is STABLE:
//                   the running count of its digit in its wave + the popcount of same-digit peers in lower lanes (a ballot match over the 8 digit bits),
//                   + the exclusive scan across the waves per digit, + the exclusive scan across the digits.  The chunk is staged in LDS at those ranks
//                   (digit order), then lane i stores staged pair i at scan[digit][chunk] + (i - the digit's start): consecutive lanes store consecutive
//                   addresses of one digit's run.
//   algorithmic bytes / pair / pass: 8 (count: keys) + 12 read + 12 written (scatter) [+ 12 / 4096 * 256 of counts and scan, ~0.75]
#include "device_utils.hpp"
#include "value_rules.hpp"
#include "select_key.hpp"
#include "str_tile.hpp"
#include "kernels.hpp"
#include "launch_dispatch.hpp"
#include "../../include/dfdb_ir.h"

namespace dfdb {

constexpr int kSortBlock = 256;                                   // threads per workgroup (every kernel of this file)
constexpr int kSortWaves = kSortBlock / 64;
constexpr int kSortChunk = 4096;                                  // pairs per chunk of a pass
constexpr int kSortRounds = kSortChunk / kSortBlock;              // pairs per thread
constexpr int kSortWaveSpan = kSortChunk / kSortWaves;            // contiguous pairs per wave
constexpr int kSortBuildBlocks = 2048;                            // build: 8 workgroups per CU (the 32-wave limit; 8 x 8 KB of LDS)
constexpr size_t kSortScatterLds = (size_t)kSortChunk * 12 + (size_t)kSortWaves * 256 * 4 + 16;   // staged keys + rows, per-wave digit counts, wave totals
static_assert(kSortChunk % kSortBlock == 0 && kSortWaveSpan == kSortRounds * 64, "a wave owns kSortRounds rounds of 64 contiguous pairs");
static_assert(kSortWaves * 256 * 4 >= 256 * 8, "the digit run bases (256 x 8 B) reuse the per-wave counts' LDS");
static_assert(3 * kSortScatterLds <= 160 * 1024, "three scatter workgroups (12 waves) per CU inside the 160 KB of LDS");
static_assert(kSortChunk <= 65536, "ranks inside a chunk fit 32 bits with room");

void sort_geometry(int64_t out[2]) { out[0] = kSortChunk; out[1] = kSortBlock; }
int64_t sort_chunks(int64_t npairs) { return (npairs + kSortChunk - 1) / kSortChunk; }

// the lanes (among `valid`) that hold the same 8-bit digit as this lane
__device__ __forceinline__ uint64_t match_digit(uint32_t d, bool valid) {
  uint64_t m = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; b++) {
    const bool bit = (d >> b) & 1u;
    const uint64_t bal = __ballot(bit);
    m &= bit ? bal : ~bal;
  }
  return m;
}

// the wave's kept keys (kmask: their lanes) into the per-byte digit histograms hist[byte * 256 + digit] in LDS
template <int NB>
__device__ __forceinline__ void hist_add_keys(uint32_t* hist, uint64_t key, bool kept, uint64_t kmask, int lane) {
  if (kmask == 0) return;
  const int src = __ffsll((unsigned long long)kmask) - 1;
#pragma unroll
  for (int b = 0; b < NB; b++) {
    const uint32_t d = (uint32_t)(key >> (8 * b)) & 255u;
    const uint32_t d0 = (uint32_t)__shfl((int)d, src, 64);
    if (__ballot(kept && d != d0) == 0) {                        // one digit in the whole wave: one add
      if (lane == src) atomicAdd(&hist[b * 256 + d0], (uint32_t)__popcll(kmask));
    } else if (kept) atomicAdd(&hist[b * 256 + d], 1u);
  }
}

// PHASE 0: the kept and the missing selected rows per tile -> B.live_cnt / B.miss_cnt (zeroed by the caller: dead tiles write nothing)
// PHASE 1: the pairs, the missing rows' list, the per-byte histograms
template <int DT, int PHASE>
__global__ __launch_bounds__(kSortBlock) void k_sort_build(const typename SelT<DT>::type* __restrict__ col, const uint64_t* __restrict__ missing, SortBuild B) {
  using T = typename SelT<DT>::type;
  constexpr int NB = select_key_bits(DT, false) / 8;
  __shared__ uint32_t hist[PHASE == 1 ? NB * 256 : 1];
  if (PHASE == 1) {
    for (int i = threadIdx.x; i < NB * 256; i += kSortBlock) hist[i] = 0;
    __syncthreads();
  }
  const int lane = lane_id();
  const uint64_t below = (1ull << lane) - 1ull;
  const int64_t wave = (int64_t)blockIdx.x * kSortWaves + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kSortWaves;
  const int64_t nwords = (B.nrows + 63) / 64, ntiles = (nwords + 15) / 16;
  for (int64_t tile = wave; tile < ntiles; tile += nwaves) {     // 1024 rows per wave step, 16 column loads in flight
    if (B.tile_counts[tile] == 0) continue;                      // wave-uniform: dead tiles touch neither the bitmaps nor the column
    const int64_t wi = tile * 16 + lane;
    const bool mine = lane < 16 && wi < nwords;
    const uint64_t myw = mine ? B.bitmap[wi] : 0ull;
    const uint64_t mym = (missing && mine) ? missing[wi] : 0ull;
    if (__ballot(myw != 0) == 0) continue;
    const T* p = col + tile * 1024 + lane;
    T v[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const uint64_t w = __shfl(myw, j, 64) & ~__shfl(mym, j, 64);           // word j, broadcast: selected and not missing
      v[j] = T(0);
      if ((w >> lane) & 1ull) v[j] = __builtin_nontemporal_load(p + j * 64);  // those rows only (never past nrows, never under a missing bit)
    }
    uint32_t lrun = 0, mrun = 0;                                 // wave-uniform: kept / missing rows of the tile so far
    uint64_t lbase = 0, mbase = 0;
    if (PHASE == 1) { lbase = B.live_base[tile]; mbase = B.miss_base ? B.miss_base[tile] : 0ull; }
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const uint64_t ws = __shfl(myw, j, 64), wm = __shfl(mym, j, 64);
      const bool live = ((ws & ~wm) >> lane) & 1ull;
      const uint64_t key = select_key<DT, false>(&v[j]) ^ B.flip;
      const bool kept = live && (B.keep == SORT_KEEP_ALL || (B.keep == SORT_KEEP_CUT && key <= B.cut));
      const uint64_t kmask = __ballot(kept), mmask = ws & wm;
      if (PHASE == 1) {
        const uint32_t row = (uint32_t)(tile * 1024 + j * 64 + lane);
        if (kept) {
          const uint64_t pos = lbase + lrun + (uint32_t)__popcll(kmask & below);
          if (pos < (uint64_t)B.cap) { B.keys[pos] = key; B.rows[pos] = row; }
        }
        if ((mmask >> lane) & 1ull) {
          const uint64_t pos = mbase + mrun + (uint32_t)__popcll(mmask & below);
          if (pos < (uint64_t)B.miss_cap) B.miss_rows[pos] = row;
        }
        hist_add_keys<NB>(hist, key, kept, kmask, lane);
      }
      lrun += (uint32_t)__popcll(kmask); mrun += (uint32_t)__popcll(mmask);
    }
    if (PHASE == 0 && lane == 0) { B.live_cnt[tile] = lrun; B.miss_cnt[tile] = mrun; }
  }
  if (PHASE == 1) {
    __syncthreads();
    for (int i = threadIdx.x; i < NB * 256; i += kSortBlock) { const uint32_t h = hist[i]; if (h) atomicAdd(&B.ghist[i], (unsigned long long)h); }
  }
}

void launch_sort_build(hipStream_t s, const ColRef& col, const SortBuild& B, bool count_phase) {
  const int64_t nwords = (B.nrows + 63) / 64, ntiles = (nwords + 15) / 16;
  int grid = (int)((ntiles + kSortWaves - 1) / kSortWaves);
  if (grid > kSortBuildBlocks) grid = kSortBuildBlocks;
  if (grid < 1) grid = 1;
  with_dtype<DtValues>(col.dtype, [&](auto c) {      // (Bool as DFDB_U8)
    constexpr int DT = decltype(c)::dtype;
    using T = typename SelT<DT>::type;
    if (count_phase) hipLaunchKernelGGL((k_sort_build<DT, 0>), dim3(grid), dim3(kSortBlock), 0, s, (const T*)col.data, col.missing, B);
    else hipLaunchKernelGGL((k_sort_build<DT, 1>), dim3(grid), dim3(kSortBlock), 0, s, (const T*)col.data, col.missing, B);
  });
}

// REKEY (k_sort_rekey): the build of the NEXT key of a sort by several columns — it starts from a row order instead of the selection.  One wave owns 1024
// consecutive entries of `order` in 16 rounds of 64, lane = entry: 16 coalesced loads of the entries, then the 16 loads of the rows' missing words (32-bit
// halves of the bitmap's words), then the 16 column loads of the live entries — two rounds of gathers, each 16 deep.  The positions are the build's
// arithmetic over the list: base of the tile + the running count in the wave + the popcount of the ballot below the lane, so pairs and missing rows keep
// the order they have in `order`.  An entry at or beyond n does nothing; a row that is not < nrows is treated as absent (a guard: no list made here has one).
// PHASE 0: the live and the missing entries per tile -> R.live_cnt / R.miss_cnt (every tile writes)
// PHASE 1: the pairs, the missing rows' list, the per-byte histograms
//   algorithmic bytes / entry: 4 (order) + 12 written; what it MOVES is a 128-byte line per gathered value (and per missing word) when the rows are scattered
template <int DT, int PHASE>
__global__ __launch_bounds__(kSortBlock) void k_sort_rekey(const typename SelT<DT>::type* __restrict__ col, const uint64_t* __restrict__ missing, SortRekey R) {
  using T = typename SelT<DT>::type;
  constexpr int NB = select_key_bits(DT, false) / 8;
  __shared__ uint32_t hist[PHASE == 1 ? NB * 256 : 1];
  if (PHASE == 1) {
    for (int i = threadIdx.x; i < NB * 256; i += kSortBlock) hist[i] = 0;
    __syncthreads();
  }
  const int lane = lane_id();
  const uint64_t below = (1ull << lane) - 1ull;
  const int64_t wave = (int64_t)blockIdx.x * kSortWaves + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kSortWaves;
  const int64_t ntiles = (R.n + 1023) / 1024;
  const uint32_t* mhalf = (const uint32_t*)missing;              // little-endian: bit (r & 31) of half (r >> 5) is bit (r & 63) of word (r >> 6)
  for (int64_t tile = wave; tile < ntiles; tile += nwaves) {
    const int64_t e0 = tile * 1024 + lane;
    uint32_t r[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const int64_t i = e0 + j * 64;
      r[j] = i < R.n ? __builtin_nontemporal_load(R.order + i) : 0xffffffffu;
    }
    uint32_t mh[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
      mh[j] = 0;
      if (missing && (int64_t)r[j] < R.nrows) mh[j] = mhalf[r[j] >> 5];
    }
    uint32_t pres = 0, miss = 0;                                 // bit j: entry j of this lane is there / is missing in this column
#pragma unroll
    for (int j = 0; j < 16; j++) {
      if ((int64_t)r[j] < R.nrows) pres |= 1u << j;
      if ((mh[j] >> (r[j] & 31u)) & 1u) miss |= 1u << j;
    }
    const uint32_t livem = pres & ~miss;
    T v[PHASE == 1 ? 16 : 1];
    if (PHASE == 1) {
#pragma unroll
      for (int j = 0; j < 16; j++) {
        v[j] = T(0);
        if ((livem >> j) & 1u) v[j] = col[r[j]];                 // the live entries only (a row of the table, never under a missing bit)
      }
    }
    uint32_t lrun = 0, mrun = 0;                                 // wave-uniform: live / missing entries of the tile so far
    uint64_t lbase = 0, mbase = 0;
    if (PHASE == 1) { lbase = R.live_base ? R.live_base[tile] : (uint64_t)tile * 1024; mbase = R.miss_base ? R.miss_base[tile] : 0ull; }
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const bool live = (livem >> j) & 1u;
      const uint64_t kmask = __ballot(live), mmask = __ballot((miss >> j) & 1u);
      if (PHASE == 1) {
        const uint64_t key = select_key<DT, false>(&v[j]) ^ R.flip;
        if (live) {
          const uint64_t pos = lbase + lrun + (uint32_t)__popcll(kmask & below);
          if (pos < (uint64_t)R.cap) { R.keys[pos] = key; R.rows[pos] = r[j]; }
        }
        if ((mmask >> lane) & 1ull) {
          const uint64_t pos = mbase + mrun + (uint32_t)__popcll(mmask & below);
          if (pos < (uint64_t)R.miss_cap) R.miss_rows[pos] = r[j];
        }
        hist_add_keys<NB>(hist, key, live, kmask, lane);
      }
      lrun += (uint32_t)__popcll(kmask); mrun += (uint32_t)__popcll(mmask);
    }
    if (PHASE == 0 && lane == 0) { R.live_cnt[tile] = lrun; R.miss_cnt[tile] = mrun; }
  }
  if (PHASE == 1) {
    __syncthreads();
    for (int i = threadIdx.x; i < NB * 256; i += kSortBlock) { const uint32_t h = hist[i]; if (h) atomicAdd(&R.ghist[i], (unsigned long long)h); }
  }
}

void launch_sort_rekey(hipStream_t s, const ColRef& col, const SortRekey& R, bool count_phase) {
  const int64_t ntiles = (R.n + 1023) / 1024;
  if (ntiles < 1) return;
  int grid = (int)((ntiles + kSortWaves - 1) / kSortWaves);
  if (grid > kSortBuildBlocks) grid = kSortBuildBlocks;
  with_dtype<DtValues>(col.dtype, [&](auto c) {      // (Bool as DFDB_U8)
    constexpr int DT = decltype(c)::dtype;
    using T = typename SelT<DT>::type;
    if (count_phase) hipLaunchKernelGGL((k_sort_rekey<DT, 0>), dim3(grid), dim3(kSortBlock), 0, s, (const T*)col.data, col.missing, R);
    else hipLaunchKernelGGL((k_sort_rekey<DT, 1>), dim3(grid), dim3(kSortBlock), 0, s, (const T*)col.data, col.missing, R);
  });
}

// STRING KEY (k_sort_strkey): the rekey over a flat String column (sizes, one arena, one byte offset per 1024-row tile: k_strings.hip).  isless on Strings
// compares bytes unsigned and calls the shorter of two that tie the smaller: the lexicographic order of (chunk_0, .., chunk_{m-1}, length), chunk_c = bytes
// [8c, 8c + 8) read big-endian, zero beyond the string's end.  The host runs those m + 1 sub-keys through the rekey's sequence, `length` first; one launch
// keys ONE of them (R.chunk; < 0: the length).  The skeleton is the rekey's: one wave per 1024 entries of `order`, 16 coalesced loads of the entries, the 16
// gathers of their sizes (negative: the row is missing), and — a chunk, write phase — the 16 gathers of row_off[r] and tile_off[r >> 10] and then the 16
// 8-byte arena loads, each round 16 deep.  An entry whose string ends at or before the chunk issues none of the three and keys 0.  The arena load may look
// up to 7 bytes past its string: the arenas' padding covers it, as it covers copy_string's tail load.  Same placement arithmetic, same guards, 8 KB of LDS
// histograms (8 key bytes).  The length's write phase also leaves the largest live length in *R.max_len: a wave maximum, then one vector atomic per wave.
//   algorithmic bytes / entry: 4 (order) + 4 (size) [+ 4 (row_off) + 8 (arena) for a chunk the string reaches] + 12 written; what it MOVES is a 128-byte
//   line per gather when the rows are scattered: the size, the in-tile offset and the arena line (tile_off is one line per 1024 rows)
template <int PHASE>
__global__ __launch_bounds__(kSortBlock) void k_sort_strkey(StrSide a, const uint32_t* __restrict__ row_off, SortStrKey R) {
  __shared__ uint32_t hist[PHASE == 1 ? 8 * 256 : 1];
  if (PHASE == 1) {
    for (int i = threadIdx.x; i < 8 * 256; i += kSortBlock) hist[i] = 0;
    __syncthreads();
  }
  const int lane = lane_id();
  const uint64_t below = (1ull << lane) - 1ull;
  const int64_t wave = (int64_t)blockIdx.x * kSortWaves + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kSortWaves;
  const int64_t ntiles = (R.n + 1023) / 1024;
  const bool by_len = R.chunk < 0;                               // wave-uniform
  const uint32_t cb = by_len ? 0u : 8u * (uint32_t)R.chunk;      // the chunk's first byte
  uint32_t lmax = 0;                                             // the longest live string this lane has seen
  for (int64_t tile = wave; tile < ntiles; tile += nwaves) {
    const int64_t e0 = tile * 1024 + lane;
    uint32_t r[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const int64_t i = e0 + j * 64;
      r[j] = i < R.n ? __builtin_nontemporal_load(R.order + i) : 0xffffffffu;
    }
    int32_t sz[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
      sz[j] = 0;
      if ((int64_t)r[j] < R.nrows) sz[j] = a.sizes[r[j]];
    }
    uint32_t pres = 0, miss = 0;                                 // bit j: entry j of this lane is there / is missing in this column
#pragma unroll
    for (int j = 0; j < 16; j++) {
      if ((int64_t)r[j] < R.nrows) pres |= 1u << j;
      if (sz[j] < 0) miss |= 1u << j;
    }
    const uint32_t livem = pres & ~miss;
    uint64_t v[PHASE == 1 ? 16 : 1];
    if (PHASE == 1) {
      if (by_len) {
#pragma unroll
        for (int j = 0; j < 16; j++) {
          const uint32_t len = (livem >> j) & 1u ? (uint32_t)sz[j] : 0u;
          v[j] = len;
          lmax = len > lmax ? len : lmax;
        }
      } else {
        uint32_t need = 0;                                       // bit j: entry j is live and its string reaches into the chunk
#pragma unroll
        for (int j = 0; j < 16; j++) if (((livem >> j) & 1u) && (uint32_t)sz[j] > cb) need |= 1u << j;
        uint32_t ro[16]; int64_t to[16];
#pragma unroll
        for (int j = 0; j < 16; j++) {
          ro[j] = 0; to[j] = 0;
          if ((need >> j) & 1u) { ro[j] = row_off[r[j]]; to[j] = a.tile_off[r[j] >> 10]; }
        }
#pragma unroll
        for (int j = 0; j < 16; j++) {
          v[j] = 0;
          if ((need >> j) & 1u) v[j] = load_u64_unaligned(a.bytes + to[j] + (int64_t)ro[j] + (int64_t)cb);      // (inside the row: cb < its length)
        }
#pragma unroll
        for (int j = 0; j < 16; j++) {
          const uint32_t rem = (uint32_t)sz[j] - cb;             // the string's bytes from the chunk's first on (used under `need` only: >= 1)
          uint64_t k = __builtin_bswap64(v[j]);                  // the first byte of the chunk becomes the key's top byte
          if (rem - 1u < 7u) k &= ~0ull << (8u * (8u - rem));    // 1..7 bytes left: the bytes behind the string's end are not its own
          v[j] = (need >> j) & 1u ? k : 0ull;
        }
      }
    }
    uint32_t lrun = 0, mrun = 0;                                 // wave-uniform: live / missing entries of the tile so far
    uint64_t lbase = 0, mbase = 0;
    if (PHASE == 1) { lbase = R.live_base ? R.live_base[tile] : (uint64_t)tile * 1024; mbase = R.miss_base ? R.miss_base[tile] : 0ull; }
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const bool live = (livem >> j) & 1u;
      const uint64_t kmask = __ballot(live), mmask = __ballot((miss >> j) & 1u);
      if (PHASE == 1) {
        const uint64_t key = v[j] ^ R.flip;
        if (live) {
          const uint64_t pos = lbase + lrun + (uint32_t)__popcll(kmask & below);
          if (pos < (uint64_t)R.cap) { R.keys[pos] = key; R.rows[pos] = r[j]; }
        }
        if ((mmask >> lane) & 1ull) {
          const uint64_t pos = mbase + mrun + (uint32_t)__popcll(mmask & below);
          if (pos < (uint64_t)R.miss_cap) R.miss_rows[pos] = r[j];
        }
        hist_add_keys<8>(hist, key, live, kmask, lane);
      }
      lrun += (uint32_t)__popcll(kmask); mrun += (uint32_t)__popcll(mmask);
    }
    if (PHASE == 0 && lane == 0) { R.live_cnt[tile] = lrun; R.miss_cnt[tile] = mrun; }
  }
  if (PHASE == 1) {
    if (by_len && R.max_len) {
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)lmax, d, 64); lmax = o > lmax ? o : lmax; }
      if (lane == 0 && lmax) atomicMax(R.max_len, lmax);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 8 * 256; i += kSortBlock) { const uint32_t h = hist[i]; if (h) atomicAdd(&R.ghist[i], (unsigned long long)h); }
  }
}

void launch_sort_strkey(hipStream_t s, const StrSide& col, const uint32_t* row_off, const SortStrKey& R, bool count_phase) {
  const int64_t ntiles = (R.n + 1023) / 1024;
  if (ntiles < 1) return;
  int grid = (int)((ntiles + kSortWaves - 1) / kSortWaves);
  if (grid > kSortBuildBlocks) grid = kSortBuildBlocks;
  if (count_phase) hipLaunchKernelGGL((k_sort_strkey<0>), dim3(grid), dim3(kSortBlock), 0, s, col, row_off, R);
  else hipLaunchKernelGGL((k_sort_strkey<1>), dim3(grid), dim3(kSortBlock), 0, s, col, row_off, R);
}

// the selected rows, ascending and 0-based, at live_base[tile] + their rank in the tile: the build's walk and placement, no column and no key
__global__ __launch_bounds__(kSortBlock) void k_sort_rows(const uint64_t* __restrict__ bitmap, const uint32_t* __restrict__ tile_counts,
                                                          const uint64_t* __restrict__ live_base, int64_t nrows, uint32_t* __restrict__ order, int64_t cap) {
  const int lane = lane_id();
  const uint64_t below = (1ull << lane) - 1ull;
  const int64_t wave = (int64_t)blockIdx.x * kSortWaves + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kSortWaves;
  const int64_t nwords = (nrows + 63) / 64, ntiles = (nwords + 15) / 16;
  for (int64_t tile = wave; tile < ntiles; tile += nwaves) {
    if (tile_counts[tile] == 0) continue;                        // wave-uniform: dead tiles do not touch the bitmap
    const int64_t wi = tile * 16 + lane;
    const uint64_t myw = (lane < 16 && wi < nwords) ? bitmap[wi] : 0ull;
    const uint64_t base = live_base[tile];
    uint32_t run = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const uint64_t ws = __shfl(myw, j, 64);
      const int64_t row = tile * 1024 + j * 64 + lane;
      if (((ws >> lane) & 1ull) && row < nrows) {
        const uint64_t pos = base + run + (uint32_t)__popcll(ws & below);
        if (pos < (uint64_t)cap) order[pos] = (uint32_t)row;
      }
      run += (uint32_t)__popcll(ws);
    }
  }
}
void launch_sort_rows(hipStream_t s, const uint64_t* bitmap, const uint32_t* tile_counts, const uint64_t* live_base, int64_t nrows, uint32_t* order, int64_t cap) {
  const int64_t nwords = (nrows + 63) / 64, ntiles = (nwords + 15) / 16;
  if (ntiles < 1) return;
  int grid = (int)((ntiles + kSortWaves - 1) / kSortWaves);
  if (grid > kSortBuildBlocks) grid = kSortBuildBlocks;
  hipLaunchKernelGGL(k_sort_rows, dim3(grid), dim3(kSortBlock), 0, s, bitmap, tile_counts, live_base, nrows, order, cap);
}

// one workgroup per chunk: counts[bin * nchunks + chunk] =the chunk's pairs whose key bits [shift, shift + 8) are `bin`
__global__ __launch_bounds__(kSortBlock) void k_sort_count(const uint64_t* __restrict__ keys, int64_t n, int shift, uint32_t* __restrict__ counts, int64_t nchunks) {
  __shared__ uint32_t hist[256];
  hist[threadIdx.x] = 0;
  __syncthreads();
  const int lane = lane_id();
  const int64_t chunk = blockIdx.x, base = chunk * kSortChunk;
  uint64_t k[kSortRounds];
#pragma unroll
  for (int r = 0; r < kSortRounds; r++) {
    const int64_t i = base + r * kSortBlock + threadIdx.x;
    k[r] = i < n ? __builtin_nontemporal_load(keys + i) : 0ull;
  }
#pragma unroll
  for (int r = 0; r < kSortRounds; r++) {
    const bool valid = base + r * kSortBlock + threadIdx.x < n;
    const uint32_t d = (uint32_t)(k[r] >> shift) & 255u;
    const uint64_t m = match_digit(d, valid);                    // one LDS add per distinct digit of the wave's 64 pairs
    if (valid && lane == __ffsll((unsigned long long)m) - 1) atomicAdd(&hist[d], (uint32_t)__popcll(m));
  }
  __syncthreads();
  counts[(int64_t)threadIdx.x * nchunks + chunk] = hist[threadIdx.x];
}

__global__ __launch_bounds__(kSortBlock) void k_sort_scatter(const uint64_t* __restrict__ keys_in, const uint32_t* __restrict__ rows_in, int64_t n, int shift,
                                                             const uint64_t* __restrict__ starts, int64_t nchunks, uint64_t* __restrict__ keys_out,
                                                             uint32_t* __restrict__ rows_out) {
  __shared__ uint64_t skeys[kSortChunk];
  __shared__ uint32_t srows[kSortChunk];
  __shared__ uint64_t wbuf[kSortWaves * 256 / 2];                // first wcnt[wave][digit] (u32), then gbase[digit] (u64)
  __shared__ uint32_t wtot[kSortWaves];
  uint32_t* wcnt = (uint32_t*)wbuf;
  const int lane = lane_id(), w = (int)(threadIdx.x >> 6);
  const uint64_t below = (1ull << lane) - 1ull;
  const int64_t chunk = blockIdx.x, base = chunk * kSortChunk;
  const int cnt = (int)(n - base < kSortChunk ? n - base : kSortChunk);
  for (int i = threadIdx.x; i < kSortWaves * 256; i += kSortBlock) wcnt[i] = 0;
  uint64_t k[kSortRounds]; uint32_t rw[kSortRounds], rk[kSortRounds];
#pragma unroll
  for (int r = 0; r < kSortRounds; r++) {                        // wave w: pairs [w * kSortWaveSpan, (w + 1) * kSortWaveSpan) of the chunk, 64 per round
    const int li = w * kSortWaveSpan + r * 64 + lane;
    k[r] = 0; rw[r] = 0;
    if (li < cnt) { k[r] = __builtin_nontemporal_load(keys_in + base + li); rw[r] = __builtin_nontemporal_load(rows_in + base + li); }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kSortRounds; r++) {
    const bool valid = w * kSortWaveSpan + r * 64 + lane < cnt;
    const uint32_t d = (uint32_t)(k[r] >> shift) & 255u;
    const uint64_t m = match_digit(d, valid);
    const uint32_t before = valid ? wcnt[w * 256 + d] : 0u;      // the digit's pairs in this wave's earlier rounds
    rk[r] = before + (uint32_t)__popcll(m & below);
    wave_lds_fence();
    if (valid && lane == __ffsll((unsigned long long)m) - 1) wcnt[w * 256 + d] = before + (uint32_t)__popcll(m);
    wave_lds_fence();
  }
  __syncthreads();
  // thread = digit: exclusive scan across the waves, then across the digits; wcnt[w][d] becomes where wave w's pairs of digit d start in the staged chunk
  uint64_t gbase;
  {
    const int d = threadIdx.x;
    uint32_t c[kSortWaves], tot = 0;
#pragma unroll
    for (int x = 0; x < kSortWaves; x++) { c[x] = wcnt[x * 256 + d]; tot += c[x]; }
    const uint32_t incl = wave_incl_scan(tot);
    if (lane == 63) wtot[w] = incl;
    __syncthreads();
    uint32_t dstart = incl - tot;
    for (int x = 0; x < w; x++) dstart += wtot[x];
    uint32_t run = dstart;
#pragma unroll
    for (int x = 0; x < kSortWaves; x++) { wcnt[x * 256 + d] = run; run += c[x]; }
    gbase = starts[(int64_t)d * nchunks + chunk] - dstart;       // staged position i of digit d goes to gbase + i
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kSortRounds; r++) {
    if (w * kSortWaveSpan + r * 64 + lane < cnt) {
      const uint32_t d = (uint32_t)(k[r] >> shift) & 255u;
      const uint32_t pos = wcnt[w * 256 + d] + rk[r];
      skeys[pos] = k[r]; srows[pos] = rw[r];
    }
  }
  __syncthreads();
  wbuf[threadIdx.x] = gbase;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kSortRounds; r++) {
    const int i = r * kSortBlock + threadIdx.x;
    if (i < cnt) {
      const uint64_t key = skeys[i];
      const uint64_t g = wbuf[(uint32_t)(key >> shift) & 255u] + (uint64_t)i;
      if (g < (uint64_t)n) { keys_out[g] = key; rows_out[g] = srows[i]; }
    }
  }
}

void launch_sort_count(hipStream_t s, const uint64_t* keys, int64_t n, int shift, uint32_t* counts) {
  const int64_t nchunks = sort_chunks(n);
  if (nchunks > 0) hipLaunchKernelGGL(k_sort_count, dim3((unsigned)nchunks), dim3(kSortBlock), 0, s, keys, n, shift, counts, nchunks);
}
void launch_sort_scatter(hipStream_t s, const uint64_t* keys_in, const uint32_t* rows_in, int64_t n, int shift, const uint64_t* starts, uint64_t* keys_out,
                         uint32_t* rows_out) {
  const int64_t nchunks = sort_chunks(n);
  if (nchunks > 0) hipLaunchKernelGGL(k_sort_scatter, dim3((unsigned)nchunks), dim3(kSortBlock), 0, s, keys_in, rows_in, n, shift, starts, nchunks, keys_out, rows_out);
}

// 0-based 32-bit rows -> 1-based table row numbers
__global__ __launch_bounds__(kSortBlock) void k_sort_emit(const uint32_t* __restrict__ rows, int64_t n, int64_t* __restrict__ out, int64_t row_base) {
  for (int64_t i = (int64_t)blockIdx.x * kSortBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSortBlock) out[i] = row_base + (int64_t)rows[i] + 1;
}
void launch_sort_emit(hipStream_t s, const uint32_t* rows, int64_t n, int64_t* out, int64_t row_base) {
  if (n <= 0) return;
  const int64_t g = (n + kSortBlock - 1) / kSortBlock;
  hipLaunchKernelGGL(k_sort_emit, dim3((unsigned)(g > 4096 ? 4096 : g)), dim3(kSortBlock), 0, s, rows, n, out, row_base);
}

// out[i] = col[rows[i] - 1 - row_base] (+ the missing bit as a byte): coalesced on the index and the output side.  A row outside the table raises *flag
// and writes nothing
template <typename T>
__global__ __launch_bounds__(kSortBlock) void k_gather_rows(const int64_t* __restrict__ rows, int64_t n, const T* __restrict__ col, T* __restrict__ out,
                                                            const uint64_t* __restrict__ missing, uint8_t* __restrict__ mout, int64_t row_base, int64_t nrows,
                                                            unsigned int* __restrict__ flag) {
  for (int64_t i = (int64_t)blockIdx.x * kSortBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSortBlock) {
    const int64_t r = rows[i] - 1 - row_base;
    if (r < 0 || r >= nrows) { atomicOr(flag, 1u); continue; }
    out[i] = col[r];
    if (mout) mout[i] = missing ? (uint8_t)((missing[r >> 6] >> (r & 63)) & 1ull) : (uint8_t)0;
  }
}
void launch_gather_rows(hipStream_t s, const int64_t* rows, int64_t n, const void* col, int width, void* out, const uint64_t* missing, uint8_t* mout, int64_t row_base,
                        int64_t nrows, uint32_t* flag) {
  if (n <= 0) return;
  const int64_t gg = (n + kSortBlock - 1) / kSortBlock;
  const dim3 g((unsigned)(gg > 8192 ? 8192 : gg)), b(kSortBlock);
  switch (width) {
    case 1: hipLaunchKernelGGL((k_gather_rows<uint8_t>), g, b, 0, s, rows, n, (const uint8_t*)col, (uint8_t*)out, missing, mout, row_base, nrows, flag); break;
    case 2: hipLaunchKernelGGL((k_gather_rows<uint16_t>), g, b, 0, s, rows, n, (const uint16_t*)col, (uint16_t*)out, missing, mout, row_base, nrows, flag); break;
    case 4: hipLaunchKernelGGL((k_gather_rows<uint32_t>), g, b, 0, s, rows, n, (const uint32_t*)col, (uint32_t*)out, missing, mout, row_base, nrows, flag); break;
    default: hipLaunchKernelGGL((k_gather_rows<uint64_t>), g, b, 0, s, rows, n, (const uint64_t*)col, (uint64_t*)out, missing, mout, row_base, nrows, flag); break;
  }
}

}  // namespace dfdb
