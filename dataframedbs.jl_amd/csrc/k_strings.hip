// k_strings.hip — K4/K5/K6: FlatStringsVector columns on gfx950.
//
// Device layout of a String column (reference: src/FlatStringsVectors.jl:5-9): int32 sizes[nrows]
// (-1 = missing, contributes 0 bytes), one byte arena for the whole resident column, and — instead of the
// reference's per-row Int64 offsets vector (rebuilt serially by unsafe_remake_offsets!, :61-70) — one
// u64 byte offset per 1024-row tile.  A row's offset is tile_off[tile] + the wave prefix-sum of the sizes
// before it, recomputed on the fly, so the scan reads 4 B (size) + len B per row and no 8-B offset.
//   K4 tile byte totals + scan              replaces unsafe_remake_offsets!
//   K5 s OP "const" -> bitmap                replaces getindex -> unsafe_string -> == per element (:83-85,116-121)
//   K6 gather sizes + bytes of selected rows replaces getindex(a, r) (:136-157)
#include "device_utils.hpp"
#include "kernels.hpp"
#include "str_tile.hpp"
#include <cstring>

namespace dfdb {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = 4;
constexpr int64_t kTile = 1024;

static inline int grid_for(int64_t nunits, int cap = 4096) {
  int64_t b = (nunits + kWavesPerBlock - 1) / kWavesPerBlock;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

// ---------------------------------------------------------------- K4
__global__ __launch_bounds__(kBlock) void k_str_tile_bytes(const int32_t* __restrict__ sizes, uint32_t* __restrict__ tile_bytes, int64_t nrows,
                                                           int64_t ntiles, uint32_t* __restrict__ max_tile_bytes) {
  const int lane = lane_id();
  const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  uint32_t most = 0;
  for (int64_t tile = wave; tile < ntiles; tile += nwaves) {
    uint32_t s = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) { const int64_t i = tile * kTile + j * 64 + lane; if (i < nrows) s += clamp_size(sizes[i]); }
    s = wave_sum(s);
    if (lane == 0) tile_bytes[tile] = s;
    most = s > most ? s : most;
  }
  if (max_tile_bytes && lane == 0 && most) atomicMax(max_tile_bytes, most);      // (one per wave: K5 stages a tile's bytes in LDS when the largest tile fits)
}
void launch_str_tile_bytes(hipStream_t s, const int32_t* sizes, uint32_t* tile_bytes, int64_t nrows, uint32_t* max_tile_bytes) {
  const int64_t ntiles = (nrows + kTile - 1) / kTile;
  if (ntiles == 0) return;
  hipLaunchKernelGGL(k_str_tile_bytes, dim3(grid_for(ntiles)), dim3(kBlock), 0, s, sizes, tile_bytes, nrows, ntiles, max_tile_bytes);
}

// ---------------------------------------------------------------- K5
struct Pattern { uint64_t w[8]; int32_t len; };   // patterns up to 64 bytes travel in the kernel arguments

// compare `len` bytes at p with the pattern (8 bytes at a time; the arena is padded so the last probe is safe)
__device__ __forceinline__ bool bytes_equal(const uint8_t* p, const Pattern& pat, int len) {
  int k = 0, wi = 0;
  for (; k + 8 <= len; k += 8, wi++) if (load_u64_unaligned(p + k) != pat.w[wi]) return false;
  const int rem = len - k;
  if (rem > 0) {
    const uint64_t mask = ~0ull >> (64 - 8 * rem);
    if ((load_u64_unaligned(p + k) & mask) != (pat.w[wi] & mask)) return false;
  }
  return true;
}
__device__ __forceinline__ bool bytes_equal_long(const uint8_t* p, const uint8_t* pat, int len) {
  for (int k = 0; k < len; k++) if (p[k] != pat[k]) return false;
  return true;
}

template <bool AND_EXISTING>
__global__ __launch_bounds__(kBlock) void k_str_match(const int32_t* __restrict__ sizes, const int64_t* __restrict__ tile_off,
                                                      const uint8_t* __restrict__ bytes, Pattern pat, const uint8_t* __restrict__ pat_long,
                                                      int mode, uint64_t* __restrict__ bitmap, uint32_t* __restrict__ tile_counts, int64_t nrows,
                                                      int64_t ntiles) {
  const int lane = lane_id();
  const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  const int plen = pat.len;
  for (int64_t tile = wave; tile < ntiles; tile += nwaves) {
    uint64_t existing = ~0ull;
    if (AND_EXISTING) {
      existing = lane < 16 ? bitmap[tile * 16 + lane] : 0ull;
      if (__ballot(existing != 0) == 0) { if (lane == 0) tile_counts[tile] = 0; continue; }
    }
    int64_t run = tile_off[tile];
    const int64_t base = tile * kTile;
    int32_t sz[16];
    tile_sizes<false>(sizes, base, nrows, lane, 0, sz);
    uint64_t myword = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const uint32_t c = clamp_size(sz[j]);
      const uint32_t incl = wave_incl_scan(c);
      const int64_t off = run + (int64_t)(incl - c);
      run += (int64_t)__shfl(incl, 63, 64);
      const bool inb = base + j * 64 + lane < nrows && sz[j] >= 0;          // (a missing row — size -1 — selects nothing under any of the four terms)
      bool r = false;
      const int len = (int)c;
      if (inb) {
        if (mode <= 1) {            // == / != : length first, then bytes
          bool eq = len == plen;
          if (eq && plen > 0) eq = plen <= 64 ? bytes_equal(bytes + off, pat, plen) : bytes_equal_long(bytes + off, pat_long, plen);
          r = mode == 0 ? eq : !eq;
        } else if (len >= plen) {   // startswith / endswith
          const uint8_t* p = bytes + off + (mode == 3 ? len - plen : 0);
          r = plen == 0 ? true : (plen <= 64 ? bytes_equal(p, pat, plen) : bytes_equal_long(p, pat_long, plen));
        }
      }
      const uint64_t m = __ballot(r);
      if (lane == j) myword = m;
    }
    if (AND_EXISTING) myword &= existing;
    tile_close<false>(bitmap, tile_counts, tile, lane, myword);
  }
}

// Patterns up to 64 bytes (brand / event-type equality; the first 8 bytes decide for almost every row): three phases per 8 steps so that
// the byte probes of 8 x 64 rows are all in flight together instead of one dependent round trip per 64 rows:
//   A  wave prefix-sums of the sizes -> per-row byte offsets       (ALU only)
//   B  one unaligned 8-byte probe per candidate row (size matches) (8 loads in flight per lane)
//   C  masked compare + ballot = bitmap word
// round 4: the tile's bytes arrive through LDS.  The probes of the candidate rows used to be the only readers of the arena — 8-byte loads at byte-granular
// addresses, a few active lanes per instruction, every 128-byte line of the arena fetched anyway because a line holds ~20 strings — and the pass ran at 0.58-0.64
// of the HBM peak.  Now the wave streams the tile's byte range [tile_off[t], tile_off[t+1]) with aligned 16-byte loads that are in flight together with the sixteen
// size loads, parks it in 8 KB of LDS, and the probes read there.  A tile whose strings do not fit (mean length above ~7) keeps the direct probes.
constexpr uint32_t kStageBytes = kStrStageBytes;
__device__ __forceinline__ uint64_t lds_probe(const uint32_t* st, uint32_t off) {     // 8 bytes at byte offset `off` of the staged range
  const uint32_t i = off >> 2, sh = off & 3u;
  const uint32_t w0 = st[i], w1 = st[i + 1], w2 = st[i + 2];
  return (uint64_t)__builtin_amdgcn_alignbyte(w1, w0, sh) | ((uint64_t)__builtin_amdgcn_alignbyte(w2, w1, sh) << 32);
}

// CAP (dfdb_query_hint_materialize, the string column itself is projected): the pass that decides the rows also keeps them — the
// size of every selected row at cap_sizes[tile * 1024 + rank], its bytes packed at the tile's own arena offset in cap_bytes, the
// tile's selected byte total in sel_tile_bytes — so K6 does not read the column again: the projection is a contiguous copy per tile.
// LONG: patterns of 9..64 bytes (a second probe rides along, the rest is compared where 16 bytes matched); !LONG keeps the one-probe kernel as it was
template <bool AND_EXISTING, int MODE, bool CAP, bool LONG, bool STAGE>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(CAP ? 2 : 4))) void k_str_match_short(const int32_t* __restrict__ sizes, const int64_t* __restrict__ tile_off,
                                                            const uint8_t* __restrict__ bytes, uint64_t patw, uint64_t patw1, int plen,
                                                            const uint8_t* __restrict__ pat_dev, uint64_t* __restrict__ bitmap, uint32_t* __restrict__ tile_counts, int64_t nrows,
                                                            int64_t ntiles, int32_t* __restrict__ cap_sizes, uint8_t* __restrict__ cap_bytes,
                                                            uint32_t* __restrict__ sel_tile_bytes) {
  // patw / patw1: bytes 0..7 / 8..15 of the pattern; pat_dev: the whole pattern in device memory (read only where 16 bytes matched)
  const int lane = lane_id();
  const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  const uint64_t mask = plen >= 8 ? ~0ull : ((1ull << (8 * plen)) - 1ull);
  const uint64_t want = patw & mask;
  const uint64_t mask2 = plen >= 16 ? ~0ull : (plen > 8 ? ((1ull << (8 * (plen - 8))) - 1ull) : 0ull);
  const uint64_t want2 = patw1 & mask2;
  __shared__ __attribute__((aligned(16))) uint32_t stage_sh[STAGE ? kWavesPerBlock : 1][STAGE ? kStageBytes / 4 + 8 : 4];
  uint32_t* const stage = stage_sh[STAGE ? (threadIdx.x >> 6) : 0];
  for (int64_t tile = wave; tile < ntiles; tile += nwaves) {
    uint64_t existing = ~0ull;
    if (AND_EXISTING) {
      existing = lane < 16 ? bitmap[tile * 16 + lane] : 0ull;
      if (__ballot(existing != 0) == 0) { if (lane == 0) tile_counts[tile] = 0; continue; }
    }
    const uint8_t* tb = bytes + tile_off[tile];
    const int64_t base = tile * kTile;
    int32_t sz[16];
#pragma unroll   // (not tile_sizes: through the helper the compiler allocates this kernel's registers differently, and the occupancy of several forms moves)
    for (int j = 0; j < 16; j++) { const int64_t i = base + j * 64 + lane; sz[j] = i < nrows ? __builtin_nontemporal_load(sizes + i) : -2; }
    // the tile's byte range, eight 1-KB pieces at most, all in flight with the size loads (the launcher has checked that the column's largest tile fits)
    const TileSpan ts = tile_span(tile_off, tile);
    if (STAGE) stage_tile<8, kStageBytes>(bytes, ts, (uint8_t*)stage, lane);
    uint64_t myword = 0;
    uint32_t run = 0;
    uint32_t cap_n = 0, cap_b = 0;                                    // CAP: selected rows / bytes of this tile so far
    uint8_t* const cb = CAP ? cap_bytes + tile_off[tile] : nullptr;
#pragma unroll
    for (int h = 0; h < 2; h++) {
      uint32_t rel[8]; uint64_t v[8], v2[LONG ? 8 : 1]; bool cand[8];
#pragma unroll
      for (int j = 0; j < 8; j++) {                                   // A
        const uint32_t c = clamp_size(sz[h * 8 + j]);
        const uint32_t incl = wave_incl_scan(c);
        rel[j] = run + incl - c;
        run += __shfl(incl, 63, 64);
      }
#pragma unroll
      for (int j = 0; j < 8; j++) {                                   // B
        const int32_t s0 = sz[h * 8 + j];
        const int len = s0 > 0 ? s0 : 0;
        cand[j] = s0 >= 0 && (MODE <= 1 ? len == plen : len >= plen);          // (-2: past the last row; -1: missing — a comparison with missing selects nothing: coalesce(term, false))
        v[j] = 0; if (LONG) v2[j] = 0;
        if (cand[j] && plen > 0) {
          const uint32_t po = rel[j] + (uint32_t)(MODE == 3 ? len - plen : 0);
          if (STAGE) {
            v[j] = lds_probe(stage, ts.lead + po);
            if (LONG) v2[j] = lds_probe(stage, ts.lead + po + 8u);
          } else {
            v[j] = load_u64_unaligned(tb + po);
            if (LONG) v2[j] = load_u64_unaligned(tb + po + 8);         // bytes 8..15 of the compared span ride along
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 8; j++) {                                   // C
        bool eq = cand[j] && ((v[j] & mask) == want);
        if (LONG) eq = eq && ((v2[j] & mask2) == want2);
        if (LONG && plen > 16 && eq) {                                        // still longer: the few rows whose first 16 bytes match compare the rest
          const int32_t s1 = sz[h * 8 + j];
          const uint8_t* p = tb + rel[j] + (MODE == 3 ? (s1 > 0 ? s1 : 0) - plen : 0);
          eq = bytes_equal_long(p + 16, pat_dev + 16, plen - 16);
        }
        const bool r = MODE == 1 ? (sz[h * 8 + j] >= 0 && !eq) : eq;
        const uint64_t m = __ballot(r);
        if (lane == h * 8 + j) myword = m;
        if (CAP && m != 0) {
          const int32_t s0 = sz[h * 8 + j];
          const uint32_t len = s0 > 0 ? (uint32_t)s0 : 0u;
          const uint32_t rank = cap_n + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
          uint32_t bpos;
          if (MODE == 0) { bpos = rank * (uint32_t)plen; cap_b += (uint32_t)__popcll(m) * (uint32_t)plen; }   // every selected row is plen bytes long
          else {
            const uint32_t sl = r ? len : 0u;
            const uint32_t incl = wave_incl_scan(sl);
            bpos = cap_b + incl - sl;
            cap_b += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
          }
          if (r) {
            cap_sizes[base + rank] = s0;
            if (MODE == 0 && !LONG) store_small(cb + bpos, v[j], len);       // the probe already holds the whole string (<= 8 bytes)
            else if (len) copy_string(cb + bpos, tb + rel[j], len);
          }
          cap_n += (uint32_t)__popcll(m);
        }
      }
    }
    if (CAP && lane == 0) sel_tile_bytes[tile] = cap_b;
    if (AND_EXISTING) myword &= existing;
    tile_close<true>(bitmap, tile_counts, tile, lane, myword);       // write-through: see k_scan_cmp
  }
}

template <int MODE, bool STAGE>
static void launch_short(hipStream_t s, int grid, bool ae, const int32_t* sizes, const int64_t* tile_off, const uint8_t* bytes, const Pattern& pat,
                         const uint8_t* pat_dev, uint64_t* bitmap, uint32_t* tc, int64_t nrows, int64_t ntiles, const StrCapture* cap) {
  dim3 g(grid), b(kBlock);
  int32_t* cs = cap ? cap->sizes : nullptr; uint8_t* cby = cap ? cap->bytes : nullptr; uint32_t* ctb = cap ? cap->tile_bytes : nullptr;
  if (pat.len > 8) {
    // the two-probe form keeps fewer waves resident and has little in flight per wave: with more workgroups than fit at once the last round runs on a
    // part-empty chip (s == "microsoft" over 5e8 rows: 1.38 ms on 2048 workgroups, 1.18 on exactly the resident 1280; the one-probe form does not care)
    static int resident = 0;
    if (resident == 0) {
      int per_cu = 0, dev = 0; hipDeviceProp_t pr;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)k_str_match_short<false, MODE, false, true, STAGE>, kBlock, 0) == hipSuccess && per_cu > 0 &&
          hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess) resident = per_cu * pr.multiProcessorCount;
      else { (void)hipGetLastError(); resident = -1; }
    }
    if (resident > 0 && (int)g.x > resident) g.x = (unsigned)resident;
    if (cap) hipLaunchKernelGGL((k_str_match_short<false, MODE, true, true, STAGE>), g, b, 0, s, sizes, tile_off, bytes, pat.w[0], pat.w[1], (int)pat.len, pat_dev, bitmap, tc, nrows, ntiles, cs, cby, ctb);
    else if (ae) hipLaunchKernelGGL((k_str_match_short<true, MODE, false, true, STAGE>), g, b, 0, s, sizes, tile_off, bytes, pat.w[0], pat.w[1], (int)pat.len, pat_dev, bitmap, tc, nrows, ntiles, cs, cby, ctb);
    else hipLaunchKernelGGL((k_str_match_short<false, MODE, false, true, STAGE>), g, b, 0, s, sizes, tile_off, bytes, pat.w[0], pat.w[1], (int)pat.len, pat_dev, bitmap, tc, nrows, ntiles, cs, cby, ctb);
  } else {
    if (cap) hipLaunchKernelGGL((k_str_match_short<false, MODE, true, false, STAGE>), g, b, 0, s, sizes, tile_off, bytes, pat.w[0], pat.w[1], (int)pat.len, pat_dev, bitmap, tc, nrows, ntiles, cs, cby, ctb);
    else if (ae) hipLaunchKernelGGL((k_str_match_short<true, MODE, false, false, STAGE>), g, b, 0, s, sizes, tile_off, bytes, pat.w[0], pat.w[1], (int)pat.len, pat_dev, bitmap, tc, nrows, ntiles, cs, cby, ctb);
    else hipLaunchKernelGGL((k_str_match_short<false, MODE, false, false, STAGE>), g, b, 0, s, sizes, tile_off, bytes, pat.w[0], pat.w[1], (int)pat.len, pat_dev, bitmap, tc, nrows, ntiles, cs, cby, ctb);
  }
}

void launch_str_match(hipStream_t s, const StrSide& a, const StrPattern& p, int mode, uint64_t* bitmap, uint32_t* tile_counts, int64_t nrows, bool and_existing,
                      const StrCapture* cap, uint32_t max_tile_bytes) {
  const int64_t ntiles = (nrows + kTile - 1) / kTile;
  if (ntiles == 0) return;
  const int32_t* sizes = a.sizes; const int64_t* tile_off = a.tile_off; const uint8_t* bytes = a.bytes;
  const uint8_t* pat_dev = p.dev; const int32_t patlen = p.len;
  Pattern pat; memset(&pat, 0, sizeof pat); pat.len = patlen;
  if (patlen > 0 && patlen <= 64) memcpy(pat.w, p.host, (size_t)patlen);   // short patterns ride in the kernel arguments
  const int grid = grid_for(ntiles, 2048);
  const StrMatchForm form = str_match_form(patlen, max_tile_bytes);
  if (form != STR_MATCH_LONG) {
    const bool stage = form == STR_MATCH_STAGED;      // every tile of the column fits the 8 KB a wave stages: the bytes come through LDS
#define DFDB_SHORT(M) do { if (stage) launch_short<M, true>(s, grid, and_existing, sizes, tile_off, bytes, pat, pat_dev, bitmap, tile_counts, nrows, ntiles, cap); \
                           else launch_short<M, false>(s, grid, and_existing, sizes, tile_off, bytes, pat, pat_dev, bitmap, tile_counts, nrows, ntiles, cap); } while (0)
    switch (mode) { case 0: DFDB_SHORT(0); break; case 1: DFDB_SHORT(1); break; case 2: DFDB_SHORT(2); break; default: DFDB_SHORT(3); break; }
#undef DFDB_SHORT
    return;
  }
  if (and_existing) hipLaunchKernelGGL((k_str_match<true>), dim3(grid), dim3(kBlock), 0, s, sizes, tile_off, bytes, pat, pat_dev, mode, bitmap, tile_counts, nrows, ntiles);
  else hipLaunchKernelGGL((k_str_match<false>), dim3(grid), dim3(kBlock), 0, s, sizes, tile_off, bytes, pat, pat_dev, mode, bitmap, tile_counts, nrows, ntiles);
}

// ---------------------------------------------------------------- K5b: s1 OP s2 over two String columns
// Base.cmp(::String, ::String): memcmp over the common prefix, then the lengths, bytes unsigned.  One wave per 1024-row tile, K5's three phases per 8 steps:
//   A  wave prefix sums of BOTH size streams -> the rows' byte offsets in the two arenas
//   B  one 8-byte probe per side of every row the sizes do not settle (== / != with unequal sizes never read a byte; a missing or dead row neither)
//   C  the first differing byte decides: both words masked to min(la, lb), compared byte-reversed as unsigned; equal words of longer strings walk on 8 bytes
//      at a time; an equal common prefix leaves it to the lengths
// The probes go to the arenas directly: parking both tiles' byte ranges in LDS first (2 x 8 KB per wave) was measured slower at config 4's
// string lengths (profiles/str_pair.txt) and is not built.  Nothing read past a string's end is trusted: the words are masked.
// -1 / 0 / 1 of two 8-byte words whose first m (1..8) bytes count: the lowest byte is the string's first, so the byte-reversed words order as memcmp does
__device__ __forceinline__ int pair_cmp_word(uint64_t x, uint64_t y, int m) {
  const uint64_t mk = m >= 8 ? ~0ull : ((1ull << (8 * m)) - 1ull);
  x &= mk; y &= mk;
  if (x == y) return 0;
  return __builtin_bswap64(x) < __builtin_bswap64(y) ? -1 : 1;
}
__device__ __forceinline__ bool pair_result(int op, int c) {
  switch (op) {
    case CMP_EQ: return c == 0; case CMP_NE: return c != 0; case CMP_LT: return c < 0;
    case CMP_LE: return c <= 0; case CMP_GT: return c > 0; default: return c >= 0;
  }
}

template <bool AND_EXISTING>
__global__ __launch_bounds__(kBlock) void k_str_pair(const int32_t* __restrict__ sizes_a, const int64_t* __restrict__ toff_a, const uint8_t* __restrict__ bytes_a,
                                                      const int32_t* __restrict__ sizes_b, const int64_t* __restrict__ toff_b, const uint8_t* __restrict__ bytes_b,
                                                      int op, uint64_t* __restrict__ bitmap, uint32_t* __restrict__ tile_counts, int64_t nrows, int64_t ntiles) {
  const int lane = lane_id();
  const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + wid, nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  const bool ordered = op >= CMP_LT;                                    // (== / != are settled by unequal sizes alone)
  for (int64_t tile = wave; tile < ntiles; tile += nwaves) {
    uint32_t ex_lo = ~0u, ex_hi = ~0u;
    if (AND_EXISTING) {
      const uint64_t existing = lane < 16 ? bitmap[tile * 16 + lane] : 0ull;
      if (__ballot(existing != 0) == 0) { if (lane == 0) tile_counts[tile] = 0; continue; }
      ex_lo = (uint32_t)existing; ex_hi = (uint32_t)(existing >> 32);
    }
    const int64_t base = tile * kTile;
    int32_t sa[16], sb[16];
    tile_sizes(sizes_a, base, nrows, lane, -2, sa);
    tile_sizes(sizes_b, base, nrows, lane, -2, sb);
    const int64_t oa0 = toff_a[tile], ob0 = toff_b[tile];
    const uint8_t* const ta = bytes_a + oa0;
    const uint8_t* const tb = bytes_b + ob0;
    uint64_t myword = 0;
    uint32_t run_a = 0, run_b = 0;
#pragma unroll
    for (int h = 0; h < 2; h++) {
      uint32_t ra[8], rb[8]; uint64_t va[8], vb[8]; bool probe[8], alive[8];
#pragma unroll
      for (int j = 0; j < 8; j++) {                                   // A
        const uint32_t ca = clamp_size(sa[h * 8 + j]), cb = clamp_size(sb[h * 8 + j]);
        const uint32_t ia = wave_incl_scan(ca), ib = wave_incl_scan(cb);
        ra[j] = run_a + ia - ca; rb[j] = run_b + ib - cb;
        run_a += __shfl(ia, 63, 64); run_b += __shfl(ib, 63, 64);
      }
#pragma unroll
      for (int j = 0; j < 8; j++) {                                   // B
        const int32_t s0 = sa[h * 8 + j], s1 = sb[h * 8 + j];
        const uint32_t la = clamp_size(s0), lb = clamp_size(s1);
        // (-2: past the last row; -1: missing — a comparison with a missing side selects nothing: coalesce(term, false))
        alive[j] = s0 >= 0 && s1 >= 0;
        if (AND_EXISTING) {
          alive[j] = alive[j] && ((tile_word(ex_lo, ex_hi, h * 8 + j) >> lane) & 1ull);   // a row the stages before dropped reads nothing (a dead word: nobody probes)
        }
        probe[j] = alive[j] && la > 0 && lb > 0 && (ordered || la == lb);
        va[j] = 0; vb[j] = 0;
        // (an 8-byte probe reads up to 7 bytes past its string, so past the arena's last byte for the last row: every arena — resident, decoded, a chunk's —
        // is allocated with 64 bytes of slack behind it (table.cpp), as K5's tail probe needs too)
        if (probe[j]) { va[j] = load_u64_unaligned(ta + ra[j]); vb[j] = load_u64_unaligned(tb + rb[j]); }
      }
#pragma unroll
      for (int j = 0; j < 8; j++) {                                   // C
        const int la = (int)clamp_size(sa[h * 8 + j]), lb = (int)clamp_size(sb[h * 8 + j]);
        const int m = la < lb ? la : lb;
        int c = la < lb ? -1 : (la > lb ? 1 : 0);                     // what the lengths say: it stands unless a byte of the common prefix differs
        if (probe[j]) {
          int d = pair_cmp_word(va[j], vb[j], m);
          for (int k = 8; d == 0 && k < m; k += 8) {                  // longer than 8 bytes and equal so far
            d = pair_cmp_word(load_u64_unaligned(ta + ra[j] + k), load_u64_unaligned(tb + rb[j] + k), m - k);
          }
          if (d) c = d;
        }
        const uint64_t mw = __ballot(alive[j] && pair_result(op, c));
        if (lane == h * 8 + j) myword = mw;
      }
    }
    tile_close<true>(bitmap, tile_counts, tile, lane, myword);         // write-through: see k_scan_cmp
  }
}

void launch_str_pair(hipStream_t s, const StrSide& a, const StrSide& b, int op, uint64_t* bitmap, uint32_t* tile_counts, int64_t nrows, bool and_existing) {
  const int64_t ntiles = (nrows + kTile - 1) / kTile;
  if (ntiles == 0) return;
  const int g = grid_for(ntiles, 2048);
  if (and_existing) hipLaunchKernelGGL((k_str_pair<true>), dim3(g), dim3(kBlock), 0, s, a.sizes, a.tile_off, a.bytes, b.sizes, b.tile_off, b.bytes, op, bitmap, tile_counts, nrows, ntiles);
  else hipLaunchKernelGGL((k_str_pair<false>), dim3(g), dim3(kBlock), 0, s, a.sizes, a.tile_off, a.bytes, b.sizes, b.tile_off, b.bytes, op, bitmap, tile_counts, nrows, ntiles);
}

// ---------------------------------------------------------------- K6
// Both passes work on 1024-row tiles, one wave per tile.  Lane l owns a 16-bit slice of the tile's bitmap
// (rows 16l..16l+15) and expands it into a 2-KB LDS list of selected in-tile positions (wave prefix-sum of
// popcounts), so everything after that is proportional to the SELECTED rows.

// tiles a wave looks at together (their emptiness decided by one load): as many as leave ~8192 waves busy — a dense selection of a small table keeps a wave per tile
static int gather_group(int64_t nt) { int g = 1; while (g < 64 && nt / (g * 2) >= 8192) g *= 2; return g; }
// stage the selected positions of `tile`; returns how many
__device__ __forceinline__ uint32_t stage_tile_positions(const uint64_t* __restrict__ bitmap, int64_t tile, uint16_t* pos, int lane) {
  uint32_t w = (uint32_t)(bitmap[tile * 16 + (lane >> 2)] >> ((lane & 3) * 16)) & 0xffffu;
  const uint32_t pc = (uint32_t)__popc(w);
  const uint32_t incl = wave_incl_scan(pc);
  const uint32_t total = __shfl(incl, 63, 64);
  uint32_t o = incl - pc;
  const uint32_t lbase = (uint32_t)lane << 4;
  while (w) { const int b = __builtin_ctz(w); w &= w - 1; pos[o++] = (uint16_t)(lbase + (uint32_t)b); }
  wave_lds_fence();
  return total;
}

// Row i of the output is a[i], or — FILL — what stands behind a missing row (size -1) of a: nothing (STR_FILL_NONE, the plain projection: the sizes go out as
// they are, -1 included), one constant (STR_FILL_CONST: device memory, padded for copy_string's 8-byte tail load) or row i of a second column of the same table
// (STR_FILL_COL): coalesce(a, b).  A row missing on both sides stays -1 and adds no byte.  The plain form reads, computes and keeps nothing for a second side.

// pass 1: selected sizes -> out_sizes at the tile's row offset, plus the selected byte total of the tile
template <StrFillKind FILL>
__global__ __launch_bounds__(kBlock) void k_str_gather_sizes(const uint64_t* __restrict__ bitmap, const uint64_t* __restrict__ prefix,
                                                             const int32_t* __restrict__ sizes_a, const int32_t* __restrict__ sizes_b, int32_t clen,
                                                             int32_t* __restrict__ out_sizes, uint32_t* __restrict__ sel_tile_bytes, int64_t ntiles,
                                                             int64_t out_cap, int group) {
  __shared__ uint16_t pos_sh[kWavesPerBlock][1024];
  static_assert(sizeof pos_sh == 8192, "workgroup LDS of the sizes pass");
  const int lane = lane_id();
  const int wib = threadIdx.x >> 6;
  uint16_t* pos = pos_sh[wib];
  const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + wib;
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  // `group` (<= 64) tiles at a time: their selected-row counts come out of the prefix sums with one coalesced load, the empty ones get their zero and are never looked at (a
  // sparse selection — ten first rows in 5e8 — used to pay one dependent bitmap load per tile: 60 us per pass)
  for (int64_t c0 = wave * group; c0 < ntiles; c0 += nwaves * group) {
   const int64_t tl = c0 + lane;
   const bool mine = lane < group && tl < ntiles;
   const bool some = mine && prefix[tl + 1] > prefix[tl];
   if (mine && !some) sel_tile_bytes[tl] = 0;
   for (uint64_t todo = __ballot(some); todo; todo &= todo - 1) {
    const int64_t tile = c0 + __builtin_ctzll(todo);
    const uint32_t total = stage_tile_positions(bitmap, tile, pos, lane);
    const int64_t obase = (int64_t)prefix[tile];
    const int32_t* ta = sizes_a + tile * kTile;
    const int32_t* tb = FILL == STR_FILL_COL ? sizes_b + tile * kTile : nullptr;
    uint32_t bsum = 0;
    for (uint32_t k = lane; k < total; k += 64) {
      const uint32_t p = pos[k];
      const int32_t sa = ta[p];
      const int32_t sz = FILL == STR_FILL_NONE || sa >= 0 ? sa : (FILL == STR_FILL_COL ? tb[p] : clen);
      bsum += clamp_size(sz);
      if (obase + k < out_cap) out_sizes[obase + k] = sz;
    }
    bsum = wave_sum(bsum);
    if (lane == 0) sel_tile_bytes[tile] = bsum;
    wave_lds_fence();
   }
  }
}

// pass 2: bytes.  Per side, the byte offset of every row of the tile from the tile's first byte (exclusive prefix of the clamped sizes of ALL its rows) goes to
// LDS once: 16 coalesced size loads + 16 in-register scans (STR_FILL_COL: 4 KB more per wave for b's).  Then 64 selected rows at a time: destination offsets by a
// wave prefix-sum of the selected sizes, and every lane copies its own string out of a's arena, b's arena or the constant.
template <StrFillKind FILL>
__global__ __launch_bounds__(kBlock) void k_str_gather_bytes(const uint64_t* __restrict__ bitmap, StrSide a, StrSide b, const uint8_t* __restrict__ cbytes,
                                                             uint32_t clen, const uint64_t* __restrict__ out_tile_off, uint8_t* __restrict__ out_bytes,
                                                             int64_t nrows, int64_t ntiles, int64_t out_cap, int group) {
  constexpr bool TWO = FILL == STR_FILL_COL;
  __shared__ uint16_t pos_sh[kWavesPerBlock][1024];
  __shared__ uint32_t pre_sh[TWO ? 2 : 1][kWavesPerBlock][1024];
  static_assert(sizeof pos_sh + sizeof pre_sh == (TWO ? 40960 : 24576), "workgroup LDS of the bytes pass");
  const int lane = lane_id();
  const int wib = threadIdx.x >> 6;
  uint16_t* pos = pos_sh[wib];
  uint32_t* pre_a = pre_sh[0][wib];
  uint32_t* pre_b = pre_sh[TWO ? 1 : 0][wib];
  const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + wib;
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  for (int64_t c0 = wave * group; c0 < ntiles; c0 += nwaves * group) {      // (`group` tiles at a time, as in pass 1: a tile without selected BYTES has nothing to copy)
   const int64_t tl = c0 + lane;
   const bool some = lane < group && tl < ntiles && out_tile_off[tl + 1] > out_tile_off[tl];
   for (uint64_t todo = __ballot(some); todo; todo &= todo - 1) {
    const int64_t tile = c0 + __builtin_ctzll(todo);
    const uint32_t total = stage_tile_positions(bitmap, tile, pos, lane);
    if (total == 0) { wave_lds_fence(); continue; }        // wave-uniform: late materialization of the arena
    const int64_t base = tile * kTile;
#pragma unroll   // (the loop written here, not in a helper: through one the compiler hoists and allocates differently, and the plain form stays as it was measured)
    for (int side = 0; side < (TWO ? 2 : 1); side++) {
      const int32_t* ss = side ? b.sizes : a.sizes;
      uint32_t* pre = side ? pre_b : pre_a;
      int32_t sz[16];
#pragma unroll
      for (int j = 0; j < 16; j++) { const int64_t i = base + j * 64 + lane; sz[j] = i < nrows ? ss[i] : 0; }
      uint32_t run = 0;
#pragma unroll
      for (int j = 0; j < 16; j++) {
        const uint32_t c = clamp_size(sz[j]);
        const uint32_t incl = wave_incl_scan(c);
        pre[j * 64 + lane] = run + incl - c;
        run += __shfl(incl, 63, 64);
      }
    }
    wave_lds_fence();
    const uint8_t* ba = a.bytes + a.tile_off[tile];
    const uint8_t* bb = TWO ? b.bytes + b.tile_off[tile] : cbytes;
    int64_t drun = (int64_t)out_tile_off[tile];
    const int32_t* tsa = a.sizes + base;
    const int32_t* tsb = TWO ? b.sizes + base : nullptr;
    for (uint32_t k0 = 0; k0 < total; k0 += 64) {
      const uint32_t k = k0 + lane;
      const bool valid = k < total;
      const uint32_t p = valid ? pos[k] : 0u;
      const int32_t sa = valid ? tsa[p] : 0;
      const bool from_a = FILL == STR_FILL_NONE || sa >= 0;
      uint32_t cs = clamp_size(sa);
      if (valid && !from_a) cs = TWO ? clamp_size(tsb[p]) : clen;
      const uint32_t incl = wave_incl_scan(cs);
      if (cs) {
        const uint8_t* sp = from_a ? ba + pre_a[p] : (TWO ? bb + pre_b[p] : bb);
        const int64_t d0 = drun + (int64_t)(incl - cs);
        if (d0 + cs <= out_cap) copy_string(out_bytes + d0, sp, cs);
      }
      drun += (int64_t)__shfl(incl, 63, 64);
    }
    wave_lds_fence();
   }
  }
}

void launch_str_gather_sizes(hipStream_t s, const uint64_t* bitmap, const uint64_t* prefix, const StrSide& a, const StrFill& fill, int32_t* out_sizes,
                             uint32_t* sel_tile_bytes, int64_t nrows, int64_t out_cap) {
  const int64_t nt = (nrows + kTile - 1) / kTile;
  if (nt == 0) return;
  const int group = gather_group(nt);
  const dim3 g(grid_for((nt + group - 1) / group)), b(kBlock);
#define DFDB_SIZES(F) hipLaunchKernelGGL((k_str_gather_sizes<F>), g, b, 0, s, bitmap, prefix, a.sizes, fill.b.sizes, fill.clen, out_sizes, sel_tile_bytes, nt, out_cap, group)
  switch (fill.kind) { case STR_FILL_NONE: DFDB_SIZES(STR_FILL_NONE); break; case STR_FILL_CONST: DFDB_SIZES(STR_FILL_CONST); break; default: DFDB_SIZES(STR_FILL_COL); break; }
#undef DFDB_SIZES
}
void launch_str_gather_bytes(hipStream_t s, const uint64_t* bitmap, const StrSide& a, const StrFill& fill, const uint64_t* out_tile_off, uint8_t* out_bytes,
                             int64_t nrows, int64_t out_bytes_cap) {
  const int64_t nt = (nrows + kTile - 1) / kTile;
  if (nt == 0) return;
  const int group = gather_group(nt);
  const dim3 g(grid_for((nt + group - 1) / group)), b(kBlock);
#define DFDB_BYTES(F) hipLaunchKernelGGL((k_str_gather_bytes<F>), g, b, 0, s, bitmap, a, fill.b, fill.const_dev, (uint32_t)fill.clen, out_tile_off, out_bytes, nrows, nt, out_bytes_cap, group)
  switch (fill.kind) { case STR_FILL_NONE: DFDB_BYTES(STR_FILL_NONE); break; case STR_FILL_CONST: DFDB_BYTES(STR_FILL_CONST); break; default: DFDB_BYTES(STR_FILL_COL); break; }
#undef DFDB_BYTES
}

// projection of a String column whose selected rows K5 kept (CAP): per 1024-row tile a contiguous copy of its sizes and bytes
__global__ __launch_bounds__(kBlock) void k_str_compact_captured(const int32_t* __restrict__ cap_sizes, const uint8_t* __restrict__ cap_bytes,
                                                                 const uint64_t* __restrict__ prefix, const int64_t* __restrict__ tile_off,
                                                                 const uint64_t* __restrict__ out_tile_off, int32_t* __restrict__ out_sizes,
                                                                 uint8_t* __restrict__ out_bytes, int64_t ntiles, int64_t out_rows, int64_t out_bytes_cap) {
  // A tile keeps ~100 rows at 10 % selectivity: two dependent round trips (offsets, then the copy) for ~0.8 KB.  One tile per wave per trip was
  // latency-bound (0.256 ms per 5e8 rows = 3.1 TB/s); each 16-lane quarter of the wave takes its own tile, four tiles in flight per trip.
  const int lane = lane_id();
  const int sub = lane >> 4, sl = lane & 15;
  const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  typedef uint64_t __attribute__((aligned(1), may_alias)) u64u;
  for (int64_t t0 = wave * 4; t0 < ntiles; t0 += nwaves * 4) {
    const int64_t tile = t0 + sub;
    if (tile >= ntiles) continue;
    const int64_t r0 = (int64_t)prefix[tile], r1 = (int64_t)prefix[tile + 1];
    const int64_t b0 = (int64_t)out_tile_off[tile], b1 = (int64_t)out_tile_off[tile + 1];
    const int32_t* ss = cap_sizes + tile * kTile;
    const uint8_t* sb = cap_bytes + tile_off[tile];
    for (int64_t k = sl; k < r1 - r0; k += 16) if (r0 + k < out_rows) out_sizes[r0 + k] = ss[k];
    const int64_t nb = b1 <= out_bytes_cap ? b1 - b0 : 0;
    const int64_t n8 = nb & ~7ll;
    for (int64_t k = (int64_t)sl * 8; k < n8; k += 128) *(u64u*)(out_bytes + b0 + k) = *(const u64u*)(sb + k);
    for (int64_t k = n8 + sl; k < nb; k += 16) out_bytes[b0 + k] = sb[k];
  }
}
void launch_str_compact_captured(hipStream_t s, const StrCapture& cap, const uint64_t* prefix, const int64_t* tile_off, const uint64_t* out_tile_off,
                                 int32_t* out_sizes, uint8_t* out_bytes, int64_t nrows, int64_t out_rows, int64_t out_bytes_cap) {
  const int64_t nt = (nrows + kTile - 1) / kTile;
  if (nt == 0) return;
  hipLaunchKernelGGL(k_str_compact_captured, dim3(grid_for((nt + 3) / 4)), dim3(kBlock), 0, s, cap.sizes, cap.bytes, prefix, tile_off, out_tile_off, out_sizes, out_bytes, nt,
                     out_rows, out_bytes_cap);
}

}  // namespace dfdb
