// k_str_rows.hip — K13: a flat String column at given rows, in the given order (gfx950): the String side of dfdb_gather_rows_any.
//
// Replaces sort!(materialize(v), cols) over Base.iterate(::DFColumn) (src/tables/column.jl:102-126) for String columns: the reference builds one String per
// selected element on the host and permutes the vector.
//
// A String column holds sizes[nrows], one arena and one byte offset per 1024-row tile (k_strings.hip); there is no per-row offset, and the rows asked for come
// in any order, with repeats.  Three steps, no kernel waits on another workgroup, integer adds only (no result depends on the grid):
//   SIZES  (k_str_rows_sizes)  one wave owns 1024 consecutive OUTPUTS (a group) in 16 rounds of 64, lane = output: 16 coalesced loads of the rows, then the
//          16 gathers of their sizes in flight together.  It writes out_sizes[i] = sizes[r], src_off[i] = where row r's bytes start in the arena, and the
//          group's byte total (u32) for the scan.  A row outside the table raises the flag word with a vector atomic and writes nothing.
//          The start of row r is tile_off[r >> 10] + the bytes of its tile's rows before it.  That in-tile prefix comes in two forms (str_gather_form):
//            offsets  k_str_row_offsets runs over the column first — one wave per 1024-row tile, 16 coalesced size loads in flight, in-register wave scans
//                     (tile_prefix of str_tile.hpp) — and leaves row_off[nrows] (u32) in scratch that lives for the call; the sizes pass gathers row_off[r].
//                     8 B per column row + one more 4-byte gather per output.
//            direct   no column-wide array: k_str_rows_direct, one wave per output row, sums the clamped sizes of [tile * 1024, r): at most 16 loads per
//                     lane, then a wave_sum.  At most 4 KB per output.
//          The layout call (dfdb_gather_rows_string_bytes) runs the sizes pass in the form that writes neither out_sizes nor src_off: totals only.
//   SCAN   launch_scan_counts over the group totals -> out_off[groups + 1] (u64); the last entry is the call's byte total, which the host compares with the
//          caller's capacity before a byte moves.
//   BYTES  (k_str_rows_bytes)  one wave per group again: coalesced loads of out_sizes and src_off, destination = out_off[g] + the running total + the wave
//          exclusive scan of the clamped sizes, copy_string per lane (the arenas' padding covers its 8-byte tail load; stores are exact lengths).  A group
//          without bytes is skipped, as K6 skips its tiles.
// LDS: none in any of the four kernels (every scan is in registers).  Registers from the gfx950 resource report: see DESIGN.md §4 (K13).
#include "device_utils.hpp"
#include "kernels.hpp"
#include "str_tile.hpp"

namespace dfdb {

constexpr int kRowsBlock = 256;                                   // threads per workgroup (every kernel of this file)
constexpr int kRowsWaves = kRowsBlock / 64;
constexpr int64_t kRowsGroup = 1024;                              // outputs per wave step: sixteen rounds of 64
constexpr int kRowsGridCap = 4096;                                // most workgroups of the offsets build, the sizes pass and the bytes pass (grid-stride beyond)
constexpr int kRowsDirectGridCap = 8192;                          // ... of the direct form (one wave per output)
static_assert(kRowsGroup == 16 * 64 && kRowsGroup == kTileRows, "a group is sixteen 64-output rounds of one wave, as a tile is sixteen 64-row steps");
static_assert(kStrGatherMaxTileBytes * (uint64_t)kRowsGroup <= (1ull << 32), "a group's byte total fits 32 bits even when its 1024 outputs repeat the longest row");

static inline int rows_grid(int64_t nwaves, int cap) {
  int64_t b = (nwaves + kRowsWaves - 1) / kRowsWaves;
  return (int)(b > cap ? cap : (b < 1 ? 1 : b));
}

// offsets form, step 0: row_off[i] = the bytes of i's tile that lie before row i
__global__ __launch_bounds__(kRowsBlock) void k_str_row_offsets(const int32_t* __restrict__ sizes, uint32_t* __restrict__ row_off, int64_t nrows, int64_t ntiles) {
  const int lane = lane_id();
  const int64_t wave = (int64_t)blockIdx.x * kRowsWaves + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * kRowsWaves;
  for (int64_t tile = wave; tile < ntiles; tile += nwaves) {
    const int64_t base = tile * kTileRows;
    int32_t sz[16]; uint32_t pre[16];
    tile_sizes(sizes, base, nrows, lane, 0, sz);
    tile_prefix(sz, pre);
#pragma unroll
    for (int j = 0; j < 16; j++) { const int64_t i = base + j * 64 + lane; if (i < nrows) row_off[i] = pre[j]; }
  }
}
void launch_str_row_offsets(hipStream_t s, const int32_t* sizes, uint32_t* row_off, int64_t nrows) {
  const int64_t ntiles = (nrows + kTileRows - 1) / kTileRows;
  if (ntiles == 0) return;
  hipLaunchKernelGGL(k_str_row_offsets, dim3(rows_grid(ntiles, kRowsGridCap)), dim3(kRowsBlock), 0, s, sizes, row_off, nrows, ntiles);
}

// the sizes pass.  WRITE: out_sizes goes out; OFFS: src_off goes out, from row_off (the offsets form).  Neither: the layout call
template <bool WRITE, bool OFFS>
__global__ __launch_bounds__(kRowsBlock) void k_str_rows_sizes(const int64_t* __restrict__ rows, int64_t n, StrSide a, const uint32_t* __restrict__ row_off,
                                                               int32_t* __restrict__ out_sizes, int64_t* __restrict__ src_off, uint32_t* __restrict__ grp_bytes,
                                                               int64_t row_base, int64_t nrows, unsigned int* __restrict__ flag) {
  static_assert(WRITE || !OFFS, "the offsets are written beside the sizes");
  const int lane = lane_id();
  const int64_t wave = (int64_t)blockIdx.x * kRowsWaves + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * kRowsWaves;
  const int64_t ngroups = (n + kRowsGroup - 1) / kRowsGroup;
  for (int64_t g = wave; g < ngroups; g += nwaves) {
    const int64_t i0 = g * kRowsGroup + lane;
    int64_t r[16];
#pragma unroll
    for (int j = 0; j < 16; j++) { const int64_t i = i0 + j * 64; r[j] = i < n ? __builtin_nontemporal_load(rows + i) - 1 - row_base : -1; }
    uint32_t ok = 0;                                             // bit j: output j of this lane names a row of the table
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const bool in = r[j] >= 0 && r[j] < nrows;
      if (in) ok |= 1u << j;
      bad = bad || (!in && i0 + j * 64 < n);
    }
    if (bad) atomicOr(flag, 1u);
    int32_t sz[16];
#pragma unroll
    for (int j = 0; j < 16; j++) sz[j] = (ok >> j) & 1u ? a.sizes[r[j]] : 0;
    uint32_t bsum = 0;
    if (OFFS) {
      uint32_t ro[16]; int64_t to[16];
#pragma unroll
      for (int j = 0; j < 16; j++) { ro[j] = 0; to[j] = 0; if ((ok >> j) & 1u) { ro[j] = row_off[r[j]]; to[j] = a.tile_off[r[j] >> 10]; } }
#pragma unroll
      for (int j = 0; j < 16; j++) if ((ok >> j) & 1u) src_off[i0 + j * 64] = to[j] + (int64_t)ro[j];
    }
#pragma unroll
    for (int j = 0; j < 16; j++) {
      bsum += clamp_size(sz[j]);
      if (WRITE && ((ok >> j) & 1u)) out_sizes[i0 + j * 64] = sz[j];
    }
    bsum = wave_sum(bsum);
    if (lane == 0) grp_bytes[g] = bsum;
  }
}

// direct form: src_off[i] for every output, one wave per output: the clamped sizes of the rows of r's tile before r, summed
__global__ __launch_bounds__(kRowsBlock) void k_str_rows_direct(const int64_t* __restrict__ rows, int64_t n, StrSide a, int64_t* __restrict__ src_off, int64_t row_base,
                                                                int64_t nrows) {
  const int lane = lane_id();
  const int64_t wave = (int64_t)blockIdx.x * kRowsWaves + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * kRowsWaves;
  for (int64_t i = wave; i < n; i += nwaves) {
    const int64_t r = rows[i] - 1 - row_base;                    // wave-uniform
    if (r < 0 || r >= nrows) continue;                           // (the sizes pass has raised the flag)
    const int64_t base = r & ~(kTileRows - 1);
    const int before = (int)(r - base);                          // rows of the tile in front of r: 0..1023, all inside the column
    const int32_t* ts = a.sizes + base + lane;
    uint32_t s = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) if (j * 64 + lane < before) s += clamp_size(ts[j * 64]);
    s = wave_sum(s);
    if (lane == 0) src_off[i] = a.tile_off[r >> 10] + (int64_t)s;
  }
}

void launch_str_rows_sizes(hipStream_t s, const StrRows& R, StrGatherForm form, const uint32_t* row_off, int32_t* out_sizes, int64_t* src_off, uint32_t* grp_bytes) {
  if (R.n <= 0) return;
  const int64_t ngroups = (R.n + kRowsGroup - 1) / kRowsGroup;
  const dim3 g(rows_grid(ngroups, kRowsGridCap)), b(kRowsBlock);
  if (form == STR_GATHER_LAYOUT) hipLaunchKernelGGL((k_str_rows_sizes<false, false>), g, b, 0, s, R.rows, R.n, R.col, row_off, out_sizes, src_off, grp_bytes, R.row_base, R.nrows, R.flag);
  else if (form == STR_GATHER_OFFSETS) hipLaunchKernelGGL((k_str_rows_sizes<true, true>), g, b, 0, s, R.rows, R.n, R.col, row_off, out_sizes, src_off, grp_bytes, R.row_base, R.nrows, R.flag);
  else {
    hipLaunchKernelGGL((k_str_rows_sizes<true, false>), g, b, 0, s, R.rows, R.n, R.col, row_off, out_sizes, src_off, grp_bytes, R.row_base, R.nrows, R.flag);
    hipLaunchKernelGGL(k_str_rows_direct, dim3(rows_grid(R.n, kRowsDirectGridCap)), b, 0, s, R.rows, R.n, R.col, src_off, R.row_base, R.nrows);
  }
}

// the bytes pass: output i's bytes from arena + src_off[i] to out_bytes + (out_off[group] + the clamped sizes of the group's outputs before i)
__global__ __launch_bounds__(kRowsBlock) void k_str_rows_bytes(const int32_t* __restrict__ out_sizes, const int64_t* __restrict__ src_off, int64_t n,
                                                               const uint8_t* __restrict__ arena, const uint64_t* __restrict__ out_off, uint8_t* __restrict__ out_bytes,
                                                               int64_t out_cap) {
  const int lane = lane_id();
  const int64_t wave = (int64_t)blockIdx.x * kRowsWaves + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * kRowsWaves;
  const int64_t ngroups = (n + kRowsGroup - 1) / kRowsGroup;
  for (int64_t g = wave; g < ngroups; g += nwaves) {
    int64_t drun = (int64_t)out_off[g];
    if ((int64_t)out_off[g + 1] == drun) continue;               // wave-uniform: a group without bytes has nothing to copy
    const int64_t i0 = g * kRowsGroup + lane;
    int32_t sz[16]; int64_t so[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const int64_t i = i0 + j * 64;
      sz[j] = i < n ? __builtin_nontemporal_load(out_sizes + i) : 0;
      so[j] = i < n ? __builtin_nontemporal_load(src_off + i) : 0;
    }
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const uint32_t c = clamp_size(sz[j]);
      const uint32_t incl = wave_incl_scan(c);
      const int64_t d = drun + (int64_t)(incl - c);
      if (c && d + (int64_t)c <= out_cap) copy_string(out_bytes + d, arena + so[j], c);
      drun += (int64_t)__shfl(incl, 63, 64);
    }
  }
}
void launch_str_rows_bytes(hipStream_t s, const int32_t* out_sizes, const int64_t* src_off, int64_t n, const uint8_t* arena, const uint64_t* out_off, uint8_t* out_bytes,
                           int64_t out_cap) {
  if (n <= 0) return;
  const int64_t ngroups = (n + kRowsGroup - 1) / kRowsGroup;
  hipLaunchKernelGGL(k_str_rows_bytes, dim3(rows_grid(ngroups, kRowsGridCap)), dim3(kRowsBlock), 0, s, out_sizes, src_off, n, arena, out_off, out_bytes, out_cap);
}

}  // namespace dfdb
