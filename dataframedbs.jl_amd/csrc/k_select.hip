// k_select.hip — K11: exact order statistics of a fixed-width column over the selected rows (gfx950).
//
// Replaces Statistics.median / Statistics.quantile over Base.iterate(::DFColumn) (src/tables/column.jl:102-126): the reference collects the selected
// values one element at a time and sorts them on the host.
//
// Most-significant-digit radix select, 8 bits per pass.  Every value has a SELECT KEY: an unsigned integer whose order is isless — the order of
// order_image(value_image(..), value_kind(dtype), false) (value_rules.hpp): integers by value, floats -Inf .. -0.0 < 0.0 .. Inf, every NaN last.  A pass
// streams the column through the selection bitmap (and the missing bitmap) the way the reductions do — one wave per 1024-row tile, lane = row, 16
// nontemporal loads in flight, bitmap word j broadcast out of lane j — skips the tiles whose tile count is 0, and for each of the up to 16 pending ranks
// histograms the next 8 key bits of the rows whose already decided high bits equal that rank's prefix.  Ranks that share a prefix share a histogram
// (a GROUP); the host picks, per rank, the bin that holds it and makes the rank relative to that bin (project.cpp: query_order_statistics).  The first
// pass also counts the selected rows that are not missing, that are missing, and that are NaN.  Bytes under a set missing bit are never looked at.
//
// The key is the order image itself (64 bits, 8 passes: ctx option "select_full_image" = 1) or, by default, the same order in the 8 * W bits of a
// W-byte value — the high image bits of a narrow type are a function of its own sign bit, so they carry no order of their own and their passes are
// skipped: Int32 / Float32 take 4 passes, Int8 / Bool 1.  The two forms give the same answers (tests/test_gpu_order_stat.py runs both).
//
// Histograms: 16 groups x 256 bins x 4 B = 16 KB of LDS per workgroup, flushed once per workgroup with 64-bit atomicAdd on the global counters (the
// non-zero bins only); integer adds, so the result does not depend on the grid or on the order the workgroups arrive in.  A wave whose live lanes all
// hold one (group, digit) adds once with their popcount instead of once per lane: an all-equal column, the constant high bytes under
// "select_full_image", sorted data and the late passes of a clustered column would otherwise serialise 64 adds on one LDS address.
//   algorithmic bytes / row / pass: 1/8 (bitmap) + sigma * W (column) [+ 1/8 (missing bitmap) for a nullable column]
#include "device_utils.hpp"
#include "value_rules.hpp"
#include "select_key.hpp"
#include "kernels.hpp"
#include "launch_dispatch.hpp"
#include "../../include/dfdb_ir.h"

namespace dfdb {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = 4;
constexpr int kSelBlocks = 2048;      // 8 workgroups per CU: the 32-wave limit, 128 KB of the CU's 160 KB of LDS

// the way back: a select key -> the 64 bits of the value's accumulator (value_rules.hpp value_image: integers widened, floats as Float64; the NaN key
// is the canonical quiet NaN)
uint64_t select_key_value(int dtype, bool full, uint64_t key) {
  const uint64_t qnan = 0x7ff8000000000000ull;
  if (full || dtype == DFDB_I64 || dtype == DFDB_U64 || dtype == DFDB_F64) {
    const int kind = value_kind(dtype);
    if (kind == kAccUnsigned) return key;
    if (kind == kAccSigned) return key ^ (1ull << 63);
    return key == ~0ull ? qnan : ((key >> 63) ? (key ^ (1ull << 63)) : ~key);
  }
  switch (dtype) {
    case DFDB_F32: {
      if (key == 0xffffffffull) return qnan;
      const uint32_t k = (uint32_t)key, b = (k >> 31) ? (k ^ 0x80000000u) : ~k;
      float f; __builtin_memcpy(&f, &b, 4);
      return f64_bits((double)f);
    }
    case DFDB_I8: return (uint64_t)(int64_t)(int8_t)(uint8_t)(key ^ 0x80u);
    case DFDB_I16: return (uint64_t)(int64_t)(int16_t)(uint16_t)(key ^ 0x8000u);
    case DFDB_I32: return (uint64_t)(int64_t)(int32_t)(uint32_t)(key ^ 0x80000000u);
    default: return key;
  }
}

template <int DT, bool FULL>
__global__ __launch_bounds__(kBlock) void k_select_hist(const uint64_t* __restrict__ bitmap, const uint32_t* __restrict__ tile_counts,
                                                        const uint64_t* __restrict__ missing, const typename SelT<DT>::type* __restrict__ col,
                                                        int64_t nwords, SelectPass P, unsigned long long* __restrict__ ghist,
                                                        unsigned long long* __restrict__ gcounts) {
  using T = typename SelT<DT>::type;
  __shared__ uint32_t hist[kSelectMaxRanks * 256];
  __shared__ unsigned long long cnt[3];
  const int nbins = P.ngroups * 256;
  for (int i = threadIdx.x; i < nbins; i += kBlock) hist[i] = 0;
  if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
  __syncthreads();
  const int lane = lane_id();
  const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
  const int64_t ntiles = (nwords + 15) / 16;
  const int hshift = P.shift + 8;                              // the bits above the digit: all of them decided (64: there are none)
  uint32_t c_live = 0, c_miss = 0, c_nan = 0;
  for (int64_t tile = wave; tile < ntiles; tile += nwaves) {   // 1024 rows per wave step, 16 column loads in flight
    if (tile_counts[tile] == 0) continue;                      // wave-uniform: dead tiles touch neither the bitmaps nor the column
    const int64_t wi = tile * 16 + lane;
    const bool mine = lane < 16 && wi < nwords;
    const uint64_t myw = mine ? bitmap[wi] : 0ull;
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
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const uint64_t ws = __shfl(myw, j, 64), wm = __shfl(mym, j, 64);
      const bool live = ((ws & ~wm) >> lane) & 1ull;
      if (P.first) {
        c_live += live ? 1u : 0u;
        c_miss += (((ws & wm) >> lane) & 1ull) ? 1u : 0u;
        if constexpr (DT == DFDB_F32 || DT == DFDB_F64) c_nan += (live && v[j] != v[j]) ? 1u : 0u;
      }
      if (P.ngroups == 0) continue;
      const uint64_t key = select_key<DT, FULL>(&v[j]);
      const uint64_t hi = hshift >= 64 ? 0ull : (key >> hshift);
      int slot = -1;
#pragma unroll
      for (int g = 0; g < kSelectMaxRanks; g++) {
        if (g >= P.ngroups) break;
        if (live && hi == P.prefix[g]) slot = g * 256 + (int)((key >> P.shift) & 255ull);
      }
      const uint64_t mask = __ballot(slot >= 0);
      if (mask == 0) continue;
      const int src = __ffsll((unsigned long long)mask) - 1;
      const int s0 = __shfl(slot, src, 64);
      if (__ballot(slot == s0) == mask) {                      // one (group, digit) in the whole wave: one add
        if (lane == src) atomicAdd(&hist[s0], (uint32_t)__popcll(mask));
      } else if (slot >= 0) atomicAdd(&hist[slot], 1u);
    }
  }
  if (P.first) {
    c_live = wave_sum(c_live); c_miss = wave_sum(c_miss); c_nan = wave_sum(c_nan);
    if (lane == 0) { atomicAdd(&cnt[0], (unsigned long long)c_live); atomicAdd(&cnt[1], (unsigned long long)c_miss); atomicAdd(&cnt[2], (unsigned long long)c_nan); }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nbins; i += kBlock) { const uint32_t h = hist[i]; if (h) atomicAdd(&ghist[i], (unsigned long long)h); }
  if (P.first && threadIdx.x < 3 && cnt[threadIdx.x]) atomicAdd(&gcounts[threadIdx.x], cnt[threadIdx.x]);
}

void launch_select_hist(hipStream_t s, const uint64_t* bitmap, const uint32_t* tile_counts, const ColRef& col, bool full, int64_t nrows, const SelectPass& P, uint64_t* hist,
                        uint64_t* counts) {
  const int64_t nwords = (nrows + 63) / 64, ntiles = (nwords + 15) / 16;
  int grid = (int)((ntiles + kWavesPerBlock - 1) / kWavesPerBlock);
  if (grid > kSelBlocks) grid = kSelBlocks;
  if (grid < 1) grid = 1;
  with_dtype<DtValues>(col.dtype, [&](auto c) {      // (the kernels are instantiated by the enumerator: Bool as DFDB_U8, anything that is no number as DFDB_F64)
    constexpr int DT = decltype(c)::dtype;
    using T = typename SelT<DT>::type;
    if (full) hipLaunchKernelGGL((k_select_hist<DT, true>), dim3(grid), dim3(kBlock), 0, s, bitmap, tile_counts, col.missing, (const T*)col.data, nwords, P,
                                 (unsigned long long*)hist, (unsigned long long*)counts);
    else hipLaunchKernelGGL((k_select_hist<DT, false>), dim3(grid), dim3(kBlock), 0, s, bitmap, tile_counts, col.missing, (const T*)col.data, nwords, P,
                            (unsigned long long*)hist, (unsigned long long*)counts);
  });
}

}  // namespace dfdb
