// k_image.hip — the 4-byte scan image of an 8-byte integer column (scan_image.hpp): one streaming pass, made once per column.
//
// A lane reads 16 bytes (two rows) and writes 8 (their low halves); a wave request is 1024 bytes in, 512 out, and four such loads per lane are in flight
// before the first is looked at.  A row whose value is not its truncation extended back (sign extension for Int64, zero extension for UInt64) makes the
// whole image useless: the wave that meets one raises *misfit with one vector atomic when it is done, and the host drops the image (query.cpp).
// The same pass finds the smallest and the largest image value (in the column's signedness): per lane in registers, one wave reduction at the end, one
// vector atomicMin and one atomicMax per wave.  They are what the 2-byte coarse copy is laid out from (scan_coarse.hpp; k_scan_coarse_build below).
//   algorithmic bytes / row: 8 read + 4 written
#include "device_utils.hpp"
#include "kernels.hpp"

namespace dfdb {

constexpr int kImgBlock = 256;
constexpr int kImgUnroll = 4;                         // 16-byte loads in flight per lane

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

template <bool SIGNED>
__device__ __forceinline__ bool image_misfit(uint64_t v) {
  if (SIGNED) return (uint64_t)(int64_t)(int32_t)(uint32_t)v != v;
  return (v >> 32) != 0;
}

// an image value as an unsigned word of the same order: what the min / max words hold (flag[1]: the maximum, zeroed by the caller; flag[2]: the minimum, all ones)
template <bool SIGNED> __device__ __forceinline__ uint32_t image_ordered(uint32_t x) { return SIGNED ? x ^ 0x80000000u : x; }

// col: nrows 8-byte values (+ the column's pad: the second half of the last pair of an odd column is read, never used); image: nrows 4-byte values (+ its pad)
template <bool SIGNED>
__global__ __launch_bounds__(kImgBlock) void k_scan_image_build(const uint64_t* __restrict__ col, uint32_t* __restrict__ image, int64_t nrows, uint32_t* __restrict__ flag) {
  const int64_t npairs = (nrows + 1) / 2;
  const int64_t chunk = (int64_t)kImgBlock * kImgUnroll;                     // pairs per workgroup step
  const u64x2* __restrict__ src = (const u64x2*)col;
  u32x2* __restrict__ dst = (u32x2*)image;
  bool bad = false;
  uint32_t lo = 0xffffffffu, hi = 0u;                                        // of the ordered words this lane has truncated
  for (int64_t base = (int64_t)blockIdx.x * chunk; base < npairs; base += (int64_t)gridDim.x * chunk) {
    u64x2 v[kImgUnroll];
#pragma unroll
    for (int k = 0; k < kImgUnroll; k++) {
      const int64_t p = base + (int64_t)k * kImgBlock + threadIdx.x;
      v[k] = p < npairs ? __builtin_nontemporal_load(src + p) : u64x2{0ull, 0ull};
    }
#pragma unroll
    for (int k = 0; k < kImgUnroll; k++) {
      const int64_t p = base + (int64_t)k * kImgBlock + threadIdx.x;
      if (p >= npairs) continue;
      const bool second = 2 * p + 1 < nrows;                                 // (false only for the last pair of an odd column)
      if (!second) v[k].y = 0ull;
      bad = bad || image_misfit<SIGNED>(v[k].x) || image_misfit<SIGNED>(v[k].y);
      dst[p] = u32x2{(uint32_t)v[k].x, (uint32_t)v[k].y};
      const uint32_t ox = image_ordered<SIGNED>((uint32_t)v[k].x), oy = second ? image_ordered<SIGNED>((uint32_t)v[k].y) : ox;
      lo = min(lo, min(ox, oy)); hi = max(hi, max(ox, oy));
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { lo = min(lo, (uint32_t)__shfl_xor((int)lo, d, 64)); hi = max(hi, (uint32_t)__shfl_xor((int)hi, d, 64)); }
  const bool any_bad = __ballot(bad) != 0ull;
  if (lane_id() == 0) {
    if (any_bad) atomicOr(flag, 1u);
    if (lo <= hi) { atomicMax(flag + 1, hi); atomicMin(flag + 2, lo); }     // (a wave that met no row has nothing to say)
  }
}

// ---- the 2-byte coarse copy (scan_coarse.hpp): coarse[i] = (image[i] - min) >> shift, and how many rows fall into each of 4096 ranges of coarse values
// A lane reads 32 bytes of the image (8 rows, two 16-byte loads) and writes 16; two such units per lane and step, so four loads are in flight before the first
// is looked at.  Rows at or beyond nrows inside the last unit are written as zero and not counted.  The histogram (bin = coarse >> 4) is counted in LDS, 16 KB
// per workgroup; a wave whose live lanes all hit one bin adds once, with their popcount (an all-equal column would otherwise serialise 64 adds on one LDS
// address), and a workgroup flushes its non-zero bins once with 64-bit atomics.  A workgroup counts at most nrows / gridDim.x + 4096 rows: far inside 32 bits.
//   algorithmic bytes / row: 4 read + 2 written
constexpr int kCoarseUnits = 2;                       // 8-row units per lane and step
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(kImgBlock) void k_scan_coarse_build(const uint32_t* __restrict__ image, uint16_t* __restrict__ coarse, int64_t nrows, uint32_t vmin, int shift,
                                                                 unsigned long long* __restrict__ hist) {
  __shared__ uint32_t h[4096];
  for (int b = threadIdx.x; b < 4096; b += kImgBlock) h[b] = 0u;
  __syncthreads();
  const int64_t nunits = (nrows + 7) / 8;
  const int64_t chunk = (int64_t)kImgBlock * kCoarseUnits;                   // units per workgroup step
  const u32x4* __restrict__ src = (const u32x4*)image;
  u32x4* __restrict__ dst = (u32x4*)coarse;
  const int lane = lane_id();
  for (int64_t base = (int64_t)blockIdx.x * chunk; base < nunits; base += (int64_t)gridDim.x * chunk) {
    u32x4 v[kCoarseUnits][2];
#pragma unroll
    for (int k = 0; k < kCoarseUnits; k++) {
      const int64_t p = base + (int64_t)k * kImgBlock + threadIdx.x;
      if (p < nunits) { v[k][0] = __builtin_nontemporal_load(src + 2 * p); v[k][1] = __builtin_nontemporal_load(src + 2 * p + 1); }   // (the last unit ends < 32 bytes past the image: inside its pad)
      else { v[k][0] = u32x4{0u, 0u, 0u, 0u}; v[k][1] = u32x4{0u, 0u, 0u, 0u}; }
    }
#pragma unroll
    for (int k = 0; k < kCoarseUnits; k++) {
      const int64_t p = base + (int64_t)k * kImgBlock + threadIdx.x;
      const int64_t left = p < nunits ? nrows - 8 * p : 0;                   // rows of this lane's unit that exist (wave-uniform loop below: every lane takes part in the ballots)
      uint32_t x[8];
      __builtin_memcpy(x, &v[k][0], 16); __builtin_memcpy(x + 4, &v[k][1], 16);
      uint32_t cv[8];
#pragma unroll
      for (int e = 0; e < 8; e++) {
        const bool live = e < left;
        cv[e] = live ? ((x[e] - vmin) >> shift) & 0xffffu : 0u;
        const uint32_t bin = cv[e] >> 4;
        const uint64_t lv = __ballot(live);
        if (lv != 0ull) {                                                    // (wave-uniform)
          const uint32_t first = (uint32_t)__builtin_amdgcn_readlane((int)bin, (int)__builtin_ctzll(lv));
          if (__ballot(live && bin != first) == 0ull) { if (lane == (int)__builtin_ctzll(lv)) atomicAdd(&h[first], (uint32_t)__popcll(lv)); }
          else if (live) atomicAdd(&h[bin], 1u);
        }
      }
      if (p < nunits) dst[p] = u32x4{cv[0] | cv[1] << 16, cv[2] | cv[3] << 16, cv[4] | cv[5] << 16, cv[6] | cv[7] << 16};   // (16 bytes: the last unit ends < 16 bytes past the copy, inside its pad)
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < 4096; b += kImgBlock) { const uint32_t n = h[b]; if (n) atomicAdd(hist + b, (unsigned long long)n); }
}

void launch_scan_coarse_build(hipStream_t s, const void* image, void* coarse, int64_t nrows, uint32_t vmin, int shift, uint64_t* hist) {
  if (nrows <= 0) return;
  const int64_t nunits = (nrows + 7) / 8;
  const int64_t chunk = (int64_t)kImgBlock * kCoarseUnits;
  int64_t blocks = (nunits + chunk - 1) / chunk;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(k_scan_coarse_build, dim3((unsigned)blocks), dim3(kImgBlock), 0, s, (const uint32_t*)image, (uint16_t*)coarse, nrows, vmin, shift, (unsigned long long*)hist);
}

void launch_scan_image_build(hipStream_t s, const void* col, bool is_signed, void* image, int64_t nrows, uint32_t* misfit) {
  if (nrows <= 0) return;
  const int64_t npairs = (nrows + 1) / 2;
  const int64_t chunk = (int64_t)kImgBlock * kImgUnroll;
  int64_t blocks = (npairs + chunk - 1) / chunk;
  if (blocks > 2048) blocks = 2048;                                          // 256 CUs x 8 workgroups, grid-stride (like K1)
  if (is_signed) hipLaunchKernelGGL((k_scan_image_build<true>), dim3((unsigned)blocks), dim3(kImgBlock), 0, s, (const uint64_t*)col, (uint32_t*)image, nrows, misfit);
  else hipLaunchKernelGGL((k_scan_image_build<false>), dim3((unsigned)blocks), dim3(kImgBlock), 0, s, (const uint64_t*)col, (uint32_t*)image, nrows, misfit);
}

}  // namespace dfdb
