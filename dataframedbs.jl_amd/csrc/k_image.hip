// k_image.hip — the 4-byte scan image of an 8-byte integer column (scan_image.hpp): one streaming pass, made once per column.
//
// A lane reads 16 bytes (two rows) and writes 8 (their low halves); a wave request is 1024 bytes in, 512 out, and four such loads per lane are in flight
// before the first is looked at.  A row whose value is not its truncation extended back (sign extension for Int64, zero extension for UInt64) makes the
// whole image useless: the wave that meets one raises *misfit with one vector atomic when it is done, and the host drops the image (query.cpp).
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

// col: nrows 8-byte values (+ the column's pad: the second half of the last pair of an odd column is read, never used); image: nrows 4-byte values (+ its pad)
template <bool SIGNED>
__global__ __launch_bounds__(kImgBlock) void k_scan_image_build(const uint64_t* __restrict__ col, uint32_t* __restrict__ image, int64_t nrows, uint32_t* __restrict__ misfit) {
  const int64_t npairs = (nrows + 1) / 2;
  const int64_t chunk = (int64_t)kImgBlock * kImgUnroll;                     // pairs per workgroup step
  const u64x2* __restrict__ src = (const u64x2*)col;
  u32x2* __restrict__ dst = (u32x2*)image;
  bool bad = false;
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
    }
  }
  if (__ballot(bad) != 0ull && lane_id() == 0) atomicOr(misfit, 1u);
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
