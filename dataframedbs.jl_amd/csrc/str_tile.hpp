// str_tile.hpp — the walk of a String column one wave per 1024-row tile, and the moves of single strings, as k_parse.hip, k_strings.hip and k_dict.hip share
// them.  Device only.
//
// A tile is sixteen steps of 64 rows: row j * 64 + lane of the tile belongs to lane `lane` in step j, step j makes word j of the tile's bitmap, and lanes
// 0..15 hold the tile's sixteen words.  The layout of a String column (sizes, one arena, one byte offset per tile) is at the head of k_strings.hip.
#pragma once
#include "common.hpp"
#include "device_utils.hpp"

namespace dfdb {

static_assert(kTileRows == 16 * 64 && kTileWords == 16, "a tile is sixteen 64-row steps of one wave, one bitmap word per step");

__device__ __forceinline__ uint32_t clamp_size(int32_t s) { return s > 0 ? (uint32_t)s : 0u; }   // the bytes of a row (a missing row, -1, has none)

__device__ __forceinline__ uint64_t load_u64_unaligned(const uint8_t* p) {
  typedef uint64_t __attribute__((aligned(1), may_alias)) u64u;
  return *(const u64u*)p;
}
// exact copy of one string (len bytes): unaligned 8-byte moves, then ONE 8-byte load (the arenas are padded) and <= 3 stores
__device__ __forceinline__ void copy_string(uint8_t* dp, const uint8_t* sp, uint32_t len) {
  typedef uint64_t __attribute__((aligned(1), may_alias)) u64u;
  typedef uint32_t __attribute__((aligned(1), may_alias)) u32u;
  typedef uint16_t __attribute__((aligned(1), may_alias)) u16u;
  uint32_t b = 0;
  for (; b + 8 <= len; b += 8) *(u64u*)(dp + b) = *(const u64u*)(sp + b);
  const uint32_t rem = len - b;
  if (rem) {
    uint64_t v = *(const u64u*)(sp + b);
    uint8_t* d = dp + b;
    if (rem & 4u) { *(u32u*)d = (uint32_t)v; d += 4; v >>= 32; }
    if (rem & 2u) { *(u16u*)d = (uint16_t)v; d += 2; v >>= 16; }
    if (rem & 1u) *d = (uint8_t)v;
  }
}
// the low `len` (<= 8) bytes of v
__device__ __forceinline__ void store_small(uint8_t* d, uint64_t v, uint32_t len) {
  typedef uint64_t __attribute__((aligned(1), may_alias)) u64u;
  typedef uint32_t __attribute__((aligned(1), may_alias)) u32u;
  typedef uint16_t __attribute__((aligned(1), may_alias)) u16u;
  if (len >= 8u) { *(u64u*)d = v; return; }
  if (len & 4u) { *(u32u*)d = (uint32_t)v; d += 4; v >>= 32; }
  if (len & 2u) { *(u16u*)d = (uint16_t)v; d += 2; v >>= 16; }
  if (len & 1u) *d = (uint8_t)v;
}

// the sizes of the tile's rows, sixteen loads in flight; `past` stands for the rows behind the column's last.  NT: the loads are non-temporal
template <bool NT = true>
__device__ __forceinline__ void tile_sizes(const int32_t* sizes, int64_t base, int64_t nrows, int lane, int32_t past, int32_t (&sz)[16]) {
#pragma unroll
  for (int j = 0; j < 16; j++) { const int64_t i = base + j * 64 + lane; sz[j] = i < nrows ? (NT ? __builtin_nontemporal_load(sizes + i) : sizes[i]) : past; }
}

// Where the tile's rows start, counted in bytes from the tile's first: pre[j] of a lane = the exclusive prefix of the clamped sizes over the tile's rows in
// front of row j * 64 + lane — sixteen in-register wave scans and a running total.  Returns the tile's bytes.  (k_str_gather_bytes states the same loop in place,
// between its own loads and its LDS stores, and stays as it was measured.)
__device__ __forceinline__ uint32_t tile_prefix(const int32_t (&sz)[16], uint32_t (&pre)[16]) {
  uint32_t run = 0;
#pragma unroll
  for (int j = 0; j < 16; j++) {
    const uint32_t c = clamp_size(sz[j]);
    const uint32_t incl = wave_incl_scan(c);
    pre[j] = run + incl - c;
    run += __shfl(incl, 63, 64);
  }
  return run;
}

// The tile's byte range in the arena, from the 16-byte boundary below its first byte: o0 = tile_off[tile], a0 the boundary, lead = o0 - a0 (0..15), and
// span = the bytes from a0 that the staging moves: up to 31 bytes past the tile's end (a reader may look 15 bytes behind its string, and every arena is
// allocated with 64 bytes of slack).  Wave-uniform.
struct TileSpan { int64_t o0, a0, span; uint32_t lead; };
__device__ __forceinline__ TileSpan tile_span(const int64_t* tile_off, int64_t tile) {
  const int64_t o0 = tile_off[tile], a0 = o0 & ~15ll;
  return TileSpan{o0, a0, tile_off[tile + 1] - a0 + 16, (uint32_t)(o0 - a0)};
}

// Park ts.span bytes from bytes + ts.a0 in this wave's LDS stage (16-byte aligned, CAP bytes and room for what the caller reads past a row), as aligned
// 16-byte loads, PIECES per lane in flight per round.  The caller has seen to ts.span <= CAP; where CAP is one round's bytes there is no loop.
template <int PIECES, uint32_t CAP>
__device__ __forceinline__ void stage_tile(const uint8_t* bytes, const TileSpan& ts, uint8_t* stage, int lane) {
  static_assert(CAP % 16 == 0, "the last piece of a range of CAP bytes ends inside the stage only if CAP is a whole number of pieces");
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  constexpr uint32_t kRound = (uint32_t)PIECES * 1024u;
  const uint32_t need = (uint32_t)ts.span, lastc = (need - 1u) & ~15u;
  // (a piece past the range's end is the range's last piece once more, loaded and stored by several lanes alike: no predication, no divergence)
  uint32_t c0 = 0;
  do {
    u32x4 piece[PIECES];
#pragma unroll
    for (int i = 0; i < PIECES; i++) { uint32_t c = c0 + (uint32_t)i * 1024u + (uint32_t)lane * 16u; c = c < lastc ? c : lastc; piece[i] = __builtin_nontemporal_load((const u32x4*)(bytes + ts.a0 + c)); }
#pragma unroll
    for (int i = 0; i < PIECES; i++) { uint32_t c = c0 + (uint32_t)i * 1024u + (uint32_t)lane * 16u; c = c < lastc ? c : lastc; *(u32x4*)(stage + c) = piece[i]; }
    c0 += kRound;
  } while (CAP > kRound && c0 < need);
  wave_lds_fence();
}

// word j (wave-uniform) of a tile's bitmap, from the halves that lanes 0..15 hold of their words
__device__ __forceinline__ uint64_t tile_word(uint32_t lo, uint32_t hi, int j) {
  return (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)hi, j) << 32 | (uint32_t)__builtin_amdgcn_readlane((int)lo, j);
}

// the end of a tile that made a bitmap: its words (lane j < 16 holds word j) and its selected-row count go out.  WRITE_THROUGH: the words leave in relaxed
// system-scope atomic stores (see k_scan_cmp), else in plain stores
template <bool WRITE_THROUGH>
__device__ __forceinline__ void tile_close(uint64_t* bitmap, uint32_t* tile_counts, int64_t tile, int lane, uint64_t myword) {
  uint32_t cnt = lane < 16 ? (uint32_t)__popcll(myword) : 0u;
#pragma unroll
  for (int d = 8; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
  if (lane < 16) {
    if (WRITE_THROUGH) __hip_atomic_store(&bitmap[tile * 16 + lane], myword, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    else bitmap[tile * 16 + lane] = myword;
  }
  if (lane == 0) tile_counts[tile] = cnt;
}

}  // namespace dfdb
