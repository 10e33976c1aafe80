// join_rule.hpp — the rules of K14 (k_join.hip) that the host states too: how many pairs a left row emits from its match count, the bounded lower-bound
// search over the sorted right keys, and — the join on several keys — one refinement stage and a String key's chunk sub-key.  No HIP header is needed:
// tests/join_rule_main.cpp and tests/join_refine_main.cpp compile this file with the host compiler and the sanitizers over heap arrays of exactly as many
// keys as a search may read, so one read beyond them is caught there.
#pragma once
#include <cstdint>
#include "../../include/dfdb.h"

#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
#define DFDB_JOIN_HD __host__ __device__ __forceinline__
#define DFDB_JOIN_UNROLL _Pragma("unroll")
#else
#define DFDB_JOIN_HD inline
#define DFDB_JOIN_UNROLL
#endif

namespace dfdb {

// the pairs a selected left row with `cnt` right matches emits: inner cnt, left max(cnt, 1), semi min(cnt, 1), anti cnt == 0
DFDB_JOIN_HD uint64_t join_emitted(int kind, uint64_t cnt) {
  switch (kind) {
    case DFDB_JOIN_INNER: return cnt;
    case DFDB_JOIN_LEFT: return cnt ? cnt : 1u;
    case DFDB_JOIN_SEMI: return cnt ? 1u : 0u;
    default: return cnt ? 0u : 1u;                   // DFDB_JOIN_ANTI
  }
}

// The expand writes a round's `tot` outputs (tot <= 2^32 - 1: a 1024-entry group's total fits 32 bits, and a round is part of a group) in steps of 64, lane l
// of step s producing output 64 s + l.  The loop counts STEPS — at most 2^26 — and the output index has 64 bits: a 32-bit output counter stepping by 64 would
// wrap to 0 past 2^32 - 64 and never reach a total above that
DFDB_JOIN_HD uint32_t join_round_steps(uint32_t tot) { return (uint32_t)(((uint64_t)tot + 63u) >> 6); }
DFDB_JOIN_HD uint64_t join_step_output(uint32_t step, int lane) { return ((uint64_t)step << 6) + (uint64_t)lane; }

// the steps of a search over nr keys: the bit length of nr (0 for nr = 0: the search reads nothing and answers 0)
DFDB_JOIN_HD int join_search_steps(uint64_t nr) {
  int s = 0;
  while (nr) { s++; nr >>= 1; }
  return s;
}

// ONE step of the search, split so that a kernel can run several searches in lock step (all their loads of a step issued before any is used):
//   join_step_index  the index step `b` reads from position `pos`, or -1 when that candidate lies beyond nr (nothing is read, the position stays)
//   join_step_take   whether the key read there moves the position up: key < x (the lower bound) or, LE, key <= x (the upper bound)
// pos counts the keys known to precede x; after steps b = steps - 1 .. 0 it is the number of keys < x (LE: <= x).  nr < 2^31: positions fit 32 bits
DFDB_JOIN_HD int64_t join_step_index(uint32_t pos, int b, uint32_t nr) {
  const uint64_t cand = (uint64_t)pos + ((uint64_t)1 << b);
  return cand <= (uint64_t)nr ? (int64_t)cand - 1 : (int64_t)-1;
}
template <bool LE> DFDB_JOIN_HD bool join_step_take(uint64_t key, uint64_t x) { return LE ? key <= x : key < x; }

// the whole search: how many of keys[0 .. nr) (ascending) are < x (LE: <= x).  The count of matches of x is the LE answer minus the other: searching with <=
// — not for x + 1 — keeps the all-ones key (every NaN, typemax(UInt64), typemax(Int64)) an ordinary key
template <bool LE> DFDB_JOIN_HD uint32_t join_bound(const uint64_t* keys, uint32_t nr, int steps, uint64_t x) {
  uint32_t pos = 0;
  for (int b = steps - 1; b >= 0; b--) {
    const int64_t i = join_step_index(pos, b, nr);
    if (i >= 0 && join_step_take<LE>(keys[i], x)) pos = (uint32_t)i + 1u;
  }
  return pos;
}

// ---- the join on several keys (dfdb_query_join_n): one REFINEMENT STAGE per 8-byte sub-key, the major one first ------------------------------------------
// Every left entry carries a run [lo, lo + cnt) of the right side's rows in tuple order, on which every sub-key before this stage's equals the entry's own —
// so this stage's sub-keys rsub[lo .. lo + cnt) are ascending.  With x the entry's sub-key, a = #{rsub < x} and z = #{rsub <= x} within the run:
//   (lo, cnt, x) -> (lo + a, z - a)
// N entries IN LOCK STEP: a step issues the 2 N loads of all their searches before any is used.  steps: any count >= the bit length of the largest cnt (more
// steps read nothing more: join_step_index refuses a candidate beyond cnt).  An entry with cnt = 0 reads nothing and stays (lo, 0).  No index at or beyond
// lo + cnt is read.  The kernel (k_join_refine, N = 8) and the host test (tests/join_refine_main.cpp, over arrays of exactly cnt keys) run this text
template <int N> DFDB_JOIN_HD void join_refine_stage(const uint64_t* rsub, uint32_t* lo, uint32_t* cnt, const uint64_t* x, int steps) {
  uint32_t a[N], z[N];
  DFDB_JOIN_UNROLL
  for (int j = 0; j < N; j++) { a[j] = 0; z[j] = 0; }
  for (int b = steps - 1; b >= 0; b--) {
    uint64_t ka[N], kz[N];
    DFDB_JOIN_UNROLL
    for (int j = 0; j < N; j++) {                  // the step's 2 N loads
      const int64_t ia = join_step_index(a[j], b, cnt[j]), iz = join_step_index(z[j], b, cnt[j]);
      ka[j] = 0; kz[j] = 0;
      if (ia >= 0) ka[j] = rsub[(uint64_t)lo[j] + (uint64_t)ia];
      if (iz >= 0) kz[j] = rsub[(uint64_t)lo[j] + (uint64_t)iz];
    }
    DFDB_JOIN_UNROLL
    for (int j = 0; j < N; j++) {
      const int64_t ia = join_step_index(a[j], b, cnt[j]), iz = join_step_index(z[j], b, cnt[j]);
      if (ia >= 0 && join_step_take<false>(ka[j], x[j])) a[j] = (uint32_t)ia + 1u;
      if (iz >= 0 && join_step_take<true>(kz[j], x[j])) z[j] = (uint32_t)iz + 1u;
    }
  }
  DFDB_JOIN_UNROLL
  for (int j = 0; j < N; j++) { lo[j] += a[j]; cnt[j] = z[j] - a[j]; }
}

// A String key is the sub-keys (chunk_0, .., chunk_{m-1}, length): chunk_c = the string's bytes [8 c, 8 c + 8) read big-endian, zero beyond its end.
//   join_chunk_reaches  whether a string of `len` bytes has a byte in chunk c (else its sub-key is 0 and nothing is loaded)
//   join_chunk_key      the sub-key from `raw`, the 8 bytes at the chunk's first byte loaded little-endian (the load may look up to 7 bytes past the string:
//                       the arenas are padded), and rem = len - 8 c >= 1, the string's bytes from there on: the bytes behind its end are masked away
// (k_sort.hip's k_sort_strkey states the same rule in its own text)
DFDB_JOIN_HD bool join_chunk_reaches(uint32_t len, uint32_t chunk) { return (uint64_t)len > 8ull * chunk; }
DFDB_JOIN_HD uint64_t join_chunk_key(uint64_t raw, uint32_t rem) {
  uint64_t k = __builtin_bswap64(raw);               // the first byte of the chunk becomes the key's top byte
  if (rem - 1u < 7u) k &= ~0ull << (8u * (8u - rem));
  return k;
}

}  // namespace dfdb
