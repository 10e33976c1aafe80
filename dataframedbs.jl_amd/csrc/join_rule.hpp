// join_rule.hpp — the two rules of K14 (k_join.hip) that the host states too: how many pairs a left row emits from its match count, and the bounded lower-bound
// search over the sorted right keys.  No HIP header is needed: tests/join_rule_main.cpp compiles this file with the host compiler and the sanitizers over heap
// arrays of exactly nr keys, so one read at or beyond nr is caught there.
#pragma once
#include <cstdint>
#include "../../include/dfdb.h"

#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
#define DFDB_JOIN_HD __host__ __device__ __forceinline__
#else
#define DFDB_JOIN_HD inline
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

}  // namespace dfdb
