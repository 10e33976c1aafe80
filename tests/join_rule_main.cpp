// The two host-statable rules of the device join (csrc/join_rule.hpp) over their edge grid, as a stand-alone host program (tests/test_join_rule_cpu.py builds
// it with -fsanitize=address,undefined and runs it).  The bounded search runs over HEAP arrays of exactly nr keys — one read at or beyond nr is a
// heap-buffer-overflow — for nr = 0, 1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, on arrays with runs of equal keys (and on distinct keys), probing
// every key present, every gap, below the minimum, above the maximum and the all-ones key, against std::lower_bound / std::upper_bound.  Then join_emitted for
// every kind at cnt = 0, 1, 2 and 2^31 - 1, and join_search_steps at the powers of two.  Exit status 0 = every case as expected.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>
#include "../dataframedbs.jl_amd/csrc/join_rule.hpp"

using namespace dfdb;

static int bad = 0;
static long checks = 0;
#define CHECK(cond, ...) do { checks++; if (!(cond)) { if (bad < 20) { std::printf(__VA_ARGS__); std::printf("\n"); } bad++; } } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static void probe(const uint64_t* keys, uint32_t nr, uint64_t x, const char* shape) {
  const int steps = join_search_steps(nr);
  const uint32_t lo = join_bound<false>(keys, nr, steps, x), hi = join_bound<true>(keys, nr, steps, x);
  const uint32_t wlo = (uint32_t)(std::lower_bound(keys, keys + nr, x) - keys), whi = (uint32_t)(std::upper_bound(keys, keys + nr, x) - keys);
  CHECK(lo == wlo && hi == whi, "%s nr=%u x=%llx: lower %u (want %u), upper %u (want %u)", shape, nr, (unsigned long long)x, lo, wlo, hi, whi);
}

// shape 0: distinct keys 10, 20, ..; 1: runs of 1..5 equal keys; 2: the same ending in a run of the all-ones key; 3: every key equal; 4: every key all ones;
// 5: starting in a run of key 0
static void fill(uint64_t* keys, uint32_t nr, int shape) {
  uint64_t v = shape == 5 ? 0 : 10;
  uint32_t i = 0;
  while (i < nr) {
    uint32_t run = shape == 0 ? 1 : 1 + (uint32_t)(rnd() % 5);
    if (shape == 3 || shape == 4) run = nr;
    for (uint32_t k = 0; k < run && i < nr; k++) keys[i++] = shape == 4 ? ~0ull : v;
    v += shape == 0 ? 10 : 2 + (rnd() % 7) * 2;                 // even keys: every odd value is a gap
  }
  if (shape == 2) for (uint32_t k = 0; k < 3 && k < nr; k++) keys[nr - 1 - k] = ~0ull;
}

int main() {
  static const char* const names[] = {"distinct", "runs", "runs+ones", "equal", "ones", "zero-run"};
  for (uint32_t nr : {0u, 1u, 2u, 3u, 63u, 64u, 65u, 1023u, 1024u, 1025u, 4095u, 4096u, 4097u}) {
    CHECK(join_search_steps(nr) == (nr ? 64 - __builtin_clzll((unsigned long long)nr) : 0), "steps(%u) = %d", nr, join_search_steps(nr));
    for (int shape = 0; shape < 6; shape++) {
      uint64_t* keys = (uint64_t*)std::malloc(nr ? (size_t)nr * sizeof(uint64_t) : 1);           // exactly nr keys (nr = 0: one byte, no key fits)
      fill(keys, nr, shape);
      CHECK(std::is_sorted(keys, keys + nr), "%s nr=%u is not ascending", names[shape], nr);
      for (uint32_t i = 0; i < nr; i++) {
        probe(keys, nr, keys[i], names[shape]);                                                 // every key present
        if (keys[i] != 0) probe(keys, nr, keys[i] - 1, names[shape]);                           // every gap below a key
        if (keys[i] != ~0ull) probe(keys, nr, keys[i] + 1, names[shape]);                       // and above it
      }
      probe(keys, nr, 0, names[shape]);                                                         // below the minimum
      probe(keys, nr, nr ? keys[0] - (keys[0] ? 1 : 0) : 5, names[shape]);
      probe(keys, nr, nr && keys[nr - 1] != ~0ull ? keys[nr - 1] + 1 : ~0ull - 1, names[shape]);  // above the maximum
      probe(keys, nr, ~0ull, names[shape]);                                                     // the all-ones key: every NaN, typemax(UInt64), typemax(Int64)
      probe(keys, nr, ~0ull - 1, names[shape]);
      probe(keys, nr, 1ull << 63, names[shape]);
      for (int k = 0; k < 64; k++) probe(keys, nr, rnd() >> (rnd() % 64), names[shape]);
      std::free(keys);
    }
  }
  for (int s = 0; s < 64; s++) {
    CHECK(join_search_steps(1ull << s) == s + 1, "steps(2^%d)", s);
    if (s) CHECK(join_search_steps((1ull << s) - 1) == s, "steps(2^%d - 1)", s);
  }
  // a step whose candidate lies beyond nr reads nothing
  CHECK(join_step_index(0, 0, 0) == -1 && join_step_index(0, 2, 3) == -1 && join_step_index(0, 1, 3) == 1 && join_step_index(2, 0, 3) == 2 && join_step_index(3, 0, 3) == -1,
        "join_step_index at the end of the list");
  CHECK(join_step_index(0x7fffffffu, 30, 0x7fffffffu) == -1 && join_step_index(0x40000000u, 29, 0x7fffffffu) == 0x5fffffff, "join_step_index near 2^31");
  // the expand's steps of 64 outputs over a round's total, up to the largest total call 1 admits (2^32 - 1): the steps cover every output exactly once, the
  // last step is the only one that reaches the total, and no output index wraps — lane 63 of the last step may lie beyond 2^32 - 1
  for (uint64_t tot : {0ull, 1ull, 63ull, 64ull, 65ull, 127ull, 128ull, 4096ull, (1ull << 31) - 1, 1ull << 31, (1ull << 32) - 129, (1ull << 32) - 128, (1ull << 32) - 65,
                       (1ull << 32) - 64, (1ull << 32) - 63, (1ull << 32) - 2, (1ull << 32) - 1}) {
    const uint32_t steps = join_round_steps((uint32_t)tot);
    CHECK((uint64_t)steps * 64 >= tot && (steps == 0 || (uint64_t)(steps - 1) * 64 < tot), "join_round_steps(%llu) = %u", (unsigned long long)tot, steps);
    CHECK(steps <= (1u << 26), "join_round_steps(%llu) = %u steps", (unsigned long long)tot, steps);
    uint64_t covered = 0, prev_last = 0;
    for (uint32_t s : {0u, 1u, steps > 1 ? steps - 2 : 0u, steps > 0 ? steps - 1 : 0u}) {
      if (s >= steps) continue;
      const uint64_t first = join_step_output(s, 0), last = join_step_output(s, 63);
      CHECK(first == (uint64_t)s * 64 && last == first + 63 && first < tot, "step %u of %llu: outputs %llu .. %llu", s, (unsigned long long)tot, (unsigned long long)first, (unsigned long long)last);
      CHECK(s == 0 || first > prev_last || first == prev_last - 63, "step %u of %llu does not advance", s, (unsigned long long)tot);
      prev_last = last;
      if (s == steps - 1) covered = first + (tot - first);       // the last step's lanes below tot - first write: everything up to tot is written
    }
    CHECK(steps == 0 ? tot == 0 : covered == tot, "the steps of %llu cover %llu outputs", (unsigned long long)tot, (unsigned long long)covered);
  }
  const uint64_t big = (1ull << 31) - 1;
  for (uint64_t cnt : {(uint64_t)0, (uint64_t)1, (uint64_t)2, big}) {
    CHECK(join_emitted(DFDB_JOIN_INNER, cnt) == cnt, "inner %llu", (unsigned long long)cnt);
    CHECK(join_emitted(DFDB_JOIN_LEFT, cnt) == (cnt > 1 ? cnt : 1), "left %llu", (unsigned long long)cnt);
    CHECK(join_emitted(DFDB_JOIN_SEMI, cnt) == (cnt < 1 ? cnt : 1), "semi %llu", (unsigned long long)cnt);
    CHECK(join_emitted(DFDB_JOIN_ANTI, cnt) == (cnt == 0 ? 1u : 0u), "anti %llu", (unsigned long long)cnt);
  }
  std::printf("join_rule: %ld checks, %d wrong\n", checks, bad);
  return bad ? 1 : 0;
}
