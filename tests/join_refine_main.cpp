// The refinement stage of the join on several keys and the String chunk rule (csrc/join_rule.hpp), as a stand-alone host program (tests/test_join_refine_cpu.py
// builds it with -fsanitize=address,undefined and runs it).  The kernel k_join_refine runs the same text (join_refine_stage<8>).
//  A  one stage over HEAP arrays of exactly cnt keys (the run copied out, lo = 0) — one read beyond a run is a heap-buffer-overflow — for cnt = 0, 1, 2, 3, 63,
//     64, 65, 1023, 1024, 1025, every step count from bitlength(cnt) up to 32, on distinct keys, runs of equal keys, all-equal runs and runs of the all-ones key,
//     against std::lower_bound / std::upper_bound
//  B  eight entries in lock step over eight runs packed into one heap array that ends with the last run
//  C  the stages composed over random two- and three-component right sides sorted by std::sort on tuples: (lo, cnt) against std::equal_range on the tuples
//  D  join_chunk_reaches / join_chunk_key against a byte-by-byte restatement for lengths 0 to 17 and chunks 0 to 2
// Exit status 0 = every case as expected.
#include <algorithm>
#include <array>
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

static uint64_t rng_state = 0x2545f4914f6cdd1dull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static const uint32_t kCounts[] = {0u, 1u, 2u, 3u, 63u, 64u, 65u, 1023u, 1024u, 1025u};

// shape 0: distinct keys; 1: runs of 1..5 equal keys; 2: every key equal; 3: every key all ones; 4: runs ending in a run of the all-ones key
static void fill(uint64_t* keys, uint32_t n, int shape) {
  uint64_t v = 10;
  uint32_t i = 0;
  while (i < n) {
    uint32_t run = shape == 0 ? 1 : 1 + (uint32_t)(rnd() % 5);
    if (shape == 2 || shape == 3) run = n;
    for (uint32_t k = 0; k < run && i < n; k++) keys[i++] = shape == 3 ? ~0ull : v;
    v += 2 + (rnd() % 7) * 2;                                    // even keys: every odd value is a gap
  }
  if (shape == 4) for (uint32_t k = 0; k < 3 && k < n; k++) keys[n - 1 - k] = ~0ull;
}

static void one_stage(const uint64_t* keys, uint32_t cnt, int steps, uint64_t x, int shape) {
  uint32_t lo = 0, c = cnt;
  join_refine_stage<1>(keys, &lo, &c, &x, steps);
  const uint32_t wlo = (uint32_t)(std::lower_bound(keys, keys + cnt, x) - keys), whi = (uint32_t)(std::upper_bound(keys, keys + cnt, x) - keys);
  CHECK(c == whi - wlo && (c == 0 || lo == wlo), "shape %d cnt=%u steps=%d x=%llx: (%u, %u), want (%u, %u)", shape, cnt, steps, (unsigned long long)x, lo, c, wlo, whi - wlo);
}

static void part_a() {
  for (uint32_t cnt : kCounts)
    for (int shape = 0; shape < 5; shape++) {
      uint64_t* keys = (uint64_t*)std::malloc(cnt ? (size_t)cnt * sizeof(uint64_t) : 1);          // exactly cnt keys (cnt = 0: one byte, no key fits)
      fill(keys, cnt, shape);
      for (int steps = join_search_steps(cnt); steps <= 32; steps++) {
        const uint32_t stride = steps == join_search_steps(cnt) || cnt < 100 ? 1u : 37u;           // every key at the tight step count, a sample beyond it
        for (uint32_t i = 0; i < cnt; i += stride) {
          one_stage(keys, cnt, steps, keys[i], shape);
          if (keys[i] != 0) one_stage(keys, cnt, steps, keys[i] - 1, shape);
          if (keys[i] != ~0ull) one_stage(keys, cnt, steps, keys[i] + 1, shape);
        }
        if (cnt) { one_stage(keys, cnt, steps, keys[cnt - 1], shape); one_stage(keys, cnt, steps, keys[0], shape); }
        one_stage(keys, cnt, steps, 0, shape);
        one_stage(keys, cnt, steps, ~0ull, shape);                                                // the all-ones key
        one_stage(keys, cnt, steps, ~0ull - 1, shape);
        one_stage(keys, cnt, steps, 1ull << 63, shape);
      }
      std::free(keys);
    }
}

static void part_b() {
  constexpr int N = 8;
  for (int round = 0; round < 400; round++) {
    uint32_t cnt[N], lo[N], total = 0, cmax = 0;
    for (int j = 0; j < N; j++) { cnt[j] = kCounts[rnd() % 10]; lo[j] = total; total += cnt[j]; cmax = std::max(cmax, cnt[j]); }
    uint64_t* keys = (uint64_t*)std::malloc(total ? (size_t)total * sizeof(uint64_t) : 1);        // the last run ends where the array ends
    uint64_t x[N];
    for (int j = 0; j < N; j++) {
      fill(keys + lo[j], cnt[j], (int)(rnd() % 5));
      const uint64_t pick = cnt[j] ? keys[lo[j] + rnd() % cnt[j]] : 7;
      x[j] = (rnd() % 4 == 0) ? pick + 1 : (rnd() % 8 == 0 ? ~0ull : pick);
    }
    uint32_t l[N], c[N];
    for (int j = 0; j < N; j++) { l[j] = lo[j]; c[j] = cnt[j]; }
    join_refine_stage<N>(keys, l, c, x, join_search_steps(cmax) + (int)(rnd() % 3));              // the wave's step count: the largest run's, or more
    for (int j = 0; j < N; j++) {
      const uint64_t* b = keys + lo[j];
      const uint32_t wlo = lo[j] + (uint32_t)(std::lower_bound(b, b + cnt[j], x[j]) - b), whi = lo[j] + (uint32_t)(std::upper_bound(b, b + cnt[j], x[j]) - b);
      CHECK(c[j] == whi - wlo && (c[j] == 0 || l[j] == wlo), "lock step round %d entry %d: (%u, %u), want (%u, %u)", round, j, l[j], c[j], wlo, whi - wlo);
    }
    std::free(keys);
  }
}

template <size_t K> static void compose(uint32_t nr, uint32_t nl, uint64_t span) {
  typedef std::array<uint64_t, K> Tup;
  std::vector<Tup> right(nr);
  for (Tup& t : right) for (size_t k = 0; k < K; k++) t[k] = (rnd() % 16 == 0) ? ~0ull : rnd() % span;
  std::sort(right.begin(), right.end());
  std::vector<uint64_t*> rsub(K);
  for (size_t k = 0; k < K; k++) {
    rsub[k] = (uint64_t*)std::malloc(nr ? (size_t)nr * sizeof(uint64_t) : 1);                     // exactly nr sub-keys per stage
    for (uint32_t i = 0; i < nr; i++) rsub[k][i] = right[i][k];
  }
  for (uint32_t q = 0; q < nl; q++) {
    Tup x;
    if (nr && rnd() % 2) { x = right[rnd() % nr]; if (rnd() % 3 == 0) x[rnd() % K] = rnd() % span; }
    else for (size_t k = 0; k < K; k++) x[k] = rnd() % span;
    uint32_t lo = 0, cnt = nr;
    for (size_t k = 0; k < K; k++) join_refine_stage<1>(rsub[k], &lo, &cnt, &x[k], join_search_steps(cnt) + (int)(rnd() % 2));
    const auto er = std::equal_range(right.begin(), right.end(), x);
    const uint32_t wlo = (uint32_t)(er.first - right.begin()), wcnt = (uint32_t)(er.second - er.first);
    CHECK(cnt == wcnt && (cnt == 0 || lo == wlo), "compose K=%zu nr=%u: (%u, %u), want (%u, %u)", K, nr, lo, cnt, wlo, wcnt);
  }
  for (uint64_t* p : rsub) std::free(p);
}

static void part_d() {
  for (uint32_t len = 0; len <= 17; len++)
    for (int fillv = 0; fillv < 4; fillv++) {
      uint8_t buf[17 + 24];
      for (uint32_t i = 0; i < sizeof buf; i++) buf[i] = i < len ? (fillv == 0 ? 0x00 : fillv == 1 ? 0xff : (uint8_t)rnd()) : (uint8_t)(0xa5 + i);      // behind the string: not its own
      for (uint32_t chunk = 0; chunk <= 2; chunk++) {
        uint64_t want = 0;
        for (uint32_t k = 0; k < 8; k++) want |= (uint64_t)(8 * chunk + k < len ? buf[8 * chunk + k] : 0) << (8 * (7 - k));
        const bool reaches = join_chunk_reaches(len, chunk);
        CHECK(reaches == (len > 8 * chunk), "reaches(%u, %u)", len, chunk);
        uint64_t got = 0;
        if (reaches) { uint64_t raw; std::memcpy(&raw, buf + 8 * chunk, 8); got = join_chunk_key(raw, len - 8 * chunk); }
        CHECK(got == want, "chunk %u of %u bytes: %llx, want %llx", chunk, len, (unsigned long long)got, (unsigned long long)want);
      }
    }
}

int main() {
  part_a();
  part_b();
  for (uint32_t nr : {0u, 1u, 2u, 65u, 1025u, 5000u}) {
    compose<2>(nr, 600, 5); compose<2>(nr, 600, 40); compose<2>(nr, 300, 1ull << 40);
    compose<3>(nr, 600, 4); compose<3>(nr, 600, 12);
  }
  part_d();
  std::printf("join_refine: %ld checked, %d wrong\n", checks, bad);
  return bad ? 1 : 0;
}
