// The host rule of the 2-byte coarse scan copy (csrc/scan_coarse.hpp) over its edge grid, as a stand-alone host program (tests/test_scan_coarse_cpu.py builds it
// with -fsanitize=address,undefined and runs it): the plan at the limits of both signednesses, what a coarse comparison decides against the exact comparison for
// every operator over a seeded grid of (min, max, c, x), the refusal of constants outside [min, max], and the dense-bucket guard's arithmetic at its edge.
// Exit status 0 = every case as expected.
#include <cstdio>
#include <initializer_list>
#include "../dataframedbs.jl_amd/csrc/scan_coarse.hpp"

using namespace dfdb;

static int bad = 0;
static long checks = 0;
#define CHECK(cond, ...) do { checks++; if (!(cond)) { if (bad < 20) { std::printf(__VA_ARGS__); std::printf("\n"); } bad++; } } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static bool exact(bool sg, int op, uint32_t x, uint32_t c) {
  const int64_t a = sg ? (int64_t)(int32_t)x : (int64_t)x, b = sg ? (int64_t)(int32_t)c : (int64_t)c;
  switch (op) { case kCoarseEq: return a == b; case kCoarseNe: return a != b; case kCoarseLt: return a < b; case kCoarseLe: return a <= b; case kCoarseGt: return a > b; default: return a >= b; }
}
static const int kOps[6] = {kCoarseEq, kCoarseNe, kCoarseLt, kCoarseLe, kCoarseGt, kCoarseGe};

// the expected shift of a span, by its definition: the fewest low bits to drop so that span fits 16 bits
static int want_shift(uint32_t span) { int s = 0; while ((span >> s) > 0xffffu) s++; return s; }

static void check_plan(bool sg, uint32_t mn, uint32_t mx) {
  const CoarsePlan p = scan_coarse_plan(mn, mx);
  const uint32_t span = mx - mn;
  CHECK(p.min == mn && p.shift == want_shift(span), "plan(%08x, %08x): min %08x shift %d, expected shift %d", mn, mx, p.min, p.shift, want_shift(span));
  CHECK(scan_coarse_value(p, mn) == 0, "plan(%08x, %08x): coarse(min) != 0", mn, mx);
  CHECK((uint32_t)scan_coarse_value(p, mx) == (span >> p.shift) && (span >> p.shift) <= 0xffffu, "plan(%08x, %08x): coarse(max) %u", mn, mx, (unsigned)scan_coarse_value(p, mx));
  if (p.shift > 0) CHECK((span >> p.shift) >= 0x8000u, "plan(%08x, %08x): shift %d drops more bits than needed", mn, mx, p.shift);
  uint16_t cc = 0xdead;
  CHECK(scan_coarse_const(sg, mn, mx, mn, &cc) && cc == 0, "plan(%08x, %08x): the minimum refused as a constant", mn, mx);
  CHECK(scan_coarse_const(sg, mn, mx, mx, &cc) && cc == scan_coarse_value(p, mx), "plan(%08x, %08x): the maximum refused as a constant", mn, mx);
  const uint32_t type_min = sg ? 0x80000000u : 0u, type_max = sg ? 0x7fffffffu : 0xffffffffu;
  if (mn != type_min) CHECK(!scan_coarse_const(sg, mn, mx, mn - 1u, &cc), "plan(%08x, %08x): min - 1 accepted", mn, mx);
  if (mx != type_max) CHECK(!scan_coarse_const(sg, mn, mx, mx + 1u, &cc), "plan(%08x, %08x): max + 1 accepted", mn, mx);
}

// every operator for one (min, max, c, x) with x inside [min, max]
static void check_rows(bool sg, uint32_t mn, uint32_t mx, uint32_t c, uint32_t x) {
  const CoarsePlan p = scan_coarse_plan(mn, mx);
  uint16_t cc = 0;
  const bool inside = exact(sg, kCoarseLe, mn, c) && exact(sg, kCoarseLe, c, mx);
  const bool took = scan_coarse_const(sg, mn, mx, c, &cc);
  CHECK(took == inside, "const(%d, %08x, %08x, %08x): taken %d, inside %d", (int)sg, mn, mx, c, (int)took, (int)inside);
  if (!took) return;
  const uint16_t cx = scan_coarse_value(p, x);
  for (int op : kOps) {
    const int d = scan_coarse_decide(op, p.shift, cx, cc);
    const bool want = exact(sg, op, x, c);
    if (p.shift == 0) CHECK(d == (int)want, "decide(op %d, shift 0, x %08x, c %08x in [%08x, %08x]): %d, exact %d", op, x, c, mn, mx, d, (int)want);
    else if (cx == cc) CHECK(d == 2, "decide(op %d, x %08x, c %08x): equal coarse values decided as %d", op, x, c, d);
    else CHECK(d == (int)want, "decide(op %d, shift %d, x %08x, c %08x in [%08x, %08x]): %d, exact %d", op, p.shift, x, c, mn, mx, d, (int)want);
  }
}

int main() {
  // ---- the plan at its limits, both signednesses (signed values as their 32-bit two's-complement bits)
  check_plan(true, 5u, 5u); check_plan(false, 5u, 5u);                                  // min == max
  check_plan(true, (uint32_t)-7, (uint32_t)-7);
  check_plan(true, (uint32_t)-30000, (uint32_t)(-30000 + 65535)); check_plan(false, 1000u, 1000u + 65535u);   // a span of 65535: the last with shift 0
  check_plan(true, (uint32_t)-30000, (uint32_t)(-30000 + 65536)); check_plan(false, 1000u, 1000u + 65536u);   // a span of 65536: the first with shift 1
  check_plan(true, 0x80000000u, 0x7fffffffu);                                           // I32_MIN .. I32_MAX
  check_plan(false, 0u, 0xffffffffu);                                                   // 0 .. U32_MAX
  {
    const CoarsePlan a = scan_coarse_plan(0x80000000u, 0x7fffffffu), b = scan_coarse_plan(0u, 0xffffffffu), z = scan_coarse_plan(9u, 9u);
    const CoarsePlan e = scan_coarse_plan(1000u, 1000u + 65535u), f = scan_coarse_plan(1000u, 1000u + 65536u);
    CHECK(a.shift == 16 && b.shift == 16 && z.shift == 0 && e.shift == 0 && f.shift == 1, "limit shifts %d %d %d %d %d", a.shift, b.shift, z.shift, e.shift, f.shift);
    CHECK(scan_coarse_value(a, 0x7fffffffu) == 0xffffu && scan_coarse_value(a, 0xffffffffu) == 0x7fffu && scan_coarse_value(a, 0u) == 0x8000u, "signed full range coarse values");
  }
  for (int k = 0; k <= 32; k++) {                                                       // spans of 2^k - 1 and 2^k for every k
    const uint32_t lo = k == 32 ? 0xffffffffu : (uint32_t)((1ull << k) - 1ull);
    for (uint32_t span : {lo, k < 32 ? (uint32_t)(1ull << k) : lo}) {
      check_plan(false, 0u, span);
      check_plan(false, 0xffffffffu - span, 0xffffffffu);
      if (span <= 0x7fffffffu) { check_plan(true, (uint32_t)-17, (uint32_t)-17 + span); check_plan(true, 0x7fffffffu - span, 0x7fffffffu); }
      check_plan(true, 0x80000000u, 0x80000000u + span);                                // (from I32_MIN upwards every span fits the signed type)
      const CoarsePlan p = scan_coarse_plan(0u, span);
      const int bits = span == lo ? k : k + 1;                                          // 2^k - 1 has k significant bits, 2^k has k + 1
      CHECK(p.shift == (bits > 16 ? bits - 16 : 0), "span %08x (k %d): shift %d", span, k, p.shift);
    }
  }
  // ---- decided rows against the exact comparison: a seeded grid of (min, max, c, x), all six operators
  const uint32_t spans[] = {0u, 1u, 15u, 16u, 17u, 65535u, 65536u, 65537u, 999999u, 1u << 20, (1u << 24) + 3u, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu};
  for (int sg = 0; sg < 2; sg++) {
    for (uint32_t span : spans) {
      for (int rep = 0; rep < 6; rep++) {
        // a minimum such that [min, min + span] does not wrap in the type's order
        const uint32_t type_min = sg ? 0x80000000u : 0u;
        const uint32_t room = 0xffffffffu - span;                                        // how far min may sit above the type's minimum
        const uint32_t off = rep == 0 ? 0u : rep == 1 ? room : (uint32_t)(rnd() % ((uint64_t)room + 1ull));
        const uint32_t mn = type_min + off, mx = mn + span;
        const CoarsePlan p = scan_coarse_plan(mn, mx);
        const uint32_t step = 1u << p.shift;
        for (int ci = 0; ci < 24; ci++) {
          uint32_t c;
          switch (ci) {
            case 0: c = mn; break; case 1: c = mx; break; case 2: c = mn - 1u; break; case 3: c = mx + 1u; break;
            case 4: c = mn + (uint32_t)(rnd() % ((uint64_t)span + 1ull)) / step * step; break;                       // the first value of a bucket
            case 5: c = mn + (uint32_t)(rnd() % ((uint64_t)span + 1ull)) / step * step + (step - 1u); if (c - mn > span) c = mx; break;   // the last of a bucket
            case 6: c = type_min; break; case 7: c = type_min - 1u; break;                                              // the type's limits
            default: c = ci < 20 ? mn + (uint32_t)(rnd() % ((uint64_t)span + 1ull)) : (uint32_t)rnd(); break;
          }
          const uint32_t cin = c - mn <= span ? c - mn : 0u;                              // an offset near the constant's (0 where the constant is outside)
          const uint32_t xs[] = {0u, span, cin, cin - 1u, cin + 1u, cin / step * step, cin / step * step + step - 1u, cin / step * step - 1u, cin / step * step + step,
                                 (uint32_t)(rnd() % ((uint64_t)span + 1ull)), (uint32_t)(rnd() % ((uint64_t)span + 1ull)), (uint32_t)(rnd() % ((uint64_t)span + 1ull))};
          for (uint32_t xo : xs) if (xo <= span) check_rows(sg != 0, mn, mx, c, mn + xo);
        }
      }
    }
  }
  // ---- the guard: hist * 128 <= nrows, at equality and one row to either side
  for (uint64_t h : {0ull, 1ull, 2ull, 7813ull, 1ull << 20, 7812500ull, (1ull << 56) - 1ull}) {
    const int64_t at = (int64_t)(h * 128ull);
    CHECK(scan_coarse_guard(h, at), "guard(%llu, %lld) refused at equality", (unsigned long long)h, (long long)at);
    CHECK(scan_coarse_guard(h, at + 1), "guard(%llu, %lld) refused above equality", (unsigned long long)h, (long long)at + 1);
    if (h > 0) CHECK(!scan_coarse_guard(h, at - 1), "guard(%llu, %lld) passed below equality", (unsigned long long)h, (long long)at - 1);
  }
  CHECK(scan_coarse_guard(256ull * 1000ull, 1000000000ll), "the benchmark's bucket refused");       // 256 of 1e6 values over 1e9 rows: 1/3906 of the rows
  CHECK(!scan_coarse_guard(UINT64_MAX, INT64_MAX) && !scan_coarse_guard(1ull, 0), "guard at the integer limits");
  CHECK(kCoarseHistBins == 4096 && kCoarseGuard == 128, "constants");
  std::printf("%ld checks, %d wrong\n", checks, bad);
  return bad ? 1 : 0;
}
