// Which form a lone `col OP const` scan takes (csrc/scan_route.hpp) over its edge grid, as a stand-alone host program (tests/test_scan_coarse_cpu.py builds it with
// -fsanitize=address,undefined and runs it).  The expected route is stated here from DESIGN.md §3 in plain 64-bit arithmetic on the VALUES — the column's smallest
// and largest value, the constant, the rows in the constant's histogram bin — without calling scan_image.hpp or scan_coarse.hpp; scan_route and scan_route_notes
// must agree with it for both signednesses, every span of tests/scan_coarse_main.cpp's list, constants at and beside min and max, past the 32-bit type's limits,
// at the first and last value of a bucket, scan_coarse = 0 / 1 / 2, with and without a coarse copy, for every state of the image, and with the constant's bin
// at exactly nrows / 128 rows and one more.  Then the build trigger over every state, option value, scan count and row count at the threshold.
// Exit status 0 = every case as expected.
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <vector>
#include "../dataframedbs.jl_amd/csrc/scan_route.hpp"

using namespace dfdb;

static int bad = 0;
static long checks = 0;
#define CHECK(cond, ...) do { checks++; if (!(cond)) { if (bad < 20) { std::printf(__VA_ARGS__); std::printf("\n"); } bad++; } } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

struct Want { int form; bool dense; int32_t image_dtype; uint64_t image_cbits; unsigned cc; const char* notes[2]; int nnotes; };

// DESIGN.md §3.  mn, mx: the column's smallest and largest value; cbits: the constant's 64 bits in the column's type; in_bin: the rows whose coarse value >> 4
// is the constant's (asked for only where the rule consults it)
static Want want_route(bool sg, bool built, bool coarse, int64_t mn, int64_t mx, uint64_t cbits, int64_t nrows, int64_t coarse_opt, uint64_t in_bin) {
  Want w{kScanFlat, false, 0, 0, 0, {nullptr, nullptr}, 0};
  if (!built) return w;
  // a constant the 32-bit type cannot hold takes the flat column
  if (sg) { const int64_t c = (int64_t)cbits; if (c < -2147483648ll || c > 2147483647ll) return w; }
  else if (cbits > 4294967295ull) return w;
  const int64_t c = sg ? (int64_t)cbits : (int64_t)(cbits & 0xffffffffull);
  w.form = kScanImage; w.image_dtype = sg ? DFDB_I32 : DFDB_U32; w.image_cbits = cbits & 0xffffffffull;
  const char* const image_note = sg ? "scan_image.int32" : "scan_image.uint32";
  w.notes[0] = image_note; w.nnotes = 1;
  if (coarse_opt == 0 || !coarse || c < mn || c > mx) return w;
  int shift = 0;
  while (((mx - mn) >> shift) > 65535) shift++;
  w.cc = (unsigned)((c - mn) >> shift);
  if (shift == 0) { w.form = kScanCoarseExact; w.notes[0] = "scan_image.coarse_exact"; return w; }
  if (coarse_opt == 2 || in_bin * 128ull <= (uint64_t)nrows) { w.form = kScanCoarse; w.notes[0] = "scan_image.coarse"; return w; }
  w.dense = true; w.notes[0] = "scan_image.coarse_dense"; w.notes[1] = image_note; w.nnotes = 2;
  return w;
}

static long seen[5] = {0, 0, 0, 0, 0};       // expected routes per form, [4]: the dense ones — the grid must reach every one

static const char* nz(const char* s) { return s ? s : "(none)"; }

static void check_route(bool sg, int state, bool coarse, int64_t mn, int64_t mx, uint64_t cbits, int64_t nrows, int64_t coarse_opt, uint64_t in_bin, const uint64_t* hist) {
  const int32_t dtype = sg ? DFDB_I64 : DFDB_U64;
  int shift = 0;
  while (((mx - mn) >> shift) > 65535) shift++;
  ScanCopyFacts f;
  f.built = state == kImageBuilt; f.coarse = coarse; f.min = (uint32_t)(uint64_t)mn; f.max = (uint32_t)(uint64_t)mx; f.shift = shift; f.hist = hist; f.nrows = nrows;
  const ScanRoute r = scan_route(dtype, cbits, f, coarse_opt);
  const Want w = want_route(sg, state == kImageBuilt, coarse, mn, mx, cbits, nrows, coarse_opt, in_bin);
  seen[w.form]++; seen[4] += w.dense;
  CHECK(r.form == w.form && r.dense == w.dense && r.image_dtype == w.image_dtype && r.image_cbits == w.image_cbits && (unsigned)r.cc == w.cc,
        "route(%s, state %d, coarse %d, [%lld, %lld], c %016llx, nrows %lld, opt %lld, bin %llu): form %d dense %d dtype %d cbits %llx cc %u, expected %d %d %d %llx %u",
        sg ? "i64" : "u64", state, (int)coarse, (long long)mn, (long long)mx, (unsigned long long)cbits, (long long)nrows, (long long)coarse_opt, (unsigned long long)in_bin,
        r.form, (int)r.dense, r.image_dtype, (unsigned long long)r.image_cbits, (unsigned)r.cc, w.form, (int)w.dense, w.image_dtype, (unsigned long long)w.image_cbits, w.cc);
  const ScanNotes n = scan_route_notes(r);
  bool same = n.n == w.nnotes;
  for (int k = 0; same && k < n.n; k++) same = n.note[k] && !std::strcmp(n.note[k], w.notes[k]);
  CHECK(same, "notes(%s, state %d, coarse %d, [%lld, %lld], c %016llx, opt %lld, bin %llu): %d (%s, %s), expected %d (%s, %s)", sg ? "i64" : "u64", state, (int)coarse,
        (long long)mn, (long long)mx, (unsigned long long)cbits, (long long)coarse_opt, (unsigned long long)in_bin, n.n, nz(n.note[0]), nz(n.note[1]), w.nnotes, nz(w.notes[0]), nz(w.notes[1]));
}

int main() {
  const uint32_t spans[] = {0u, 1u, 15u, 16u, 17u, 65535u, 65536u, 65537u, 999999u, 1u << 20, (1u << 24) + 3u, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu};
  const int states[] = {kImageNone, kImageBuilt, kImageMisfit, kImageNoRoom};
  const int64_t rows[] = {1000064, 1000000, 127, 0};        // a multiple of 128, one that is not, fewer than 128 (only an empty bin passes), none
  std::vector<uint64_t> hist((size_t)kCoarseHistBins, 0);
  for (int sg = 0; sg < 2; sg++) {
    const int64_t type_min = sg ? -2147483648ll : 0ll, type_max = sg ? 2147483647ll : 4294967295ll;
    for (uint32_t span : spans) {
      for (int rep = 0; rep < 4; rep++) {
        const int64_t room = 4294967295ll - (int64_t)span;    // how far min may sit above the type's minimum
        const int64_t mn = type_min + (rep == 0 ? 0 : rep == 1 ? room : (int64_t)(rnd() % ((uint64_t)room + 1ull))), mx = mn + (int64_t)span;
        int shift = 0;
        while (((mx - mn) >> shift) > 65535) shift++;
        const int64_t step = 1ll << shift;
        const int64_t b0 = mn + (int64_t)(rnd() % ((uint64_t)span + 1ull)) / step * step;       // the first value of some bucket
        const int64_t consts[] = {mn, mx, mn - 1, mx + 1, b0, b0 + step - 1 <= mx ? b0 + step - 1 : mx, mn + (int64_t)(rnd() % ((uint64_t)span + 1ull)),
                                  type_min, type_max, type_min - 1, type_max + 1, type_min - 65536, type_max + 65536};
        std::vector<uint64_t> cbits;
        for (int64_t c : consts) if (sg || c >= 0) cbits.push_back((uint64_t)c);                 // (a UInt64 constant below zero does not exist)
        if (sg) { cbits.push_back(0x8000000000000000ull); cbits.push_back(0x7fffffffffffffffull); cbits.push_back(0x00000001ffffffffull); cbits.push_back(0xffffffff00000000ull); }
        else { cbits.push_back(0xffffffffffffffffull); cbits.push_back(0x8000000000000000ull); cbits.push_back(0xffffffff80000000ull); cbits.push_back(0x0000000100000000ull + (uint64_t)mn); }
        for (uint64_t cb : cbits) {
          // the constant's histogram bin, where it has one (inside the type and inside [min, max])
          const bool in_type = sg ? ((int64_t)cb >= type_min && (int64_t)cb <= type_max) : cb <= (uint64_t)type_max;
          const int64_t c = (int64_t)cb;
          const bool inside = in_type && c >= mn && c <= mx;
          const size_t bin = inside ? (size_t)(((c - mn) >> shift) >> 4) : 0;
          for (int state : states) for (int coarse = 0; coarse < 2; coarse++) for (int64_t opt = 0; opt <= 2; opt++) for (int64_t nrows : rows) {
            const uint64_t edge = (uint64_t)nrows / 128ull;
            for (uint64_t in_bin : {(uint64_t)0, edge, edge + (uint64_t)1}) {
              hist[bin] = in_bin;
              if (bin + 1 < hist.size()) hist[bin + 1] = ~0ull;                                 // (a neighbour the guard must not look at)
              if (bin > 0) hist[bin - 1] = ~0ull;
              check_route(sg != 0, state, coarse != 0, mn, mx, cb, nrows, opt, in_bin, coarse ? hist.data() : nullptr);
              hist[bin] = 0;
              if (bin + 1 < hist.size()) hist[bin + 1] = 0;
              if (bin > 0) hist[bin - 1] = 0;
            }
          }
        }
      }
    }
  }
  // a dtype that gets no image routes flat whatever the copies say
  {
    ScanCopyFacts f; f.built = true; f.coarse = true; f.max = 10; f.hist = hist.data(); f.nrows = 1000;
    for (int32_t dt : {(int32_t)DFDB_I32, (int32_t)DFDB_U32, (int32_t)DFDB_F64, (int32_t)DFDB_U16}) {
      const ScanRoute r = scan_route(dt, 5, f, 1);
      CHECK(r.form == kScanFlat && scan_route_notes(r).n == 0, "dtype %d routed to form %d", dt, r.form);
    }
  }
  // ---- the build trigger: only a column without an image, only when the option allows, at the second eligible scan (option 2: the first), never below min_rows
  for (int state : states) for (int64_t opt = 0; opt <= 2; opt++) for (int64_t scans = 1; scans <= 3; scans++) for (int64_t min_rows : {(int64_t)1, (int64_t)1 << 24}) for (int below = 0; below < 2; below++) {
    const int64_t nrows = min_rows - below;
    bool want = false;
    if (state == kImageNone && !below) want = opt == 2 ? true : opt == 1 ? scans != 1 : false;
    CHECK(scan_image_builds(state, scans, opt, nrows, min_rows) == want, "builds(state %d, scans %lld, opt %lld, nrows %lld, min_rows %lld): expected %d", state, (long long)scans,
          (long long)opt, (long long)nrows, (long long)min_rows, (int)want);
  }
  CHECK(seen[kScanFlat] > 0 && seen[kScanImage] > 0 && seen[kScanCoarseExact] > 0 && seen[kScanCoarse] > 0 && seen[4] > 0, "forms reached: %ld %ld %ld %ld, dense %ld", seen[0], seen[1], seen[2], seen[3], seen[4]);
  CHECK(kImageNone == 0 && kImageBuilt == 1 && kImageMisfit == 2 && kImageNoRoom == 3, "states");
  std::printf("%ld checks (flat %ld, image %ld of them dense %ld, exact %ld, coarse %ld), %d wrong\n", checks, seen[0], seen[1], seen[4], seen[2], seen[3], bad);
  return bad ? 1 : 0;
}
