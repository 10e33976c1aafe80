// k_join.hip — K14: the row lists of a join of two selections on one fixed-width key (gfx950): inner, left, semi and anti.
//
// The reference has no join ("several tables with possibility of joins" is on its roadmap, docs/src/index.md:598); a user materializes both sides and
// merges on the host.  Here the right side's selected, non-missing keys are sorted by K12 (k_sort.hip: stable, so equal keys lie in ascending row order)
// and every selected left row finds its run of equal keys in that list by binary search.  No hash table, no atomics on the result path, no kernel that waits
// on another workgroup: the answer does not depend on the grid or on scheduling.
//
// PROBE (k_join_probe, K14a): k_sort_rekey's skeleton over the left rows laid ascending into `order` — one wave owns 1024 consecutive entries in 16 rounds of
// 64, lane = entry: 16 coalesced loads of the entries, the 16 gathers of the rows' missing words (nullable column only), the 16 column loads of the live
// entries.  The keys are select_key<DT, false>: the sorted list's own keys.  Then the searches, in two halves of 8 entries: every entry runs the bounded lower
// bound of join_rule.hpp twice — with < (lo) and with <= (lo + cnt) — and the 16 searches of a half run IN LOCK STEP: one step issues their 16 independent
// 8-byte loads before any is used.  The step count is wave-uniform (the bit length of nr, from the host).  Searching with <= instead of for key + 1 keeps the
// all-ones key (every NaN, typemax(UInt64), typemax(Int64)) an ordinary key.  No index at or beyond nr is read; nr = 0 takes no step.  The group's total of
// join_emitted is a 64-bit wave sum, stored in 32 bits; 2^32 or more raises the flag word (one vector atomic).  The missing left rows leave with one 64-bit
// vector atomicAdd per wave that has any.  No LDS, no scratch.
//   algorithmic bytes / entry: 4 (order) + the key + 8 written; what it MOVES is a 128-byte line per gathered key and per search step that leaves the cache:
//   2 * bitlength(nr) dependent 8-byte gathers per entry, of which the first steps hit the same few lines for every entry
//
// EXPAND (k_join_expand, K14b): one wave per 1024-entry group, groups without output skipped.  Per round of 64 entries each lane loads its order, lo and cnt,
// e = join_emitted(kind, cnt), and the wave scans e.  The round's outputs are then produced 64 AT A TIME BY ALL LANES: output o finds its owning lane by a
// 6-step search over the inclusive scan (shuffles), takes that lane's order / lo / cnt, and stores left_rows and right_rows at out_base[group] + the outputs of
// the rounds before + o — consecutive lanes store consecutive addresses, and the loads of one entry's run of right rows are coalesced.  A hot key does not
// serialise on one lane.  (A round whose 64 entries emit one pair each — a join into unique keys — skips the search: output o belongs to lane o.)
#include "device_utils.hpp"
#include "value_rules.hpp"
#include "select_key.hpp"
#include "join_rule.hpp"
#include "kernels.hpp"
#include "launch_dispatch.hpp"
#include "../../include/dfdb_ir.h"

namespace dfdb {

constexpr int kJoinBlock = 256;                                   // threads per workgroup (both kernels)
constexpr int kJoinWaves = kJoinBlock / 64;
constexpr int kJoinMaxBlocks = 2048;                              // the rekey's cap: 8 workgroups per CU, grid-stride beyond
constexpr int kJoinHalf = 8;                                      // entries per lane whose searches run in lock step (two searches each: 16 loads per step)

template <int DT>
__global__ __launch_bounds__(kJoinBlock) void k_join_probe(const typename SelT<DT>::type* __restrict__ col, const uint64_t* __restrict__ missing, JoinProbe P) {
  using T = typename SelT<DT>::type;
  const int lane = lane_id();
  const int64_t wave = (int64_t)blockIdx.x * kJoinWaves + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kJoinWaves;
  const int64_t ngroups = (P.nl + 1023) / 1024;
  const uint32_t* mhalf = (const uint32_t*)missing;              // little-endian: bit (r & 31) of half (r >> 5) is bit (r & 63) of word (r >> 6)
  uint32_t lmiss = 0;                                            // this lane's missing left rows (nl < 2^31)
  for (int64_t g = wave; g < ngroups; g += nwaves) {
    const int64_t e0 = g * 1024 + lane;
    uint32_t r[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const int64_t i = e0 + j * 64;
      r[j] = i < P.nl ? __builtin_nontemporal_load(P.order + i) : 0xffffffffu;
    }
    uint32_t mh[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
      mh[j] = 0;
      if (missing && (int64_t)r[j] < P.nrows) mh[j] = mhalf[r[j] >> 5];
    }
    uint32_t pres = 0, miss = 0;                                 // bit j: entry j of this lane is there / its key is missing
#pragma unroll
    for (int j = 0; j < 16; j++) {
      if ((int64_t)r[j] < P.nrows) pres |= 1u << j;
      if ((mh[j] >> (r[j] & 31u)) & 1u) miss |= 1u << j;
    }
    const uint32_t livem = pres & ~miss;
    lmiss += (uint32_t)__popc(miss);
    T v[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
      v[j] = T(0);
      if ((livem >> j) & 1u) v[j] = col[r[j]];                   // the live entries only (a row of the table, never under a missing bit)
    }
    uint64_t key[16];
#pragma unroll
    for (int j = 0; j < 16; j++) key[j] = select_key<DT, false>(&v[j]);
    uint64_t tot = 0;                                            // this lane's share of the group's pairs
#pragma unroll
    for (int h = 0; h < 16 / kJoinHalf; h++) {
      uint32_t a[kJoinHalf], z[kJoinHalf];                       // keys < key, keys <= key: the two searches of every entry
#pragma unroll
      for (int j = 0; j < kJoinHalf; j++) { a[j] = 0; z[j] = 0; }
      for (int b = P.steps - 1; b >= 0; b--) {                   // wave-uniform trip count
        uint64_t ka[kJoinHalf], kz[kJoinHalf];
#pragma unroll
        for (int j = 0; j < kJoinHalf; j++) {                    // the step's 16 loads, all issued before any is used
          const bool live = (livem >> (h * kJoinHalf + j)) & 1u;
          const int64_t ia = join_step_index(a[j], b, P.nr), iz = join_step_index(z[j], b, P.nr);
          ka[j] = 0; kz[j] = 0;
          if (live && ia >= 0) ka[j] = P.rkeys[ia];
          if (live && iz >= 0) kz[j] = P.rkeys[iz];
        }
#pragma unroll
        for (int j = 0; j < kJoinHalf; j++) {
          const bool live = (livem >> (h * kJoinHalf + j)) & 1u;
          const int64_t ia = join_step_index(a[j], b, P.nr), iz = join_step_index(z[j], b, P.nr);
          if (live && ia >= 0 && join_step_take<false>(ka[j], key[h * kJoinHalf + j])) a[j] = (uint32_t)ia + 1u;
          if (live && iz >= 0 && join_step_take<true>(kz[j], key[h * kJoinHalf + j])) z[j] = (uint32_t)iz + 1u;
        }
      }
#pragma unroll
      for (int j = 0; j < kJoinHalf; j++) {                      // lo and cnt hold ngroups * 1024 entries: every entry writes (not live: 0 and 0)
        const int64_t i = e0 + (int64_t)(h * kJoinHalf + j) * 64;
        const uint32_t c = z[j] - a[j];
        P.lo[i] = a[j]; P.cnt[i] = c;
        if (i < P.nl) tot += join_emitted(P.kind, c);
      }
    }
    tot = wave_sum64(tot);
    if (lane == 0) {
      P.grp_total[g] = (uint32_t)tot;
      if (tot >> 32) atomicOr(P.flag, 1u);
    }
  }
  const uint32_t wmiss = wave_sum(lmiss);
  if (lane == 0 && wmiss) atomicAdd(P.nmiss, (unsigned long long)wmiss);
}

void launch_join_probe(hipStream_t s, const ColRef& col, const JoinProbe& P) {
  const int64_t ngroups = (P.nl + 1023) / 1024;
  if (ngroups < 1) return;
  int grid = (int)((ngroups + kJoinWaves - 1) / kJoinWaves);
  if (grid > kJoinMaxBlocks) grid = kJoinMaxBlocks;
  with_dtype<DtValues>(col.dtype, [&](auto c) {      // (Bool as DFDB_U8)
    constexpr int DT = decltype(c)::dtype;
    using T = typename SelT<DT>::type;
    hipLaunchKernelGGL((k_join_probe<DT>), dim3(grid), dim3(kJoinBlock), 0, s, (const T*)col.data, col.missing, P);
  });
}

__global__ __launch_bounds__(kJoinBlock) void k_join_expand(JoinExpand E) {
  const int lane = lane_id();
  const int64_t wave = (int64_t)blockIdx.x * kJoinWaves + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kJoinWaves;
  const int64_t ngroups = (E.nl + 1023) / 1024;
  for (int64_t g = wave; g < ngroups; g += nwaves) {
    uint64_t run = E.out_base[g];                                // wave-uniform: where the round's first output goes
    if (E.out_base[g + 1] == run) continue;                      // a group without output touches nothing else
    for (int j = 0; j < 16; j++) {
      const int64_t i = g * 1024 + j * 64 + lane;
      const bool valid = i < E.nl;
      uint32_t o = 0, l = 0, c = 0;
      if (valid) { o = E.order[i]; l = E.lo[i]; c = E.cnt[i]; }
      const uint32_t e = valid ? (uint32_t)join_emitted(E.kind, c) : 0u;     // (the group's total is below 2^32, so is every entry's and every round's)
      const uint32_t incl = wave_incl_scan(e);
      const uint32_t tot = (uint32_t)__shfl((int)incl, 63, 64);
      if (tot == 0) continue;                                    // wave-uniform
      const bool one_each = __ballot(e == 1u) == ~0ull;          // wave-uniform: output o is lane o's
      const uint32_t nsteps = join_round_steps(tot);             // steps of 64 outputs; counted in steps, so a total near 2^32 cannot wrap the loop
      for (uint32_t st = 0; st < nsteps; st++) {
        const uint64_t out = join_step_output(st, lane);         // 64 bits: the last step's outputs may lie beyond 2^32 - 1 (and beyond tot)
        int own = lane;
        if (!one_each) {                                         // the lanes whose inclusive sum is <= out precede the owner: a 6-step search, at most 63
          own = 0;
#pragma unroll
          for (int b = 32; b >= 1; b >>= 1) {
            const uint32_t s = (uint32_t)__shfl((int)incl, own + b - 1, 64);
            if (s <= out) own += b;
          }
        }
        const uint32_t oo = (uint32_t)__shfl((int)o, own, 64), ll = (uint32_t)__shfl((int)l, own, 64), cc = (uint32_t)__shfl((int)c, own, 64);
        const uint32_t first = (uint32_t)__shfl((int)(incl - e), own, 64);      // the owner's first output of the round
        const uint64_t pos = run + out;
        if (out < tot && pos < (uint64_t)E.cap) {
          E.left_rows[pos] = E.lbase + (int64_t)oo + 1;
          if (E.right_rows) E.right_rows[pos] = cc ? E.rbase + (int64_t)E.rrows[ll + (uint32_t)(out - first)] + 1 : (int64_t)0;
        }
      }
      run += tot;
    }
  }
}

void launch_join_expand(hipStream_t s, const JoinExpand& E) {
  const int64_t ngroups = (E.nl + 1023) / 1024;
  if (ngroups < 1) return;
  int grid = (int)((ngroups + kJoinWaves - 1) / kJoinWaves);
  if (grid > kJoinMaxBlocks) grid = kJoinMaxBlocks;
  hipLaunchKernelGGL(k_join_expand, dim3(grid), dim3(kJoinBlock), 0, s, E);
}

}  // namespace dfdb
