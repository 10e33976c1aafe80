// k_join.hip — K14: the row lists of a join of two selections (gfx950): inner, left, semi and anti — on one fixed-width key (probe, expand) and on several keys,
// String keys among them (K14c at the end of this file: live, refine; the expand is the same).
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
#include "str_tile.hpp"
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

// ---- K14c: the join on several keys -------------------------------------------------------------------------------------------------------------------
// LIVE (k_join_live): the probe's skeleton over a row order — 16 coalesced loads of the entries, then per nullable key 16 gathers (the rows' missing halves,
// or a String column's sizes) —; the placement is the rekey's arithmetic: base of the tile + the running count + the popcount of the ballot below the lane
template <int MODE>
__global__ __launch_bounds__(kJoinBlock) void k_join_live(JoinLive L) {
  const int lane = lane_id();
  const uint64_t below = (1ull << lane) - 1ull;
  const int64_t wave = (int64_t)blockIdx.x * kJoinWaves + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kJoinWaves;
  const int64_t ntiles = (L.n + 1023) / 1024;
  uint32_t ldead = 0;                                            // START: this lane's entries with a missing component
  for (int64_t tile = wave; tile < ntiles; tile += nwaves) {
    const int64_t e0 = tile * 1024 + lane;
    uint32_t r[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const int64_t i = e0 + j * 64;
      r[j] = i < L.n ? __builtin_nontemporal_load(L.order + i) : 0xffffffffu;
    }
    uint32_t pres = 0, miss = 0;                                 // bit j: entry j of this lane is there / has a missing component
#pragma unroll
    for (int j = 0; j < 16; j++) if ((int64_t)r[j] < L.nrows) pres |= 1u << j;
    for (int k = 0; k < L.keys.n; k++) {                         // wave-uniform
      const uint32_t* mhalf = (const uint32_t*)L.keys.missing[k];
      const int32_t* sizes = L.keys.sizes[k];
      uint32_t w[16];
#pragma unroll
      for (int j = 0; j < 16; j++) {
        w[j] = 0;
        if ((pres >> j) & 1u) w[j] = mhalf ? (mhalf[r[j] >> 5] >> (r[j] & 31u)) & 1u : (uint32_t)(sizes[r[j]] < 0);
      }
#pragma unroll
      for (int j = 0; j < 16; j++) miss |= w[j] << j;
    }
    const uint32_t livem = pres & ~miss;
    if (MODE == JOIN_LIVE_START) {
#pragma unroll
      for (int j = 0; j < 16; j++) {                             // lo and cnt hold ntiles * 1024 entries: every entry writes
        const int64_t i = e0 + j * 64;
        L.lo[i] = 0u; L.cnt[i] = (livem >> j) & 1u ? L.nr : 0u;
        if (i < L.n && !((livem >> j) & 1u)) ldead++;
      }
      if (L.grp_total && lane == 0) {
        const int64_t left = L.n - tile * 1024;
        L.grp_total[tile] = (uint32_t)(left < 1024 ? left : 1024) * L.emit0;
      }
    } else {
      uint32_t run = 0;                                          // wave-uniform: live entries of the tile so far
      const uint64_t base = MODE == JOIN_LIVE_PLACE ? L.live_base[tile] : 0ull;
#pragma unroll
      for (int j = 0; j < 16; j++) {
        const bool live = (livem >> j) & 1u;
        const uint64_t kmask = __ballot(live);
        if (MODE == JOIN_LIVE_PLACE && live) {
          const uint64_t pos = base + run + (uint32_t)__popcll(kmask & below);
          if (pos < (uint64_t)L.cap) L.out[pos] = r[j];
        }
        run += (uint32_t)__popcll(kmask);
      }
      if (MODE == JOIN_LIVE_COUNT && lane == 0) L.live_cnt[tile] = run;
    }
  }
  if (MODE == JOIN_LIVE_START) {
    const uint32_t wdead = wave_sum(ldead);
    if (lane == 0 && wdead) atomicAdd(L.nmiss, (unsigned long long)wdead);
  }
}

void launch_join_live(hipStream_t s, const JoinLive& L, JoinLiveMode mode) {
  const int64_t ntiles = (L.n + 1023) / 1024;
  if (ntiles < 1) return;
  int grid = (int)((ntiles + kJoinWaves - 1) / kJoinWaves);
  if (grid > kJoinMaxBlocks) grid = kJoinMaxBlocks;
  if (mode == JOIN_LIVE_COUNT) hipLaunchKernelGGL((k_join_live<JOIN_LIVE_COUNT>), dim3(grid), dim3(kJoinBlock), 0, s, L);
  else if (mode == JOIN_LIVE_PLACE) hipLaunchKernelGGL((k_join_live<JOIN_LIVE_PLACE>), dim3(grid), dim3(kJoinBlock), 0, s, L);
  else hipLaunchKernelGGL((k_join_live<JOIN_LIVE_START>), dim3(grid), dim3(kJoinBlock), 0, s, L);
}

// REFINE (k_join_refine): one stage of the join on several keys — the probe's skeleton, one wave per 1024 entries of `order`, 16 entries per lane.  The wave
// loads its 16 x 64 counts first: their maximum (a wave reduction) gives the wave-uniform step count, and a wave whose counts are all 0 — after the first
// sub-keys most waves of a selective join — loads no row, no key and no right sub-key.  Else, in two halves of 8 entries: the rows and the left sub-keys of
// the entries that still have a run (16 gathers deep for a fixed-width key; sizes, then offsets, then arena for a String chunk), then join_refine_stage<8>,
// the lock-step searches of join_rule.hpp: 16 independent 8-byte loads per step.  No LDS, no scratch, no atomics but the overflow flag.
//   algorithmic bytes / entry with a run: 8 (lo, cnt) + 4 (order) + the key + 8 written; what it MOVES is a 128-byte line per gathered key and per search step
//   that leaves the cache: 2 * bitlength(largest cnt of the wave) dependent 8-byte gathers per entry
struct JoinFixedSub {                                            // the left sub-key of a fixed-width column: its select key
  template <int DT> struct Of {
    const typename SelT<DT>::type* col;
    __device__ __forceinline__ void load(const uint32_t (&r)[kJoinHalf], uint32_t livem, uint64_t (&x)[kJoinHalf]) const {
      using T = typename SelT<DT>::type;
      T v[kJoinHalf];
#pragma unroll
      for (int j = 0; j < kJoinHalf; j++) {
        v[j] = T(0);
        if ((livem >> j) & 1u) v[j] = col[r[j]];                 // an entry with a run only: a row of the table, never under a missing bit
      }
#pragma unroll
      for (int j = 0; j < kJoinHalf; j++) x[j] = select_key<DT, false>(&v[j]);
    }
  };
};
struct JoinStringSub {                                           // the left sub-key of a String column: a chunk (join_chunk_key) or the length
  JoinStrSub K;
  __device__ __forceinline__ void load(const uint32_t (&r)[kJoinHalf], uint32_t livem, uint64_t (&x)[kJoinHalf]) const {
    int32_t sz[kJoinHalf];
#pragma unroll
    for (int j = 0; j < kJoinHalf; j++) {
      sz[j] = 0;
      if ((livem >> j) & 1u) sz[j] = K.col.sizes[r[j]];          // (not negative: an entry whose String is missing has no run)
    }
    if (K.chunk < 0) {                                           // wave-uniform
#pragma unroll
      for (int j = 0; j < kJoinHalf; j++) x[j] = (uint32_t)sz[j];
      return;
    }
    const uint32_t cb = 8u * (uint32_t)K.chunk;
    uint32_t need = 0;                                           // bit j: the entry has a run and its string reaches into the chunk
#pragma unroll
    for (int j = 0; j < kJoinHalf; j++) if (((livem >> j) & 1u) && sz[j] > 0 && join_chunk_reaches((uint32_t)sz[j], (uint32_t)K.chunk)) need |= 1u << j;
    uint32_t ro[kJoinHalf]; int64_t to[kJoinHalf];
#pragma unroll
    for (int j = 0; j < kJoinHalf; j++) {
      ro[j] = 0; to[j] = 0;
      if ((need >> j) & 1u) { ro[j] = K.row_off[r[j]]; to[j] = K.col.tile_off[r[j] >> 10]; }
    }
    uint64_t raw[kJoinHalf];
#pragma unroll
    for (int j = 0; j < kJoinHalf; j++) {
      raw[j] = 0;
      if ((need >> j) & 1u) raw[j] = load_u64_unaligned(K.col.bytes + to[j] + (int64_t)ro[j] + (int64_t)cb);     // (inside the row: cb < its length)
    }
#pragma unroll
    for (int j = 0; j < kJoinHalf; j++) x[j] = (need >> j) & 1u ? join_chunk_key(raw[j], (uint32_t)sz[j] - cb) : 0ull;
  }
};

template <class Sub>
__device__ __forceinline__ void join_refine_body(const JoinRefine& P, const Sub& sub) {
  const int lane = lane_id();
  const int64_t wave = (int64_t)blockIdx.x * kJoinWaves + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kJoinWaves;
  const int64_t ngroups = (P.nl + 1023) / 1024;
  for (int64_t g = wave; g < ngroups; g += nwaves) {
    const int64_t e0 = g * 1024 + lane;
    uint32_t c[16], l[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const int64_t i = e0 + j * 64;
      c[j] = i < P.nl ? P.cnt[i] : 0u;
    }
    uint32_t cmax = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) cmax = c[j] > cmax ? c[j] : cmax;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)cmax, d, 64); cmax = o > cmax ? o : cmax; }
    if (cmax != 0) {                                             // wave-uniform
      const int steps = 32 - __clz((int)cmax);                   // the bit length of the wave's largest count
#pragma unroll
      for (int j = 0; j < 16; j++) {
        const int64_t i = e0 + j * 64;
        l[j] = c[j] ? P.lo[i] : 0u;
      }
#pragma unroll
      for (int h = 0; h < 16 / kJoinHalf; h++) {
        uint32_t r[kJoinHalf];
        uint32_t livem = 0;                                      // bit j: entry h * 8 + j has a run (and a row of the table: a guard)
#pragma unroll
        for (int j = 0; j < kJoinHalf; j++) {
          const int64_t i = e0 + (int64_t)(h * kJoinHalf + j) * 64;
          r[j] = c[h * kJoinHalf + j] ? __builtin_nontemporal_load(P.order + i) : 0xffffffffu;
          if ((int64_t)r[j] < P.nrows) livem |= 1u << j; else c[h * kJoinHalf + j] = 0u;
        }
        uint64_t x[kJoinHalf];
        sub.load(r, livem, x);
        join_refine_stage<kJoinHalf>(P.rsub, &l[h * kJoinHalf], &c[h * kJoinHalf], x, steps);
      }
#pragma unroll
      for (int j = 0; j < 16; j++) {                             // lo and cnt hold ngroups * 1024 entries
        const int64_t i = e0 + j * 64;
        P.lo[i] = l[j]; P.cnt[i] = c[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 16; j++) P.cnt[e0 + j * 64] = 0u;
    }
    if (P.last) {                                                // wave-uniform
      uint64_t tot = 0;                                          // this lane's share of the group's pairs
#pragma unroll
      for (int j = 0; j < 16; j++) if (e0 + j * 64 < P.nl) tot += join_emitted(P.kind, c[j]);
      tot = wave_sum64(tot);
      if (lane == 0) {
        P.grp_total[g] = (uint32_t)tot;
        if (tot >> 32) atomicOr(P.flag, 1u);
      }
    }
  }
}

template <int DT>
__global__ __launch_bounds__(kJoinBlock) void k_join_refine(const typename SelT<DT>::type* __restrict__ col, JoinRefine P) {
  join_refine_body(P, typename JoinFixedSub::template Of<DT>{col});
}
__global__ __launch_bounds__(kJoinBlock) void k_join_refine_str(JoinStrSub K, JoinRefine P) { join_refine_body(P, JoinStringSub{K}); }

static int join_refine_grid(const JoinRefine& P) {
  const int64_t ngroups = (P.nl + 1023) / 1024;
  if (ngroups < 1) return 0;
  const int64_t grid = (ngroups + kJoinWaves - 1) / kJoinWaves;
  return (int)(grid > kJoinMaxBlocks ? kJoinMaxBlocks : grid);
}
void launch_join_refine(hipStream_t s, const ColRef& col, const JoinRefine& P) {
  const int grid = join_refine_grid(P);
  if (grid < 1) return;
  with_dtype<DtValues>(col.dtype, [&](auto c) {      // (Bool as DFDB_U8)
    constexpr int DT = decltype(c)::dtype;
    using T = typename SelT<DT>::type;
    hipLaunchKernelGGL((k_join_refine<DT>), dim3(grid), dim3(kJoinBlock), 0, s, (const T*)col.data, P);
  });
}
void launch_join_refine_str(hipStream_t s, const JoinStrSub& K, const JoinRefine& P) {
  const int grid = join_refine_grid(P);
  if (grid < 1) return;
  hipLaunchKernelGGL(k_join_refine_str, dim3(grid), dim3(kJoinBlock), 0, s, K, P);
}

}  // namespace dfdb
