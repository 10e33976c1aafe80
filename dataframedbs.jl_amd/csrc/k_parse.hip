// k_parse.hip — the conversion kernel: a projected column that is exactly `CAST T (COL s)` over a String column.  One kernel, k_str_convert, and two
// conversions: parse.(T, s) — the tutorial's add_column!(t, :id, parse.(Int64, t.s)) and materialize — and, for `CAST DFDB_CAST_DATETIME (COL s)`,
// datetime19.(s): the tutorial's timestamp column to a DateTime column (include/dfdb_ir.h has the contracts).
//
// The interpreter's H_PARSE and H_DATETIME (k_interp_device.inc: slow_parse / parse_bytes, slow_datetime / datetime_bytes / datetime_fields) are the
// definitions, and this file compiles that very text: every row a conversion's fast path does not settle goes through the same function, so the two paths
// cannot disagree on a value, an error kind or an error row.
//
// One wave per 1024-row tile, the walk of str_tile.hpp: the sixteen size loads and the tile's byte range [tile_off[t], tile_off[t+1]), as aligned 16-byte
// loads, are in flight together; the bytes are parked in LDS and row offsets are wave prefix sums of the sizes.  A lane reads its row's first 24 bytes as
// four aligned 8-byte LDS words shifted into place and hands them to the conversion's fast path; a row that is not eligible for it, or that it does not
// settle, is the slow path's, over the same LDS bytes.  A tile whose bytes do not fit the stage is converted straight from the arena.  Row j * 64 + lane
// belongs to lane `lane`, so the results of 64 neighbouring rows leave in one coalesced store.  SELECTED: only the rows of the bitmap, written compacted at
// prefix[tile] + rank (as k_gather does).
//
// parse: [sign] + 1..19 digits, eight at a time in registers (SWAR); anything else — whitespace, other characters, 20 digits, a value outside the target, a
// missing row, Float64 — is slow_parse's.  Its stage is 19968 bytes per wave: 1024 rows x 19 bytes + the lead (<= 15) + the 16 bytes of the last piece =
// 19487 at most.  With the 64 spare bytes that is 20032 bytes per wave, 40064 per two-wave workgroup, and floor(163840 / 40064) = 4 workgroups = 8 waves
// on a CU's 160 KiB of LDS.
// datetime: n >= 19, ASCII and the 14 digit positions checked with masks, the six fields formed pairwise in registers, rules 4-6 from datetime_fields; a
// row that is not a plain value (missing, short, non-digit, out of range, hour 24, non-ASCII) is slow_datetime's.  The tutorial's rows are 23 bytes
// ("yyyy-mm-dd HH:MM:SS UTC"), so its stage is 24576 bytes per wave: 1024 x 23 + the lead + the last piece = 23583 at most.  With the 64 spare bytes that
// is 24640 bytes per wave, 49280 per two-wave workgroup, and floor(163840 / 49280) = 3 workgroups = 6 waves per CU (one wave per workgroup would give the
// same 6 waves).
#include "device_utils.hpp"
#include "value_rules.hpp"
#include "engine.hpp"
#include "str_tile.hpp"

namespace dfdb {

#include "k_interp_device.inc"

void settle_launch_errors(dfdb_query* q, int mode, const int* derr);   // k_interp.hip

constexpr int kParseWaves = 2;               // waves per workgroup: 39 KB (parse) or 48 KB (datetime) of LDS each

__device__ __forceinline__ uint64_t parse_get8(uint64_t x0, uint64_t x1, uint64_t x2, uint32_t o) {   // 8 bytes at byte offset o (0..15) of the 24 bytes x0 x1 x2
  const uint64_t lo = (o & 8u) ? x1 : x0, hi = (o & 8u) ? x2 : x1;
  const uint32_t sh = (o & 7u) * 8u;
  return sh ? (lo >> sh) | (hi << (64u - sh)) : lo;
}
__device__ __forceinline__ bool swar_digits8(uint64_t x) {       // all eight bytes are '0'..'9'
  return ((x & 0xF0F0F0F0F0F0F0F0ull) | (((x + 0x0606060606060606ull) & 0xF0F0F0F0F0F0F0F0ull) >> 4)) == 0x3333333333333333ull;
}
__device__ __forceinline__ uint64_t swar_value8(uint64_t x) {    // eight ASCII digits, the first in the lowest byte
  x -= 0x3030303030303030ull;
  x = x * 10 + (x >> 8);
  return (((x & 0x000000FF000000FFull) * 0x000F424000000064ull) + (((x >> 16) & 0x000000FF000000FFull) * 0x0000271000000001ull)) >> 32;
}
// [sign] + 1..19 digits that fit the target: true and the register image; anything else is the slow path's to decide
__device__ __forceinline__ bool parse_fast(uint64_t x0, uint64_t x1, uint64_t x2, int len, int rt, uint64_t& out) {
  const uint32_t c0 = (uint32_t)x0 & 0xffu;
  const uint32_t s = (c0 == '+' || (is_signed(rt) && c0 == '-')) ? 1u : 0u;
  const bool neg = s && c0 == '-';
  const int nd = len - (int)s;
  if (nd < 1 || nd > 19) return false;
  const uint32_t k = (uint32_t)nd & 7u, full = (uint32_t)nd >> 3;
  uint32_t o = s; uint64_t v = 0; bool ok = true;
  if (k) {
    const uint64_t x = (parse_get8(x0, x1, x2, o) << ((8u - k) * 8u)) | (0x3030303030303030ull >> (k * 8u));      // left-padded with '0'
    ok = swar_digits8(x); v = swar_value8(x); o += k;
  }
  if (full >= 1) { const uint64_t x = parse_get8(x0, x1, x2, o); ok = ok && swar_digits8(x); v = v * 100000000ull + swar_value8(x); o += 8; }
  if (full >= 2) { const uint64_t x = parse_get8(x0, x1, x2, o); ok = ok && swar_digits8(x); v = v * 100000000ull + swar_value8(x); }
  uint64_t lim = int_hi(rt);                                     // the largest magnitude of this sign (19 digits never overflow 64 bits)
  if (neg) lim += 1;
  out = neg ? 0 - v : v;
  return ok && v <= lim;
}

// n >= 19 ASCII bytes whose 14 field bytes are digits and whose fields are a DateTime Julia accepts: true and the value; anything else is the slow path's
__device__ __forceinline__ bool datetime_fast(uint64_t x0, uint64_t x1, uint64_t x2, int len, uint64_t& out) {
  constexpr uint64_t kM0 = 0x00FFFF00FFFFFFFFull, kM1 = 0xFFFF00FFFF00FFFFull, kM2 = 0x0000000000FFFF00ull, kZ = 0x3030303030303030ull;   // the field bytes of bytes 0-7, 8-15, 16-23
  const bool ascii = (((x0 | x1) & 0x8080808080808080ull) | (x2 & 0x0000000000808080ull)) == 0;                                         // bytes 0 .. 18
  const uint64_t f0 = (x0 & kM0) | (kZ & ~kM0), f1 = (x1 & kM1) | (kZ & ~kM1), f2 = (x2 & kM2) | (kZ & ~kM2);                           // '0' wherever a byte is ignored
  const bool digits = swar_digits8(f0) && swar_digits8(f1) && swar_digits8(f2);
  uint64_t v0 = f0 - kZ, v1 = f1 - kZ, v2 = f2 - kZ;
  v0 = v0 * 10 + (v0 >> 8); v1 = v1 * 10 + (v1 >> 8); v2 = v2 * 10 + (v2 >> 8);                                                         // byte i: digit i * 10 + digit i + 1 (at most 99)
  const int y = (int)(v0 & 0xff) * 100 + (int)((v0 >> 16) & 0xff), mo = (int)((v0 >> 40) & 0xff);
  const int d = (int)(v1 & 0xff), h = (int)((v1 >> 24) & 0xff), mi = (int)((v1 >> 48) & 0xff), s = (int)((v2 >> 8) & 0xff);
  int reason = PR_OK;
  out = (uint64_t)datetime_fields(digits ? y : 1, digits ? mo : 1, digits ? d : 1, digits ? h : 0, digits ? mi : 0, digits ? s : 0, reason);
  return len >= 19 && ascii && digits && reason == PR_OK;
}

// What a conversion is: kStage (a wave's stage, bytes), kPieces (16-byte loads per lane in flight per staging round), eligible (the rows that may try the
// fast path), fast (the first 24 bytes of a row in registers: true and the value, or false), slow (the interpreter's function), store, and kLdsBytes (what a workgroup's
// stages must come to).
template <int W>
struct ParseConv {
  static constexpr uint32_t kStage = 19968;  // 1024 rows x 19 bytes + the lead of the 16-byte boundary below + the last piece, see the head of the file
  static constexpr int kPieces = 5;          // 5 KB per wave and round, four rounds for a full stage
  static constexpr uint32_t kLdsBytes = 40064;   // per workgroup: four workgroups on a CU
  int rt;
  __device__ __forceinline__ bool eligible(int32_t s0) const { return rt != DFDB_F64 && s0 > 0; }
  __device__ __forceinline__ bool fast(uint64_t x0, uint64_t x1, uint64_t x2, int len, uint64_t& out) const { return parse_fast(x0, x1, x2, len, rt, out); }
  __device__ __forceinline__ uint64_t slow(const uint8_t* p, int len, bool missing, bool alive, int* err, uint64_t row) const { return slow_parse(p, len, missing, rt, alive, err, row); }
  __device__ __forceinline__ static void store(void* out, int64_t o, uint64_t v) {
    if (W == 1) ((uint8_t*)out)[o] = (uint8_t)v; else if (W == 2) ((uint16_t*)out)[o] = (uint16_t)v;
    else if (W == 4) ((uint32_t*)out)[o] = (uint32_t)v; else ((uint64_t*)out)[o] = v;
  }
};
struct DatetimeConv {
  static constexpr uint32_t kStage = 24576;  // 1024 rows x 23 bytes + the lead + the last 16-byte piece (23583), see the head of the file
  static constexpr int kPieces = 6;          // 6 KB per wave and round, four rounds for a full stage
  static constexpr uint32_t kLdsBytes = 49280;   // per workgroup: three workgroups on a CU
  __device__ __forceinline__ bool eligible(int32_t s0) const { return s0 >= 19; }
  __device__ __forceinline__ bool fast(uint64_t x0, uint64_t x1, uint64_t x2, int len, uint64_t& out) const { return datetime_fast(x0, x1, x2, len, out); }
  __device__ __forceinline__ uint64_t slow(const uint8_t* p, int len, bool missing, bool alive, int* err, uint64_t row) const { return slow_datetime(p, len, missing, alive, err, row); }
  __device__ __forceinline__ static void store(void* out, int64_t o, uint64_t v) { ((uint64_t*)out)[o] = v; }
};

template <class CONV, bool SELECTED>
__global__ __launch_bounds__(kParseWaves * 64) void k_str_convert(const int32_t* __restrict__ sizes, const int64_t* __restrict__ tile_off, const uint8_t* __restrict__ bytes,
                                                                  const uint64_t* __restrict__ bitmap, const uint64_t* __restrict__ prefix, void* __restrict__ out,
                                                                  int64_t out_cap, int64_t nrows, int64_t ntiles, CONV conv, int* __restrict__ err) {
  constexpr uint32_t kRound = (uint32_t)CONV::kPieces * 1024u, kRounds = (CONV::kStage + kRound - 1) / kRound;
  static_assert(CONV::kStage % 16 == 0 && CONV::kStage <= kRound * kRounds, "the stage is whole 16-byte pieces, filled in whole rounds");
  __shared__ __attribute__((aligned(16))) uint64_t stage_sh[kParseWaves][CONV::kStage / 8 + 8];
  static_assert(sizeof(stage_sh) == CONV::kLdsBytes, "the LDS per workgroup is what the head of the file counts on");
  const int lane = lane_id();
  const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint64_t* const stage = stage_sh[wid];
  const int64_t wave = (int64_t)blockIdx.x * kParseWaves + wid, nwaves = (int64_t)gridDim.x * kParseWaves;
  for (int64_t tile = wave; tile < ntiles; tile += nwaves) {
    uint32_t m_lo = ~0u, m_hi = ~0u;
    if (SELECTED) {
      const uint64_t w = lane < 16 ? bitmap[tile * 16 + lane] : 0ull;
      if (__ballot(w != 0) == 0) continue;                               // nothing selected in this tile
      m_lo = (uint32_t)w; m_hi = (uint32_t)(w >> 32);
    }
    const int64_t base = tile * kTile;
    int32_t sz[16];
    tile_sizes(sizes, base, nrows, lane, 0, sz);
    const TileSpan ts = tile_span(tile_off, tile);
    const bool staged = ts.span <= (int64_t)CONV::kStage;               // wave-uniform
    if (staged) stage_tile<CONV::kPieces, CONV::kStage>(bytes, ts, (uint8_t*)stage, lane);
    uint32_t run = 0, run_sel = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const int32_t s0 = sz[j];
      const uint32_t len = clamp_size(s0);
      const uint32_t incl = wave_incl_scan(len);
      const uint32_t rel = run + incl - len;
      run += __shfl(incl, 63, 64);
      const uint64_t mw = SELECTED ? tile_word(m_lo, m_hi, j) : ~0ull;
      const int64_t row = base + j * 64 + lane;
      const bool alive = row < nrows && ((mw >> lane) & 1ull);
      uint64_t v = 0;
      bool done = false;
      if (staged && alive && conv.eligible(s0)) {
        // (the four words stay inside the stage: a row starts at least its own length before `span - 16`, and the array has 64 bytes to spare)
        const uint32_t p = ts.lead + rel, a = p >> 3, sh = (p & 7u) * 8u;
        const uint64_t w0 = stage[a], w1 = stage[a + 1], w2 = stage[a + 2], w3 = stage[a + 3];
        const uint64_t x0 = sh ? (w0 >> sh) | (w1 << (64u - sh)) : w0, x1 = sh ? (w1 >> sh) | (w2 << (64u - sh)) : w1, x2 = sh ? (w2 >> sh) | (w3 << (64u - sh)) : w2;
        done = conv.fast(x0, x1, x2, (int)len, v);
      }
      if (!done) {
        const uint8_t* p = staged ? (const uint8_t*)stage + ts.lead + rel : bytes + ts.o0 + rel;
        v = conv.slow(p, (int)len, s0 < 0, alive, err, (uint64_t)row);
      }
      const int64_t o = SELECTED ? (int64_t)prefix[tile] + run_sel + (int64_t)__popcll(mw & ((1ull << lane) - 1ull)) : row;
      if (alive && o < out_cap) CONV::store(out, o, v);
      run_sel += (uint32_t)__popcll(mw);
    }
  }
}

// `e` is CAST T (COL s) over a resident String column, T a number type (parse) or DFDB_CAST_DATETIME (Int64 milliseconds): the selected rows' values,
// compacted, into dst (cap elements)
void run_str_convert(dfdb_query* q, const Node& e, void* dst, int64_t cap) {
  dfdb_table* t = q->t; dfdb_ctx* ctx = t->ctx; hipStream_t s = ctx->stream;
  const Column& c = t->cols[(size_t)e.a->col];
  if (!c.resident) fail(DFDB_ERR_ARGUMENT, "column %s is not resident on the device (dfdb_table_load it first)", c.name.c_str());
  const int64_t ntiles = ceil_div(t->nrows, kTile);
  if (ntiles == 0) return;
  DevBuf& db = q->tmp_a; db.ensure(64);
  struct { int flags, pad; uint64_t row[3]; } init{0, 0, {~0ull, ~0ull, ~0ull}};      // the interpreter's error block
  HIP_CHECK(hipMemcpyAsync(db.p, &init, sizeof init, hipMemcpyHostToDevice, s));
  stream_wait(ctx);
  int* derr = (int*)db.p;
  const bool datetime = e.cast_to == DFDB_CAST_DATETIME;
  const int rt = dt_base(e.cast_to);
  const bool all = cap == t->nrows;                                     // every row is selected: no bitmap, no compaction
  int64_t grid = ceil_div(ntiles, kParseWaves); if (grid > 32768) grid = 32768;
  {
    LaunchTimer lt(ctx, datetime ? "str_datetime" : "str_parse");
    auto launch = [&](auto conv) {
      using CONV = decltype(conv);
      hipLaunchKernelGGL((all ? k_str_convert<CONV, false> : k_str_convert<CONV, true>), dim3((unsigned)grid), dim3(kParseWaves * 64), 0, s, c.data.as<int32_t>(),
                         (const int64_t*)c.tile_off.p, c.bytes.as<uint8_t>(), q->bitmap.as<uint64_t>(), q->prefix.as<uint64_t>(), dst, cap, t->nrows, ntiles, conv, derr);
    };
    if (datetime) launch(DatetimeConv{});
    else switch (dt_width(rt)) { case 1: launch(ParseConv<1>{rt}); break; case 2: launch(ParseConv<2>{rt}); break; case 4: launch(ParseConv<4>{rt}); break; default: launch(ParseConv<8>{rt}); break; }
    HIP_CHECK(hipGetLastError());
  }
  settle_launch_errors(q, 1, derr);
}

}  // namespace dfdb
