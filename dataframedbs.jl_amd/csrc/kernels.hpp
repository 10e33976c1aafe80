// kernels.hpp — host-callable launchers of the gfx950 kernels (definitions in k_*.hip).
// Every launcher enqueues on `s` and returns immediately; none allocates or synchronises.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include "../../include/dfdb.h"

namespace dfdb {

// a kernel that may take more than 64 KB of dynamic LDS: its limit raised to `bytes` before EVERY launch (the attribute belongs to the function on the current
// device, and one process may drive several).  An earlier call's error is cleared first, so that the launcher's hipGetLastError() after the launch is the
// launch's own.  false, the error cleared: the launch must not be made
inline bool allow_dynamic_lds(const void* kernel, size_t bytes) {
  (void)hipGetLastError();
  if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess) return true;
  (void)hipGetLastError();
  return false;
}

// ---- how a column reaches a launcher.  A fixed-width column is a ColRef (engine.hpp: col_ref), a flat String column a StrSide (below; engine.hpp: str_side);
// what a kernel family needs beyond the columns travels in that family's argument record (AccArgs, RankArgs, MultiAccArgs, StrTable, RadixGroup ...), filled by
// the caller with named fields.  A value-initialised ColRef is "no column": the count-only reducer
struct ColRef { const void* data; int32_t dtype; const uint64_t* missing; };   // dtype: the base dtype; missing: the column's missing bitmap, null = not nullable

enum CmpOp : int { CMP_EQ = 0, CMP_NE = 1, CMP_LT = 2, CMP_LE = 3, CMP_GT = 4, CMP_GE = 5 };

// one simple term `col OP const` of a conjunction/disjunction (K1 multi-column form).  op2 >= 0: the term is the INTERVAL
// `col OP const  &  col OP2 const2` — two AND-ed comparisons of the same column (`65 > x > 34`, test/selection.jl:53) read it once
struct ScanTerm {
  const void* col;
  int32_t dtype;     // DFDB_* base dtype of the column
  int32_t op;        // CmpOp
  uint64_t cbits;    // constant already converted to the column's own type (bit pattern)
  int32_t op2 = -1;  // CmpOp of the second comparison, -1 = none
  uint64_t cbits2 = 0;
  // pre = 1: the compared value is rem(col, m) for a signed integer column and a constant m (`a % 50 == 0`, test/selection.jl:21): computed in
  // Int64 as sign(x) * (|x| mod |m|), |x| / |m| by multiplication with a precomputed magic number (pre_magic, pre_shift); cbits / cbits2 are Int64
  // pre = 2: the compared value is col * pre_magic + pre_d in wrapping Int64 (`a * 2 + 1 > c`; a signed integer column, integer constants);
  // pre = 3: the same in Float64 — fl(fl(Float64(x) * k) + d), two roundings, never fused (pre_magic / pre_d hold the doubles' bits);
  // pre = 4: Float64(x) / k (Julia's `/`: one correctly rounded division)
  int32_t pre = 0, pre_shift = 0;
  uint64_t pre_magic = 0, pre_d = 0;
};
constexpr int kMaxTerms = 6;
struct ScanTerms {
  ScanTerm t[kMaxTerms];
  int32_t n;
  int32_t combine_or;  // 0 = AND of all terms, 1 = OR
};

// ---- K1: predicate scan -> bitmap (+ per-1024-row tile counts) ----------------------------------
// single column `x OP c` (term: its col, dtype, op and cbits; no second comparison, no transform); and_existing: bitmap &= result (a predicate stage after a range stage)
void launch_scan_cmp(hipStream_t s, const ScanTerm& term, uint64_t* bitmap, uint32_t* tile_counts, int64_t nrows, bool and_existing, bool nt = true, void* cap = nullptr,
                     int wt_store = 3 /* bit 0: the bitmap leaves with write-through stores (ctx option "scan_wt_store"); bits 1-2: ctx option "scan_narrow" — which
                                         narrow columns take k_scan_cmp_narrow (16 bytes per lane): 1 = 1-byte (default), 2 = 1-, 2- and 4-byte, 0 = none */);
// K1's read stream alone (k_read_probe): an 8-byte column of nrows rows, nothing written (sink: one device word that is never stored to)
void launch_read_probe(hipStream_t s, const void* col, int64_t nrows, uint64_t* sink);
// the 4-byte scan image of an Int64 (is_signed) / UInt64 column (k_image.hip; scan_image.hpp): image[i] = the low half of col[i]; *misfit (a device word the caller
// zeroed) is raised when some value is not its truncation extended back.  col and image are 16-byte aligned and carry the columns' 256-byte pad.
// misfit[1] (zeroed) and misfit[2] (all ones) receive the largest and the smallest image value as unsigned words of the same order (signed: x ^ 0x80000000)
void launch_scan_image_build(hipStream_t s, const void* col, bool is_signed, void* image, int64_t nrows, uint32_t* misfit);
// the 2-byte coarse copy of a scan image (k_image.hip; scan_coarse.hpp): coarse[i] = (image[i] - vmin) >> shift, rows past nrows of the last 8 written as zero;
// hist: 4096 zeroed 64-bit device words, hist[k] += rows with coarse >> 4 == k.  image and coarse are 16-byte aligned and carry the 256-byte pad
void launch_scan_coarse_build(hipStream_t s, const void* image, void* coarse, int64_t nrows, uint32_t vmin, int shift, uint64_t* hist);
// `x OP c` over a scan image through its coarse copy, shift > 0 (k_scan.hip k_scan_cmp_coarse): a row whose coarse value differs from cc is decided by the two,
// the others are compared exactly as image[row] OP c in the image's signedness.  Same outputs as launch_scan_cmp over the image
void launch_scan_cmp_coarse(hipStream_t s, const void* coarse, const void* image, bool is_signed, int op, uint16_t cc, uint32_t c, uint64_t* bitmap, uint32_t* tile_counts,
                            int64_t nrows, bool and_existing, bool wt_store);
// extra = 1 (capture): the LAST term's 8-byte column at the finally selected rows, compacted per tile at extra_out[tile*1024 + rank];
// extra = 2 (sum): one partial sum of that column per 1024-row tile in extra_out[tile] (double, or wrapping 64-bit integer).  AND only.
// extra = 5 (capture two): the last term's column like extra = 1, and the 8-byte column of the term before it into extra_out2, same layout.
// (3 / 4: per-tile minimum / maximum in extra_out[tile], like the sum.)  The host names these values; the kernels take the int.
enum ScanExtra : int { EX_NONE = 0, EX_CAPTURE = 1, EX_SUM = 2, EX_MIN = 3, EX_MAX = 4, EX_CAPTURE2 = 5 };
void launch_scan_terms(hipStream_t s, const ScanTerms& terms, uint64_t* bitmap, uint32_t* tile_counts, int64_t nrows,
                       bool and_existing, int extra = 0, void* extra_out = nullptr,
                       int pair = 1 /* ctx option "scan_pair": two plain 8-byte terms go to the pipelined k_scan_pair */, void* extra_out2 = nullptr);
// whether launch_scan_terms hands these terms to k_scan_pair (pair != 0): an AND of exactly two plain comparisons / intervals on Int64 / Float64 columns, fresh mask
bool scan_pair_applies(const ScanTerms& terms, bool and_existing);
// captured values (per-tile compact) -> the output column: out[prefix[tile] + k] = cap[tile*1024 + k]
void launch_compact_captured(hipStream_t s, const uint64_t* cap, const uint64_t* prefix, uint64_t* out, int64_t nrows, int64_t out_cap);
// the same with the transform of launch_gather_transform applied to the captured values (their column's dtype: Int64 / UInt64 / Float64)
void launch_compact_captured_transform(hipStream_t s, const uint64_t* cap, const uint64_t* prefix, int32_t src_dtype, const ScanTerm& tf, uint64_t* out, int64_t nrows, int64_t out_cap);

// ---- tile-count scan: u32 counts[ntiles] -> u64 prefix[ntiles+1] (prefix[ntiles] = total) -------
// scratch: >= (ceil(ntiles/4096)+1) * 8 bytes
// carry_in/carry_out (device, optional): continue the scan of the previous piece of the same column
void launch_scan_counts(hipStream_t s, const uint32_t* counts, uint64_t* prefix, int64_t ntiles, uint64_t* scratch,
                        const uint64_t* carry_in = nullptr, uint64_t* carry_out = nullptr);
size_t scan_counts_scratch_bytes(int64_t ntiles);

// ---- range stages (selection.jl:94-111 on the packed mask) --------------------------------------
struct RangeSpec {
  int32_t kind;        // 0 = a:s:b (first/last/step normalised ascending), 1 = sorted unique index list
  int64_t first, last, step;
  const int64_t* sorted; int64_t nsorted;
};
// implicit_ones: the incoming mask is all ones and rank = rank_base + local row + 1 (a leading range stage);
// otherwise rank = rank_base + prefix[tile] + position among the survivors.
void launch_range_stage(hipStream_t s, const RangeSpec& r, uint64_t* bitmap, const uint64_t* prefix, uint32_t* tile_counts,
                        int64_t nrows, int64_t rank_base, bool implicit_ones);
// ismissing(col) / !ismissing(col): the column's missing bitmap (words padded like the selection bitmap) is the mask
void launch_missing_mask(hipStream_t s, const uint64_t* missing, bool negate, bool and_existing, uint64_t* bitmap, uint32_t* tile_counts, int64_t nrows);
// all-ones mask (empty SelectionQueue): bitmap + counts
void launch_fill_ones(hipStream_t s, uint64_t* bitmap, uint32_t* tile_counts, int64_t nrows);

// ---- K2: bitmap -> ascending 1-based row numbers -------------------------------------------------
// store (ctx option "compact_store"): 0 / 1 / 2 = one ctile per wave step, plain / nontemporal / write-through 8-byte stores (round 2: 1);
// 3 / 4 = wide: two ctiles per wave, nontemporal / plain 16-byte stores (round 3 default: 3); 5 / 6 = wide with 4 KB of LDS per wave.
// grid_cap (ctx option "compact_grid_cap"; wide forms): most workgroups launched, 0 = the shipped 65 536
void launch_compact_indices(hipStream_t s, const uint64_t* bitmap, const uint64_t* prefix, int64_t* out, int64_t nrows,
                            int64_t row_base, int64_t out_cap, int store = 3, int grid_cap = 0);
// ---- K3: projection gather of a fixed-width column (width 1,2,4,8 bytes) -------------------------
void launch_gather(hipStream_t s, const uint64_t* bitmap, const uint64_t* prefix, const void* src, void* dst, int width,
                   int64_t nrows, int64_t out_cap);
// K3 with a column transform (ScanTerm::pre = 1..4: rem / col * k + d / col / k) applied to the gathered values; dst holds 8-byte results (Int64 or Float64)
void launch_gather_transform(hipStream_t s, const uint64_t* bitmap, const uint64_t* prefix, const void* src, int32_t src_dtype, const ScanTerm& tf, void* dst,
                             int64_t nrows, int64_t out_cap);
// bitmap (1 = missing) of the source gathered into one byte per selected row
void launch_gather_bits(hipStream_t s, const uint64_t* bitmap, const uint64_t* prefix, const uint64_t* srcbits, uint8_t* dst,
                        int64_t nrows, int64_t out_cap);

// ---- synthetic generators --------------------------------------------------------
void launch_gen_i64_mod1m(hipStream_t s, int64_t* out, uint64_t seed, int64_t row_first, int64_t n);
void launch_gen_i64_iota(hipStream_t s, int64_t* out, int64_t row_first, int64_t n);
void launch_gen_f64_u2000(hipStream_t s, double* out, uint64_t seed, int64_t row_first, int64_t n);
void launch_gen_brand_sizes(hipStream_t s, int32_t* sizes, uint64_t seed, int64_t row_first, int64_t n, bool with_missing = false);
void launch_gen_brand_bytes(hipStream_t s, const int32_t* sizes, const int64_t* tile_off, uint8_t* bytes, uint64_t seed,
                            int64_t row_first, int64_t n);

// ---- strings (K4-K6) -------------------------------------------------------------------------------
struct StrSide { const int32_t* sizes; const int64_t* tile_off; const uint8_t* bytes; };   // a String column on the device: int32 sizes, u64 byte offset per tile, arena
// per-1024-row byte totals of max(size,0)  (first half of unsafe_remake_offsets!)
void launch_str_tile_bytes(hipStream_t s, const int32_t* sizes, uint32_t* tile_bytes, int64_t nrows, uint32_t* max_tile_bytes = nullptr);   // (max: one zeroed device word)
// K5: s OP "const" (EQ / NE / STARTSWITH / ENDSWITH) -> bitmap + counts.  mode: 0 EQ, 1 NE, 2 STARTSWITH, 3 ENDSWITH
// StrPattern: host — the pattern in host memory (<= 64 bytes travel as kernel arguments); dev — device copy for longer ones
struct StrCapture { int32_t* sizes; uint8_t* bytes; uint32_t* tile_bytes; };   // K5 CAP outputs (see k_str_match_short)
// the form launch_str_match takes: patterns above 64 bytes run k_str_match; shorter ones k_str_match_short, staged through LDS when every tile of the column
// fits the 8 KB a wave stages (+ 15 bytes below the tile's first, + 16 behind its last), with direct probes otherwise (and for the empty pattern, which reads nothing)
constexpr uint32_t kStrStageBytes = 8192;
enum StrMatchForm { STR_MATCH_STAGED = 0, STR_MATCH_DIRECT = 1, STR_MATCH_LONG = 2 };
inline StrMatchForm str_match_form(int32_t patlen, uint32_t max_tile_bytes) {
  if (patlen > 64) return STR_MATCH_LONG;
  return patlen > 0 && max_tile_bytes > 0 && max_tile_bytes + 48u <= kStrStageBytes ? STR_MATCH_STAGED : STR_MATCH_DIRECT;
}
struct StrPattern { const uint8_t* host; const uint8_t* dev; int32_t len; };
void launch_str_match(hipStream_t s, const StrSide& a, const StrPattern& pat, int mode, uint64_t* bitmap, uint32_t* tile_counts, int64_t nrows, bool and_existing,
                      const StrCapture* cap = nullptr, uint32_t max_tile_bytes = 0);   // max_tile_bytes: Column::max_tile_bytes (0 = not known: probes straight from memory)
// K5b: s1 OP s2 (CmpOp) over two String columns -> bitmap + counts; a row with a missing side (size -1) selects nothing
void launch_str_pair(hipStream_t s, const StrSide& a, const StrSide& b, int op, uint64_t* bitmap, uint32_t* tile_counts, int64_t nrows, bool and_existing);
void launch_str_compact_captured(hipStream_t s, const StrCapture& cap, const uint64_t* prefix, const int64_t* tile_off, const uint64_t* out_tile_off,
                                 int32_t* out_sizes, uint8_t* out_bytes, int64_t nrows, int64_t out_rows, int64_t out_bytes_cap);
// K6: the selected rows of String column `a` -> out sizes (+ per-ctile selected byte totals); then bytes.  StrFill says what stands behind a missing row
// (size -1) of a: nothing (the plain projection, -1 goes out), a constant (const_dev: clen bytes and 8 of padding, read by the bytes pass only) or row i of a
// second column b: coalesce(a, b).  One kernel pair in three forms (k_strings.hip)
enum StrFillKind { STR_FILL_NONE = 0, STR_FILL_CONST = 1, STR_FILL_COL = 2 };
struct StrFill { StrFillKind kind; StrSide b; const uint8_t* const_dev; int32_t clen; };
void launch_str_gather_sizes(hipStream_t s, const uint64_t* bitmap, const uint64_t* prefix, const StrSide& a, const StrFill& fill, int32_t* out_sizes,
                             uint32_t* sel_tile_bytes, int64_t nrows, int64_t out_cap);
void launch_str_gather_bytes(hipStream_t s, const uint64_t* bitmap, const StrSide& a, const StrFill& fill, const uint64_t* out_tile_off, uint8_t* out_bytes,
                             int64_t nrows, int64_t out_bytes_cap);

// K13 (k_str_rows.hip): String column `col` at the 1-based table rows rows[0 .. n), in that order (any order, repeats allowed): sizes pass, scan, bytes pass.
// A row's bytes start at tile_off[its tile] + the bytes of the tile's rows before it, and that in-tile prefix comes in two forms:
//   offsets  launch_str_row_offsets first leaves row_off[nrows] (u32), the sizes pass gathers row_off[r]:  8 B per COLUMN row + 4 B per output
//   direct   one wave per output sums the sizes of the tile's rows before r:                                at most 4 KB per OUTPUT
// str_gather_form is the rule: direct when n * 512 <= nrows, which is where the direct form's worst-case bytes (4 KB * n) equal the build's (8 B * nrows).  The
// constant is derived from those bytes, not from a measurement.  Measured (profiles/str_gather_rows.txt, 5e8 rows of short strings): the forms cross at
// n = rows / 281, 1.82 x away — within the factor of 2 inside which the derived constant stays.  forced: ctx option "str_gather_form"
// (1 = offsets, 2 = direct, anything else = the rule).  STR_GATHER_LAYOUT is the sizes pass that writes neither sizes nor offsets: the byte totals alone.
enum StrGatherForm : int { STR_GATHER_LAYOUT = 0, STR_GATHER_OFFSETS = 1, STR_GATHER_DIRECT = 2 };
constexpr int64_t kStrGatherDirectRatio = 512;
inline StrGatherForm str_gather_form(int64_t n, int64_t nrows, int64_t forced = 0) {
  if (forced == STR_GATHER_OFFSETS || forced == STR_GATHER_DIRECT) return (StrGatherForm)forced;
  return n <= nrows / kStrGatherDirectRatio ? STR_GATHER_DIRECT : STR_GATHER_OFFSETS;      // (n * 512 <= nrows, without the product)
}
// the per-1024-output byte totals are 32-bit and the outputs of a group may all name the longest row: a column whose largest TILE holds this much or more is refused
constexpr uint32_t kStrGatherMaxTileBytes = 1u << 22;
struct StrRows { const int64_t* rows; int64_t n; StrSide col; int64_t row_base, nrows; uint32_t* flag; };   // flag: raised (vector atomic OR) by a row outside [0, nrows), which writes nothing
void launch_str_row_offsets(hipStream_t s, const int32_t* sizes, uint32_t* row_off, int64_t nrows);
// out_sizes[i] = sizes[r_i], src_off[i] = the arena offset of row r_i (both not in the LAYOUT form), grp_bytes[g] = the bytes of outputs [1024 g, 1024 (g + 1))
void launch_str_rows_sizes(hipStream_t s, const StrRows& R, StrGatherForm form, const uint32_t* row_off, int32_t* out_sizes, int64_t* src_off, uint32_t* grp_bytes);
// out_off: launch_scan_counts of grp_bytes; nothing is stored at or beyond out_bytes + out_cap
void launch_str_rows_bytes(hipStream_t s, const int32_t* out_sizes, const int64_t* src_off, int64_t n, const uint8_t* arena, const uint64_t* out_off, uint8_t* out_bytes,
                           int64_t out_cap);

// n rows that all hold the same string: sizes[i] = plen, bytes = the pattern (device memory) n times
void launch_fill_const_strings(hipStream_t s, int32_t* out_sizes, uint8_t* out_bytes, int64_t n, const uint8_t* pat_dev, int32_t plen);

// ---- K9: dictionary codes of a low-cardinality String column (k_dict.hip) ------------------------------
struct DictSlot { uint64_t key8; uint32_t len, code, off, pad; };      // open addressing; len = 0xffffffff: empty.  key8 = the first min(len, 8) bytes
struct DictMiss {                                                     // rows whose string is not in the table yet report here
  unsigned long long* count; unsigned long long* bytes_used;          // rows reported in all; bytes of `arena` handed out
  uint32_t* rec_off; int32_t* rec_len; uint8_t* arena;                // per reported row (the first max_records): its bytes in the arena (len -1: no room, -2: too long)
  int64_t max_records, bytes_cap; int32_t max_len;
};
uint64_t dict_hash_host(uint64_t key8, uint32_t len);
void launch_dict_encode(hipStream_t s, const StrSide& a, const DictSlot* slots, uint32_t nslots, const uint8_t* dict_bytes, uint16_t* codes, int64_t nrows, const DictMiss& miss);
// lut: one bit per code, 1 = the row is selected; lut_words = ceil(entries / 32) <= 2048
void launch_dict_scan(hipStream_t s, const uint16_t* codes, const uint32_t* lut, int32_t lut_words, uint64_t* bitmap, uint32_t* tile_counts, int64_t nrows,
                      bool and_existing);
// two dictionary columns compared: each side's rank gives every one of its n codes its rank in the bytewise sorted union of the two dictionaries (equal strings, equal rank)
struct DictSide { const uint16_t* codes; const uint32_t* rank; int32_t n; };
void launch_dict_pair(hipStream_t s, const DictSide& a, const DictSide& b, int op, uint64_t* bitmap, uint32_t* tile_counts, int64_t nrows, bool and_existing);
// the projection of a dictionary column over n selected rows whose codes K3 has compacted: sizes + per-1024-output-row byte totals, then the bytes
void launch_dict_expand_sizes(hipStream_t s, const uint16_t* codes, int64_t n, const int32_t* dict_len, int32_t* out_sizes, uint32_t* out_tile_bytes);
void launch_dict_expand_bytes(hipStream_t s, const uint16_t* codes, int64_t n, const int32_t* dict_len, const uint32_t* dict_off, const uint8_t* dict_bytes,
                              const uint64_t* out_tile_off, uint8_t* out_bytes, int64_t out_bytes_cap);

// ---- reductions ------------------------------------------------------------------------------------
// sum/min/max of a fixed-width column over the selected rows -> partials then final (2 launches)
void launch_reduce(hipStream_t s, const uint64_t* bitmap, const void* col, int32_t dtype, int op, int64_t nrows, void* partials,
                   void* result /* 16 bytes: i64/u64 or f64 result + count */);
size_t reduce_scratch_bytes();

// ---- K11: order statistics by radix select (k_select.hip) -------------------------------------------
// One pass: per group g < ngroups, the histogram of key bits [shift, shift + 8) over the selected, non-missing rows whose key bits above them equal
// prefix[g] (distinct prefixes), added to hist[g * 256 + digit]; first: also the counts {not missing, missing, NaN} of the selected rows, added to
// counts[0 .. 3).  Both are 64-bit counters the caller zeroes; ngroups = 0 with first counts only.
// full: the key is the 64-bit order image (select_key_bits = 64) instead of the same order in the column's own width.
constexpr int kSelectMaxRanks = 16;
struct SelectPass { uint64_t prefix[kSelectMaxRanks]; int32_t ngroups; int32_t shift; int32_t first; };
void launch_select_hist(hipStream_t s, const uint64_t* bitmap, const uint32_t* tile_counts, const ColRef& col, bool full,
                        int64_t nrows, const SelectPass& P, uint64_t* hist /* [kSelectMaxRanks * 256] */, uint64_t* counts /* [3] */);
// (select_key_bits, the number of key bits of a dtype: select_key.hpp)
uint64_t select_key_value(int dtype, bool full, uint64_t key);      // a finished key -> the value's 64 accumulator bits (integers widened, floats as Float64)

// ---- K12: stable sortperm of the selected rows by radix sort, and the gather that follows a row list (k_sort.hip) ------------------
// The build: every selected row that is not missing and that `keep` admits becomes a pair {key ^ flip, 0-based row} at live_base[tile] + its rank among the
// tile's kept rows (live_base: the selection's own prefix when every selected row is kept, else the scan of the count phase's live_cnt); every selected
// missing row goes to miss_rows at miss_base[tile] + its rank (null: the column has no missing bitmap).  The write phase adds the kept keys' per-byte
// histograms to ghist[byte * 256 + digit] (64-bit counters the caller zeroes).  The count phase fills live_cnt / miss_cnt [tiles] (zeroed by the caller).
enum SortKeep : int { SORT_KEEP_ALL = 0, SORT_KEEP_CUT = 1 /* key ^ flip <= cut */, SORT_KEEP_NONE = 2 };
struct SortBuild {
  const uint64_t* bitmap; const uint32_t* tile_counts; int64_t nrows;
  const uint64_t* live_base; const uint64_t* miss_base;
  uint64_t flip, cut; int32_t keep;
  uint64_t* keys; uint32_t* rows; int64_t cap; uint32_t* miss_rows; int64_t miss_cap;
  uint32_t* live_cnt; uint32_t* miss_cnt;
  unsigned long long* ghist;
};
void launch_sort_build(hipStream_t s, const ColRef& col, const SortBuild& B, bool count_phase);
// The build that starts from a row order (the next key of a sort by several columns): order[0 .. n) holds 0-based rows; every entry whose row is not
// missing in `col` becomes a pair {key ^ flip, row}, every other one goes to miss_rows, both IN THE ORDER OF `order`: entry i of 1024-entry tile t lands at
// live_base[t] (miss_base[t]) + its rank among the tile's live (missing) entries.  live_base null: the column has no missing bitmap and tile t starts at
// t * 1024 (entry i becomes pair i, one launch).  The count phase fills live_cnt / miss_cnt [ceil(n / 1024)]; the write phase adds to ghist like the build
struct SortRekey {
  const uint32_t* order; int64_t n; int64_t nrows;
  const uint64_t* live_base; const uint64_t* miss_base;
  uint64_t flip;
  uint64_t* keys; uint32_t* rows; int64_t cap; uint32_t* miss_rows; int64_t miss_cap;
  uint32_t* live_cnt; uint32_t* miss_cnt;
  unsigned long long* ghist;
};
void launch_sort_rekey(hipStream_t s, const ColRef& col, const SortRekey& R, bool count_phase);
// The rekey over a flat String column: ONE 8-byte sub-key of it per launch.  A String key orders as the tuple (chunk_0, .., chunk_{m-1}, length) of such
// sub-keys (isless on Strings: bytes unsigned, the shorter of two that tie is smaller):  chunk >= 0: bytes [8 chunk, 8 chunk + 8) of the row's string read
// big-endian, zero beyond its end (a row of at most 8 chunk bytes loads nothing from the arena);  chunk < 0: the row's byte length, and the write phase also
// leaves the largest live length in *max_len (a zeroed word; one vector atomic max per wave).  A row whose size is negative is missing.  row_off: the in-tile
// byte offset of every row of the column (launch_str_row_offsets).  Positions, phases, guards and ghist (8 key bytes) as SortRekey's
struct SortStrKey {
  const uint32_t* order; int64_t n; int64_t nrows;
  const uint64_t* live_base; const uint64_t* miss_base;
  uint64_t flip; int32_t chunk;
  uint64_t* keys; uint32_t* rows; int64_t cap; uint32_t* miss_rows; int64_t miss_cap;
  uint32_t* live_cnt; uint32_t* miss_cnt;
  unsigned long long* ghist;
  uint32_t* max_len;
};
void launch_sort_strkey(hipStream_t s, const StrSide& col, const uint32_t* row_off, const SortStrKey& R, bool count_phase);
// order[live_base[tile] + rank] = the 0-based selected rows, ascending (the build's placement without a key): the order a String key that is the most minor
// key of a call starts from.  live_base: the selection's own per-tile scan; nothing is written at or beyond cap
void launch_sort_rows(hipStream_t s, const uint64_t* bitmap, const uint32_t* tile_counts, const uint64_t* live_base, int64_t nrows, uint32_t* order, int64_t cap);
void sort_geometry(int64_t out[2]);                  // {pairs per chunk of a pass, threads per workgroup}
int64_t sort_chunks(int64_t npairs);
// one pass over key bits [shift, shift + 8): counts [256 * sort_chunks(n)] bin-major, their exclusive scan `starts` (launch_scan_counts), the stable scatter
void launch_sort_count(hipStream_t s, const uint64_t* keys, int64_t n, int shift, uint32_t* counts);
void launch_sort_scatter(hipStream_t s, const uint64_t* keys_in, const uint32_t* rows_in, int64_t n, int shift, const uint64_t* starts, uint64_t* keys_out, uint32_t* rows_out);
void launch_sort_emit(hipStream_t s, const uint32_t* rows, int64_t n, int64_t* out, int64_t row_base);      // out[i] = row_base + rows[i] + 1
// out[i] = col[rows[i] - 1 - row_base], mout[i] = that row's missing bit (mout null: none wanted); a row outside [0, nrows) raises *flag and writes nothing
void launch_gather_rows(hipStream_t s, const int64_t* rows, int64_t n, const void* col, int width, void* out, const uint64_t* missing, uint8_t* mout, int64_t row_base,
                        int64_t nrows, uint32_t* flag);

// ---- K14: the row lists of a join of two selections on one fixed-width key (k_join.hip; the rules: join_rule.hpp) ---------------------------------
// The probe: order[0 .. nl) holds the selected left rows (0-based, ascending: launch_sort_rows); rkeys[0 .. nr) the right side's select keys, ascending (the
// sorted pairs of k_sort.hip).  Entry i gets lo[i] = the right keys below its key and cnt[i] = the right keys equal to it; a left row whose key is missing, and
// every entry of the last 1024-entry group at or beyond nl, gets cnt = 0 (lo and cnt hold groups * 1024 entries).  grp_total[g] = the sum of
// join_emitted(kind, cnt) over the group's entries below nl; a sum of 2^32 or more raises *flag.  *nmiss (zeroed) += the left rows whose key is missing.
// steps = join_search_steps(nr)
struct JoinProbe {
  const uint32_t* order; int64_t nl; int64_t nrows;
  const uint64_t* rkeys; uint32_t nr; int32_t steps; int32_t kind;
  uint32_t* lo; uint32_t* cnt; uint32_t* grp_total;
  unsigned long long* nmiss; uint32_t* flag;
};
void launch_join_probe(hipStream_t s, const ColRef& col, const JoinProbe& P);
// The expand: the pairs of entry i start at out_base[i / 1024] (launch_scan_counts of grp_total) + the pairs of the group's entries before it.  Pair k of an
// entry: left_rows = lbase + order[i] + 1, right_rows = cnt ? rbase + rrows[lo + k] + 1 : 0 (rrows: the sorted pairs' rows; right_rows null: not written).
// Nothing is stored at or beyond cap
struct JoinExpand {
  const uint32_t* order; const uint32_t* lo; const uint32_t* cnt; int64_t nl;
  const uint64_t* out_base; const uint32_t* rrows; int32_t kind;
  int64_t lbase, rbase; int64_t* left_rows; int64_t* right_rows; int64_t cap;
};
void launch_join_expand(hipStream_t s, const JoinExpand& E);

// ---- K14c: the join on several keys, String keys among them (dfdb_query_join_n; k_join.hip; the rules: join_rule.hpp) -----------------------------
// Which entries of a row order have a missing component: per NULLABLE key one of a missing bitmap (a fixed-width column) or the sizes of a String column
// (negative: missing); keys that cannot be missing are not listed.  The bytes under a missing row are never read
constexpr int kJoinMaxKeys = 8;
struct JoinKeyMiss { const uint64_t* missing[kJoinMaxKeys]; const int32_t* sizes[kJoinMaxKeys]; int32_t n; };
// One walk over order[0 .. n) (0-based rows; a row that is not < nrows counts as missing: a guard), one wave per 1024 entries, in three modes:
//   COUNT  live_cnt[tile] = the tile's entries without a missing component
//   PLACE  those entries' rows, in the order of `order`, to out[live_base[tile] + rank in the tile]  (live_base: launch_scan_counts of live_cnt; nothing at or
//          beyond cap)
//   START  the left side's first ranges: lo[i] = 0 and cnt[i] = nr for such an entry, cnt[i] = 0 for every other one and for the entries of the last tile at or
//          beyond n (lo and cnt hold tiles * 1024 entries); *nmiss (zeroed) += the entries below n with a missing component, each once
enum JoinLiveMode : int { JOIN_LIVE_COUNT = 0, JOIN_LIVE_PLACE = 1, JOIN_LIVE_START = 2 };
struct JoinLive {
  const uint32_t* order; int64_t n; int64_t nrows; JoinKeyMiss keys;
  uint32_t* live_cnt; const uint64_t* live_base; uint32_t* out; int64_t cap;
  uint32_t* lo; uint32_t* cnt; uint32_t nr; unsigned long long* nmiss;
  uint32_t* grp_total; uint32_t emit0;               // START, not null (no stage follows: nr = 0): grp_total[tile] = the tile's entries below n times emit0
};
void launch_join_live(hipStream_t s, const JoinLive& L, JoinLiveMode mode);
// One refinement stage (join_rule.hpp join_refine_stage): entry i < nl with cnt[i] > 0 loads x, the sub-key of left row order[i], and narrows its run of
// rsub — the stage's sub-keys of the right rows in tuple order — to the sub-keys equal to x: lo[i] += #{< x}, cnt[i] = #{= x} within [lo, lo + cnt).  An entry
// with cnt = 0 and every entry at or beyond nl writes cnt = 0; a wave whose 1024 entries all have cnt = 0 loads no key and takes no step; the step count is
// the bit length of the wave's largest cnt.  last: grp_total[g] = the sum of join_emitted(kind, cnt) over the group's entries below nl, and a sum of 2^32 or
// more raises *flag — as the probe leaves them.  The left sub-key: a fixed-width column's select key, or (JoinStrSub) a String column's chunk / length
// (chunk < 0) through its sizes, in-tile offsets (launch_str_row_offsets) and tile offsets
struct JoinRefine {
  const uint32_t* order; int64_t nl; int64_t nrows;
  const uint64_t* rsub;
  uint32_t* lo; uint32_t* cnt;
  int32_t last, kind; uint32_t* grp_total; uint32_t* flag;
};
struct JoinStrSub { StrSide col; const uint32_t* row_off; int32_t chunk; };
void launch_join_refine(hipStream_t s, const ColRef& col, const JoinRefine& P);
void launch_join_refine_str(hipStream_t s, const JoinStrSub& K, const JoinRefine& P);

// ---- the control words of unique / groupreduce: 128 bytes of device memory through which the kernels of k_unique.hip and k_radix.hip report to the host, which
// reads every retry decision from them.  The host sets them with device memsets (all zero, then all ones where a field says so) and reads them back whole.
// KeyAux is the head every form shares — all the radix kernels and the `special` pointers of AccArgs / RankArgs see —, UniqueAux what unique's table and dense
// forms lay behind it, RadixGroupAux what groupreduce by radix lays there instead.  The static_asserts below are the layout.
enum SpecialRow : int { SPECIAL_UNSTORABLE = 0, SPECIAL_MISSING = 1 };
struct KeyAux {
  // the two keys no table holds: [SPECIAL_UNSTORABLE] the key whose image is all ones (the tables' "empty"), [SPECIAL_MISSING] the missing key.  All ones before
  // a pass: no such row; the insert / presence / partition passes lower a word (atomicMin) to the smallest selected row that holds the key; the group-number
  // kernels (k_group_ids, k_dense_group_ids) then replace a row by its group's number, which is what AccArgs::special / RankArgs::special read
  uint64_t special_row[2];
  uint64_t claims;      // hash table: the slots claimed since the host last cleared it (every reset; before a migration, which counts them again).  Zero for the other forms
  // raised (1) by a pass that cannot finish with the table it was given, cleared by the host before every pass that may raise it: an insert whose probe sequence got too
  // long (the host grows the table and repeats the chunk), a partition that outgrew its pages or its LDS table (the host falls back to the hash table), and — as
  // AccArgs::unknown_flag, or String pass 3 — a selected row whose key the table, filled from a prefix of the rows only, does not hold (everything again over every row)
  uint64_t abort;
};
struct UniqueAux {
  KeyAux head;
  uint64_t collision;     // String keys: two different strings shared a key (the host: again under the next salt).  An int: the String pass raises the low 32 bits through an int*.  Cleared by the reset only
  // the dense form (integer keys of a small range), zero after the reset unless said otherwise:
  uint64_t outside;       // k_dense_presence: a selected key lies outside [lo, lo + range)
  uint64_t distinct;      // k_dense_count: the presence bits set
  uint64_t found;         // k_dense_first: the values whose first row is known
  uint64_t min_image;     // k_dense_minmax: the smallest selected key as an order-preserving image (all ones after the reset) ...
  uint64_t max_image;     // ... and the largest
  uint64_t found_before;  // k_dense_snap: `found` as the launches before the current k_dense_first left it
  uint64_t span_lo;       // k_dense_count: the smallest value index whose presence bit is set (all ones after the reset) ...
  uint64_t span_hi;       // ... and the largest
  uint64_t reserved[3];
};
struct RadixGroupAux {
  KeyAux head;            // (claims stays zero)
  uint64_t gspec[4];      // {rows, value} of the unstorable key's group, then of the missing key's: added up by the partition pass (a minimum starts at all ones), read by the finish
  uint64_t nres;          // the results the table pass wrote; the kernels use the low 32 bits
  uint64_t reserved[7];
};
static_assert(sizeof(KeyAux) == 32 && offsetof(KeyAux, special_row) == 0 && offsetof(KeyAux, claims) == 16 && offsetof(KeyAux, abort) == 24, "words 0-3");
static_assert(sizeof(UniqueAux) == 128 && offsetof(UniqueAux, head) == 0 && offsetof(UniqueAux, collision) == 32 && offsetof(UniqueAux, outside) == 40 &&
              offsetof(UniqueAux, distinct) == 48 && offsetof(UniqueAux, found) == 56 && offsetof(UniqueAux, min_image) == 64 && offsetof(UniqueAux, max_image) == 72 &&
              offsetof(UniqueAux, found_before) == 80 && offsetof(UniqueAux, span_lo) == 88 && offsetof(UniqueAux, span_hi) == 96, "words 4-12");
static_assert(sizeof(RadixGroupAux) == 128 && offsetof(RadixGroupAux, head) == 0 && offsetof(RadixGroupAux, gspec) == 32 && offsetof(RadixGroupAux, nres) == 64, "words 4-8");

// ---- unique(col) as a selection of first occurrences (k_unique.hip: a hash table of {key, smallest row}, or — integer keys of a small range — the dense form)
struct UniqueEntry { uint64_t key, row; };
void launch_unique_insert(hipStream_t s, const uint64_t* bitmap, const ColRef& key, int64_t row0, int64_t row1, UniqueEntry* ent, uint64_t mask, UniqueAux* aux);
void launch_unique_mark(hipStream_t s, uint64_t* bitmap, uint32_t* tile_counts, const ColRef& key, int64_t nrows, const UniqueEntry* ent, uint64_t mask, const UniqueAux* aux);
void launch_unique_migrate(hipStream_t s, const UniqueEntry* from, const uint64_t* from_off, const uint32_t* from_len, uint64_t from_cap, UniqueEntry* ent,
                           uint64_t* rep_off, uint32_t* rep_len, uint64_t mask, UniqueAux* aux);
void launch_unique_scatter(hipStream_t s, const UniqueEntry* ent, uint64_t cap, const UniqueAux* aux, uint64_t* bitmap, uint32_t* tile_counts);
// the hash table of a flat String key: a slot's key is the salted hash of the string, rep_off / rep_len say where one holder's bytes lie (the representative)
struct StrTable { UniqueEntry* ent; uint64_t* rep_off; uint32_t* rep_len; uint64_t mask; UniqueAux* aux; uint64_t salt; };
// pass 0: insert the tiles [tile0, tile1), 1: verify (3: the table may not hold every string), 2: mark
void launch_unique_str(hipStream_t s, int pass, uint64_t* bitmap, uint32_t* tile_counts, const StrSide& key, int64_t nrows, int64_t tile0, int64_t tile1, const StrTable& tab);
// radix-partitioned form of the hash-table unique (k_radix.hip): partition into a pool of pages -> one LDS table per partition.  false: the launch is
// not possible or refused (LDS attribute refused, too many partition bits, a launch error): the caller stays with the hash table.  The pool: `front` [2^kbits x radix_share()] running
// positions of the streams (zero before the pass), `pt` [2^kbits x radix_share()][maxv] the streams' pages (all ones before the pass), `next_page` the pool's
// counter (zero), `dump_page` the page nobody owns (radix_pool_pages() - 1); the records' buffer holds radix_pool_record_bytes().
struct RadixPool { uint32_t* front; uint32_t* pt; uint32_t* next_page; uint32_t maxv; uint32_t dump_page;
                   uint64_t* hot /* [hot_cap x 3]: the hot keys' list {key, value, rows << 32 | first row}: chunks x radix_hot_slots() entries */; uint32_t* hot_n /* zero before */; uint32_t hot_cap; };
struct RadixGrid { int kbits; int chunks; };      // 2^kbits partitions; `chunks` workgroups share the rows (a multiple of radix_share())
int64_t radix_rows_per_chunk(int64_t nrows, int chunks);
int radix_share();
int64_t radix_pool_pages(int64_t cnt, int kbits);
int64_t radix_pool_record_bytes(int64_t cnt, int kbits, bool with_values);
int radix_group_slots();
uint32_t radix_pool_maxv(int64_t cnt, int kbits);
bool launch_radix_sample(hipStream_t s, const uint64_t* sel, const ColRef& key, int64_t nrows, const RadixGrid& grid, int step, uint32_t* counts /* [2^kbits], zero before */);
// groupreduce by radix: the records carry the row's 8-byte value (val; no column: count only); gop 0 count only, 1 wrapping integer sum, 2 double sum, 3 min, 4 max
// (of order images: vkind 0 signed, 1 unsigned, 2 double); results [<= groups] {first row, rows, value} + their count nres; gspec {rows, value} of the unstorable key
// and of the missing key (their first rows: the head's special_row), both in `aux`
struct RadixGroup { ColRef val; int gop; int vkind; void* results; RadixGroupAux* aux; };
int radix_hot_slots();
bool launch_radix_partition(hipStream_t s, const uint64_t* sel, const ColRef& key, int64_t nrows, const RadixGrid& grid, const RadixPool& pool, uint32_t* recs_out /* 12 bytes per record: key image, row; with a group: 20, + the value */, KeyAux* aux /* with a group: its aux's head */,
                            const RadixGroup* group = nullptr, bool hot = false /* the kernels that keep hot keys out of the records (values narrower than 8 bytes: always) */);
bool launch_radix_group(hipStream_t s, const uint32_t* recs, const RadixPool& pool, int kbits, bool mark, uint64_t* bitmap, uint32_t* tile_counts, const RadixGroup& group, int cus);
void launch_radix_group_finish(hipStream_t s, const RadixGroup& group, const uint64_t* ubits, const uint64_t* uprefix, uint64_t* cnt, uint64_t* val);
bool launch_radix_unique(hipStream_t s, const uint32_t* recs, const RadixPool& pool, int kbits, uint64_t* bitmap, uint32_t* tile_counts, KeyAux* aux, int cus);
int64_t unique_dense_max_range();
bool unique_dense_dtype(int dtype);
void launch_dense_minmax(hipStream_t s, const uint64_t* bitmap, const ColRef& key, int64_t nrows, int64_t tile_step, UniqueAux* aux);
void launch_dense_presence(hipStream_t s, const uint64_t* bitmap, const ColRef& key, int64_t nrows, uint64_t lo, uint32_t range,
                           uint32_t* present, UniqueAux* aux);
void launch_dense_first(hipStream_t s, const uint64_t* bitmap, const ColRef& key, int64_t row0, int64_t row1, uint64_t lo,
                        uint32_t range, uint64_t distinct, uint64_t* first, UniqueAux* aux);
void launch_dense_scatter(hipStream_t s, const uint64_t* first, uint32_t range, const UniqueAux* aux, uint64_t* bitmap, uint32_t* tile_counts);
void launch_dense_group_ids(hipStream_t s, uint64_t* first, uint32_t range, UniqueAux* aux, const uint64_t* ubits, const uint64_t* uprefix);
// K9 (dictionary codes) and groupreduce's group numbers, accumulate passes and finish (k_unique.hip)
void launch_dict_first_rows(hipStream_t s, const uint64_t* sel, const uint16_t* codes, int64_t nrows, uint64_t* first, int dict_n, int64_t tile0, int64_t tile1);
void launch_set_rows(hipStream_t s, const uint64_t* rows, int n, uint64_t* bitmap, uint32_t* tile_counts);
void launch_group_ids(hipStream_t s, UniqueEntry* ent, uint64_t cap, uint64_t* special, const uint64_t* ubits, const uint64_t* uprefix);
// groupreduce's single-reducer accumulate pass: every selected row's value to the accumulators of its key's group.  AccArgs is the kernels' argument (its
// layout is theirs); `src` says which table numbers the groups and which fields beside the common ones are read
struct AccArgs {
  const uint64_t* sel; const void* keycol; int keydt; const uint64_t* missing; const void* valcol; int valdt, op; int64_t nrows;
  const UniqueEntry* ent; uint64_t mask; const uint64_t* special;       // SRC 0 (special: KeyAux::special_row — the groups of the unstorable key and of missing)
  const uint16_t* codes; const uint32_t* rank_of_code;                  // SRC 1
  uint64_t lo; const uint64_t* gids;                                    // SRC 2 (special[SPECIAL_MISSING]: the group of missing)
  uint64_t* cnt; uint64_t* val; int ngroups; uint64_t val_init;
  uint64_t* unknown_flag;                                               // (KeyAux::abort) the LDS forms: raised by a selected row whose key has no group (an optimistic / head-only table)
  void key(const ColRef& k) { keycol = k.data; keydt = k.dtype; missing = k.missing; }
  void value(const ColRef& v) { valcol = v.data; valdt = v.dtype; }
};
enum GroupSrc : int { GROUP_SRC_HASH = 0, GROUP_SRC_CODES = 1, GROUP_SRC_DENSE = 2 };
// what the LDS forms need beside AccArgs.  hash table: gkeys, the groups' 8-byte keys in group order (null: the plain form).  dense table: it spans `range`
// values from A.lo, of which the keys cover [span_lo, span_hi]
struct GroupAccExtra { const void* gkeys; uint32_t range; uint64_t span_lo, span_hi; };
// 1: the form with the groups' table in LDS ran, 0: the plain form, -1: nothing was launched (dense table with A.unknown_flag set — the table was made from
// the head of the column, only the LDS form reports a key without a group, and it cannot take the job: the caller makes the table from every row)
int launch_group_accumulate(hipStream_t s, GroupSrc src, const AccArgs& A, const GroupAccExtra& X);
// flat String keys (k_str_pass): of A the selection, nrows, the value column, op and the outputs are read; the key side is `key` and `tab`
void launch_group_accumulate_str(hipStream_t s, const AccArgs& A, const StrSide& key, const StrTable& tab);
void launch_group_finish(hipStream_t s, uint64_t* val, int64_t ng, int kind, int op);
// groupreduce by a tuple of keys (dfdb_query_groupreduce_n): per selected row of `sel`, the rank of its key out of one of the tables above -> g_out (gprev null)
// or image = gprev[row] * n + rank -> img_out; a rank >= n raises *flag.  src 0: hash table (special = KeyAux::special_row of unique's aux), 1: dictionary codes, 2: the dense form (its table in LDS when the range is small)
struct RankArgs {
  const uint64_t* sel; const void* keycol; int keydt; const uint64_t* missing; int64_t nrows;
  const UniqueEntry* ent; uint64_t mask; const uint64_t* special;
  const uint16_t* codes; const uint32_t* rank_of_code;
  uint64_t lo; uint32_t range; const uint64_t* gids;
  const uint32_t* gprev; uint64_t n; uint32_t* g_out; uint64_t* img_out; uint64_t* flag;
};
bool launch_group_rank(hipStream_t s, int src, const RankArgs& A);
bool launch_group_rank_str(hipStream_t s, const RankArgs& A, const StrSide& key, uint64_t salt);
// one accumulate pass for up to kMaxReducers reducers over the rows' group numbers: cnt [ngroups], val [nvals][ngroups] (min / max as order images until
// launch_group_finish); kind: value_kind (value_rules.hpp) of each value column; a group number >= ngroups raises *flag.  1: LDS form, 0: global form, -1: not launched
constexpr int kMaxReducers = 16;
struct MultiAccArgs {
  const uint64_t* sel; const uint32_t* gid; int64_t nrows; int nvals;
  const void* valcol[kMaxReducers]; int valdt[kMaxReducers], op[kMaxReducers], kind[kMaxReducers];
  uint64_t* cnt; uint64_t* val; int64_t ngroups; uint64_t* flag;
};
int launch_group_accumulate_multi(hipStream_t s, const MultiAccArgs& A);
int64_t group_multi_lds_groups(int nvals);      // the most groups the LDS form holds with nvals reducers

// ---- K7: LZ4 block decode, K8: missing bitmaps, block bodies ---------------------------------------
// (dst: the decoders may READ up to 32 bytes past the end of the last block's output — far-match sources are fetched 24 bytes at a time — so the
//  destination needs that much slack behind it; table.cpp's column arrays and body arenas carry 64-256)
struct Lz4Block {      // one (column, block) unit of work
  int64_t src_off;     // offset of the compressed bytes inside the staged image
  int32_t src_len;     // compressed bytes
  int32_t dst_len;     // expected uncompressed bytes (origin)
  int64_t dst_off;     // where the decoded body goes inside the body arena
};
void launch_lz4_decode(hipStream_t s, const uint8_t* src, uint8_t* dst, const Lz4Block* blocks, int32_t nblocks, int32_t* status,
                       int pipe = -1 /* -1: two waves per block when there are fewer blocks than wave slots, 0: never, 1: always (ctx option "lz4_pipeline") */,
                       uint32_t* index = nullptr, int index_mode = 0 /* 1: record where the sequences start (one bit per byte of src, zeroed by the caller), 2: decode with it */);
bool lz4_decode_takes_index(int32_t nblocks, int pipe);
// K7 fused with the first predicate of a scan (decode -> scan fusion): 8-byte columns whose blocks start on 1024-row tiles
// op2 >= 0: the interval `col OP c & col OP2 c2`; and_existing: the mask already holds survivors — words are AND-ed into it and a block none of whose tiles
// kept a row is not decoded at all; ticket: the history-ring form's block counter (set by its launcher)
struct LzScan { uint64_t* bitmap; uint32_t* counts; uint64_t cbits; int32_t dtype; int32_t op; int32_t op2 = -1; int32_t and_existing = 0; uint64_t cbits2 = 0; uint32_t* ticket = nullptr; };
void launch_lz4_decode_scan(hipStream_t s, const uint8_t* src, uint8_t* dst, const Lz4Block* blocks, int32_t nblocks, int32_t* status, const LzScan& sc,
                            uint32_t* index = nullptr, int index_mode = 0);

// K7 without a decoded column (round 5): what leaves the decoder's LDS ring goes to a 64-KB history ring per resident wave inside `scratch`
// (lz4_hist_scratch_bytes(waves) bytes: a ticket word, then the rings) — all an LZ4 match can reach — never to a column array.  sc != nullptr: the predicate
// term is evaluated on the way (bitmap + tile counts are the only output; 8-byte columns whose blocks start on 1024-row tiles); sc == nullptr: a validating
// decode (statuses, and the sequence-start index when index_mode = 1).  waves: workgroups launched = rings used (0: lz4_hist_default_waves(device CUs)).
size_t lz4_hist_scratch_bytes(int waves);
int lz4_hist_default_waves(int compute_units);
void launch_lz4_decode_hist(hipStream_t s, const uint8_t* src, uint8_t* scratch, int waves, const Lz4Block* blocks, int32_t nblocks, int32_t* status, const LzScan* sc,
                            uint32_t* index = nullptr, int index_mode = 0);

}  // namespace dfdb
