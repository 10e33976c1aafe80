// engine.hpp — host-side objects behind the opaque C-ABI handles.
#pragma once
#include "common.hpp"
#include "expr.hpp"
#include "kernels.hpp"
#include "scan_image.hpp"
#include <functional>
#include <memory>
#include <mutex>

namespace dfdb {

// where the blocks of a column file lie (read_sizes without the bodies: BlockStreams.jl:68-78, header then skip(io, compressed)).  Walked lazily, a
// chunk's worth of headers at a time, and kept with the table's column: a second stream over the same file finds it done.  30 000 headers are 30 000
// preads (~20 ms), which a block-streamed scan of 2e9 rows used to pay before its first byte moved.
struct BlockLoc { int64_t off; int32_t rows; int64_t origin, compressed; };
struct BlockIndex {
  std::string file; size_t data_off = 0;
  int64_t file_size = -1, file_mtime_ns = 0;   // what the file looked like when the walk began (a rewritten file gets a fresh index)
  std::mutex mu;
  std::vector<BlockLoc> v;                     // guarded by mu: readers copy the slice they need
  int64_t next_pos = -1;                       // where the next header lies (-1: not started)
  bool complete = false;
};

// The copies of an Int64 / UInt64 column that lone `col OP const` scans read instead of Column::data (scan_image.cpp builds, routes and drops them; scan_route.hpp is
// the rule; k_image.hip the build kernels).  image: the column truncated to 4 bytes per row in row order with the same 256-byte pad, for a column whose values all
// fit 32 bits; made at the column's second such scan (ctx option "scan_image"), read by those scans from then on: half the bytes.  Holds exactly while `data` holds
// the contents it was made from — whoever releases, refills or re-decodes `data` calls drop_scan_image; a swap of `data` for another allocation with the same contents
// (placement calibration) keeps it.  Never made for a nullable column, one that keeps LZ4 blocks (comp / comp_only / transient), or a stream slot's chunk.  coarse:
// (image - min) >> shift in 2 bytes per row, same pad (scan_coarse.hpp), made right behind the image when ctx option "scan_coarse" allows and there is room.
struct ScanCopies {
  DevBuf image, coarse;
  int state = kImageNone;            // scan_image.hpp
  int64_t scans = 0;                 // single-term scans of this column that could have read an image
  uint32_t min = 0, max = 0;         // the bits of the smallest and largest image value (state == kImageBuilt)
  int32_t shift = 0;                 // the coarse copy's
  std::vector<uint64_t> hist;        // [k]: rows whose coarse value >> 4 is k — what the dense-bucket guard consults (kCoarseHistBins words beside a coarse copy)
  int64_t bytes() const { return (int64_t)image.bytes + (int64_t)coarse.bytes; }   // HBM held: counted under `decoded`, ctx->scan_image_bytes and "hbm_budget_mb"
  void clear() { image.release(); coarse.release(); state = kImageNone; scans = 0; min = max = 0; shift = 0; hist.clear(); }
};

// one column of a table, decoded and resident in HBM as ONE contiguous array over all resident blocks
// (every block holds block_size rows except the last, so block b starts at row b*block_size)
struct Column {
  std::string name;
  int64_t id = 0;
  int32_t dtype = 0;
  std::string logical;   // "Date" / "DateTime" / "Time" / "Char": a bits type carried as its integer representation ("" otherwise)
  bool resident = false;
  int64_t nrows = 0;
  DevBuf data;       // fixed width: nrows*width bytes (+ pad); String: int32 sizes[nrows] (-1 = missing)
  DevBuf bytes;      // String: byte arena (+16 B pad so 8-byte probes never fault)
  int64_t nbytes = 0;
  DevBuf tile_off;   // String: u64[nstrtiles+1] byte offset of each 1024-row tile (K4)
  uint32_t max_tile_bytes = 0;   // String: the most bytes any 1024-row tile holds (K4; K5 stages a tile's bytes in LDS when every tile fits)
  DevBuf missing;    // nullable fixed width: bitmap, 1 = missing, padded like the selection bitmap
  // compressed-resident form (ctx option "keep_compressed" at load time; plain fixed-width columns): the column's LZ4 blocks as they
  // sit in the file stay in HBM with their descriptors, and dfdb_table_decode_resident re-runs K7 from them into `data`
  DevBuf comp, comp_blocks, comp_status;
  int64_t comp_nblocks = 0;
  DevBuf comp_index;            // one bit per byte of comp: where an LZ4 sequence starts (recorded by the first resident decode, read by the later ones)
  int comp_index_state = 0;     // 0: not recorded yet, 1: recorded
  // COMPRESSED-ONLY form (ctx option "keep_compressed" = 2 at load time; round 5): the LZ4 blocks + the index are all the column holds —
  // `data` is empty.  `col OP const` conjuncts are evaluated by the decoder itself (K7 HIST + SCAN: no decoded byte reaches a column array), gathers decode
  // the blocks that kept a row into a per-query arena, and anything else gets a whole-column decode that lives for one ABI call (`transient`).
  bool comp_only = false;
  bool transient = false;       // `data` is such a whole-column decode: released when the ABI call that needed it returns (TransientScope)
  std::vector<Lz4Block> comp_blocks_host;   // the descriptors of comp_blocks, for decoding subsets of the blocks
  // placement calibration (query.cpp: place_mask): the selection bitmap this column's scans run fastest against, found once by timing
  // the scan against a few candidate allocations; lent to one query at a time
  DevBuf mask_pref;
  bool mask_calibrated = false, mask_lent = false;
  float mask_ms_best = 0, mask_ms_worst = 0;   // per scanned sample, for dfdb_ctx_profile / the bench's JSON
  ScanCopies scan;              // its 4-byte scan image and the 2-byte coarse copy beside it (above)
  // dictionary form of a low-cardinality String column (dfdb_table_build_dictionary / ctx option "string_dictionary"; k_dict.hip): one 16-bit code per
  // row beside the flat form, the distinct strings once on the device and on the host (predicates are evaluated on the host copy)
  DevBuf dict_codes, dict_len, dict_off, dict_bytes;
  std::vector<std::string> dict_host;
  int32_t dict_n = 0;           // 0 = no dictionary
  // on-disk source (tables opened from files)
  std::string file;
  size_t data_off = 0;  // first block inside the file
  std::shared_ptr<BlockIndex> bix;   // block locations of `file`, as far as a stream or table_column_stats has walked them
};
// a resident column as the launchers take it (kernels.hpp): a flat String column, a fixed-width column (null: no column — the count-only reducer)
inline StrSide str_side(const Column& c) { return StrSide{c.data.as<int32_t>(), (const int64_t*)c.tile_off.p, c.bytes.as<uint8_t>()}; }
inline ColRef col_ref(const Column& c) { return ColRef{c.data.p, dt_base(c.dtype), dt_nullable(c.dtype) ? c.missing.as<uint64_t>() : nullptr}; }
inline ColRef col_ref(const Column* c) { return c ? col_ref(*c) : ColRef{}; }

enum StageKind { ST_RANGE = 0, ST_INTEGER = 1, ST_INDICES = 2, ST_PRED = 3 };

struct Stage {
  int kind = ST_RANGE;
  int64_t start = 0, step = 1, stop = 0, n = 0;  // ST_RANGE (stop normalised to the last element)
  std::vector<int64_t> idx;                      // ST_INDICES / ST_INTEGER, caller order
  NodePtr pred;                                  // ST_PRED
  int64_t stage_base = 0;                        // survivors on lower ranks (multi-GPU)
  int64_t first() const;                         // minimum (RangeToProcess.first)
  int64_t last() const;                          // maximum (RangeToProcess.last)
  int64_t elem(int64_t k) const;                 // 1-based element with Julia bounds checking
};

struct ProjCol { std::string name; NodePtr expr; };

}  // namespace dfdb

namespace dfdb { struct OocState; }
struct dfdb_query;
struct dfdb_table {
  dfdb_ctx* ctx = nullptr;
  std::string path;            // empty for in-memory tables
  int64_t block_size = 65536;
  int64_t format_version = 1;
  std::vector<dfdb::Column> cols;
  int64_t nrows = -1;          // rows resident (all resident columns agree); -1 = nothing resident yet
  int64_t row_base = 0;        // global 0-based row of local row 0 (block-range shard)
  int64_t block_first = 0;     // first resident block
  // block window of the table's out-of-core streams: a shard of a multi-GPU group that is NOT resident streams only ITS block range [win_first, win_last)
  // of the column files (win_last < 0: to the end of the file); rows keep their table numbers (row_base of a chunk = its first block * block_size)
  int64_t win_first = 0, win_last = -1;
  std::vector<dfdb_query*> queries;   // live queries over this table (orphaned, not dangling, when the table closes)
  // block-loading scratch (compressed bytes staged in HBM, packed bodies, block descriptors).  Freed after a load unless
  // the table is a stream slot that reloads a new block range every few milliseconds (hipMalloc/hipFree would dominate).
  dfdb::DevBuf ld_staged, ld_bodies, ld_blocks, ld_status, ld_aux;
  bool keep_load_scratch = false;
  bool ld_prestaged = false;      // the caller has already queued the image's compressed byte range into ld_staged on this table's stream (stream.cpp)
};

struct dfdb_query {
  dfdb_table* t = nullptr;
  std::vector<dfdb::Stage> stages;
  std::vector<dfdb::ProjCol> proj;
  // device state of the last execution
  dfdb::DevBuf bitmap, tile_counts, prefix, scan_scratch, idx_sorted, red_scratch, red_result, tmp_a, tmp_b, tmp_c,
      str_sizes, str_toff, str_bytes, str_scratch;
  // dfdb_query_hint_materialize: the projection WILL be materialised after the scan, so a single-stage scan of simple terms
  // keeps the selected values of one projected 8-byte predicate column (per-tile compact, cap_buf) and that column's
  // projection becomes a contiguous copy instead of a gather
  bool hint_materialize = false;
  // What the last execution left behind for the projection side and for query_count (query.cpp run_plan writes it, project.cpp and unique.cpp read it):
  // query_execute starts from `Left{}`.  It holds only while the bitmap reflects every stage: consumers ask reflects_all_stages(q) first.  The device
  // buffers the entries speak of (cap_buf, cap_buf2, cap_str_*, agg_partials) are members of the query itself, so a reset frees nothing.
  struct Left {
    int cap_col = -1;            // table ordinal captured by the scan (k_scan_terms EX_CAPTURE / k_scan_cmp), in cap_buf (-1: none)
    int cap_col2 = -1;           // a second captured column (EX_CAPTURE2: the term before the last), in cap_buf2
    // a projected String column filtered by ONE short-pattern string term (K5 CAP): sizes per tile, bytes at the tile's arena offset, selected byte
    // totals per tile in cap_str_sizes / cap_str_bytes / cap_str_tb
    int cap_str_col = -1;
    // a conjunct `strcol == "const"` of some stage holds for every finally selected row: the projection of that column is `const` repeated
    int const_str_col = -1; std::string const_str;
    int agg_col = -1;            // table ordinal whose per-tile sums / minima / maxima agg_partials holds (-1: none)
    int agg_dtype = 0, agg_op = 0;
    int decoded_col = -1;        // table ordinal whose resident LZ4 blocks the execution decoded on its way (decode_on_scan; -1: none)
    std::vector<int> comp_scanned;   // compressed-only columns whose blocks it decoded inside its scan (their statuses are read with the count)
  } left;
  dfdb::DevBuf cap_buf2;
  // compressed-only projection columns: the blocks that kept a row, decoded for THIS query's gathers at their natural offsets inside the span
  // [first such block, last such block] — the iterator owns its decode buffers, like the reference's (blocksiterator.jl:98-121)
  struct Arena { dfdb::DevBuf buf, blocks, status; int64_t first_row = 0; int64_t nblocks = 0; bool valid = false; const void* from = nullptr; };   // from: the blocks (Column::comp) it was decoded out of
  std::map<int, Arena> arenas;
  dfdb::DevBuf cap_buf;
  // dfdb_query_hint_aggregate: sum(projection column) WILL be asked for: when that column is a simple term of the launch that produces
  // the final mask, the scan adds up the selected values while it holds them (one partial per 1024-row tile) and dfdb_aggregate only
  // reduces the partials
  int hint_agg_op = 0, hint_agg_proj = -1;
  // the smallest rows on which a predicate of the current execution hit DivideError [0] / InexactError [1] / a parse(T, s) without a value [2] (~0: none);
  // decided at the end of query_execute.  [2] is the device's word `row << 3 | reason` (dfdb::err_word_row, dfdb::throw_parse_error)
  uint64_t err_row[3] = {~0ull, ~0ull, ~0ull};
  bool err_checking = false;   // inside error_is_reached's partial executions: errors are not raised
  uint64_t* proj_err = nullptr; // query_materialize: the first erroring row per kind of the projection column being computed lands here instead of raising
  dfdb::DevBuf agg_partials, agg_ones;
  int64_t agg_ones_tiles = -1;
  dfdb::DevBuf cap_str_sizes, cap_str_bytes, cap_str_tb;
  bool stream_owned = false;   // a chunk query handed out by dfdb_stream_next: owned by the stream
  dfdb::DevBuf dict_sel;       // K9: the selected rows' dictionary codes (materialize of a dictionary column)
  // dfdb_query_groupreduce: the full selection set aside, per-group counts / values, what the fetch needs
  dfdb::DevBuf gr_sel, gr_cnt, gr_val, gr_keys;     // (gr_keys: the key column's values at the groups' first rows, group order — k_group_acc_hash_lds)
  dfdb::DevBuf du_first, du_rows, du_rank;   // dict_unique's scratch (first row per code, the group rows, rank of every code)
  int64_t gr_n = 0; int gr_state = 0;   // state 0: none, 1: empty result, 2: results + narrowed selection pending
  // whose result is pending — gr_multi 0: a dfdb_query_groupreduce, 1: a dfdb_query_groupreduce_n call that was handed to it, 2: an _n call of its own (gr_cnt
  // [ng], gr_val [nvals][ng]) — and that call's key columns and its reducers' operators and value kinds (0 signed, 1 unsigned, 2 float); dfdb_query_groupreduce
  // records its one key, operator and kind here too
  int gr_multi = 0;
  std::vector<int32_t> gr_keys_n; std::vector<int> gr_ops_n, gr_kinds_n;
  // dfdb_query_join / dfdb_query_join_n (join.cpp's one driver, whichever plan matched): what the fetch needs, all of it copies — the selected left rows ascending
  // (jn_order), per left row the first equal right key and their number (jn_lo, jn_cnt), where each 1024-entry group's pairs start (jn_base), the right rows in key order (jn_rrows), both row bases
  dfdb::DevBuf jn_order, jn_lo, jn_cnt, jn_base, jn_rrows;
  int64_t jn_nl = 0, jn_npairs = 0, jn_lbase = 0, jn_rbase = 0; int jn_kind = 0; bool jn_pending = false;
  int mask_from = -1;          // table ordinal of the column whose calibrated bitmap this query has borrowed (-1: its own)
  int64_t bitmap_rows = -1;    // rows the bitmap was sized (and zero-padded) for
  int executed_stages = -1;    // how many stages the current bitmap reflects (-1 = none)
  bool prefix_valid = false;
  int64_t count = -1;          // host copy of the total (valid when >= 0)
  // what the query has learnt by block-streaming a table whose required columns are not resident (ooc.hpp; null until it does)
  std::shared_ptr<dfdb::OocState> ooc;
};

namespace dfdb {
// does the query's bitmap — and with it q->left — stand for the whole queue (not a partial execution, not invalidated since)?
inline bool reflects_all_stages(const dfdb_query* q) { return q->executed_stages == (int)q->stages.size(); }
// the three error words of an interpreter launch (k_interp_device.inc flag_error / flag_parse_error): the table row of word `kind`
inline uint64_t err_word_row(int kind, uint64_t w) { return (kind == 2 && w != ~0ull) ? w >> 3 : w; }
// which of the three words holds the smallest row (-1: none).  On the same row the parse word wins: the parsed leaf is evaluated before anything computed from
// it, and a row without a value continues as 0 (`x ÷ parse(T, s)` adds a DivideError of its own there, which Julia never reaches)
inline int first_error_kind(const uint64_t w[3]) {
  int best = -1;
  for (int k : {2, 0, 1}) if (w[k] != ~0ull && (best < 0 || err_word_row(k, w[k]) < err_word_row(best, w[best]))) best = k;
  return best;
}
// raises what the parse word says about its row: ArgumentError / OverflowError / MethodError (DFDB_ERR_ARGUMENT) or DFDB_ERR_UNSUPPORTED, with the global row
[[noreturn]] void throw_parse_error(uint64_t word, int64_t row_base);
// engine entry points used by c_api.cpp
void table_open(dfdb_ctx* ctx, const char* path, dfdb_table** out);
void table_add_column(dfdb_table* t, const char* name, int32_t dtype, int64_t nrows, const void* data, const uint8_t* bytes,
                      int64_t nbytes, const uint8_t* missing);
void table_add_generated(dfdb_table* t, const char* name, int32_t gen, uint64_t seed, int64_t row_first, int64_t nrows);
void table_load(dfdb_table* t, const int32_t* ordinals, int32_t ncols, int64_t block_first, int64_t block_last, dfdb_sizestats* stats);
void table_load_image(dfdb_table* t, int32_t ordinal, const uint8_t* image, size_t nbytes, int64_t block_first, int64_t block_last,
                      dfdb_sizestats* stats);

// one block of a chunk whose compressed body sits in the table's load staging buffer (stream.cpp -> table.cpp)
struct StagedBlock { int32_t rows; int64_t origin, compressed, staged_off, row_pos; };
void table_decode_staged_blocks(dfdb_table* t, int32_t ordinal, const StagedBlock* bl, int64_t n, int64_t total_rows, dfdb_sizestats* stats);
// survivors of the query's current execution per block of `block_size` rows (query.cpp; synchronises)
void query_block_counts(dfdb_query* q, int64_t block_size, std::vector<int64_t>& counts);

// jit.cpp: the interpreter's source compiled by hipRTC for one program shape (everything below is a literal of the generated kernel = the cache key)
struct JitShape {
  int mode = 0, str = 0, nul = 0, and_existing = 0, stack_levels = 0, result_dtype = 0, nstr = 0;
  std::vector<uint32_t> w0, w1, w2; std::vector<int32_t> slot, aslot, col_dtype;
  int32_t str_slot[4] = {0, 0, 0, 0};
};
struct JitKernel;
std::shared_ptr<JitKernel> jit_request(dfdb_ctx* ctx, const JitShape& sh, bool wait);
bool jit_launch(JitKernel& k, dfdb_ctx* ctx, unsigned grid, size_t lds_bytes, void** args);
void jit_shutdown();
std::string jit_cache_dir(std::string* why);   // "" = off or refused
void jit_stats(int64_t* compiled, int64_t* failed, int64_t* pending, int64_t* from_disk = nullptr);

void query_add_stage(dfdb_query* q, Stage&& s);   // composition rules of selection.jl:39-49
void query_execute(dfdb_query* q, int nstages);   // evaluate stages [0, nstages) -> bitmap + counts + prefix
int64_t query_count(dfdb_query* q, int nstages);
void query_select_bitmap(dfdb_query* q, uint64_t* out, int32_t memkind);
void query_select_indices(dfdb_query* q, int64_t* out, int64_t cap, int32_t memkind, int64_t* n);
int64_t query_string_bytes(dfdb_query* q, int i);
void query_materialize(dfdb_query* q, dfdb_outcol* outs, int32_t ncols);
void query_aggregate(dfdb_query* q, int32_t op, int32_t i, int64_t* out_i, double* out_f);
// project.cpp over k_select.hip: the select keys of up to kSelectMaxRanks ranks among the selected non-missing values of a resident column (see there)
struct SelectRanks { int n; int64_t rank[kSelectMaxRanks]; };
int select_keys(dfdb_query* q, const Column& col, bool full, bool count, int max_ranks, int64_t cnt[3], const std::function<void(SelectRanks&)>& choose, uint64_t* keys);
void query_order_statistics(dfdb_query* q, int32_t p, const int64_t* ranks, int32_t nranks, int64_t* out_i, double* out_f, int64_t* counts);   // project.cpp over k_select.hip
// sort.cpp over k_sort.hip: the stable sortperm of the selected rows by projection columns proj_cols[0] (major) .. [nkeys - 1]; one column p: its n = 1 case.
// strings: String keys are admitted (dfdb_sort_indices_any) — else refused by name
// sink: the driver emits nothing and hands out the order of ALL n selected rows on the device — ascending by the key tuple, a key's missing rows behind its
// live ones, ties in ascending row order —, the digit passes it ran and, per String key, the chunks m its longest live string has and the in-tile offsets of
// its column's rows that the driver built (launch_str_row_offsets; empty when the selection is) (see sort.cpp)
struct SortOrderSink { DevBuf order; int64_t n = 0, passes = 0; int32_t str_chunks[DFDB_SORT_MAX_KEYS] = {}; DevBuf row_off[DFDB_SORT_MAX_KEYS]; };
void query_sort_indices_n(dfdb_query* q, const int32_t* proj_cols, const int32_t* flags, int32_t nkeys, int64_t limit, int64_t* out, int64_t cap, int32_t memkind,
                          int64_t* n, int64_t* info, bool strings, SortOrderSink* sink = nullptr);
void query_sort_indices(dfdb_query* q, int32_t p, int32_t flags, int64_t limit, int64_t* out, int64_t cap, int32_t memkind, int64_t* n, int64_t* info);
// the plain fixed-width projection column p of q, resident and decoded, or the refusal that names the form after `what` ("sorting by", "joining on")
const Column& ordered_column(dfdb_query* q, int32_t p, const char* what, bool strings = false);
// the sorted {select key, row} pairs of q's selected rows that are not missing in `col`, a column the caller checked with ordered_column (ascending; see sort.cpp)
void query_sorted_key_pairs(dfdb_query* q, const Column& col, DevBuf& keys, DevBuf& rows, int64_t* npairs, int64_t* nmiss, int64_t* passes);
// join.cpp over k_join.hip, two entry points of ONE driver: the join of two selections on one fixed-width key, matched by one probe launch (dfdb_query_join)
void query_join(dfdb_query* left, int32_t left_col, dfdb_query* right, int32_t right_col, int32_t kind, int64_t* npairs, int64_t* info);
// and on nkeys (1 .. DFDB_JOIN_MAX_KEYS) key columns per side, String keys among them, matched by one refinement stage per sub-key (dfdb_query_join_n); one fetch for both
void query_join_n(dfdb_query* left, const int32_t* left_cols, dfdb_query* right, const int32_t* right_cols, int32_t nkeys, int32_t kind, int64_t* npairs, int64_t* info);
void query_join_fetch(dfdb_query* left, int64_t* left_rows, int64_t* right_rows, int64_t cap, int32_t memkind);
void query_join_drop(dfdb_query* q);              // a pending join's lists go back to the pool (dfdb_query_reset, dfdb_table_unload, a join that fails)
// the projection at given rows (strings: String columns are admitted, k_str_rows.hip — else refused), and the string bytes projection column i needs at those rows
void query_gather_rows(dfdb_query* q, const int64_t* rows, int64_t n, int32_t rows_memkind, dfdb_outcol* outs, int32_t ncols, bool strings);
int64_t query_gather_rows_string_bytes(dfdb_query* q, int32_t i, const int64_t* rows, int64_t n, int32_t rows_memkind);
void query_unique(dfdb_query* q, int32_t p);
void query_groupreduce(dfdb_query* q, int32_t key_p, int32_t val_p, int32_t op, int64_t* ngroups, int64_t* key_bytes);
void query_groupreduce_fetch(dfdb_query* q, dfdb_outcol* keys, int64_t* counts, int64_t* vals_i, double* vals_f);
void query_groupreduce_n(dfdb_query* q, const int32_t* key_cols, int32_t nkeys, const int32_t* val_cols, const int32_t* stats, int32_t nvals, int64_t* ngroups,
                         int64_t* key_bytes);
void query_groupreduce_n_fetch(dfdb_query* q, dfdb_outcol* keys, int64_t* counts, int64_t* vals_i, double* vals_f);
// THE check of groupreduce's arguments, resident or streamed, one key or a tuple: raises what dfdb_query_groupreduce / _n document, returns the reducers' value
// kinds (0 signed, 1 unsigned, 2 float; a count: 0).  by_prefix stands before "groupreduce by a computed column" (the streamed unique names itself there)
std::vector<int> groupreduce_check(const dfdb_query* q, const int32_t* key_cols, int32_t nkeys, const int32_t* val_cols, const int32_t* stats, int32_t nvals,
                                   const char* by_prefix = "");
// n 64-bit results of one reducer -> the caller's values_i / values_f (either may be null) by the value column's kind
void group_values_out(const uint64_t* bits, int64_t n, int kind, int64_t* vals_i, double* vals_f);
void query_return_mask(dfdb_query* q);            // give a borrowed calibrated bitmap back to its column
// query.cpp / project.cpp helpers that project.cpp and unique.cpp build on
size_t padded_words(int64_t nrows);               // bitmap words for n rows, padded so that K2's 64-word (4096-row) reads stay in bounds
uint64_t splitmix64_host(uint64_t x);
const Column& need_resident(dfdb_table* t, int ordinal);
void selection_changed(dfdb_query* q);            // the bitmap changed outside query_execute: drop what was derived from it
void scan_prefix(dfdb_query* q);                  // tile counts -> prefix
void ensure_executed(dfdb_query* q);              // execute every stage unless the bitmap already reflects them
void ensure_executed_checked(dfdb_query* q);      // the same for a consumer that hands results to the host: answers for a decode made on the way
void materialize_col(dfdb_query* q, int32_t p, dfdb_outcol& o, int64_t cnt);
void set_string_tile_offsets(dfdb_ctx* ctx, Column& c);   // K4 over a resident string column
bool read_file_range(const std::string& file, uint8_t* dst, int64_t lo, int64_t hi);   // table.cpp: parallel pread
bool read_file_range_fd(int fd, uint8_t* dst, int64_t lo, int64_t hi);
void set_io_threads(int64_t n);                  // table.cpp: concurrent preads per byte range (ctx option "io_threads")
// stream.cpp: block-streamed execution over a non-resident table
void stream_open(dfdb_query* q, int64_t chunk_blocks, dfdb_stream** out);
dfdb_query* stream_next(dfdb_stream* s, int64_t* chunk_rows, int64_t* first_row);
void stream_close(dfdb_stream* s);
void stream_drop_parked(dfdb_ctx* ctx);
// K9: codes + dictionary for String column `ordinal` if it has at most max_entries distinct values; returns the number of entries (0: none built)
int64_t table_build_dictionary(dfdb_table* t, int32_t ordinal, int64_t max_entries);   // dfdb_ctx_destroy: the parked stream dies with its context
void stream_stats(dfdb_stream* s, dfdb_sizestats* st);
void stream_read_stats(dfdb_stream* s, int32_t ordinal, dfdb_sizestats* st);   // what the loaders have read so far of one column (-1: of every required column)
void table_column_stats(dfdb_table* t, int32_t ordinal, dfdb_sizestats* st);
void table_decode_resident(dfdb_table* t, int32_t ordinal);   // table.cpp
// compressed-only columns (table.cpp).  column_data: the decoded array of a fixed-width column — for a compressed-only one a whole-column decode made now
// (asynchronously, on the context's stream) and kept until table_drop_transient; TransientScope drops them when the ABI call that made them returns.
const void* column_data(dfdb_table* t, Column& c);
void table_drop_transient(dfdb_table* t);
struct TransientScope { dfdb_table* t; explicit TransientScope(dfdb_table* t_) : t(t_) {} ~TransientScope() { if (t) table_drop_transient(t); } };
uint8_t* ctx_hist_scratch(dfdb_ctx* ctx, int* waves);       // the history rings of K7's HIST forms (one buffer per context, made on first use)
void table_resident_bytes(dfdb_table* t, int32_t ordinal, int64_t* decoded, int64_t* compressed);
// table.cpp: what `t` may still take into HBM — ctx option "hbm_budget_mb" less what the table holds (INT64_MAX: no bound of its own), and 80 % of what the device
// has free right now.  Returns hipMemGetInfo's status: what a failure means is the caller's business
struct HbmRoom { int64_t budget = 0, free_now = 0; };
hipError_t table_hbm_room(dfdb_table* t, HbmRoom* room);
// scan_image.cpp: the column's scan copies go (and may be built again: state none, scans counted from 0).  Called wherever Column::data is released or gets new
// contents; waits for the stream only when there is an image to free
void drop_scan_image(dfdb_ctx* ctx, Column& c);
// scan_image.cpp: the lone plain term `tm` over table column `ord` answered from the column's scan copies (profile key "scan_image"); false: the flat scan must
bool run_image_scan(dfdb_query* q, int ord, const ScanTerm& tm, bool have);
// the store-mode word of launch_scan_cmp: bit 0 = ctx option "scan_wt_store", bits 1-2 = "scan_narrow"
inline int scan_store_flags(const dfdb_ctx* ctx) { return (ctx_option(ctx, "scan_wt_store", 1) ? 1 : 0) | (int)((ctx_option(ctx, "scan_narrow", 1) & 3) << 1); }
int64_t table_decode_status(dfdb_table* t, int32_t ordinal);   // table.cpp: blocks of the last resident decode whose status is not 0 (synchronises)
int column_lz4_index(dfdb_ctx* ctx, Column& c, bool form_takes_index);   // table.cpp: 0 / 1 (record) / 2 (use) for launch_lz4_decode*
int32_t ctx_create_like(const dfdb_ctx* like, dfdb_ctx** out);   // c_api.cpp
void ctx_destroy(dfdb_ctx* c);
void table_save(dfdb_table* t, const char* path, dfdb_sizestats* stats);                       // writer.cpp
void table_save_column(dfdb_table* t, int32_t ordinal, const char* file, dfdb_sizestats* stats);
void table_compress_column(dfdb_table* t, int32_t ordinal, int32_t mode, dfdb_sizestats* stats);   // writer.cpp: resident -> compressed-resident (1) / compressed-only (2) in HBM
void table_add_from_query(dfdb_table* dst, const char* name, dfdb_query* q, int32_t p);       // add_column!(t, name, lazy column)
}  // namespace dfdb
