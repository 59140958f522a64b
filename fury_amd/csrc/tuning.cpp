// tuning.cpp — fury_set_tuning / fury_get_tuning: the table of knobs (tuning.h), the read-only
// counters, and the two entry points that look a key up in them.  Neither is on a per-batch path.
#include "tuning.h"

#include <algorithm>
#include <cstring>
#include <string>

#include "internal.h"
#include "kernels.h"

namespace fury {
namespace {

enum Rule { kRange, kList };
enum Flag { kRound16 = 1, kZeroIsDefault = 2 };

struct Row {
  const char* key;
  knob::Knob* at;
  int32_t def;           // the knob's initial value (initial() below)
  Rule rule;
  int32_t v[4];          // kRange: lo, hi (closed) and, when not 0, a step the value is a multiple
                         // of; kList: the legal values, zero-padded (0 is in no list)
  int flags;             // kRound16: the stored value is rounded up to a multiple of 16;
                         // kZeroIsDefault: setting 0 stores `def`
  const char* message;   // last error of a refused value
};

constexpr Row kRows[] = {
    // Test hook: 1 = every look-back of the variable-length decode computes a silent predecessor's
    // aggregate at once -- the path a late-dispatched predecessor takes -- instead of polling
    // first.
    {"lookback_help", &knob::lookback_help, 0, kRange, {0, 1}, 0, "lookback_help: 0..1"},
    // 0 speculative parallel stream parse (sequential walk on failure), 1 always the walk
    {"unframe", &knob::unframe, 0, kRange, {0, 1}, 0, "unframe: 0..1"},
    // fury_row_decode_host writes the outputs the kernels write exactly straight to the caller's
    // buffers (hostpath.cpp)
    {"host_decode_inplace", &knob::host_decode_inplace, 0, kRange, {0, 1}, 0,
     "host_decode_inplace: 0..1"},

    // ---- nested decode (tree.hip) ----
    // 1 level engine; 2 row walk, the level engine past its limits (default); 3 row walk, tile BFS
    // (bfs.hip) past its limits; 4 tile BFS always (A/B, tests).  The BFS falls back to the walk /
    // level engine for a batch whose tiles overflow its arena.  Measured round 6 (DESIGN §4e,
    // profiles/r06_*): at depth 3 the walk decodes 4M rows in 2.53 ms, the BFS in 3.06 ms at best
    // (its per-level chains of LDS round trips run at ~2 waves per SIMD, bounded by the LDS its
    // staged tiles take); past the walk's limits the level engine beat the BFS too (depth 6-20,
    // 128 counted nodes), so the BFS is not the default anywhere.
    {"nested_decode", &knob::nested_decode, 2, kRange, {1, 4}, 0,
     "nested_decode: 1 (level engine), 2 (row walk, level engine beyond it), 3 (row walk, tile BFS "
     "beyond it) or 4 (tile BFS)"},
    // Tile BFS: threads and rows per tile, LDS stage bytes (0: sized from the batch's average row)
    // and arena bytes (0: 60 % of the stage + 2 KB).
    {"bfs_threads", &knob::bfs_threads, 128, kList, {64, 128, 256, 512}, 0,
     "bfs_threads: 64, 128, 256 or 512"},
    {"bfs_rows", &knob::bfs_rows, 128, kRange, {1, 4096}, 0, "bfs_rows: 1..4096"},
    {"bfs_stage", &knob::bfs_stage, 0, kRange, {0, 128 * 1024}, kRound16,
     "bfs_stage: 0..131072 bytes (0: auto)"},
    {"bfs_arena", &knob::bfs_arena, 0, kRange, {0, 128 * 1024}, kRound16,
     "bfs_arena: 0..131072 bytes (0: auto)"},
    // Row-walk defaults from scripts/ab_generic.py legs at 4M depth-3 rows: 128-row count tiles
    // with a 12 KB stage (prepare 1.35 -> 1.08 ms: more tiles resident), 256-row write tiles (1.87
    // -> 1.78 ms) with the prefetch; round 5: 512-row unstaged write tiles with 24 KB output
    // windows (1.67 -> 1.62 ms: the tile prologue -- bases, window layout -- is ~16 % of a 256-row
    // tile's time), then 40 KB windows (the same time, WRITE 1.34x -> 1.23x the column bytes).
    // rows (= threads) per count tile / per write tile (a multiple)
    {"walk_threads", &knob::walk_threads, 128, kList, {64, 128, 256}, 0,
     "walk_threads: 64, 128 or 256"},
    {"walk_threads_write", &knob::walk_threads_write, 512, kList, {64, 128, 256, 512}, 0,
     "walk_threads_write: 64, 128, 256 or 512 (512: no write stage)"},
    // LDS stage cap of a count tile / of a write tile (0: its LDS-bound occupancy costs more than
    // HBM row reads save)
    {"walk_stage", &knob::walk_stage, 12 * 1024, kRange, {0, 96 * 1024}, kRound16,
     "walk_stage: 0..98304 bytes"},
    {"walk_stage_write", &knob::walk_stage_write, 0, kRange, {0, 96 * 1024}, kRound16,
     "walk_stage_write: 0..98304 bytes"},
    // write pass: LDS bitmap-window / output-window bytes
    {"walk_pool", &knob::walk_pool, 8 * 1024, kRange, {0, 96 * 1024}, kRound16,
     "walk_pool: 0..98304 bytes"},
    {"walk_out", &knob::walk_out, 40 * 1024, kRange, {0, 96 * 1024}, kRound16,
     "walk_out: 0..98304 bytes"},
    // waves pull their rows into L2 first
    {"walk_prefetch", &knob::walk_prefetch, 1, kRange, {0, 3}, 0,
     "walk_prefetch: 0..3 (bit 0 write pass, bit 1 count pass)"},
    // diagnostics (TreeArgs.skip): write-pass phases skipped, outputs WRONG
    {"walk_skip", &knob::walk_skip, 0, kRange, {0, 15}, 0, "walk_skip: 0..15"},
    // Field groups (round 6): a schema with more than "walk_group_min" counted slots walks its
    // top-level fields in groups of about "walk_group_k" slots (0 = one group), a workgroup per
    // (tile, group): the LDS cursors (4 B x slots x rows) of a 128-slot bean held one 64-row count
    // tile per ~5 waves of a CU.  1M beans of 128 / 200 counted nodes (scripts/r06_group2.sh): one
    // group 22.5 / 39.0 ms, groups of 16 / 8 / 4 / 2 slots 9.7 / 7.2 / 6.8 / 6.9 and 13.8 / 10.2 /
    // 10.2 / 10.2 ms, the level engine 16.5 / 25.7 ms.  The depth-3 schema (9 slots) in groups of
    // 4 / 2 / 1: 2.64 / 2.99 / 3.25 vs 2.53 ms -- at <= 16 slots the cursors do not limit the tiles
    // per CU, so it stays one group.  With the payload windows (late round 6,
    // profiles/r06_walk_group_size_payload_windows.jsonl) groups of 8 took over: 128 counted nodes
    // 6.52 vs 6.89 ms (4), flat id + 126 STRING fields 5.83 vs 6.14; 200 counted nodes 9.47 (4
    // doubles to 8 there: at most 32 groups).
    {"walk_group_k", &knob::walk_group_k, 8, kRange, {0, 256}, 0, "walk_group_k: 0..256"},
    {"walk_group_min", &knob::walk_group_min, 16, kRange, {0, 256}, 0, "walk_group_min: 0..256"},

    // ---- nested encode (rowenc.hip) ----
    // build-pass rows per workgroup (512 with a 152 KB image: 1.31 vs 1.33 ms, not the default),
    // its LDS image bytes, rows per workgroup (0: all)
    {"rowenc_rows", &knob::rowenc_rows, 256, kList, {128, 256, 512}, 0,
     "rowenc_rows: 128, 256 or 512"},
    {"rowenc_img", &knob::rowenc_img, 76 * 1024, kRange, {1024, 152 * 1024}, kRound16,
     "rowenc_img: 1024..155648 bytes"},
    {"rowenc_tile", &knob::rowenc_tile, 0, kRange, {0, 256}, 0, "rowenc_tile: 0..256"},

    // ---- variable-length schemas (var.hip, wide.hip, capi.cpp) ----
    // flat schemas of 17-256 fields: 1 count + write passes of the wide tiles, 0 look-back tiles
    {"var_wide", &knob::var_wide, 1, kRange, {0, 1}, 0, "var_wide: 0..1"},
    // diagnostics: phases of encode_var_reg (1 / 2 / 4) and decode_var_reg (16 / 32 / 64 / 128)
    // skipped, outputs WRONG; timing only
    {"var_skip", &knob::var_skip, 0, kRange, {0, 255}, 0, "var_skip: 0..255"},
    // percent of a tile's estimated row bytes the decode's LDS stage must hold (the rest is read
    // from HBM by the rows' threads).  95 (scripts/ab_dec.py legs, interleaved): mixed 10M 0.542 ->
    // 0.508 ms (its tiles grow 448 -> 512 rows), C4 4M unchanged (0.229 ms); 80 or less slows C4.
    {"var_dec_cover", &knob::var_dec_cover, 95, kRange, {50, 100}, kZeroIsDefault,
     "var_dec_cover: 50..100 (0 = default)"},
    // forced decode tile rows (A/B), 0 = planned
    {"var_dec_rows", &knob::var_dec_rows, 0, kRange, {0, 512, 64}, 0,
     "var_dec_rows: 0 or 64..512 in steps of 64"},
    // (round 6) 0 one tile per workgroup; 1 persistent workgroups with two row
    // stages of the planned size (fewer workgroups per CU); 2 the same with the planned LDS split
    // into images + two half stages (the tile rows shrink to fit)
    {"var_dec_pipe", &knob::var_dec_pipe, 0, kRange, {0, 2}, 0, "var_dec_pipe: 0..2"},
    // (round 6) the engine of a 17-256-field flat variable-length schema's decode plan -- 0 auto,
    // 1 the wide tiles (wide.hip), 2 the row walk (walk.hip, field groups past 16 counted fields).
    // Auto takes the walk when the batch's average row (one 8-byte read) exceeds "wide_walk_row"
    // bytes: the wide tiles stage 64 rows in at most 96 KB and read the rest from HBM lane by lane
    // (1M rows, scripts/ab_deep.py --flat / --wide33, profiles/r06_wide_engine.jsonl; id + N STRING
    // fields, wide vs walk: N = 126 / 2.45 KB rows 15.9 vs 6.1 ms, 90 / 1.75 KB 10.0 vs 4.3, 70 /
    // 1.37 KB 5.45 vs 3.34, 55 / 1.07 KB 3.82 vs 2.65, 40 / 785 B 1.72 vs 1.95; the tests' 33-field
    // schema, 520 B: 0.90 vs 1.70).
    {"wide_engine", &knob::wide_engine, 0, kRange, {0, 2}, 0, "wide_engine: 0..2"},
    // (round 6) the same for the encode -- 2: the row-walk encode (rowenc.hip, as nested schemas).
    // Auto takes the row walk when the rows' estimated average (the header + each variable-length
    // column's capacity / rows) exceeds "wide_walk_row" bytes, as the decode plan does.  The rows
    // are the same bytes either way (the Java layout).  1M rows, wide vs walk (scripts/ab_wide.py
    // --enc-engines, profiles/r06_wide_enc_engine.jsonl): id + 126 / 70 / 55 / 40 STRING fields
    // (3.2 / 1.8 / 1.4 / 1.0 KB rows) 9.56 / 5.22 / 4.10 / 2.59 vs 6.76 / 3.67 / 2.91 / 2.15 ms;
    // the tests' 33-field schema (581 B rows) 0.51 vs 1.07 ms.
    {"wide_enc_engine", &knob::wide_enc_engine, 0, kRange, {0, 2}, 0, "wide_enc_engine: 0..2"},
    {"wide_walk_row", &knob::wide_walk_row, 896, kRange, {0, INT32_MAX}, 0, "wide_walk_row: bytes >= 0"},
    // threads per 64-row tile of the wide kernels (ab_wide legs, 33 fields x 5M rows): decode 256
    // (3.22 vs 3.37 ms at 512), encode 512 (2.20 vs 2.78 ms at 256)
    {"wide_threads", &knob::wide_threads, 256, kList, {256, 512, 1024}, 0,
     "wide_threads: 256, 512 or 1024"},
    {"wide_enc_threads", &knob::wide_enc_threads, 512, kList, {256, 512, 1024}, 0,
     "wide_enc_threads: 256, 512 or 1024"},

    // ---- fixed-width schemas (fixed.hip) ----
    // (round 6 A/B, scripts/r06_fixed_enc.sh, profiles/r06_fixed_enc_ab.txt) the fast-path encode's
    // column gather with 0: 8 loads per lane in flight (rounds 1-5), 2: 16 (the default: Struct-100
    // encode 0.291 -> 0.286 ms, six alternating runs), 3: 32 (0.291), 4: 16 loads and 8 16-B stores
    // (0.287); 1: pair mode, 16-B column loads of two rows per lane (0.320)
    {"fixed_enc", &knob::fixed_enc, 2, kRange, {0, 4}, 0, "fixed_enc: 0..4"},
    // (round 6 A/B) the fast-path decode's column stores per lane in flight, 0: 8 (default), 1: 16,
    // 2: 4; 3: 8 with 8 row loads per lane in flight instead of 16
    {"fixed_dec", &knob::fixed_dec, 0, kRange, {0, 3}, 0, "fixed_dec: 0..3"},
    // (profiles/fixed_tail_ab.jsonl) KiB of trailing row bytes the fast-path encode
    // stores with the default cache policy instead of non-temporally; 0: none (all non-temporal,
    // the earlier behaviour).  Struct-100, 1M rows (816 MB of rows), seven alternating runs, encode
    // ms: 0.288 at 0, 0.277 at 256 MiB, 0.269 at 384, 0.262 at 512 (the default), 0.260 at 640,
    // 0.265 with every row in the window; the decode that follows took 0.252-0.255 ms in every
    // leg.  Host-direct calls ignore it.
    {"fixed_enc_tail_kib", &knob::fixed_enc_tail_kib, 512 * 1024, kRange, {0, 1 << 22}, 0,
     "fixed_enc_tail_kib: 0..4194304 KiB"},
};

// A knob starts at its row's default (constant initialisation: kRows is constexpr).
constexpr int32_t initial(const knob::Knob* at) {
  for (const Row& r : kRows)
    if (r.at == at) return r.def;
  return -1;
}

const Row* find_row(const char* key) {
  for (const Row& r : kRows)
    if (!std::strcmp(key, r.key)) return &r;
  return nullptr;
}

bool legal(const Row& r, int32_t v) {
  if (r.rule == kList) return v != 0 && std::find(r.v, r.v + 4, v) != r.v + 4;
  return v >= r.v[0] && v <= r.v[1] && (r.v[2] == 0 || v % r.v[2] == 0);
}

// fury_get_tuning only.
template <auto F>
int32_t as_i32() { return static_cast<int32_t>(F()); }

constexpr struct {
  const char* key;
  int32_t (*read)();
} kCounters[] = {
    {"lookback_timeouts", as_i32<lookback_timeouts>},      // synchronous device read
    {"unframe_walks", as_i32<unframe_walk_count>},
    {"unframe_repairs", as_i32<unframe_repair_count>},
    {"host_direct", as_i32<host_direct_count>},
    {"err_slots", as_i32<error_slots_in_use>},
    {"err_slots_quarantined", as_i32<error_slots_quarantined>},
    {"thread_key_exits", as_i32<thread_key_exits>},
    {"err_slot_last_key", as_i32<last_assigned_key_kind>},
    {"decode_budget_errors", as_i32<budget_errors>},
    {"var_dec_rows_rejected", as_i32<var_dec_rows_rejected>},
    {"bfs_fallbacks", as_i32<bfs_fallbacks>},
    {"workspace_live", as_i32<dev_live_blocks>},           // cached device blocks handed out now
};

}  // namespace

namespace knob {

Knob lookback_help{initial(&lookback_help)}, unframe{initial(&unframe)},
    host_decode_inplace{initial(&host_decode_inplace)};
Knob nested_decode{initial(&nested_decode)}, bfs_threads{initial(&bfs_threads)},
    bfs_rows{initial(&bfs_rows)}, bfs_stage{initial(&bfs_stage)}, bfs_arena{initial(&bfs_arena)};
Knob walk_threads{initial(&walk_threads)}, walk_threads_write{initial(&walk_threads_write)},
    walk_stage{initial(&walk_stage)}, walk_stage_write{initial(&walk_stage_write)},
    walk_pool{initial(&walk_pool)}, walk_out{initial(&walk_out)},
    walk_prefetch{initial(&walk_prefetch)}, walk_skip{initial(&walk_skip)},
    walk_group_k{initial(&walk_group_k)}, walk_group_min{initial(&walk_group_min)};
Knob rowenc_rows{initial(&rowenc_rows)}, rowenc_img{initial(&rowenc_img)},
    rowenc_tile{initial(&rowenc_tile)};
Knob var_wide{initial(&var_wide)}, var_skip{initial(&var_skip)},
    var_dec_cover{initial(&var_dec_cover)}, var_dec_rows{initial(&var_dec_rows)},
    var_dec_pipe{initial(&var_dec_pipe)};
Knob wide_engine{initial(&wide_engine)}, wide_enc_engine{initial(&wide_enc_engine)},
    wide_walk_row{initial(&wide_walk_row)}, wide_threads{initial(&wide_threads)},
    wide_enc_threads{initial(&wide_enc_threads)};
Knob fixed_enc{initial(&fixed_enc)}, fixed_dec{initial(&fixed_dec)},
    fixed_enc_tail_kib{initial(&fixed_enc_tail_kib)};

}  // namespace knob
}  // namespace fury

using namespace fury;

extern "C" {

int fury_set_tuning(const char* key, int32_t value) {
  if (!key) return set_error(FURY_ERR_INVALID_ARGUMENT, "fury_set_tuning: key is null");
  // phase accumulators on / off: allocates device memory and has no getter, so it is no table row
  if (!std::strcmp(key, "tree_debug")) {
    if (value < 0 || value > 1) return set_error(FURY_ERR_INVALID_ARGUMENT, "tree_debug: 0..1");
    return set_tree_debug(value) ? set_error(FURY_ERR_DEVICE, "tree_debug buffer") : FURY_OK;
  }
  const Row* r = find_row(key);
  if (!r) return set_error(FURY_ERR_INVALID_ARGUMENT, std::string("unknown tuning key ") + key);
  if ((r->flags & kZeroIsDefault) && value == 0) value = r->def;
  if (!legal(*r, value)) return set_error(FURY_ERR_INVALID_ARGUMENT, r->message);
  r->at->store((r->flags & kRound16) ? (value + 15) & ~15 : value);
  return FURY_OK;
}

int32_t fury_get_tuning(const char* key) {
  if (!key) return -1;
  if (const Row* r = find_row(key)) return r->at->load();
  for (const auto& c : kCounters)
    if (!std::strcmp(key, c.key)) return c.read();
  return -1;
}

}  // extern "C"
