// tuning.h — the process-wide knobs behind fury_set_tuning / fury_get_tuning: one atomic per
// settable key, named after it.  Key strings, defaults (with the measurements behind them), legal
// values and messages are the rows of the table in tuning.cpp; a new knob is one row there plus
// one name here.  Launchers read knob::x.load() where they use the value; nothing on a launch path
// looks a key up by name.
#pragma once

#include <atomic>
#include <cstdint>

namespace fury {
namespace knob {

using Knob = std::atomic<int32_t>;
extern Knob lookback_help, unframe, host_decode_inplace;
extern Knob nested_decode, bfs_threads, bfs_rows, bfs_stage, bfs_arena;
extern Knob walk_threads, walk_threads_write, walk_stage, walk_stage_write, walk_pool, walk_out,
    walk_prefetch, walk_skip, walk_group_k, walk_group_min;
extern Knob rowenc_rows, rowenc_img, rowenc_tile;
extern Knob var_wide, var_skip, var_dec_cover, var_dec_rows, var_dec_pipe;
extern Knob wide_engine, wide_enc_engine, wide_walk_row, wide_threads, wide_enc_threads;
extern Knob fixed_enc, fixed_dec, fixed_enc_tail_kib;

}  // namespace knob
}  // namespace fury
