"""fury_set_tuning / fury_get_tuning, every key: default, legal values and their read-back, illegal
values and the message each reports.  The table below is the library's behaviour as it was before
the keys moved into one table (csrc/tuning.cpp); it passed against that library unchanged.  Host
side only: no key here touches the device ("tree_debug" is only given a value it refuses, and the
counters that read the device are never read)."""
from __future__ import annotations

import pytest

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1

LDS_96K = "{key}: 0..98304 bytes"
BFS_128K = "{key}: 0..131072 bytes (0: auto)"
NESTED = ("nested_decode: 1 (level engine), 2 (row walk, level engine beyond it), 3 (row walk, tile "
          "BFS beyond it) or 4 (tile BFS)")

# key: (default, [(value set, value read back)], [illegal values], last_error of an illegal value)
KNOBS = {
    "lookback_help": (0, [(0, 0), (1, 1)], [-1, 2], "lookback_help: 0..1"),
    "unframe": (0, [(0, 0), (1, 1)], [-1, 2], "unframe: 0..1"),
    "nested_decode": (2, [(1, 1), (3, 3), (4, 4)], [0, 5, -1], NESTED),
    "bfs_threads": (128, [(64, 64), (256, 256), (512, 512)], [0, 63, 192, 1024],
                    "bfs_threads: 64, 128, 256 or 512"),
    "bfs_rows": (128, [(1, 1), (4096, 4096)], [0, 4097], "bfs_rows: 1..4096"),
    "bfs_stage": (0, [(131072, 131072), (100, 112), (1, 16), (0, 0)], [-1, 131073], BFS_128K),
    "bfs_arena": (0, [(131072, 131072), (131057, 131072), (16, 16), (0, 0)], [-1, 131073], BFS_128K),
    "var_dec_cover": (95, [(50, 50), (100, 100), (0, 95)], [-1, 1, 49, 101],
                      "var_dec_cover: 50..100 (0 = default)"),
    "var_wide": (1, [(0, 0), (1, 1)], [-1, 2], "var_wide: 0..1"),
    "wide_threads": (256, [(512, 512), (1024, 1024), (256, 256)], [0, 128, 768, 2048],
                     "wide_threads: 256, 512 or 1024"),
    "wide_enc_threads": (512, [(256, 256), (1024, 1024), (512, 512)], [0, 128, 768, 2048],
                         "wide_enc_threads: 256, 512 or 1024"),
    "var_skip": (0, [(255, 255), (0, 0)], [-1, 256], "var_skip: 0..255"),
    "fixed_dec": (0, [(3, 3), (0, 0)], [-1, 4], "fixed_dec: 0..3"),
    "fixed_enc": (2, [(0, 0), (4, 4)], [-1, 5], "fixed_enc: 0..4"),
    "fixed_enc_tail_kib": (524288, [(0, 0), (4194304, 4194304), (5, 5)],
                           [-1, 4194305, INT32_MIN, INT32_MAX], "fixed_enc_tail_kib: 0..4194304 KiB"),
    "wide_engine": (0, [(2, 2), (0, 0)], [-1, 3], "wide_engine: 0..2"),
    "wide_enc_engine": (0, [(2, 2), (0, 0)], [-1, 3], "wide_enc_engine: 0..2"),
    "wide_walk_row": (896, [(0, 0), (INT32_MAX, INT32_MAX), (897, 897)], [-1, INT32_MIN],
                      "wide_walk_row: bytes >= 0"),
    "var_dec_pipe": (0, [(2, 2), (0, 0)], [-1, 3], "var_dec_pipe: 0..2"),
    "var_dec_rows": (0, [(64, 64), (512, 512), (320, 320), (0, 0)], [-64, 1, 63, 65, 100, 576],
                     "var_dec_rows: 0 or 64..512 in steps of 64"),
    "walk_threads_write": (512, [(64, 64), (128, 128), (256, 256), (512, 512)], [0, 32, 384, 1024],
                           "walk_threads_write: 64, 128, 256 or 512 (512: no write stage)"),
    "walk_skip": (0, [(15, 15), (0, 0)], [-1, 16], "walk_skip: 0..15"),
    "host_decode_inplace": (0, [(1, 1), (0, 0)], [-1, 2], "host_decode_inplace: 0..1"),
    "walk_prefetch": (1, [(0, 0), (3, 3)], [-1, 4],
                      "walk_prefetch: 0..3 (bit 0 write pass, bit 1 count pass)"),
    "walk_threads": (128, [(64, 64), (256, 256), (128, 128)], [0, 32, 192, 512],
                     "walk_threads: 64, 128 or 256"),
    "walk_group_k": (8, [(0, 0), (256, 256)], [-1, 257], "walk_group_k: 0..256"),
    "walk_group_min": (16, [(0, 0), (256, 256)], [-1, 257], "walk_group_min: 0..256"),
    "walk_out": (40960, [(0, 0), (98304, 98304), (100, 112)], [-1, 98305], LDS_96K),
    "walk_stage": (12288, [(0, 0), (98304, 98304), (100, 112), (98289, 98304)], [-1, 98305], LDS_96K),
    "walk_pool": (8192, [(0, 0), (98304, 98304), (8177, 8192)], [-1, 98305], LDS_96K),
    "walk_stage_write": (0, [(98304, 98304), (1, 16), (0, 0)], [-1, 98305], LDS_96K),
    "rowenc_rows": (256, [(128, 128), (512, 512), (256, 256)], [0, 64, 384, 1024],
                    "rowenc_rows: 128, 256 or 512"),
    "rowenc_tile": (0, [(256, 256), (0, 0)], [-1, 257], "rowenc_tile: 0..256"),
    # the stored image size is rounded up to 16 bytes like the walk's LDS sizes
    "rowenc_img": (77824, [(1024, 1024), (155648, 155648), (1025, 1040)], [1023, 155649, 0, -1],
                   "rowenc_img: 1024..155648 bytes"),
}

# fury_get_tuning only
COUNTERS = ["lookback_timeouts", "unframe_walks", "unframe_repairs", "host_direct", "err_slots",
            "err_slots_quarantined", "thread_key_exits", "err_slot_last_key", "decode_budget_errors",
            "var_dec_rows_rejected", "bfs_fallbacks", "workspace_live"]


def _lib():
    from fury_amd import _native as N
    return N.lib(), N.last_error


@pytest.mark.parametrize("key", sorted(KNOBS))
def test_knob(key):
    L, last_error = _lib()
    default, legal, illegal, message = KNOBS[key]
    k = key.encode()
    saved = L.fury_get_tuning(k)
    try:
        assert saved == default
        for value, back in legal:
            assert L.fury_set_tuning(k, value) == 0, (key, value)
            assert L.fury_get_tuning(k) == back, (key, value)
            for bad in illegal:
                assert L.fury_set_tuning(k, bad) == 1, (key, bad)
                assert L.fury_get_tuning(k) == back, (key, bad)
                assert last_error() == message.format(key=key), (key, bad)
    finally:
        assert L.fury_set_tuning(k, saved) == 0
    assert L.fury_get_tuning(k) == default


def test_var_dec_cover_zero_restores_the_default():
    L, _ = _lib()
    try:
        assert L.fury_set_tuning(b"var_dec_cover", 60) == 0
        assert L.fury_get_tuning(b"var_dec_cover") == 60
        assert L.fury_set_tuning(b"var_dec_cover", 0) == 0
        assert L.fury_get_tuning(b"var_dec_cover") == 95
    finally:
        assert L.fury_set_tuning(b"var_dec_cover", 95) == 0


def test_unknown_and_null_keys():
    L, last_error = _lib()
    assert L.fury_set_tuning(b"no_such_knob", 0) == 1
    assert last_error() == "unknown tuning key no_such_knob"
    assert L.fury_get_tuning(b"no_such_knob") == -1
    assert L.fury_set_tuning(b"", 0) == 1
    assert last_error() == "unknown tuning key "
    assert L.fury_get_tuning(b"") == -1
    # a key is matched whole, not by prefix
    assert L.fury_set_tuning(b"walk_stage_", 16) == 1 and L.fury_get_tuning(b"walk_stag") == -1
    assert L.fury_set_tuning(None, 0) == 1
    assert last_error() == "fury_set_tuning: key is null"
    assert L.fury_get_tuning(None) == -1


@pytest.mark.parametrize("key", COUNTERS)
def test_counters_cannot_be_set(key):
    L, last_error = _lib()
    assert key not in KNOBS
    assert L.fury_set_tuning(key.encode(), 0) == 1
    assert last_error() == "unknown tuning key " + key


def test_tree_debug_range_and_no_getter():
    """Only refused values: a legal 1 allocates device memory."""
    L, last_error = _lib()
    for bad in (-1, 2):
        assert L.fury_set_tuning(b"tree_debug", bad) == 1
        assert last_error() == "tree_debug: 0..1"
    assert L.fury_get_tuning(b"tree_debug") == -1
