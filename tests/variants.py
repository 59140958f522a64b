"""Which test checks the output of the kernels each fury_set_tuning knob can select.

Plain data: no torch, no pytest.  Every key of tests.test_tuning.KNOBS is in exactly one of MATRIX,
ELSEWHERE and EXEMPT (tests/test_variants.py checks that), so a knob added without a parity test
against the oracle fails the suite.  tests/test_variants_gpu.py runs MATRIX; a value of a MATRIX
knob that cannot run is moved to KNOWN_BAD, which the same check accounts for."""
from __future__ import annotations

INT32_MAX = (1 << 31) - 1

# knob -> the values tests/test_variants_gpu.py runs against the oracle, the default among them
# (the same test's control leg).  Every legal value of a list knob and of a range of at most five
# values; representative values otherwise.
MATRIX = {
    # fixed.hip, launch_encode_fixed: U = 8 / pair mode / 16 (default) / 32 / 16 with DS = 8
    "fixed_enc": [0, 1, 2, 3, 4],
    # launch_decode_fixed: SU = 8 (default) / 16 / 4, and D = 8
    "fixed_dec": [0, 1, 2, 3],
    # 17-256 flat fields: 0 the look-back tiles (encode_var_kernel, decode_measure_kernel,
    # decode_var_kernel), 1 the wide tiles (default)
    "var_wide": [0, 1],
    # forced tile rows of the register-staged decode: planned (0), the smallest, two in between
    # and the largest
    "var_dec_rows": [0, 64, 192, 320, 512],
    # percent of a tile's row bytes the LDS stage must hold: both ends and the default
    "var_dec_cover": [50, 95, 100],
    "wide_threads": [256, 512, 1024],
    "wide_enc_threads": [256, 512, 1024],
    "walk_prefetch": [0, 1, 2, 3],
    "walk_threads": [64, 128, 256],
    # auto engine threshold: every batch to the walk, the default, every batch to the wide tiles
    "wide_walk_row": [0, 896, INT32_MAX],
}

# knob -> the GPU test that already compares the kernels it selects with the oracle
_TREE_DECODE = "tests/test_tree.py::test_tree_decode_equals_oracle_and_level_engine"
_TREE_ENCODE = "tests/test_tree.py::test_tree_encode_equals_oracle"
ELSEWHERE = {
    "nested_decode": _TREE_DECODE,
    "bfs_threads": _TREE_DECODE,
    "bfs_rows": _TREE_DECODE,
    "bfs_stage": _TREE_DECODE,
    "bfs_arena": _TREE_DECODE,
    "walk_threads_write": _TREE_DECODE,
    "walk_out": _TREE_DECODE,
    "walk_stage": _TREE_DECODE,
    "walk_pool": _TREE_DECODE,
    "walk_stage_write": _TREE_DECODE,
    "walk_group_k": _TREE_DECODE,
    "walk_group_min": _TREE_DECODE,
    "rowenc_rows": _TREE_ENCODE,
    "rowenc_img": _TREE_ENCODE,
    "rowenc_tile": _TREE_ENCODE,
    "wide_engine": "tests/test_device.py::test_wide_plan_engines",
    "wide_enc_engine": "tests/test_device.py::test_wide_encode_engines",
    "var_dec_pipe": "tests/test_device.py::test_var_decode_pipe",
    "lookback_help": "tests/test_device.py::test_var_decode_lookback_help_bit_exact",
    "unframe": "tests/test_device.py::test_unframe_parallel_equals_walk",
    "host_decode_inplace": "tests/test_host_path.py::test_host_direct_nested_page_edge",
    "fixed_enc_tail_kib": "tests/test_fixed_tail.py::test_every_window_bit_exact",
}

# knob -> why no parity test applies
EXEMPT = {
    "walk_skip": "diagnostic: skips phases of the row walk's write pass, wrong by design",
    "var_skip": "diagnostic: skips phases of encode_var_reg / decode_var_reg, wrong by design",
}

# knob -> {value: what happened}.  A value that faulted or hung on the GPU and whose cause was not
# found without running it again: its legs are left out of MATRIX until it is.  Empty: none.
KNOWN_BAD: dict = {}

# ---- the input shapes of tests/test_variants_gpu.py (the oracle produces each one on the CPU in
# tests/test_variants.py) ------------------------------------------------------------------------
# fixed-width fast path: schema -> (fields, fixed_size, rows per tile by fixed.hip's
# pick_rows_per_tile); "int64xK" = K non-null INT64 fields
FIXED = {
    "int64x20": (20, 168, 256),
    "int64x50": (50, 408, 128),
    "int64x65": (65, 536, 64),      # an odd column count at 64-row tiles
    "struct100": (100, 816, 64),
}


def rows_per_tile(row_size: int) -> int:
    """fixed.hip pick_rows_per_tile."""
    if row_size * 256 <= 48 * 1024:
        return 256
    if row_size * 128 <= 64 * 1024:
        return 128
    return 64


def fixed_ns(R: int):
    """Odd and even row counts, ragged last tiles, a single-row tile."""
    return [1, R - 1, R, R + 1, 2 * R + 1]


FIXED_TAIL_N = 64 * 5 + 7          # Struct-100: five full tiles and a ragged one

# var_wide: (fields of _wide_fields, rows, str_max)
VAR_WIDE = ([(k, n, 40) for k in (17, 33, 64, 65, 200, 256) for n in (1, 255, 256, 257, 2049)] +
            [(17, 700, 600), (64, 257, 300),      # tiles that outgrow their LDS pools
             (17, 20_001, 40)])                   # ~80 tiles chained by the look-back

# forced decode tiles: schema names ("mixed", or "<_REG_MODES key>:<fields>"), forced rows
REG_SCHEMAS = ["mixed"] + [f"{m}:{k}" for m in ("all", "bytes", "lists") for k in (3, 6, 16)]
REG_ROWS = [64, 192, 320, 512]
# var_dec_cover: (schema of fury_amd.workloads.SCHEMAS, rows, generator knobs)
COVER = [("mixed", 3000, {"str_max": 40}), ("mixed", 3000, {"str_max": 600}),
         ("nested", 1500, {"list_max": 200})]

# wide tiles: (wide_threads, wide_enc_threads) -- the diagonal and the two extremes
WIDE_THREAD_PAIRS = [(256, 256), (512, 512), (1024, 1024), (256, 1024), (1024, 256)]
# (fields, rows, str_max)
WIDE_THREADS = ([(k, n, 40) for k in (17, 33, 64, 200) for n in (257, 1500)] + [(64, 257, 300)])

# row walk: nested schemas of tests/test_tree.py::_schemas, and flat ones (fields of _wide_fields)
WALK_NESTED = ["nested7", "maps", "beana", "deep_lists"]
WALK_NESTED_N = 1000
WALK_FLAT = [33, 200]
WALK_FLAT_N = 700

# auto routing: _wide_fields(33) at 700 rows
AUTO_STR_MAX = [24, 300]
AUTO_N = 700
