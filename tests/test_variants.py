"""The variant matrix of tests/variants.py is complete and its references exist.  Host only: every
tuning knob is accounted for, every value in the matrix is one fury_set_tuning accepts, the
fixed-width schemas land in the tile classes the GPU tests mean them to, and the oracle encodes and
decodes every input shape tests/test_variants_gpu.py compares the kernels with.  The builders of
those shapes live here so that both modules make the same inputs."""
from __future__ import annotations

import importlib

import numpy as np
import pytest

from tests import variants as V
from tests.test_tuning import KNOBS

INT32_MAX = (1 << 31) - 1

_REF: dict = {}


class Ref:
    """Host columns of one shape with the oracle's rows, offsets and decoded columns: computed
    once, shared, never modified."""

    def __init__(self, oracle, fields, host, n):
        self.fields, self.host, self.n = list(fields), host, n
        self.rows, self.offs = oracle.encode(self.fields, host, n)
        self.cols = oracle.decode(self.fields, self.rows, self.offs, n)


def cached(key, make) -> Ref:
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


# ---- builders of the shapes in tests/variants.py ------------------------------------------------
def fixed_fields(schema):
    from fury_amd import types as T
    from fury_amd.workloads import SCHEMAS
    if schema == "struct100":
        return SCHEMAS[schema]
    return [T.not_null_field(f"f{i:03d}", T.INT64) for i in range(V.FIXED[schema][0])]


def fixed_ref(oracle, schema, n) -> Ref:
    from fury_amd.workloads import gen_columns

    def make():
        fields = fixed_fields(schema)
        return Ref(oracle, fields, gen_columns(schema, fields, n, seed=n + len(fields)), n)
    return cached(("fixed", schema, n), make)


def wide_ref(oracle, ncols, n, str_max, list_max=8) -> Ref:
    """_wide_fields(ncols): 10 % nulls, list and element nulls."""
    from fury_amd.workloads import gen_columns
    from tests.test_device import _wide_fields

    def make():
        fields = _wide_fields(ncols)
        host = gen_columns("wide", fields, n, seed=ncols * 13 + n, null_pct=10, str_max=str_max,
                           list_max=list_max, list_null_pct=10, elem_null_pct=10)
        return Ref(oracle, fields, host, n)
    return cached(("wide", ncols, n, str_max, list_max), make)


def reg_fields(schema):
    """"mixed", or "<_REG_MODES key>:<fields>" as tests/test_device.py builds them."""
    from fury_amd import types as T
    from fury_amd.workloads import SCHEMAS
    from tests.test_device import _REG_MODES
    if ":" not in schema:
        return SCHEMAS[schema]
    mode, ncols = schema.split(":")
    kinds = _REG_MODES[mode]
    out = []
    for i in range(int(ncols)):
        k = kinds[i % len(kinds)]
        out.append(T.array_field(f"f{i:02d}", T.INT64) if k == "list" else T.field(f"f{i:02d}", k))
    return out


def reg_ref(oracle, schema, n, str_max=40, list_max=9) -> Ref:
    from fury_amd.workloads import gen_columns

    def make():
        fields = reg_fields(schema)
        host = gen_columns("wide", fields, n, seed=n + 7 * len(fields), null_pct=10,
                           str_max=str_max, list_max=list_max, list_null_pct=10, elem_null_pct=10)
        return Ref(oracle, fields, host, n)
    return cached(("reg", schema, n, str_max, list_max), make)


# The forced tile of tuning var_dec_rows runs only when its estimated output images fit half the
# decode's LDS budget (var.hip dec_tile_plan: images = 1.08 x R rows x the payload bytes per row of
# the outputs + 80 B per string column, 160 B per list column with element validity, rounded up to
# 1 KiB, against (80 KiB - 1 KiB) / 2).  A leg whose str_max = 40 / list_max = 9 inputs are past
# that halves both until the estimate, taken from the generated columns, is inside.
_IMG_BUDGET = (80 * 1024 - 1024) // 2


def reg_image_bytes(ref: Ref, R: int) -> int:
    from fury_amd import types as T
    per_row, fix = 0.0, 0
    for f, c in zip(ref.fields, ref.cols):
        if f.type_id in (T.STRING, T.BINARY):
            per_row += int(c.offsets[ref.n]) / ref.n
            fix += 80
        elif f.type_id == T.LIST:
            per_row += int(c.offsets[ref.n]) * (8 + 1 / 8) / ref.n
            fix += 160
    return (int(per_row * R * 1.08 + fix) + 1023) & ~1023


def reg_forced_ref(oracle, schema, n, R) -> Ref:
    """The largest of str_max / list_max = 40 / 9, 20 / 4, 10 / 2, 5 / 1 whose forced R-row tile
    the plan accepts, with a tenth of the budget to spare."""
    for str_max, list_max in ((40, 9), (20, 4), (10, 2), (5, 1)):
        ref = reg_ref(oracle, schema, n, str_max, list_max)
        if reg_image_bytes(ref, R) <= _IMG_BUDGET * 9 // 10:
            return ref
    raise AssertionError(f"{schema}: no input fits a forced {R}-row tile")


def cover_ref(oracle, name, n, knobs) -> Ref:
    from fury_amd.workloads import SCHEMAS, gen_columns

    def make():
        fields = SCHEMAS[name]
        return Ref(oracle, fields, gen_columns(name, fields, n, seed=n + 3, **knobs), n)
    return cached(("cover", name, n, tuple(sorted(knobs.items()))), make)


def nested_ref(oracle, name, n) -> Ref:
    from fury_amd.beans import beans_to_columns
    from tests.test_tree import _beans, _schemas

    def make():
        fields = _schemas()[name]
        return Ref(oracle, fields, beans_to_columns(fields, _beans(fields, n, len(name) * 29)), n)
    return cached(("nested", name, n), make)


# ---- completeness -----------------------------------------------------------------------------
def test_every_knob_is_in_exactly_one_table():
    tables = {"MATRIX": V.MATRIX, "ELSEWHERE": V.ELSEWHERE, "EXEMPT": V.EXEMPT}
    for key in KNOBS:
        where = [name for name, t in tables.items() if key in t]
        assert len(where) == 1, f"{key}: in {where or 'no table'} of tests/variants.py"
    for name, t in tables.items():
        assert not set(t) - set(KNOBS), f"{name}: {sorted(set(t) - set(KNOBS))} are no knobs"
    assert set(V.EXEMPT) == {"walk_skip", "var_skip"}


def test_matrix_covers_the_legal_values():
    """The default of every knob is a leg; a value left out for a fault is in KNOWN_BAD, and only
    there."""
    for key, values in V.MATRIX.items():
        default, legal, _, _ = KNOBS[key]
        assert default in values, key
        assert len(set(values)) == len(values), key
        assert not set(values) & set(V.KNOWN_BAD.get(key, {})), key
    assert not set(V.KNOWN_BAD) - set(V.MATRIX)
    every = {"fixed_enc": range(5), "fixed_dec": range(4), "var_wide": range(2),
             "walk_prefetch": range(4), "wide_threads": (256, 512, 1024),
             "wide_enc_threads": (256, 512, 1024), "walk_threads": (64, 128, 256),
             "var_dec_cover": (50, 95, 100), "var_dec_rows": (0, 64, 192, 320, 512),
             "wide_walk_row": (0, 896, INT32_MAX)}
    for key, want in every.items():
        have = set(V.MATRIX[key]) | set(V.KNOWN_BAD.get(key, {}))
        assert have == set(want), key


@pytest.mark.parametrize("key", sorted(V.ELSEWHERE))
def test_elsewhere_targets_resolve(key):
    path, _, name = V.ELSEWHERE[key].partition("::")
    assert path.endswith(".py") and name.startswith("test_"), V.ELSEWHERE[key]
    module = importlib.import_module(path[:-3].replace("/", "."))
    assert callable(getattr(module, name, None)), V.ELSEWHERE[key]


@pytest.mark.parametrize("key", sorted(V.MATRIX))
def test_matrix_values_are_accepted(key):
    from fury_amd import _native as N
    L = N.lib()
    k = key.encode()
    saved = L.fury_get_tuning(k)
    try:
        assert saved == KNOBS[key][0]
        for value in V.MATRIX[key]:
            assert L.fury_set_tuning(k, value) == 0, (key, value, N.last_error())
            assert L.fury_get_tuning(k) == value, (key, value)
    finally:
        assert L.fury_set_tuning(k, saved) == 0
    assert L.fury_get_tuning(k) == KNOBS[key][0]


# ---- the shapes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("schema", sorted(V.FIXED))
def test_fixed_schemas_land_in_their_tile_class(schema):
    from fury_amd.encoder import Schema
    ncols, size, R = V.FIXED[schema]
    fields = fixed_fields(schema)
    s = Schema(fields)
    assert len(fields) == ncols and s.is_fixed
    assert s.fixed_size == size == (ncols + 63) // 64 * 8 + 8 * ncols
    assert V.rows_per_tile(s.fixed_size) == R
    assert all(not f.nullable for f in fields)       # the fast path: 8-byte columns, no validity
    assert V.FIXED_TAIL_N * V.FIXED["struct100"][1] > 51 * 1024 > 0


def _check_ref(ref: Ref):
    """The oracle's own round trip: int32-sized, and the decode gives the inputs back."""
    from tests.helpers import assert_columns_equal
    assert ref.rows.dtype == np.uint8 and ref.rows.size < INT32_MAX
    if ref.offs is not None:
        assert len(ref.offs) == ref.n + 1 and int(ref.offs[ref.n]) == ref.rows.size
    assert_columns_equal(ref.fields, ref.cols, ref.host, ref.n)


@pytest.mark.parametrize("schema", sorted(V.FIXED))
def test_oracle_makes_the_fixed_references(oracle, schema):
    size, R = V.FIXED[schema][1:]
    for n in V.fixed_ns(R) + ([V.FIXED_TAIL_N] if schema == "struct100" else []):
        ref = fixed_ref(oracle, schema, n)
        assert ref.rows.size == n * size
        _check_ref(ref)


@pytest.mark.parametrize("ncols", sorted({k for k, _, _ in V.VAR_WIDE + V.WIDE_THREADS}))
def test_oracle_makes_the_wide_references(oracle, ncols):
    shapes = {s for s in V.VAR_WIDE + V.WIDE_THREADS if s[0] == ncols}
    if ncols in V.WALK_FLAT:
        shapes.add((ncols, V.WALK_FLAT_N, 40))
    if ncols == 33:
        shapes |= {(33, V.AUTO_N, m) for m in V.AUTO_STR_MAX}
    for k, n, str_max in sorted(shapes):
        _check_ref(wide_ref(oracle, k, n, str_max))


@pytest.mark.parametrize("schema", V.REG_SCHEMAS)
def test_oracle_makes_the_forced_tile_references(oracle, schema):
    for R in V.REG_ROWS:
        for n in (1300, 2 * R + 1):
            ref = reg_forced_ref(oracle, schema, n, R)
            _check_ref(ref)
            assert reg_image_bytes(ref, R) <= _IMG_BUDGET
    if schema == "mixed":      # the leg the plan must refuse
        assert reg_image_bytes(reg_ref(oracle, "mixed", 1300, 600), 512) > _IMG_BUDGET


def test_oracle_makes_the_cover_and_walk_references(oracle):
    for name, n, knobs in V.COVER:
        _check_ref(cover_ref(oracle, name, n, knobs))
    for name in V.WALK_NESTED:
        ref = nested_ref(oracle, name, V.WALK_NESTED_N)
        assert int(ref.offs[ref.n]) == ref.rows.size < INT32_MAX
