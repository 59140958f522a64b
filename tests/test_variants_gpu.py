"""Every kernel variant a fury_set_tuning knob can select, against the oracle.

tests/variants.py MATRIX lists the knobs and values; each test here sets one (the default among
them, as the same test's control) and compares what the selected kernels write with
oracle.encode / oracle.decode of the same inputs: rows and row offsets byte for byte, decoded
columns with assert_columns_equal, as tests/test_device.py does.  Encodes read the generated
columns and decodes read the oracle's rows, so no leg depends on another variant of this library.
The shapes are the smallest that reach each variant's edges; nothing here measures speed.
Marked gpu."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import variants as V  # noqa: E402
from tests.helpers import assert_columns_equal  # noqa: E402
from tests.test_device import _dev_cols, _encode_measured, _roundtrip  # noqa: E402
from tests.test_tuning import KNOBS  # noqa: E402
from tests.test_variants import (Ref, cover_ref, fixed_ref, nested_ref,  # noqa: E402
                                 reg_forced_ref, reg_ref, wide_ref)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _lib():
    from fury_amd import _native as N
    return N.lib()


def _tune(key, v):
    from fury_amd import _native as N
    assert N.lib().fury_set_tuning(key.encode(), v) == 0, (key, v, N.last_error())


def _get(key):
    return _lib().fury_get_tuning(key.encode())


@pytest.fixture(autouse=True)
def _restore_knobs():
    """Every knob is put back after a test, and is then at its default."""
    saved = {k: _get(k) for k in KNOBS}
    yield
    for k, v in saved.items():
        _tune(k, v)
    for k in KNOBS:
        assert _get(k) == KNOBS[k][0], k


class _Case:
    """One reference on the device: the encoder, the input columns and the oracle's rows as a
    batch.  Made once per shape, shared by the knob values, never modified."""

    def __init__(self, ref: Ref, dev):
        from fury_amd.encoder import Encoders, RowBatch
        self.ref, self.dev, self.n, self.fields = ref, dev, ref.n, ref.fields
        self.enc = Encoders.bean(ref.fields, device=dev)
        self.dcols = _dev_cols(ref.host, dev)
        rows = torch.from_numpy(ref.rows).to(dev)
        offs = None if self.enc.schema().is_fixed else torch.from_numpy(ref.offs).to(dev)
        self.batch = RowBatch(rows, offs, ref.n, self.enc.schema_hash)


_CASES: dict = {}


def _case(ref: Ref, dev) -> _Case:
    if id(ref) not in _CASES:
        _CASES[id(ref)] = _Case(ref, dev)
    return _CASES[id(ref)]


def _same(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    want = want.cpu().numpy() if hasattr(want, "cpu") else want
    got = np.ascontiguousarray(got).view(np.uint8).reshape(-1)
    want = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
    assert got.shape == want.shape, f"{what}: {got.shape} bytes, the oracle has {want.shape}"
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        raise AssertionError(f"{what}: {len(bad)} bytes differ, first at {bad[:8]}")


def _check_encode(c: _Case, what):
    """measure + encode: rows and offsets."""
    b = c.enc.encode_batch(c.dcols, c.n)
    if b.row_offsets is not None:
        _same(b.row_offsets, c.ref.offs, f"{what}: row offsets")
    _same(b.rows, c.ref.rows, f"{what}: rows")


def _check_measured(c: _Case, what):
    rows, offs, total = _encode_measured(c.enc, c.dcols, c.n, c.dev)
    assert total == c.ref.rows.size, what
    _same(offs, c.ref.offs, f"{what}: measured row offsets")
    _same(rows[:total], c.ref.rows, f"{what}: measured rows")
    assert bool((rows[total:] == 0xEE).all()), f"{what}: bytes written past the rows"


def _check_cols(c: _Case, cols):
    from fury_amd.encoder import column_to_host
    assert_columns_equal(c.fields, [column_to_host(x) for x in cols], c.ref.cols, c.n)


def _check_arrow(c: _Case):
    from fury_amd.encoder import ArrowWriter
    w = ArrowWriter(c.enc)
    w.write(c.batch)
    _check_cols(c, w.finish())


# ---- fixed-width fast path: fixed_enc, fixed_dec ------------------------------------------------
class _Guarded:
    """n 8-byte values inside a 0x5A-filled buffer with 16 bytes in front and behind; `shift` 16
    puts them at a 16-byte aligned address, 8 at an 8- but not 16-byte aligned one."""

    def __init__(self, n, shift, dev):
        self.buf = torch.full((16 + 8 * n + 16,), 0x5A, dtype=torch.uint8, device=dev)
        assert self.buf.data_ptr() % 16 == 0 and shift in (8, 16)
        self.lo, self.hi = shift, shift + 8 * n
        self.values = self.buf[self.lo:self.hi]
        assert self.values.data_ptr() % 16 == (0 if shift == 16 else 8)

    def untouched_outside(self):
        return bool((self.buf[:self.lo] == 0x5A).all()) and bool((self.buf[self.hi:] == 0x5A).all())


def _fixed_encode(c: _Case, what, misalign=None):
    """encode_batch, and an encode into a guarded row buffer; `misalign`: that input column read
    from an address that is not 16-byte aligned."""
    from fury_amd.workloads import Column
    cols = list(c.dcols)
    g = None
    if misalign is not None:
        g = _Guarded(c.n, 8, c.dev)
        g.values.copy_(cols[misalign].values.view(torch.uint8))
        cols[misalign] = Column(values=g.values)
    _same(c.enc.encode_batch(cols, c.n).rows, c.ref.rows, f"{what}: rows")
    total = c.ref.rows.size
    out = torch.full((total + 64,), 0xEE, dtype=torch.uint8, device=c.dev)
    c.enc.encode_into(cols, c.n, out[:total], None)
    _same(out[:total], c.ref.rows, f"{what}: rows (encode_into)")
    assert bool((out[total:] == 0xEE).all()), f"{what}: bytes written past the rows"
    if g is not None:
        assert g.untouched_outside(), what
        _same(g.values, c.dcols[misalign].values, f"{what}: the input column")


def _fixed_decode(c: _Case, what, misalign=None):
    """decode_into without validity buffers (the fast path) into 0x5A-filled columns, each with
    guard bytes around it."""
    from fury_amd.workloads import Column
    gs = [_Guarded(c.n, 8 if k == misalign else 16, c.dev) for k in range(len(c.fields))]
    out = [Column(values=g.values) for g in gs]
    c.enc.decode_into(c.batch, out)
    torch.cuda.synchronize()
    for k, g in enumerate(gs):
        assert g.untouched_outside(), f"{what}: bytes written outside column {k}"
    _check_cols(c, out)


def _fixed_cases(oracle, dev, schema):
    R = V.FIXED[schema][2]
    return [_case(fixed_ref(oracle, schema, n), dev) for n in V.fixed_ns(R)]


@pytest.mark.parametrize("value", V.MATRIX["fixed_enc"])
@pytest.mark.parametrize("schema", sorted(V.FIXED))
def test_fixed_enc(oracle, dev, schema, value):
    """Each instantiation of encode_fixed_kernel the knob selects (U = 8 / 16 / 32 column loads in
    flight, DS = 8 stores, pair mode) at each tile height writes the oracle's rows for one row,
    ragged and full tiles, odd and even row counts, and writes nothing past them.  Pair mode (1)
    also with one input column at an address that is not 16-byte aligned, where it gives way to
    the default kernel."""
    for c in _fixed_cases(oracle, dev, schema):
        _tune("fixed_enc", value)
        what = f"{schema} n={c.n} fixed_enc={value}"
        _fixed_encode(c, what)
        if value == 1:
            _fixed_encode(c, what + " misaligned", misalign=len(c.fields) // 2)


@pytest.mark.parametrize("value", V.MATRIX["fixed_dec"])
@pytest.mark.parametrize("schema", sorted(V.FIXED))
def test_fixed_dec(oracle, dev, schema, value):
    """Each instantiation of decode_fixed_kernel the knob selects (pair mode with SU = 8 / 16 / 4
    column stores and D = 16 / 8 row loads in flight) decodes the oracle's rows to the oracle's
    columns and writes nothing outside them; with one output column at an address that is not
    16-byte aligned every value takes the non-pair kernel, with the same result.  int64x65 leaves
    the upper half of the last wave of a 64-row tile without a column."""
    for c in _fixed_cases(oracle, dev, schema):
        _tune("fixed_dec", value)
        what = f"{schema} n={c.n} fixed_dec={value}"
        _fixed_decode(c, what)
        _fixed_decode(c, what + " misaligned", misalign=len(c.fields) // 2)


@pytest.mark.parametrize("value", V.MATRIX["fixed_enc"])
def test_fixed_enc_tail_window(oracle, dev, value):
    """fixed_enc x fixed_enc_tail_kib: no window, exactly one 64-row Struct-100 tile (51 KiB) and
    a window larger than the batch pick the store policy of copy_tile inside each variant's
    store_tile<NT, DS>; the rows are the oracle's either way."""
    c = _case(fixed_ref(oracle, "struct100", V.FIXED_TAIL_N), dev)
    _tune("fixed_enc", value)
    for tail in (0, 64 * 816 // 1024, 1 << 18):
        _tune("fixed_enc_tail_kib", tail)
        _fixed_encode(c, f"struct100 n={c.n} fixed_enc={value} tail={tail}")


# ---- 17-256 flat fields: var_wide ---------------------------------------------------------------
@pytest.mark.parametrize("value", V.MATRIX["var_wide"])
@pytest.mark.parametrize("ncols,n,str_max", V.VAR_WIDE)
def test_var_wide(oracle, dev, ncols, n, str_max, value):
    """var_wide 0 routes a flat schema of 17-256 fields to encode_var_kernel<MetaMap> (past 64
    fields, with the column table in device memory, <MetaMapWide>), the exact-size measure to
    decode_measure_kernel / decode_measure_fix and the decode to the decoupled look-back
    decode_var_kernel; 1 (the default, the control) to the wide tiles.  Under lookback_help 0 and
    1 (every look-back computes its predecessor's aggregate itself): measure + encode,
    encode_measured, the exact-sized and the bound-sized decode and rows -> Arrow are the
    oracle's, and no look-back timed out."""
    c = _case(wide_ref(oracle, ncols, n, str_max), dev)
    _tune("var_wide", value)
    for help_ in ((0, 1) if value == 0 else (0,)):
        _tune("lookback_help", help_)
        what = f"{ncols} fields n={n} str_max={str_max} var_wide={value} lookback_help={help_}"
        _check_encode(c, what)
        _check_measured(c, what)
        _check_cols(c, c.enc.decode_batch(c.batch))
        _check_cols(c, c.enc.decode_batch(c.batch, sizing="bound"))
        _check_arrow(c)
    assert _get("lookback_timeouts") == 0


# ---- register-staged decode: var_dec_rows x var_dec_pipe, var_dec_cover -------------------------
@pytest.mark.parametrize("R", V.MATRIX["var_dec_rows"])
@pytest.mark.parametrize("schema", V.REG_SCHEMAS)
def test_var_dec_rows(oracle, dev, schema, R):
    """Forced R-row tiles of decode_var_reg (0: the planned tile, the control), one tile per
    workgroup and under both persistent two-stage forms of var_dec_pipe (the 3- and 6-column
    instances have them, the others run one tile per workgroup under every value): the oracle's
    columns, from 1,300 rows and from two tiles and a row.  A forced tile only runs when the plan
    accepts it, so every leg checks that var_dec_rows_rejected did not move (the inputs shrink with
    R until it does not, see tests/test_variants.py reg_forced_ref)."""
    _tune("var_dec_rows", R)
    for n in ((1300,) if R == 0 else (1300, 2 * R + 1)):
        ref = reg_ref(oracle, schema, n) if R == 0 else reg_forced_ref(oracle, schema, n, R)
        c = _case(ref, dev)
        for pipe in (0, 1, 2):
            _tune("var_dec_pipe", pipe)
            before = _get("var_dec_rows_rejected")
            cols = c.enc.decode_batch(c.batch)
            assert _get("var_dec_rows_rejected") == before, (schema, n, R, pipe)
            _check_cols(c, cols)
    assert _get("lookback_timeouts") == 0


def test_var_dec_rows_refused(oracle, dev):
    """Strings of up to 600 bytes: the images of a forced 512-row tile are past the budget, the
    plan refuses it and says so, and the planned tile decodes the oracle's columns."""
    c = _case(reg_ref(oracle, "mixed", 1300, str_max=600), dev)
    _tune("var_dec_rows", 512)
    before = _get("var_dec_rows_rejected")
    cols = c.enc.decode_batch(c.batch)
    assert _get("var_dec_rows_rejected") > before
    _check_cols(c, cols)


@pytest.mark.parametrize("cover", V.MATRIX["var_dec_cover"])
@pytest.mark.parametrize("name,n,gen", V.COVER)
def test_var_dec_cover(oracle, dev, name, n, gen, cover):
    """The share of a tile's row bytes the LDS stage must hold moves the planned tile rows and
    which rows are read from the stage and which from HBM; short rows, rows that outgrow the
    stage, and both output sizings (the bound one plans from over-estimated row sizes)."""
    c = _case(cover_ref(oracle, name, n, gen), dev)
    _tune("var_dec_cover", cover)
    _check_cols(c, c.enc.decode_batch(c.batch))
    _check_cols(c, c.enc.decode_batch(c.batch, sizing="bound"))
    _check_arrow(c)
    assert _get("lookback_timeouts") == 0


# ---- wide tiles: wide_threads, wide_enc_threads -------------------------------------------------
@pytest.mark.parametrize("threads,enc_threads", V.WIDE_THREAD_PAIRS)
@pytest.mark.parametrize("ncols,n,str_max", V.WIDE_THREADS)
def test_wide_threads(oracle, dev, ncols, n, str_max, threads, enc_threads):
    """The wide tiles (wide_engine 1, wide_enc_engine 1) with 256 / 512 / 1024 threads per 64-row
    tile on each side: encode, encode_measured, the plan decode and rows -> Arrow are the
    oracle's."""
    c = _case(wide_ref(oracle, ncols, n, str_max), dev)
    _tune("wide_engine", 1)
    _tune("wide_enc_engine", 1)
    _tune("wide_threads", threads)
    _tune("wide_enc_threads", enc_threads)
    what = f"{ncols} fields n={n} str_max={str_max} threads={threads}/{enc_threads}"
    _check_encode(c, what)
    _check_measured(c, what)
    _check_cols(c, c.enc.decode_batch(c.batch))
    _check_arrow(c)


# ---- row walk: walk_prefetch x walk_threads -----------------------------------------------------
def _walk_case(oracle, dev, schema):
    if isinstance(schema, int):
        return _case(wide_ref(oracle, schema, V.WALK_FLAT_N, 40), dev)
    return _case(nested_ref(oracle, schema, V.WALK_NESTED_N), dev)


def _walk_decode(c: _Case):
    """The plan decode (fury_decode_prepare / execute)."""
    _check_cols(c, c.enc._decode_nested(c.batch, True, False, None))


@pytest.mark.parametrize("threads", V.MATRIX["walk_threads"])
@pytest.mark.parametrize("schema", V.WALK_NESTED + V.WALK_FLAT)
def test_walk_prefetch_and_threads(oracle, dev, schema, threads):
    """The row walk (nested_decode 2; for the flat 33- and 200-field schemas wide_engine 2) with
    64 / 128 / 256 rows per count tile and each walk_prefetch: bit 1 adds the count pass's L2 pull,
    changes its LDS sizing and can halve the tile (walk_count_lds).  beana and the 200-field schema
    have more than walk_group_min counted slots, so they walk in field groups, where the library
    turns the prefetch off: on those two only the tile rows vary."""
    c = _walk_case(oracle, dev, schema)
    _tune("nested_decode", 2)
    _tune("wide_engine", 2)
    _tune("walk_threads", threads)
    for prefetch in V.MATRIX["walk_prefetch"]:
        _tune("walk_prefetch", prefetch)
        _walk_decode(c)


def test_walk_groups_with_count_prefetch(oracle, dev):
    """Field groups of about one counted slot (walk_group_min 0, walk_group_k 1) at walk_prefetch
    3 and 256-row tiles: the group cursors and the count pass's prefetch claim the same LDS."""
    c = _walk_case(oracle, dev, "nested7")
    for key, v in (("nested_decode", 2), ("walk_group_min", 0), ("walk_group_k", 1),
                   ("walk_prefetch", 3), ("walk_threads", 256)):
        _tune(key, v)
    _walk_decode(c)


# ---- auto engine: wide_walk_row -----------------------------------------------------------------
@pytest.mark.parametrize("threshold", V.MATRIX["wide_walk_row"])
@pytest.mark.parametrize("str_max", V.AUTO_STR_MAX)
def test_wide_walk_row(oracle, dev, str_max, threshold):
    """wide_engine and wide_enc_engine stay 0 (auto); the threshold sends batches whose average row
    is larger to the row walk: 0 every batch, INT32_MAX none, the default 896 bytes the long-string
    batch only.  Nothing observable says which engine ran, so this asserts only that whichever
    route the threshold picks encodes the oracle's rows and decodes the oracle's columns."""
    assert _get("wide_engine") == 0 and _get("wide_enc_engine") == 0
    c = _case(wide_ref(oracle, 33, V.AUTO_N, str_max), dev)
    _tune("wide_walk_row", threshold)
    what = f"33 fields str_max={str_max} wide_walk_row={threshold}"
    _check_encode(c, what)
    _check_measured(c, what)
    _check_cols(c, c.enc.decode_batch(c.batch))
    # the same through the library's own rows (tests/test_device.py _roundtrip)
    _roundtrip(oracle, None, c.n, dev, fields=c.fields, cols=c.ref.host)
