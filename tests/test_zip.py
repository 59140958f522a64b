"""Zip on the GPU (fury_row_zip, RowEncoder.zip_fields / zip_fields_into / bind_zip_fields /
with_fields): the whole output buffer, 4096 guard bytes on each side included, and the whole
out_offsets equal the numpy model of tests/test_zip_model.py (pinned there to the oracle), computed
from the source bytes alone.  Marked gpu."""
from __future__ import annotations

import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from fury_amd import types as T  # noqa: E402
from tests.helpers import assert_columns_equal  # noqa: E402
from tests.test_select import (COUNTS, FILL, GUARD, VALUE_EDITS, _get, _is_null, _put,  # noqa: E402
                               _slot_pos, _upload, assert_same, source)
from tests.test_select_model import Want, expect_select  # noqa: E402
from tests.test_zip_model import Source, expect_zip, split_picks  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


class Part:
    """Rows that are not the oracle's own (the halves of a split batch) as a source: the attributes
    of tests.test_select._Src that uploading and modelling need."""

    def __init__(self, dev, fields, rows, offs, n):
        from fury_amd.encoder import Encoders
        self.dev, self.fields, self.rows, self.offs, self.n = dev, list(fields), rows, offs, n
        self.enc = Encoders.bean(self.fields, device=dev)
        self.fixed = bool(self.enc.schema().is_fixed)


def split_fixed(src):
    """The two halves of tests.test_zip_model.split_picks of a fixed-width batch the oracle wrote (its
    null slots are 0, so selecting is a gather of bits and slots), and the restoring picks."""
    s1, s2, restore = split_picks(len(src.fields))
    n, bm = src.n, src.enc.schema().bitmap_bytes
    rows = src.rows.reshape(n, -1)
    bits = np.unpackbits(rows[:, :bm], axis=1, bitorder="little")
    slots = rows[:, bm:].reshape(n, -1, 8)
    parts = []
    for sel in (s1, s2):
        pad = np.zeros((n, -len(sel) % 64), np.uint8)
        half = np.concatenate([np.packbits(np.concatenate([bits[:, sel], pad], axis=1), axis=1,
                                           bitorder="little"), slots[:, sel].reshape(n, -1)], axis=1)
        data = np.ascontiguousarray(half).reshape(-1)
        offs = np.arange(n + 1, dtype=np.int64) * half.shape[1]
        if n <= 65:
            h = expect_select(src.rows, src.offs, n, src.fields, sel)
            assert not h.bad and np.array_equal(h.data, data) and np.array_equal(h.offs, offs)
        parts.append(Part(src.dev, [src.fields[k] for k in sel], data, offs, n))
    return parts, restore


def resolve(srcs, picks):
    return srcs[0].enc._picks([s.enc for s in srcs], picks)


def model(srcs, picks, edits=None):
    edits = edits or {}
    return expect_zip([Source(*edits.get(i, (s.rows, s.offs)), s.n, s.fields)
                       for i, s in enumerate(srcs)], resolve(srcs, picks))


def check_zip(srcs, picks, what, cap=None, out_shift=0, measure=False, stream=None, bound=False,
              calls=1, edits=None, with_offsets=True, batches=None, want=None):
    """One call into guarded buffers, everything compared.  edits: {source index: (rows, offs)} host
    copies uploaded in place of the source's own bytes; batches: uploaded batches to use (aliasing)."""
    dev, n = srcs[0].dev, srcs[0].n
    edits = edits or {}
    w = want if want is not None else model(srcs, picks, edits)
    cap = len(w.data) if cap is None else cap
    if batches is None:
        batches = [_upload(s, 8 * (i & 1), *edits.get(i, (None, None))) for i, s in enumerate(srcs)]
    t = torch.full((GUARD + 16 + cap + GUARD,), FILL, dtype=torch.uint8, device=dev)
    assert t.data_ptr() % 16 == 0
    at = GUARD + out_shift
    out = t[at:at + cap]
    ooffs = torch.full((n + 2,), -7, dtype=torch.int64, device=dev)
    others = [(s.enc, b) for s, b in zip(srcs[1:], batches[1:])]
    args = (batches[0], others, picks, None if measure else out, ooffs[:n + 1] if with_offsets else None)
    torch.cuda.synchronize()
    if bound:
        call = srcs[0].enc.bind_zip_fields(*args, stream=stream)
        for _ in range(calls):
            call()
    else:
        for _ in range(calls):
            srcs[0].enc.zip_fields_into(*args, stream=stream)
    torch.cuda.synchronize()
    assert_same(ooffs.cpu().numpy(), np.concatenate([w.offs, [-7]]) if with_offsets
                else np.full(n + 2, -7, np.int64), f"{what}: out_offsets")
    expect = np.full(t.numel(), FILL, np.uint8)
    if not measure:
        k = min(cap & ~7, len(w.data))             # a capacity off a multiple of 8 is rounded down
        expect[at:at + k] = w.data[:k]
    assert_same(t.cpu().numpy(), expect, f"{what}: output buffer")
    return w


def interleave(srcs, slots):
    """Picks that take slots[s] of source s in turn."""
    out = []
    for i in range(max(len(x) for x in slots)):
        out += [(s, slots[s][i]) for s in range(len(srcs)) if i < len(slots[s])]
    return out


# 1. the fixed kernel -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
def test_struct100_halves_rezipped(dev, n):
    src = source(dev, "struct100", n)
    parts, restore = split_fixed(src)
    assert all(p.fixed for p in parts)
    want = Want()
    want.data, want.offs, want.bad = src.rows, src.offs, []       # the source bytes themselves
    if n <= 65:
        w = model(parts, restore)
        assert not w.bad and np.array_equal(w.data, src.rows) and np.array_equal(w.offs, src.offs)
    for out_shift in (0, 8):
        check_zip(parts, restore, f"struct100 halves n={n} shift {out_shift}", out_shift=out_shift,
                  with_offsets=not out_shift, want=want)
    src.enc.device_status()


@pytest.mark.parametrize("npicks", [15, 16, 64, 65, 130])
def test_fixed_picks_of_a_fixed_and_a_variable_source(dev, npicks):
    """struct100 (row_offsets NULL) and the 65 INT32 fields of `wide` (rows at row_offsets), across the
    ballot threshold and one, two and three bitmap words."""
    n = 257
    srcs = [source(dev, "struct100", n), source(dev, "wide", n)]
    assert srcs[0].fixed and not srcs[1].fixed
    picks = interleave(srcs, [list(range(99, -1, -1)), list(range(0, 130, 2))])[:npicks]
    assert srcs[0].enc.zipped_encoder([srcs[1].enc], picks).schema().is_fixed
    w = model(srcs, picks)
    assert not w.bad and len(w.data) == n * (((npicks + 63) // 64) * 8 + 8 * npicks)
    for out_shift in (0, 8):
        check_zip(srcs, picks, f"{npicks} fixed picks shift {out_shift}", out_shift=out_shift,
                  with_offsets=not out_shift, want=w)
    srcs[0].enc.device_status()


# 2. the three-pass path ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
def test_foo_and_struct100(dev, n):
    srcs = [source(dev, "foo", n), source(dev, "struct100", n)]
    picks = interleave(srcs, [["f5", "f4", "f3", "f2", "f1"], list(range(3, 100, 10))])
    w = model(srcs, picks)
    assert not w.bad
    for out_shift in (0, 8):
        check_zip(srcs, picks, f"foo + struct100 n={n} shift {out_shift}", out_shift=out_shift, want=w)
    srcs[0].enc.device_status()


def test_mixed_and_value_sizes(dev):
    """Value sizes 0, 1, 7, 8, 9, 300 and nulls, and one value of 70,000 bytes across several spans."""
    n = 65
    srcs = [source(dev, "mixed", n), source(dev, "sizes", n)]
    assert int(srcs[1].offs[18] - srcs[1].offs[17]) > 70000
    for picks in (interleave(srcs, [list(range(len(srcs[0].fields))), ["t", "id", "s"]]),
                  [(1, "s"), (0, "s2")], [(0, "s1"), (1, "t"), (1, "s"), (0, "a")]):
        w = model(srcs, picks)
        assert not w.bad
        for out_shift in (0, 8):
            check_zip(srcs, picks, f"mixed + sizes {picks} shift {out_shift}", out_shift=out_shift,
                      want=w)
    srcs[0].enc.device_status()


def test_four_wide_sources_520_picks(dev):
    """The table beyond the argument block and beyond its LDS staging; sources 0 / 2 and 1 / 3 are the
    same batch."""
    n = 65
    src = source(dev, "wide", n)
    picks = [(j % 4, (37 * (j // 4) + 11 * (j % 4)) % 130) for j in range(520)]
    assert len(set(picks)) == 520
    b0, b1 = _upload(src), _upload(src, 8)
    w = model([src] * 4, picks)
    assert not w.bad
    for out_shift in (0, 8):
        check_zip([src] * 4, picks, f"4 x wide, 520 picks, shift {out_shift}", out_shift=out_shift,
                  batches=[b0, b1, b0, b1], want=w)
    src.enc.device_status()


@pytest.mark.parametrize("n", [65, 4097])
def test_the_same_batch_as_two_sources(dev, n):
    src = source(dev, "foo", n)
    b = _upload(src)
    picks = [(1, "f5"), (0, "f1"), (0, "f5"), (1, "f3"), (1, "f1"), (0, "f2")]
    w = check_zip([src, src], picks, f"foo twice n={n}", batches=[b, b])
    assert not w.bad
    src.enc.device_status()


# 3. forms ---------------------------------------------------------------------------------------------------------
def test_capacities_and_the_measure_form(dev):
    n = 257
    srcs = [source(dev, "foo", n), source(dev, "mixed", n)]
    picks = [(0, "f5"), (1, "s2"), (0, "f1"), (1, "a"), (0, "f3")]
    w = model(srcs, picks)
    total = len(w.data)
    assert total > 2048
    for cap in (0, 8, int(w.offs[1]), total - 8, total):
        for out_shift in (0, 8):
            check_zip(srcs, picks, f"capacity {cap} of {total}", cap=cap, out_shift=out_shift, want=w)
    check_zip(srcs, picks, "measure form", measure=True, want=w)
    srcs[0].enc.device_status()


def test_write_pass_rounds_and_end_words(dev):
    """tests.test_select.test_write_pass_rounds_and_end_words for zip_write, which stages 512 rows a
    round: 24 + 2049 x 16 bytes are three rounds in the second span, 8 mod 16 in all; capacities inside a
    row, on and off a multiple of 8.  (A value across several spans: test_mixed_and_value_sizes.)"""
    src = source(dev, "nulls", 2050)
    picks = [(1, "s")]
    w = model([src, src], picks)
    total = len(w.data)
    assert total == 24 + 2049 * 16 and total % 16 == 8 and not w.bad
    for out_shift in (0, 8):
        for cap in (None, total - 24, total - 20):
            check_zip([src, src], picks, f"nulls shift {out_shift} capacity {cap}", cap=cap,
                      out_shift=out_shift, want=w)
    src.enc.device_status()


def test_fixed_capacity_and_measure_form(dev):
    from fury_amd.encoder import CapacityError
    n = 257
    srcs = [source(dev, "struct100", n), source(dev, "foo", n)]
    picks = [(0, 3), (1, "f1"), (0, 13)]
    check_zip(srcs, picks, "fixed measure form", measure=True)
    check_zip(srcs, picks, "fixed spare capacity", cap=n * 32 + 24)
    with pytest.raises(CapacityError, match="rows of 32 bytes"):
        check_zip(srcs, picks, "fixed short capacity", cap=n * 32 - 8)
    srcs[0].enc.device_status()


def test_zip_of_no_rows(dev):
    from fury_amd.encoder import Encoders, RowBatch
    from fury_amd.workloads import SCHEMAS
    a = Encoders.bean(SCHEMAS["foo"], device=dev)
    b = Encoders.bean(SCHEMAS["struct100"], device=dev)
    ea = RowBatch(torch.zeros(16, dtype=torch.uint8, device=dev)[:0],
                  torch.zeros(1, dtype=torch.int64, device=dev), 0, a.schema_hash)
    eb = RowBatch(torch.zeros(16, dtype=torch.uint8, device=dev)[:0], None, 0, b.schema_hash)
    out = torch.full((64,), FILL, dtype=torch.uint8, device=dev)
    for picks in ([(0, "f5"), (1, 7)], [(0, "f1"), (1, 7)]):
        ooffs = torch.full((2,), -7, dtype=torch.int64, device=dev)
        a.zip_fields_into(ea, [(b, eb)], picks, out, ooffs[:1])
        torch.cuda.synchronize()
        assert ooffs.tolist() == [0, -7] and bool((out == FILL).all())
    a.zip_fields_into(ea, [(b, eb)], [(0, "f1"), (1, 7)], out, None)
    got = a.zip_fields(ea, [(b, eb)], [(0, "f5"), (1, 7)])
    assert got.nrows == 0 and got.rows.numel() == 0 and got.row_offsets.tolist() == [0]
    assert got.schema_hash == a.zipped_encoder([b], [(0, "f5"), (1, 7)]).schema_hash
    a.device_status()


def test_side_stream_and_bound_twice(dev):
    s = torch.cuda.Stream(device=dev)
    n = 4097
    srcs = [source(dev, "foo", n), source(dev, "struct100", n)]
    for picks in ([(1, 3), (0, "f1"), (1, 13)], [(0, "f5"), (1, 3), (0, "f3"), (0, "f1")]):
        w = model(srcs, picks)
        check_zip(srcs, picks, f"{picks}: zip_fields_into on a side stream", stream=s, out_shift=8, want=w)
        check_zip(srcs, picks, f"{picks}: bind_zip_fields called twice", bound=True, calls=2, want=w)
        check_zip(srcs, picks, f"{picks}: bound twice on a side stream", bound=True, calls=2, stream=s,
                  want=w)
        srcs[0].enc.device_status(s)
        srcs[0].enc.device_status()


def test_zip_fields_returns_a_batch(dev):
    n = 257
    srcs = [source(dev, "foo", n), source(dev, "struct100", n)]
    for picks, fixed in (([(0, "f5"), (1, 3), (0, "f3"), (0, "f1")], False), ([(1, 3), (0, "f1")], True)):
        w = model(srcs, picks)
        got = srcs[0].enc.zip_fields(_upload(srcs[0]), [(srcs[1].enc, _upload(srcs[1]))], picks)
        child = srcs[0].enc.zipped_encoder([srcs[1].enc], picks)
        assert got.nrows == n and got.schema_hash == child.schema_hash
        assert_same(got.rows.cpu().numpy(), w.data, f"zip_fields {picks}: rows")
        if fixed:
            assert got.row_offsets is None
        else:
            assert_same(got.row_offsets.cpu().numpy(), w.offs, f"zip_fields {picks}: offsets")


def test_with_fields_replaces_and_appends(dev):
    from fury_amd.encoder import Encoders, RowBatch, column_to_host
    from fury_amd.workloads import gen_columns
    from oracle import oracle as O
    n = 257
    src = source(dev, "mixed", n)
    names = [f.name for f in src.fields]
    k = names.index("s2")
    ofields = [T.field("extra", T.INT64), T.field("s2", T.STRING)]
    ohost = gen_columns(None, ofields, n, seed=21, null_pct=20, str_max=40)
    orows, ooffs = O.encode(ofields, ohost, n)
    other = Encoders.bean(ofields, device=dev)
    ob = RowBatch(torch.from_numpy(np.asarray(orows, np.uint8).copy()).to(dev),
                  torch.from_numpy(np.asarray(ooffs, np.int64).copy()).to(dev), n, other.schema_hash)
    enc, got = src.enc.with_fields(_upload(src), other, ob)
    fields = list(enc.schema().fields)
    assert [f.name for f in fields] == names + ["extra"] and got.schema_hash == enc.schema_hash
    cols = list(src.host)
    cols[k] = ohost[1]
    cols.append(ohost[0])
    want, want_offs = O.encode(fields, cols, n)                  # the joined columns, as rows
    dec = [column_to_host(c) for c in enc.decode_batch(got)]
    assert_columns_equal(fields, dec, O.decode(fields, want, want_offs, n), n)
    assert_same(got.rows.cpu().numpy(), np.asarray(want, np.uint8), "with_fields: rows")
    assert_same(got.row_offsets.cpu().numpy(), np.asarray(want_offs, np.int64), "with_fields: offsets")


# 4. identities on the device ---------------------------------------------------------------------------------------
def _select_on_device(src, sel, rows=None, offs=None, reports=()):
    """fury_row_select into exact buffers; reports: the rows either call may report (none: clean)."""
    n = src.n
    batch = _upload(src, 0, rows, offs)
    fixed = src.enc.selected_encoder(sel).schema().is_fixed
    o = torch.empty(n + 1, dtype=torch.int64, device=src.dev)
    src.enc.select_fields_into(batch, sel, None, o)
    total = int(o[n].item())
    if reports:                                               # a pending error would fail the next call
        assert _reported_row(src.enc) in reports
    out = torch.empty(max(total, 16), dtype=torch.uint8, device=src.dev)
    src.enc.select_fields_into(batch, sel, out, None if fixed else o)
    torch.cuda.synchronize()
    if reports:
        assert _reported_row(src.enc) in reports
    w = Want()
    w.data, w.offs, w.bad = out[:total].cpu().numpy(), o.cpu().numpy(), None
    return w


@pytest.mark.parametrize("name", ["foo", "beana", "struct100"])
def test_one_source_equals_select_fields(dev, name):
    src = source(dev, name, 257)
    nf = len(src.fields)
    for sel in (list(range(nf - 1, -1, -2)), [nf // 2], list(range(nf))):
        want = _select_on_device(src, sel)
        src.enc.device_status()
        check_zip([src], [(0, k) for k in sel], f"{name} {sel}: zip of one source = select", want=want)
    src.enc.device_status()


def test_split_and_rezip_on_the_device(dev):
    """zip of select_fields(A, S1) and select_fields(A, S2) with the restoring picks is A."""
    for name in ("foo", "beana"):
        src = source(dev, name, 257)
        s1, s2, restore = split_picks(len(src.fields))
        a = _upload(src)
        h1, h2 = src.enc.select_fields(a, s1), src.enc.select_fields(a, s2)
        e1, e2 = src.enc.selected_encoder(s1), src.enc.selected_encoder(s2)
        got = e1.zip_fields(h1, [(e2, h2)], restore)
        assert got.schema_hash == src.enc.schema_hash
        assert_same(got.rows.cpu().numpy(), src.rows, f"{name}: split and zipped back")
        assert_same(got.row_offsets.cpu().numpy(), src.offs, f"{name}: its offsets")


# 5. malformed input: edited host copies, every read bounds-checked by the rules -------------------------------------
def _reported_row(enc):
    from fury_amd.encoder import IndexOutOfBoundsException
    with pytest.raises(IndexOutOfBoundsException, match=r"row \d+ ") as e:
        enc.device_status()
    enc.device_status()                                       # raised once, then clear
    return int(re.search(r"row (\d+) ", str(e.value)).group(1))


def _check_malformed(srcs, picks, what, edits, victim=None, **kw):
    srcs[0].enc.device_status()
    w = check_zip(srcs, picks, what, edits=edits, out_shift=8, **kw)
    assert w.bad and (victim is None or w.bad == [victim]), (what, w.bad)
    assert _reported_row(srcs[0].enc) in w.bad, what
    return w


PICKS = [(1, "f5"), (0, "s"), (1, "f3"), (1, "f2"), (0, "id"), (1, "f1"), (0, "t")]


def _intact(w, clean, picks, r, s):
    """The fields picked from source s are, in output row r, what they are for clean input."""
    head, chead = w.data[int(w.offs[r]):], clean.data[int(clean.offs[r]):]
    for j, (src, _) in enumerate(picks):
        if src == s:
            assert (head[0] >> j) & 1 == (chead[0] >> j) & 1, j
            got, want = _get(head, 8 + 8 * j), _get(chead, 8 + 8 * j)
            assert got[1] == want[1], j                       # the same size (or fixed-width value)
            if not (chead[0] >> j) & 1 and j in (1, 6):       # STRING / BINARY: the same bytes
                assert head[got[0]:got[0] + got[1]].tobytes() == chead[want[0]:want[0] + want[1]].tobytes()


@pytest.mark.parametrize("edit", list(VALUE_EDITS))
def test_malformed_value_in_one_source(dev, edit):
    srcs = [source(dev, "sizes", 65), source(dev, "full", 65)]
    full = srcs[1]
    name, fn = VALUE_EDITS[edit]
    rows = full.rows.copy()
    pos, k = _slot_pos(full, 3, name)
    assert not _is_null(full, 3, k)
    _put(rows, pos, *fn(*_get(rows, pos), len(rows)))
    clean = model(srcs, PICKS)
    w = _check_malformed(srcs, PICKS, edit, {1: (rows, full.offs)}, victim=3)
    j = PICKS.index((1, name))
    head = w.data[int(w.offs[3]):int(w.offs[4])]
    assert (head[0] >> j) & 1 and not head[8 + 8 * j:16 + 8 * j].any()         # null, slot 0
    _intact(w, clean, PICKS, 3, 0)
    check_zip(srcs, PICKS, f"{edit}: the next call is clean", want=clean)
    srcs[0].enc.device_status()


def test_decimal_of_another_size_in_one_source(dev):
    srcs = [source(dev, "sizes", 65), source(dev, "beana", 65)]
    beana = srcs[1]
    rows = beana.rows.copy()
    pos, k = _slot_pos(beana, 3, "f16")
    assert not _is_null(beana, 3, k)
    off, size = _get(rows, pos)
    assert size == 16
    _put(rows, pos, off, 8)
    picks = [(1, "f17"), (0, "s"), (1, "f16"), (0, "id"), (1, "f1")]
    _check_malformed(srcs, picks, "decimal of 8 bytes", {1: (rows, beana.offs)}, victim=3)


def test_malformed_row_nulls_only_its_source(dev):
    srcs = [source(dev, "sizes", 65), source(dev, "full", 65)]
    full = srcs[1]
    F = full.enc.schema().fixed_size
    clean = model(srcs, PICKS)
    ones = sum(1 << j for j, (s, _) in enumerate(PICKS) if s == 1)

    def check(what, rows, offs, victim, row=3):
        w = _check_malformed(srcs, PICKS, what, {1: (rows, offs)}, victim=victim)
        assert w.data[int(w.offs[row])] & ones == ones, what      # every pick of source 1 is null
        _intact(w, clean, PICKS, row, 0)
        return w

    offs = full.offs.copy()
    offs[3] += 1                                                  # a row start off an 8-byte boundary
    check("odd row offset", full.rows, offs, 3)
    offs = full.offs.copy()
    offs[65] = offs[64] + F - 8                                   # the last header leaves the batch
    check("truncated last row", full.rows[:int(offs[65])].copy(), offs, 64, row=64)
    offs = full.offs.copy()
    offs[4] = offs[3] + F - 8                                     # an extent shorter than the header
    check("row 3 shorter than its header", full.rows, offs, None)


@pytest.mark.parametrize("npicks", [3, 40])
def test_malformed_row_in_the_fixed_kernel(dev, npicks):
    """Below and above the ballot threshold: only the INT32 picked from the misplaced row is null."""
    srcs = [source(dev, "struct100", 65), source(dev, "full", 65)]
    picks = [(0, k) for k in range(npicks - 1)]
    picks.insert(1, (1, "f1"))
    offs = srcs[1].offs.copy()
    offs[3] += 1
    w = _check_malformed(srcs, picks, f"odd row offset, {npicks} fixed picks", {1: (srcs[1].rows, offs)},
                         victim=3)
    clean = model(srcs, picks)
    diff = np.flatnonzero(w.data != clean.data)
    Fz = 8 + 8 * npicks
    assert len(diff) and all(3 * Fz <= i < 4 * Fz for i in diff)
    assert w.data[3 * Fz] == clean.data[3 * Fz] | 2 and not w.data[3 * Fz + 16:3 * Fz + 24].any()


def test_one_source_malformed_equals_select_fields(dev):
    """The same malformed buffers through fury_row_select and a one-source fury_row_zip."""
    src = source(dev, "full", 65)
    sel = ["f5", "f3", "f2", "f1"]
    idx = list(src.sel(sel))
    offs = src.offs.copy()
    offs[3] += 1
    rows = src.rows.copy()
    pos, _ = _slot_pos(src, 5, "f2")
    _put(rows, pos, len(rows) + 64, 8)
    for what, r, o in (("odd row offset", None, offs), ("off past the batch", rows, None)):
        src.enc.device_status()
        want = _select_on_device(src, idx, r, o, reports=(3, 5))
        check_zip([src], [(0, k) for k in idx], f"{what}: zip of one source = select", want=want,
                  edits={0: (src.rows if r is None else r, src.offs if o is None else o)})
        assert _reported_row(src.enc) in (3, 5)
        m = model([src], [(0, k) for k in idx], {0: (src.rows if r is None else r,
                                                     src.offs if o is None else o)})
        assert_same(want.data, m.data, f"{what}: and both equal the model")


def test_foreign_schema_hash_and_row_counts(dev):
    from fury_amd.encoder import ClassNotCompatibleException, IllegalArgumentException, RowBatch
    a, b = source(dev, "foo", 65), source(dev, "struct100", 65)
    ba, bb = _upload(a), _upload(b)
    with pytest.raises(ClassNotCompatibleException, match="Schema is not consistent"):
        a.enc.zip_fields(ba, [(b.enc, RowBatch(bb.rows, None, 65, b.enc.schema_hash + 1))], [(1, 0)])
    with pytest.raises(IllegalArgumentException, match="source 1 has 64 rows"):
        a.enc.zip_fields(ba, [(b.enc, RowBatch(bb.rows, None, 64, b.enc.schema_hash))], [(1, 0)])


def test_output_row_across_2g(dev):
    """Regression (found by tests/test_high_offsets_gpu.py::test_dense_select_zip): zip_write shared
    select_write's 32-bit narrowing of a word's position in its row, which sent the second word of
    every 16-byte chunk of the output row across byte 2^31 to a source position 2^32 too low.  Two
    sources over the same 40 rows of 64 and 48 MiB in turn: row 36 is that row."""
    import gc
    from tests.test_high_offsets_gpu import across_2g, check_across_2g
    enc, src, order, big, _ = across_2g(dev)
    picks = [(1, "id"), (0, "a")]
    try:
        def write(rows, offs):
            enc.zip_fields_into(big, [(enc, big)], picks, rows, offs)
            enc.device_status()
        check_across_2g(dev, enc.zip_fields(src, [(enc, src)], picks), order, write)
    finally:
        del big, _
        gc.collect()
        torch.cuda.empty_cache()
