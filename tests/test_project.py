"""Projected decode on the GPU (fury_row_project / RowEncoder.project_batch): the selected columns
equal the oracle's decode of the same rows with those columns picked out, byte for byte; for flat
schemas also this library's own full decode.  Marked gpu."""
from __future__ import annotations

import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from fury_amd import types as T  # noqa: E402
from fury_amd.workloads import SCHEMAS, create_beana, gen_columns  # noqa: E402
from tests.helpers import as_u8, assert_columns_equal  # noqa: E402

GUARD = 4096


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


class _Case:
    """One encoded batch with its reference decodes, computed once and shared (never modified)."""

    def __init__(self, oracle, dev, fields, host, n, full=True):
        from fury_amd.encoder import Encoders, column_to_device, column_to_host
        self.fields, self.n, self.dev = list(fields), n, dev
        self.enc = Encoders.bean(self.fields, device=dev)
        self.batch = self.enc.encode_batch([column_to_device(c, dev) for c in host], n)
        self.rows = self.batch.rows.cpu().numpy()
        self.offs = None if self.batch.row_offsets is None else self.batch.row_offsets.cpu().numpy()
        self.ref = oracle.decode(self.fields, self.rows, self.offs, n)
        # this library's own full decode (flat schemas)
        self.own = ([column_to_host(c) for c in self.enc.decode_batch(self.batch)]
                    if full and not self.enc.nested else None)
        self._arrow = None

    def arrow(self):
        from fury_amd.encoder import ArrowWriter, column_to_host
        if self._arrow is None:
            w = ArrowWriter(self.enc)
            w.write(self.batch)
            self._arrow = [column_to_host(c) for c in w.finish()]
        return self._arrow

    def idx(self, select):
        return self.enc._select(select)

    def check(self, select, validity=True, arrow=False, batch=None, stream=None):
        from fury_amd.encoder import column_to_host
        idx = self.idx(select)
        sel_fields = [self.fields[k] for k in idx]
        cols = self.enc.project_batch(batch or self.batch, select, validity=validity, stream=stream,
                                      arrow=arrow)
        if stream is not None:
            self.enc.device_status(stream)
        got = [column_to_host(c) for c in cols]
        assert len(got) == len(idx)
        assert_columns_equal(sel_fields, got, [self.ref[k] for k in idx], self.n)
        if self.own is not None:
            assert_columns_equal(sel_fields, got, [self.own[k] for k in idx], self.n)
        if arrow:
            assert_columns_equal(sel_fields, got, [self.arrow()[k] for k in idx], self.n)
        return got


_CACHE: dict = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# 1. Struct-100 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4097])
def test_struct100_selections(oracle, dev, n):
    from fury_amd.encoder import RowBatch
    fields = SCHEMAS["struct100"]
    case = _cached(("struct100", n), lambda: _Case(oracle, dev, fields,
                                                   gen_columns("struct100", fields, n, seed=3), n))
    assert case.batch.row_offsets is None
    offs = (torch.arange(n + 1, dtype=torch.int64, device=dev) * case.enc.schema().fixed_size)
    explicit = RowBatch(case.batch.rows, offs, n, case.enc.schema_hash)
    for sel in ([0], [99], [0, 99], [7, 8, 9], [99, 0, 50], list(range(64))):
        case.check(sel)
        case.check(sel, batch=explicit)
    case.check(["f99", "f00", "f50"])                       # by name, order kept
    case.check([7, 8, 9], validity=False)


# 2. bitmap-word and piece boundaries ---------------------------------------------------------------
def _fields130():
    kinds = [T.BOOL, T.INT8, T.INT16, T.INT32, T.INT64, T.FLOAT32, T.FLOAT64, T.DATE32, T.TIMESTAMP]
    return [T.field(f"c{k:03d}", kinds[k % len(kinds)]) for k in range(130)]


@pytest.mark.parametrize("validity", [True, False])
def test_bitmap_word_and_piece_boundaries(oracle, dev, validity):
    fields = _fields130()
    n = 257
    case = _cached(("f130", n), lambda: _Case(oracle, dev, fields,
                                              gen_columns(None, fields, n, null_pct=30), n))
    bools = [k for k, f in enumerate(fields) if f.type_id == T.BOOL]
    for sel in ([63, 64], [127, 128, 129], [0, 129], bools):
        case.check(sel, validity=validity)


# 3. every flat kind --------------------------------------------------------------------------------
@pytest.mark.parametrize("arrow", [False, True])
@pytest.mark.parametrize("n", [1, 129, 2000])
def test_every_flat_kind(oracle, dev, n, arrow):
    fields = SCHEMAS["narrow"]
    case = _cached(("narrow", n), lambda: _Case(oracle, dev, fields,
                                                gen_columns("narrow", fields, n, seed=3), n))
    for f in fields:
        case.check([f.name], arrow=arrow)
    case.check(["h_dec", "i_bin", "k_ints"], arrow=arrow)
    case.check([f.name for f in fields], arrow=arrow)
    if not arrow:
        case.check(["i_bin", "k_ints", "a_bool"], validity=False)


# 4. string edge lengths ------------------------------------------------------------------------------
_STRINGS = ["", "x", "abcdefg", "abcdefgh", "abcdefghi", "é" * 37, None, "ü中😀", "z" * 300, None, "",
            "q" * 8191]


@pytest.mark.parametrize("lead", [0, 2])
def test_string_edge_lengths(oracle, dev, lead):
    from fury_amd.beans import beans_to_columns
    fields = ([T.field(f"p{j}", T.INT8) for j in range(lead)] +
              [T.field("a", T.STRING), T.field("b", T.BINARY)])
    beans = []
    for i, v in enumerate(_STRINGS):
        b = {"a": v, "b": (v.encode() if v is not None else None)}
        for j in range(lead):
            b[f"p{j}"] = (i * 7 + j) % 100
        beans.append(b)
    case = _Case(oracle, dev, fields, beans_to_columns(fields, beans), len(beans))
    case.check(["a"])
    case.check(["b"])
    case.check(["b", "a"], arrow=True)


# 5. list edge lengths --------------------------------------------------------------------------------
def test_list_edge_lengths(oracle, dev):
    from fury_amd.beans import beans_to_columns
    fields = [T.array_field("l", T.INT64), T.array_field("i", T.INT32),
              T.array_field("b", T.BOOL), T.array_field("s", T.INT16, elem_nullable=False)]
    lens = [0, 1, 63, 64, 65, 130, 2, 0]
    rng = np.random.default_rng(0)
    beans = []
    for k, m in enumerate(lens):
        if k == 6:
            beans.append({"l": None, "i": None, "b": None, "s": None})
            continue
        beans.append({
            "l": [None if (j % 7 == 3) else int(x) for j, x in
                  enumerate(rng.integers(-2**62, 2**62, m))],
            "i": [int(x) for x in rng.integers(-2**31, 2**31, m)],
            "b": [None if j % 5 == 0 else bool(j & 1) for j in range(m)],
            "s": [int(x) for x in rng.integers(-2**15, 2**15, m)],
        })
    case = _Case(oracle, dev, fields, beans_to_columns(fields, beans), len(beans))
    for f in fields:
        case.check([f.name])
        case.check([f.name], arrow=True)
    case.check(["s", "b", "l", "i"])


# 6. nested schemas -----------------------------------------------------------------------------------
def test_nested_beana(oracle, dev):
    from fury_amd.beans import beans_to_columns
    from fury_amd.encoder import UnsupportedOperationException
    fields = SCHEMAS["beana"]
    n = 65
    beans = [create_beana(3 if i % 5 else i % 4) for i in range(n)]
    case = _Case(oracle, dev, fields, beans_to_columns(fields, beans), n)
    assert case.enc.nested
    case.check(["f12", "f16", "f17", "bytes", "f3"])
    case.check(["f12", "f16", "f17", "bytes", "f3"], arrow=True)
    with pytest.raises(UnsupportedOperationException, match="bean_b"):
        case.enc.project_batch(case.batch, ["bean_b"])
    case.check(["f3"])                                    # the error left no state behind


def test_nested_row_test_schema(oracle, dev):
    from fury_amd.beans import beans_to_columns
    from fury_amd.encoder import UnsupportedOperationException
    from tests.test_device import _random_value
    fields = SCHEMAS["row_test"]
    n = 300
    rng = np.random.default_rng(12)
    beans = [{f.name: _random_value(f, rng) for f in fields} for _ in range(n)]
    case = _Case(oracle, dev, fields, beans_to_columns(fields, beans), n)
    assert case.enc.nested
    case.check(["f2", "f1", "f3"])
    with pytest.raises(UnsupportedOperationException, match="f5"):
        case.enc.project_batch(case.batch, ["f1", "f5"])


# 7. capacity -----------------------------------------------------------------------------------------
def test_capacity_clips_payload(oracle, dev):
    from fury_amd.encoder import CapacityError
    fields = SCHEMAS["mixed"]
    n = 3000
    case = _cached(("mixed", n), lambda: _Case(oracle, dev, fields,
                                               gen_columns("mixed", fields, n, seed=3), n))
    k = case.idx(["s2"])[0]
    want = case.ref[k]
    need = int(as_u8(want.offsets).view(np.int32)[n])
    half = need // 2
    assert half > 0
    buf = torch.full((half + GUARD,), 0xAB, dtype=torch.uint8, device=dev)
    cols = case.enc.alloc_projected(["s2"], n)
    cols[0].values = buf[:half]
    case.enc.project_into(case.batch, ["s2"], cols)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.array_equal(got[:half], as_u8(want.values)[:half])
    assert (got[half:] == 0xAB).all()
    offs = cols[0].offsets.cpu().numpy()
    assert np.array_equal(offs, as_u8(want.offsets).view(np.int32)[:n + 1])
    assert int(offs[n]) == need
    with pytest.raises(CapacityError, match="s2"):
        case.enc.check_capacity(cols, n, select=["s2"])
    cols[0].values = torch.empty(need, dtype=torch.uint8, device=dev)
    case.enc.project_into(case.batch, ["s2"], cols)
    case.enc.check_capacity(cols, n, select=["s2"])


# 8. corrupt rows -------------------------------------------------------------------------------------
def test_corrupt_slot_of_unselected_field_is_not_an_error(oracle, dev):
    from fury_amd.encoder import Encoders, IndexOutOfBoundsException, RowBatch, column_to_host
    fields = SCHEMAS["mixed"]
    n, victim = 257, 100
    host = gen_columns("mixed", fields, n, seed=5)
    rows, offs = oracle.encode(fields, host, n)
    rows = rows.copy()
    offs = np.asarray(offs, dtype=np.int64)
    enc = Encoders.bean(fields, device=dev)
    k = [f.name for f in fields].index("s1")
    base = int(offs[victim])
    rows[base + (k >> 3)] &= ~(1 << (k & 7)) & 0xFF                # s1 of the victim row: not null
    bad = rows.copy()
    total = int(offs[n])
    struct.pack_into("<Q", bad, base + enc.schema().bitmap_bytes + 8 * k,
                     (((total - base + 8) & 0xFFFFFFFF) << 32) | 5)
    null = rows.copy()
    null[base + (k >> 3)] |= 1 << (k & 7)
    ref = oracle.decode(fields, null, offs, n)              # the victim value decoded as null

    def batch_of(r):
        buf = np.full(len(r) + GUARD, 0xAB, np.uint8)
        buf[:len(r)] = r
        t = torch.from_numpy(buf).to(dev)
        return RowBatch(t[:len(r)], torch.from_numpy(offs).to(dev), n, enc.schema_hash)

    b = batch_of(bad)
    sel = ["a", "s3"]
    idx = enc._select(sel)
    got = [column_to_host(c) for c in enc.project_batch(b, sel)]      # device_status inside: clean
    assert_columns_equal([fields[i] for i in idx], got, [ref[i] for i in idx], n)
    enc.device_status()
    with pytest.raises(IndexOutOfBoundsException, match=f"row {victim} "):
        enc.project_batch(b, ["s1"])
    # the columns themselves: the victim decodes as null, nothing past the batch is read
    cols = enc.alloc_projected(["s1"], n)
    cols[0].values = torch.zeros(total, dtype=torch.uint8, device=dev)
    enc.project_into(b, ["s1"], cols)
    with pytest.raises(IndexOutOfBoundsException):
        enc.device_status()
    assert_columns_equal([fields[k]], [column_to_host(c) for c in cols], [ref[k]], n)
    enc.device_status()                                    # the error state is clear again


# 9. non-default stream -------------------------------------------------------------------------------
def test_non_default_stream(oracle, dev):
    fields = SCHEMAS["narrow"]
    n = 2000
    case = _cached(("narrow", n), lambda: _Case(oracle, dev, fields,
                                                gen_columns("narrow", fields, n, seed=3), n))
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    case.check([f.name for f in fields], stream=s)
    case.enc.device_status(s)
