"""In-place update on the GPU (fury_row_update / RowEncoder.update_fields): the whole rows buffer,
guard bytes included, equals (a) a numpy restatement of the setters' semantics and / or (b) the
oracle's encode of the original columns with the selected ones replaced.  Marked gpu."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from fury_amd import types as T  # noqa: E402
from fury_amd.workloads import SCHEMAS, Column, gen_column, gen_columns  # noqa: E402
from tests.helpers import as_u8, assert_columns_equal, bits  # noqa: E402

GUARD = 4096
FILL = 0xAB


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _width(f):
    return 1 if f.type_id == T.BOOL else T.type_width(f.type_id)


def _words(a, n):
    """A bitmap of n bits padded to whole 32-bit words (the kernels read bitmaps as words)."""
    out = np.zeros(((n + 31) // 32) * 4, np.uint8)
    out[:(n + 7) // 8] = as_u8(a)[:(n + 7) // 8]
    return out


def new_columns(fields, idx, n, nulls, seed=77):
    """Fresh input columns for the selected fields; `nulls`: a validity bitmap with 30 % nulls,
    the values under a null left as they are (non-zero: the update must not write them)."""
    rng = np.random.default_rng(seed + n)
    out = []
    for k in idx:
        f = fields[k]
        c = gen_column(T.field(f.name, f.type_id), seed, k, 0, n, null_pct=0)
        vals = _words(c.values, n) if f.type_id == T.BOOL else c.values
        val = _words(np.packbits(rng.random(n) >= 0.3, bitorder="little"), n) if nulls else None
        out.append(Column(values=vals, validity=val))
    return out


def model_update(rows, offs, n, fields, idx, cols, mask=None):
    """The semantics of fury_row_update restated: setX = clear the null bit + write the value's own
    w bytes, setNullAt = set the bit + zero the slot; masked-out rows and rows that fail the write
    bounds are left alone; nothing else changes."""
    out = rows.copy()
    bmb = ((len(fields) + 63) // 64) * 8
    fixed = bmb + 8 * len(fields)
    base = np.arange(n, dtype=np.int64) * fixed if offs is None else np.asarray(offs[:n], np.int64)
    total = n * fixed if offs is None else int(offs[n])
    ok = (base >= 0) & (base + fixed <= total)
    if offs is not None:
        ok &= (np.asarray(offs[1:n + 1], np.int64) - base) >= fixed
    if mask is not None:
        ok &= bits(mask, n)
    for k, c in zip(idx, cols):
        w = _width(fields[k])
        valid = np.ones(n, bool) if c.validity is None else bits(c.validity, n)
        if fields[k].type_id == T.BOOL:
            vb = bits(c.values, n).astype(np.uint8).reshape(n, 1)
        else:
            vb = as_u8(c.values)[:n * w].reshape(n, w)
        bit = np.uint8(1 << (k & 7))
        setv, setn = ok & valid, ok & ~valid
        out[base[setv] + (k >> 3)] &= np.uint8(~bit & 0xFF)
        out[base[setn] + (k >> 3)] |= bit
        slot = base + bmb + 8 * k
        out[slot[setv][:, None] + np.arange(w)] = vb[setv]
        out[slot[setn][:, None] + np.arange(8)] = 0
    return out, ok


def oracle_update(oracle, fields, host, n, idx, cols):
    """Expectation (b): encode of the original columns with the selected ones replaced."""
    repl = list(host)
    for k, c in zip(idx, cols):
        repl[k] = c
    rows, offs = oracle.encode(fields, repl, n)
    return np.asarray(rows, np.uint8)


class _Batch:
    """Rows encoded once by this library, kept on the host and never modified."""

    def __init__(self, dev, fields, host, n):
        from fury_amd.encoder import Encoders, column_to_device
        self.fields, self.host, self.n, self.dev = list(fields), host, n, dev
        self.enc = Encoders.bean(self.fields, device=dev)
        b = self.enc.encode_batch([column_to_device(c, dev) for c in host], n)
        self.rows = b.rows.cpu().numpy()
        self.offs = None if b.row_offsets is None else b.row_offsets.cpu().numpy()


def run_update(enc, dev, rows, offs, n, select, cols, mask=None, stream=None, bound=False):
    """Runs the update on a copy of `rows` followed by guard bytes; returns the whole buffer."""
    from fury_amd.encoder import RowBatch, column_to_device
    buf = np.full(len(rows) + GUARD, FILL, np.uint8)
    buf[:len(rows)] = rows
    t = torch.from_numpy(buf).to(dev)
    toffs = None if offs is None else torch.from_numpy(np.asarray(offs, np.int64)).to(dev)
    batch = RowBatch(t[:len(rows)], toffs, n, enc.schema_hash)
    dcols = [column_to_device(c, dev) for c in cols]
    dmask = None if mask is None else torch.from_numpy(mask).to(dev)
    torch.cuda.synchronize()
    if bound:
        enc.bind_update(batch, select, dcols, row_mask=dmask, stream=stream)()
    else:
        enc.update_fields(batch, select, dcols, row_mask=dmask, stream=stream)
    torch.cuda.synchronize()
    return t.cpu().numpy()


def with_guard(rows):
    return np.concatenate([rows, np.full(GUARD, FILL, np.uint8)])


def assert_same(got, want, what):
    if not np.array_equal(got, want):
        at = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {len(at)} bytes differ, first at {at[:8]} "
                             f"(got {got[at[:8]]}, want {want[at[:8]]})")


_CACHE: dict = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# 1. Struct-100 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4097])
def test_struct100_selections(oracle, dev, n):
    fields = SCHEMAS["struct100"]
    b = _cached(("struct100", n), lambda: _Batch(dev, fields, gen_columns("struct100", fields, n, seed=3), n))
    assert b.offs is None
    explicit = np.arange(n + 1, dtype=np.int64) * b.enc.schema().fixed_size
    sels = ([0], [99], [0, 99], [7, 8, 9], [99, 0, 50], ["f99", "f00", "f50"], list(range(0, 100, 2)))
    for sel in sels:
        idx = b.enc._select(sel)
        for nulls in (False, True):
            cols = new_columns(fields, idx, n, nulls)
            want = with_guard(oracle_update(oracle, fields, b.host, n, idx, cols))
            for offs in (None, explicit):
                got = run_update(b.enc, dev, b.rows, offs, n, sel, cols)
                assert_same(got, want, f"{sel} nulls={nulls} offsets={'explicit' if offs is not None else 'NULL'}")
    b.enc.device_status()


# 2. bitmap-word and piece boundaries ---------------------------------------------------------------
def _fields130():
    kinds = [T.BOOL, T.INT8, T.INT16, T.INT32, T.INT64, T.FLOAT32, T.FLOAT64, T.DATE32, T.TIMESTAMP]
    return [T.field(f"c{k:03d}", kinds[k % len(kinds)]) for k in range(130)]


def _batch130(dev, n):
    fields = _fields130()
    return _cached(("f130", n), lambda: _Batch(dev, fields, gen_columns(None, fields, n, null_pct=30), n))


@pytest.mark.parametrize("nulls", [True, False])
def test_bitmap_word_and_piece_boundaries(oracle, dev, nulls):
    n = 257
    b = _batch130(dev, n)
    fields = b.fields
    bools = [k for k, f in enumerate(fields) if f.type_id == T.BOOL]
    word0 = [5, 0, 63, 17, 33, 62, 1, 40]          # eight fields in bitmap word 0: the LDS merge hazard
    for sel in ([63, 64], [127, 128, 129], [0, 129], bools, word0):
        cols = new_columns(fields, sel, n, nulls)
        model, ok = model_update(b.rows, None, n, fields, sel, cols)
        want = oracle_update(oracle, fields, b.host, n, sel, cols)
        assert ok.all()
        assert_same(model, want, f"{sel}: the model against the oracle")
        got = run_update(b.enc, dev, b.rows, None, n, sel, cols)
        assert_same(got, with_guard(want), f"{sel} nulls={nulls}")
    b.enc.device_status()


# 3. upper bytes of narrow slots are preserved --------------------------------------------------------
def test_upper_bytes_preserved(dev):
    fields = SCHEMAS["narrow"]
    n = 257
    b = _cached(("narrow", n), lambda: _Batch(dev, fields, gen_columns("narrow", fields, n, seed=3), n))
    sel = ["a_bool", "b_byte", "c_short", "d_int", "e_float"]
    idx = b.enc._select(sel)
    bmb = b.enc.schema().bitmap_bytes
    rows = b.rows.copy()
    rng = np.random.default_rng(5)
    for k in idx:                                   # non-zero garbage in bytes [w, 8) of every slot
        w = _width(fields[k])
        at = (b.offs[:n] + bmb + 8 * k)[:, None] + np.arange(w, 8)
        rows[at] = rng.integers(1, 256, at.shape, dtype=np.uint8)
    cols = new_columns(fields, idx, n, True)
    want, ok = model_update(rows, b.offs, n, fields, idx, cols)
    assert ok.all()
    got = run_update(b.enc, dev, rows, b.offs, n, sel, cols)
    assert_same(got, with_guard(want), "narrow slots with garbage upper bytes")
    for k, c in zip(idx, cols):                     # and said directly
        w = _width(fields[k])
        valid = bits(c.validity, n)
        slots = got[(b.offs[:n] + bmb + 8 * k)[:, None] + np.arange(8)]
        old = rows[(b.offs[:n] + bmb + 8 * k)[:, None] + np.arange(8)]
        assert np.array_equal(slots[valid][:, w:], old[valid][:, w:]) and (old[valid][:, w:] != 0).all()
        assert (slots[~valid] == 0).all() and (~valid).any() and valid.any()
    b.enc.device_status()


# 4. variable-length and nested schemas ---------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 129, 2000])
@pytest.mark.parametrize("name,sel", [("mixed", ["a", "b", "c"]), ("nested", ["score", "id"])])
def test_variable_length_schemas(oracle, dev, name, sel, n):
    from fury_amd.encoder import RowBatch, column_to_host
    fields = SCHEMAS[name]
    b = _cached((name, n), lambda: _Batch(dev, fields, gen_columns(name, fields, n, seed=3), n))
    idx = b.enc._select(sel)
    cols = new_columns(fields, idx, n, True)
    want = oracle_update(oracle, fields, b.host, n, idx, cols)
    assert len(want) == len(b.rows)                 # fixed-width values: the row sizes do not change
    got = run_update(b.enc, dev, b.rows, b.offs, n, sel, cols)
    assert_same(got, with_guard(want), f"{name} {sel}")
    # the read-side mirror returns what was written
    batch = RowBatch(torch.from_numpy(got[:len(want)].copy()).to(dev),
                     torch.from_numpy(b.offs).to(dev), n, b.enc.schema_hash)
    back = [column_to_host(c) for c in b.enc.project_batch(batch, sel)]
    ref = oracle.decode(fields, want, b.offs, n)
    assert_columns_equal([fields[k] for k in idx], back, [ref[k] for k in idx], n)
    for c, g in zip(cols, back):
        valid = bits(c.validity, n)
        assert np.array_equal(bits(g.validity, n), valid)
        w = len(as_u8(c.values)) // n
        assert np.array_equal(as_u8(g.values)[:n * w].reshape(n, w)[valid],
                              as_u8(c.values).reshape(n, w)[valid])


# 5. row mask -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 257])
def test_row_mask(dev, n):
    b = _batch130(dev, n)
    fields = b.fields
    sel = [0, 3, 64, 129, 4]
    cols = new_columns(fields, sel, n, True)
    masks = {"zeros": np.zeros(n, bool), "ones": np.ones(n, bool), "alternating": np.arange(n) % 2 == 1,
             "single": np.arange(n) == 37, "last": np.arange(n) == n - 1}
    for what, m in masks.items():
        mask = _words(np.packbits(m, bitorder="little"), n)
        want, ok = model_update(b.rows, None, n, fields, sel, cols, mask)
        assert np.array_equal(ok, m)
        got = run_update(b.enc, dev, b.rows, None, n, sel, cols, mask=mask)
        assert_same(got, with_guard(want), f"mask {what}")
        if what == "zeros":
            assert_same(got, with_guard(b.rows), "mask zeros: the buffer is unchanged")
    b.enc.device_status()


# 6. bounds -------------------------------------------------------------------------------------------
def test_rows_outside_the_batch_are_not_written(dev):
    from fury_amd.encoder import Encoders, IndexOutOfBoundsException
    fields = SCHEMAS["mixed"]
    enc = Encoders.bean(fields, device=dev)
    fixed = enc.schema().fixed_size                  # 56
    n = 300                                          # two tiles
    sizes = np.full(n, 64, np.int64)
    sizes[5] = fixed - 8                             # row 5 is shorter than its header
    offs = np.zeros(n + 1, np.int64)
    np.cumsum(sizes, out=offs[1:])
    offs[0] = -64                                    # row 0 starts before the batch
    rows = np.zeros(int(offs[n]), np.uint8)
    sel = ["c", "a"]
    idx = enc._select(sel)
    cols = new_columns(fields, idx, n, True)
    want, ok = model_update(rows, offs, n, fields, idx, cols)
    assert list(np.flatnonzero(~ok)) == [0, 5]
    enc.device_status()
    got = run_update(enc, dev, rows, offs, n, sel, cols)
    assert_same(got, with_guard(want), "hand-made offsets")
    for r in (0, 5):
        lo = max(int(offs[r]), 0)
        assert (got[lo:int(offs[r + 1])] == 0).all()
    assert (got[len(rows):] == FILL).all()
    with pytest.raises(IndexOutOfBoundsException, match="row [05] "):
        enc.device_status()
    enc.device_status()                              # raised once, then clear


# 7. bound call on a side stream ------------------------------------------------------------------------
def test_bind_update_on_a_side_stream(dev):
    fields = SCHEMAS["struct100"]
    n = 257
    b = _cached(("struct100", n), lambda: _Batch(dev, fields, gen_columns("struct100", fields, n, seed=3), n))
    sel = ["f07", 8, 9, 64]
    cols = new_columns(fields, b.enc._select(sel), n, True)
    mask = _words(np.packbits(np.arange(n) % 3 != 0, bitorder="little"), n)
    plain = run_update(b.enc, dev, b.rows, None, n, sel, cols, mask=mask)
    s = torch.cuda.Stream(device=dev)
    side = run_update(b.enc, dev, b.rows, None, n, sel, cols, mask=mask, stream=s, bound=True)
    b.enc.device_status(s)
    assert_same(side, plain, "bind_update on a side stream")
    assert not np.array_equal(plain, with_guard(b.rows))
