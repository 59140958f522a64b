"""Row selection on the GPU (fury_row_take / fury_row_filter, RowEncoder.take / filter): the whole
output buffer, 4096 guard bytes on each side included, the whole out_offsets and, for filter,
out_count and out_indices equal an expectation computed in numpy from the source bytes alone: the
concatenation of rows[offs[i]:offs[i + 1]] in selection order.  Marked gpu."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from fury_amd import types as T  # noqa: E402
from fury_amd.workloads import SCHEMAS, Column, gen_columns  # noqa: E402
from tests.helpers import assert_columns_equal  # noqa: E402

GUARD = 4096
FILL = 0xAB
COUNTS = [1, 63, 64, 65, 257, 4097]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


class _Src:
    """A batch encoded once by this library, kept on the host and never modified.  `offs` is
    explicit for fixed-width schemas too (the expectation uses it; the calls pass NULL)."""

    def __init__(self, dev, enc, host, n):
        from fury_amd.encoder import column_to_device
        self.enc, self.host, self.n, self.dev = enc, host, n, dev
        b = enc.encode_batch([column_to_device(c, dev) for c in host], n)
        self.rows = b.rows.cpu().numpy().copy()
        self.fixed = b.row_offsets is None
        self.offs = (np.arange(n + 1, dtype=np.int64) * enc.schema().fixed_size if self.fixed
                     else b.row_offsets.cpu().numpy().copy())
        assert int(self.offs[n]) == len(self.rows)


_CACHE: dict = {}


def _pair_fields():
    return [T.field("a", T.INT64), T.field("b", T.INT32)]          # 8 + 2 * 8 = 24-byte rows


def source(dev, name, n) -> _Src:
    from fury_amd.encoder import Encoders
    key = (name, n)
    if key not in _CACHE:
        if name == "array":
            enc = Encoders.array_encoder(T.field("item", T.INT64), device=dev)
            host = gen_columns(None, [enc.field()], n, seed=5)
            host[0].validity = None
        elif name == "foo":                           # a map and a struct: gen_columns has no
            from fury_amd.beans import beans_to_columns   # generator for them, so from row values
            fields = SCHEMAS["foo"]
            enc = Encoders.bean(fields, device=dev)
            host = beans_to_columns(fields, [
                {"f1": i, "f2": None if i % 3 == 0 else f"s{i}" * (i % 5),
                 "f3": [f"x{j}" for j in range(i % 4)],
                 "f4": [(f"k{j}", j) for j in range(i % 3)] if i % 5 else None,
                 "f5": None if i % 7 == 0 else {"f1": i, "f2": "b" * (i % 11)}} for i in range(n)])
        else:
            fields = _pair_fields() if name == "pair" else SCHEMAS[name]
            enc = Encoders.bean(fields, device=dev)
            host = gen_columns(name if name != "pair" else None, fields, n, seed=3)
        _CACHE[key] = _Src(dev, enc, host, n)
    return _CACHE[key]


def expect(rows, offs, n, sel, fixed_size=None):
    """Bytes and offsets of the selected rows, from the source bytes alone.  An index outside
    [0, n), or a row whose extent leaves [0, offs[n]) or is not a non-negative multiple of 8, has
    size 0 (a fixed-width schema, where only the index can fail: fixed_size zero bytes)."""
    total = int(offs[n])
    parts, sizes, bad = [], [], []
    for j, i in enumerate(sel):
        i = int(i)
        ok = 0 <= i < n
        if ok:
            b, e = int(offs[i]), int(offs[i + 1])
            ok = 0 <= b <= e <= total and b % 8 == 0 and e % 8 == 0
        if ok:
            parts.append(rows[b:e])
        else:
            bad.append(j)
            parts.append(np.zeros(fixed_size or 0, np.uint8))
        sizes.append(len(parts[-1]))
    out_offs = np.zeros(len(sel) + 1, np.int64)
    np.cumsum(np.asarray(sizes, np.int64), out=out_offs[1:])
    data = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return data.astype(np.uint8), out_offs, bad


def _device_src(src, shift, offs=None):
    from fury_amd.encoder import RowBatch
    t = torch.empty(len(src.rows) + 16, dtype=torch.uint8, device=src.dev)
    assert t.data_ptr() % 16 == 0
    rows = t[shift:shift + len(src.rows)]
    rows.copy_(torch.from_numpy(src.rows))
    offs = src.offs if offs is None else offs
    toffs = None if src.fixed else torch.from_numpy(np.asarray(offs, np.int64)).to(src.dev)
    return RowBatch(rows, toffs, src.n, src.enc.schema_hash)


def _out_buffer(dev, cap, shift):
    t = torch.full((GUARD + 16 + cap + GUARD,), FILL, dtype=torch.uint8, device=dev)
    assert t.data_ptr() % 16 == 0
    at = GUARD + shift
    return t, t[at:at + cap], at


def _filled(size, at, data, cap):
    want = np.full(size, FILL, np.uint8)
    k = min(cap & ~7, len(data))                   # a capacity off a multiple of 8 is rounded down
    want[at:at + k] = data[:k]
    return want


def assert_same(got, want, what):
    if got.shape != want.shape or not np.array_equal(got, want):
        at = np.flatnonzero(got != want) if got.shape == want.shape else []
        raise AssertionError(f"{what}: shapes {got.shape} / {want.shape}, {len(at)} entries differ, "
                             f"first at {at[:8]} (got {got[at[:8]]}, want {want[at[:8]]})")


def run_take(src, sel, cap=None, src_shift=0, out_shift=0, measure=False, stream=None, bound=False,
             offs=None, with_offsets=True):
    """Runs the take into a guarded buffer; returns (whole buffer, out_offsets, expected bytes,
    expected offsets, where the output starts, its capacity, bad positions)."""
    dev, n = src.dev, src.n
    fs = src.enc.schema().fixed_size if src.fixed else None
    data, eoffs, bad = expect(src.rows, src.offs if offs is None else offs, n, sel, fs)
    cap = len(data) if cap is None else cap
    batch = _device_src(src, src_shift, offs)
    t, out, at = _out_buffer(dev, cap, out_shift)
    idx = torch.from_numpy(np.array(sel, dtype=np.int64)).to(dev)
    ooffs = torch.full((len(sel) + 1,), -7, dtype=torch.int64, device=dev) if with_offsets else None
    torch.cuda.synchronize()
    target = None if measure else out
    if bound:
        src.enc.bind_take(batch, idx, target, ooffs, stream=stream)()
    else:
        src.enc.take_into(batch, idx, target, ooffs, stream=stream)
    torch.cuda.synchronize()
    return (t.cpu().numpy(), None if ooffs is None else ooffs.cpu().numpy(), data, eoffs, at, cap,
            bad)


def check_take(src, sel, what, **kw):
    got, goffs, data, eoffs, at, cap, bad = run_take(src, sel, **kw)
    if goffs is not None:
        assert_same(goffs, eoffs, f"{what}: out_offsets")
    want = np.full(len(got), FILL, np.uint8) if kw.get("measure") else _filled(
        len(got), at, data, cap)
    assert_same(got, want, f"{what}: output buffer")
    return bad


def selections(n, seed):
    rng = np.random.default_rng(seed)
    return {"empty": np.zeros(0, np.int64), "identity": np.arange(n), "reversed": np.arange(n)[::-1],
            "random": rng.integers(0, n, 2 * n), "repeat": np.full(1000, int(rng.integers(0, n)))}


# 1. every schema shape x row count x selection x alignment -------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("name", ["struct100", "pair", "mixed", "narrow", "foo", "array"])
def test_take_selections(dev, name, n):
    src = source(dev, name, n)
    if name == "struct100":
        assert src.enc.schema().fixed_size == 816 and src.fixed
    if name == "pair":
        assert src.enc.schema().fixed_size == 24 and src.fixed
    for what, sel in selections(n, n).items():
        for src_shift, out_shift in ((0, 0), (8, 0), (0, 8), (8, 8)):
            bad = check_take(src, sel, f"{name} n={n} {what} shifts {src_shift}/{out_shift}",
                             src_shift=src_shift, out_shift=out_shift)
            assert not bad
    if src.fixed:                                   # out_offsets is optional for fixed-width schemas
        check_take(src, selections(n, n)["random"], f"{name} n={n} no out_offsets", with_offsets=False)
    src.enc.device_status()


# 2. a row larger than a workgroup's span among tiny rows ----------------------------------------------
def _string_source(dev):
    from fury_amd.encoder import Encoders
    if "long" not in _CACHE:
        lens = [0, 1, 7, 8, 9, 300, 8191, 3, 0, 200_000, 0, 5, 8, 1, 8191, 300, 9, 0]
        rng = np.random.default_rng(11)
        offs = np.zeros(len(lens) + 1, np.int32)
        np.cumsum(lens, out=offs[1:])
        col = Column(values=rng.integers(1, 256, int(offs[-1]), dtype=np.uint8), offsets=offs)
        enc = Encoders.bean([T.field("s", T.STRING)], device=dev)
        _CACHE["long"] = _Src(dev, enc, [col], len(lens))
    return _CACHE["long"]


def test_take_long_row(dev):
    src = _string_source(dev)
    sizes = np.diff(src.offs)
    assert sizes.max() >= 200_000 + 16 and sizes.min() == 16
    n = src.n
    rng = np.random.default_rng(2)
    sels = {"identity": np.arange(n), "reversed": np.arange(n)[::-1], "random": rng.integers(0, n, 2 * n),
            "long twice": np.array([0, 9, 1, 9, 2])}
    for what, sel in sels.items():
        for src_shift, out_shift in ((0, 0), (8, 0), (0, 8), (8, 8)):
            check_take(src, sel, f"long row, {what}, shifts {src_shift}/{out_shift}",
                       src_shift=src_shift, out_shift=out_shift)
    src.enc.device_status()


def test_copy_rounds_and_end_words(dev):
    """The index arithmetic of write_spans / store_split (take_dev.h) in copy_rows at its edges.  A row
    whose index is bad has no bytes: one 24-byte row, 2100 such rows, 1100 rows of 16 bytes, the
    200,016-byte row and three more short ones.  The first 16 KB span then touches more than 3,000 rows
    in four staging rounds, the second of which has no byte at all -- at 8 mod 16 in an aligned buffer,
    the round without a single aligned chunk -- the long row crosses a dozen spans whose first and last
    hold other rows too, and the total is 8 mod 16: into a buffer at 8 mod 16 the head and the tail word
    are single 8-byte stores.  Capacities inside a row, on and off a multiple of 8: bytes below cap & ~7
    are the full result's, the fill stays from there on, the offsets are complete."""
    from fury_amd.encoder import IndexOutOfBoundsException
    src = _string_source(dev)
    sel = np.array([3] + [-1] * 2100 + [0] * 1100 + [9, 0, 0, 0], np.int64)
    data, eoffs, bad = expect(src.rows, src.offs, src.n, sel)
    total = len(data)
    assert eoffs[1] == 24 and eoffs[2101] == 24 and total == 24 + 1103 * 16 + 200_016 and total % 16 == 8
    src.enc.device_status()
    for out_shift in (0, 8):
        for cap in (None, total - 24, total - 20, 16384 + 24):
            got = check_take(src, sel, f"zero-byte rows, shift {out_shift} capacity {cap}", cap=cap,
                             out_shift=out_shift)
            assert got == list(range(1, 2101))
            with pytest.raises(IndexOutOfBoundsException):
                src.enc.device_status()
    src.enc.device_status()


# 3. capacity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "foo"])
def test_take_capacity(dev, name):
    src = source(dev, name, 257)
    sel = selections(257, 9)["random"]
    data, eoffs, _ = expect(src.rows, src.offs, src.n, sel)
    total = len(data)
    assert total == int(eoffs[-1]) and total > 4096
    for cap in (total - 8, (total // 2) & ~7, 0):
        for out_shift in (0, 8):
            # bytes before the capacity are correct, bytes at or past it still hold the fill, the
            # offsets are complete: check_take compares the whole buffer and all offsets
            check_take(src, sel, f"{name} capacity {cap} of {total}", cap=cap, out_shift=out_shift)
    check_take(src, sel, f"{name} measure form", measure=True)      # only the offsets are written
    src.enc.device_status()


def test_fixed_schema_capacity_error(dev):
    from fury_amd.encoder import CapacityError
    src = source(dev, "struct100", 65)
    batch = _device_src(src, 0)
    out = torch.full((10 * 816 - 8,), FILL, dtype=torch.uint8, device=dev)
    with pytest.raises(CapacityError, match="fury_row_take"):
        src.enc.take_into(batch, torch.arange(10, device=dev), out)
    mask = torch.zeros(12, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    with pytest.raises(CapacityError, match="fury_row_filter"):
        src.enc.filter_into(batch, mask, out, None, cnt)
    torch.cuda.synchronize()
    assert bool((out == FILL).all())


# 4. bounds: argument checks the kernel answers by design ------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "struct100"])
def test_take_bad_indices(dev, name):
    from fury_amd.encoder import IndexOutOfBoundsException
    src = source(dev, name, 257)
    n = src.n
    sel = np.array([3, -1, 5, n, 2 ** 40, 0, 256, 7], np.int64)
    src.enc.device_status()
    bad = check_take(src, sel, f"{name}: indices outside the batch", out_shift=8)
    assert bad == [1, 3, 4]
    with pytest.raises(IndexOutOfBoundsException, match="row [134] "):
        src.enc.device_status()
    src.enc.device_status()                          # raised once, then clear
    check_take(src, np.array([3, 5, 0]), f"{name}: the next call is clean")
    src.enc.device_status()


def test_take_bad_source_offsets(dev):
    from fury_amd.encoder import IndexOutOfBoundsException
    src = source(dev, "mixed", 257)
    n = src.n
    total = int(src.offs[n])
    offs = src.offs.copy()
    offs[100] = total + 64                            # one entry past the total: rows 99 and 100 fail
    offs[201], offs[202] = offs[202], offs[201]       # a decreasing pair: row 201 has a negative size
    assert offs[202] < offs[201]
    sel = np.arange(n)
    data, eoffs, bad = expect(src.rows, offs, n, sel)
    assert bad == [99, 100, 201]                      # rows 200 / 202: other bytes, still in bounds
    src.enc.device_status()
    assert check_take(src, sel, "hand-made source offsets", offs=offs) == bad
    with pytest.raises(IndexOutOfBoundsException, match="row (99|100|201) "):
        src.enc.device_status()
    src.enc.device_status()
    check_take(src, sel, "the next call is clean")
    src.enc.device_status()


# 5. filter ----------------------------------------------------------------------------------------------
def _pack(m, garbage=False):
    n = len(m)
    w = np.zeros(((n + 31) // 32) * 32, bool)
    w[:n] = m
    if garbage:
        w[n:] = True                                  # bits at or past nrows in the last word
    return np.packbits(w, bitorder="little")


def check_filter(src, m, what, garbage=False, out_shift=0, cap=None, measure=False, indices=True,
                 offs=None):
    dev, n = src.dev, src.n
    fs = src.enc.schema().fixed_size if src.fixed else None
    sel = np.flatnonzero(m)
    data, eoffs, bad = expect(src.rows, src.offs if offs is None else offs, n, sel, fs)
    count = len(sel)
    want_offs = np.concatenate([eoffs, np.full(n - count, eoffs[-1], np.int64)])
    want_idx = np.concatenate([sel, np.full(n - count, -1, np.int64)])
    if cap is None:
        cap = n * fs if src.fixed else len(data)      # fixed: the host cannot know the count
    batch = _device_src(src, 0, offs)
    t, out, at = _out_buffer(dev, cap, out_shift)
    mask = torch.from_numpy(_pack(m, garbage)).to(dev)
    ooffs = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
    cnt = torch.full((1,), -7, dtype=torch.int64, device=dev)
    oidx = torch.full((n,), -7, dtype=torch.int64, device=dev) if indices else None
    torch.cuda.synchronize()
    src.enc.filter_into(batch, mask, None if measure else out, ooffs, cnt, oidx)
    torch.cuda.synchronize()
    assert int(cnt.item()) == count, what
    assert_same(ooffs.cpu().numpy(), want_offs, f"{what}: out_offsets")
    if indices:
        assert_same(oidx.cpu().numpy(), want_idx, f"{what}: out_indices")
    want = np.full(t.numel(), FILL, np.uint8) if measure else _filled(t.numel(), at, data, cap)
    assert_same(t.cpu().numpy(), want, f"{what}: output buffer")
    return [int(sel[j]) for j in bad]


def masks(n, seed):
    rng = np.random.default_rng(seed)
    return {"zeros": np.zeros(n, bool), "ones": np.ones(n, bool), "alternating": np.arange(n) % 2 == 1,
            "random": rng.random(n) < 0.5, "last": np.arange(n) == n - 1}


@pytest.mark.parametrize("name", ["struct100", "pair", "mixed", "foo"])
def test_filter_masks(dev, name):
    n = 4097
    src = source(dev, name, n)
    for what, m in masks(n, 4).items():
        check_filter(src, m, f"{name} mask {what}", out_shift=8 if what == "random" else 0)
    m = masks(n, 5)["random"]
    check_filter(src, m, f"{name} garbage bits past nrows", garbage=True)
    check_filter(src, m, f"{name} without out_indices", indices=False)
    check_filter(src, m, f"{name} measure form", measure=True)
    src.enc.device_status()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_filter_row_counts(dev, n):
    for name in ("narrow", "array", "struct100"):
        src = source(dev, name, n)
        for what, m in masks(n, n).items():
            check_filter(src, m, f"{name} n={n} mask {what}", garbage=True)
        src.enc.device_status()


def test_filter_capacity_and_bounds(dev):
    from fury_amd.encoder import IndexOutOfBoundsException
    src = source(dev, "mixed", 257)
    n = src.n
    m = masks(n, 6)["random"]
    m[[99, 100, 200, 201]] = True
    total = int(expect(src.rows, src.offs, n, np.flatnonzero(m))[1][-1])
    for cap in (total - 8, (total // 2) & ~7, 0):
        check_filter(src, m, f"filter capacity {cap} of {total}", cap=cap)
    src.enc.device_status()
    offs = src.offs.copy()
    offs[100] = int(offs[n]) + 64
    offs[201], offs[202] = offs[202], offs[201]
    bad = check_filter(src, m, "filter with hand-made source offsets", offs=offs)
    assert bad == [99, 100, 201]                      # the SOURCE rows that failed
    with pytest.raises(IndexOutOfBoundsException, match="row (99|100|201) "):
        src.enc.device_status()
    src.enc.device_status()
    check_filter(src, m, "the next call is clean")
    src.enc.device_status()


# 6. the Python surface ------------------------------------------------------------------------------------
def _index_columns(fields, cols, idx, n):
    """Host columns indexed by rows, through per-row values (independent of the codec)."""
    from fury_amd.beans import beans_to_columns, columns_to_beans
    beans = columns_to_beans(fields, cols, n)
    return beans_to_columns(fields, [beans[int(i)] for i in idx])


@pytest.mark.parametrize("name", ["mixed", "nested"])
def test_take_and_filter_decode_to_the_indexed_columns(dev, name):
    from fury_amd.encoder import column_to_host
    n = 257
    src = source(dev, name, n)
    fields = SCHEMAS[name]
    base = src.host                                  # the original host columns
    rng = np.random.default_rng(8)
    idx = rng.integers(0, n, 300)
    for given in (torch.from_numpy(idx).to(dev), torch.from_numpy(idx.astype(np.int32)).to(dev),
                  [int(i) for i in idx]):
        b = src.enc.take(_device_src(src, 0), given)
        assert b.nrows == len(idx) and b.schema_hash == src.enc.schema_hash
        got = [column_to_host(c) for c in src.enc.decode_batch(b)]
        assert_columns_equal(fields, got, _index_columns(fields, base, idx, n), len(idx))
    data, eoffs, _ = expect(src.rows, src.offs, n, idx)
    assert_same(b.rows.cpu().numpy(), data, "take: rows")
    assert_same(b.row_offsets.cpu().numpy(), eoffs, "take: offsets")
    m = rng.random(n) < 0.4
    kept = np.flatnonzero(m)
    for mask in (torch.from_numpy(_pack(m)).to(dev), torch.from_numpy(m).to(dev)):
        f, fi = src.enc.filter(_device_src(src, 0), mask, return_indices=True)
        assert f.nrows == int(m.sum()) and f.row_offsets.numel() == f.nrows + 1
        assert_same(fi.cpu().numpy(), kept, "filter: indices")
        got = [column_to_host(c) for c in src.enc.decode_batch(f)]
        assert_columns_equal(fields, got, _index_columns(fields, base, kept, n), f.nrows)
    data, eoffs, _ = expect(src.rows, src.offs, n, kept)
    assert_same(f.rows.cpu().numpy(), data, "filter: rows")
    assert_same(f.row_offsets.cpu().numpy(), eoffs, "filter: offsets")


def test_take_and_filter_of_a_fixed_schema(dev):
    n = 4097
    src = source(dev, "struct100", n)
    rng = np.random.default_rng(3)
    idx = rng.permutation(n)
    b = src.enc.take(_device_src(src, 0), torch.from_numpy(idx).to(dev))
    assert b.row_offsets is None and b.nrows == n
    assert_same(b.rows.cpu().numpy(), expect(src.rows, src.offs, n, idx)[0], "take: rows")
    m = rng.random(n) < 0.1
    f = src.enc.filter(_device_src(src, 0), torch.from_numpy(m).to(dev))
    assert f.nrows == int(m.sum()) and f.row_offsets is None
    assert_same(f.rows.cpu().numpy(), expect(src.rows, src.offs, n, np.flatnonzero(m))[0], "filter: rows")
    e = src.enc.filter(_device_src(src, 0), torch.zeros(n, dtype=torch.bool, device=dev))
    assert e.nrows == 0 and e.rows.numel() == 0
    e = src.enc.take(_device_src(src, 0), torch.zeros(0, dtype=torch.int64, device=dev))
    assert e.nrows == 0 and e.rows.numel() == 0


def test_bind_take_on_a_side_stream(dev):
    src = source(dev, "mixed", 4097)
    sel = selections(4097, 1)["random"]
    s = torch.cuda.Stream(device=dev)
    plain = run_take(src, sel, out_shift=8)
    side = run_take(src, sel, out_shift=8, stream=s, bound=True)
    src.enc.device_status(s)
    assert_same(side[0], plain[0], "bind_take on a side stream: output buffer")
    assert_same(side[1], plain[1], "bind_take on a side stream: out_offsets")
    assert_same(plain[0], _filled(len(plain[0]), plain[4], plain[2], plain[5]),
                "take_into: output buffer")


def test_foreign_schema_hash(dev):
    from fury_amd.encoder import ClassNotCompatibleException, RowBatch
    src = source(dev, "mixed", 65)
    b = _device_src(src, 0)
    foreign = RowBatch(b.rows, b.row_offsets, b.nrows, b.schema_hash + 1)
    idx = torch.arange(3, device=dev)
    with pytest.raises(ClassNotCompatibleException, match="Schema is not consistent"):
        src.enc.take(foreign, idx)
    with pytest.raises(ClassNotCompatibleException, match="Schema is not consistent"):
        src.enc.filter(foreign, torch.ones(65, dtype=torch.bool, device=dev))
    with pytest.raises(ClassNotCompatibleException, match="Schema is not consistent"):
        src.enc.bind_take(foreign, idx, None, torch.empty(4, dtype=torch.int64, device=dev))
