"""Nested values as batches on the GPU (fury_row_extract, RowEncoder.extract / extract_into /
bind_extract): the whole output buffer, 4096 guard bytes on each side included, the whole
out_offsets, out_count, out_indices and out_validity equal an expectation computed in numpy from the
source bytes alone -- the path walked per row by the rules of include/fury_row.h, the value slices
concatenated.  Marked gpu."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from fury_amd import types as T  # noqa: E402
from fury_amd.workloads import SCHEMAS  # noqa: E402
from tests.test_extract_abi import deep_fields  # noqa: E402

GUARD = 4096
FILL = 0xAB
COUNTS = [1, 63, 64, 65, 257, 4097]
FOO_PATHS = [("f3",), ("f4",), ("f5",)]
DEEP_PATHS = [("outer",), ("outer", "inner"), ("outer", "inner", "v"), ("outer", "fx"), ("outer", "m")]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


# -- sources: encoded once by the library, kept on the host, never modified ---------------------------
def _foo_beans(n, mode):
    """The value mix of test_take.py; mode "null" / "valid": every nested field null / present."""
    def f(i):
        f3 = [f"x{j}" for j in range(i % 4)]
        f4 = [(f"k{j}", j) for j in range(i % 3)] if i % 5 else None
        f5 = None if i % 7 == 0 else {"f1": i, "f2": "b" * (i % 11)}
        if mode == "null":
            f3 = f4 = f5 = None
        if mode == "valid":
            f4 = f4 if f4 is not None else []
            f5 = f5 if f5 is not None else {"f1": -i, "f2": None}
        return {"f1": i, "f2": None if i % 3 == 0 else f"s{i}" * (i % 5), "f3": f3, "f4": f4, "f5": f5}
    return [f(i) for i in range(n)]


def _deep_beans(n, mode):
    """outer / outer.inner / outer.fx / outer.m null in a different row pattern each: row 0 has none
    of them null, row 11 every one (11 = 1 mod 5 = 2 mod 3 = 3 mod 4 = 4 mod 7)."""
    def f(i):
        null = lambda k, m: mode == "null" or (mode == "mix" and i % m == k)   # noqa: E731
        inner = None if null(2, 3) else {"s": None if i % 6 == 1 else "t" * (i % 9),
                                         "v": None if null(3, 8) else [i * j for j in range(i % 5)]}
        fx = None if null(3, 4) else {"p": i * 1000003, "q": None if i % 2 else -i}
        m = None if null(4, 7) else [(f"k{j}", i + j) for j in range(i % 4)]
        outer = None if null(1, 5) else {"a": i, "inner": inner, "fx": fx, "m": m}
        return {"id": i, "outer": outer}
    return [f(i) for i in range(n)]


class _Src:
    def __init__(self, dev, fields, beans):
        from fury_amd.beans import beans_to_columns
        from fury_amd.encoder import Encoders, column_to_device
        self.dev, self.fields, self.beans, self.n = dev, fields, beans, len(beans)
        self.enc = Encoders.bean(fields, device=dev)
        host = beans_to_columns(fields, beans)
        b = self.enc.encode_batch([column_to_device(c, dev) for c in host], self.n)
        self.rows = b.rows.cpu().numpy().copy()
        self.offs = b.row_offsets.cpu().numpy().copy()
        assert int(self.offs[self.n]) == len(self.rows)
        self._want: dict = {}

    def want(self, path):
        """The expectation for the unmodified bytes, computed once per path."""
        if path not in self._want:
            self._want[path] = expect(self.rows, self.offs, self.n, levels_of(self.fields, path))
        return self._want[path]


_CACHE: dict = {}


def source(dev, name, n, mode="mix") -> _Src:
    key = (name, n, mode)
    if key not in _CACHE:
        if name == "foo":
            _CACHE[key] = _Src(dev, SCHEMAS["foo"], _foo_beans(n, mode))
        else:
            _CACHE[key] = _Src(dev, deep_fields(), _deep_beans(n, mode))
    return _CACHE[key]


# -- the expectation: the path walked in numpy ----------------------------------------------------------
def levels_of(fields, path):
    """[(fields of the struct, slot followed)] per level, and (least size, exact) of the value: from
    the Field tree alone."""
    out = []
    for name in path:
        k = [f.name for f in fields].index(name)
        out.append((len(fields), k))
        node, fields = fields[k], fields[k].children
    if node.type_id == T.STRUCT:
        last = (T.fixed_size(node.children), all(T.type_width(c.type_id) > 0 for c in node.children))
    else:
        last = (8, False)
    return out, last


def _header(nf):
    return ((nf + 63) // 64) * 8 + 8 * nf


def _i32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >> 31 else x


def walk(rows, offs, n, r, levels):
    """Row r: ("value", start, size) | ("null",) | ("fail",), and the base of every level reached."""
    lv, (least, exact) = levels
    total = int(offs[n])
    u64 = lambda p: int.from_bytes(rows[p:p + 8].tobytes(), "little")   # noqa: E731
    base, bases = int(offs[r]), []
    if base % 8:
        return ("fail",), bases
    for k, (nf, slot) in enumerate(lv):
        bm = ((nf + 63) // 64) * 8
        if not (0 <= base and base + _header(nf) <= total):
            return ("fail",), bases
        bases.append(base)
        if (u64(base + 8 * (slot >> 6)) >> (slot & 63)) & 1:
            return ("null",), bases
        s = u64(base + bm + 8 * slot)
        off, size = _i32(s >> 32), _i32(s)
        final = k + 1 == len(lv)
        need = least if final else _header(lv[k + 1][0])
        if (off < 0 or size < 0 or off % 8 or size % 8 or not (0 <= base + off and base + off + size <= total)
                or size < need or (final and exact and size != need)):
            return ("fail",), bases
        base += off
    return ("value", base, size), bases


class Want:
    pass


def expect(rows, offs, n, levels) -> Want:
    w = Want()
    parts, kept, w.bad = [], [], []
    for r in range(n):
        res, _ = walk(rows, offs, n, r, levels)
        if res[0] == "value":
            parts.append(rows[res[1]:res[1] + res[2]])
            kept.append(r)
        elif res[0] == "fail":
            w.bad.append(r)
    w.count = len(kept)
    w.kept = np.asarray(kept, np.int64)
    w.parts = parts
    w.data = np.concatenate(parts).astype(np.uint8) if parts else np.zeros(0, np.uint8)
    w.offs = np.zeros(n + 1, np.int64)
    np.cumsum([len(p) for p in parts], out=w.offs[1:w.count + 1])
    w.offs[w.count + 1:] = w.offs[w.count]
    w.idx = np.concatenate([w.kept, np.full(n - w.count, -1, np.int64)])
    bits = np.zeros(((n + 31) // 32) * 32, bool)
    bits[w.kept] = True
    w.valid = np.packbits(bits, bitorder="little")
    return w


# -- one call into guarded buffers, everything compared ---------------------------------------------------
def assert_same(got, want, what):
    if got.shape != want.shape or not np.array_equal(got, want):
        at = np.flatnonzero(got != want) if got.shape == want.shape else []
        raise AssertionError(f"{what}: shapes {got.shape} / {want.shape}, {len(at)} entries differ, "
                             f"first at {at[:8]} (got {got[at[:8]]}, want {want[at[:8]]})")


def _upload(src, shift=0, rows=None, offs=None):
    from fury_amd.encoder import RowBatch
    rows = src.rows if rows is None else rows
    t = torch.empty(len(rows) + 16, dtype=torch.uint8, device=src.dev)
    assert t.data_ptr() % 16 == 0
    d = t[shift:shift + len(rows)]
    d.copy_(torch.from_numpy(rows))
    o = torch.from_numpy(np.asarray(src.offs if offs is None else offs, np.int64)).to(src.dev)
    return RowBatch(d, o, src.n, src.enc.schema_hash)


def check_extract(src, path, what, cap=None, src_shift=0, out_shift=0, measure=False, stream=None,
                  bound=False, calls=1, rows=None, offs=None, indices=True, validity=True) -> Want:
    dev, n = src.dev, src.n
    if rows is None and offs is None:
        w = src.want(path)
    else:
        w = expect(src.rows if rows is None else rows, src.offs if offs is None else offs, n,
                   levels_of(src.fields, path))
    cap = len(w.data) if cap is None else cap
    batch = _upload(src, src_shift, rows, offs)
    t = torch.full((GUARD + 16 + cap + GUARD,), FILL, dtype=torch.uint8, device=dev)
    assert t.data_ptr() % 16 == 0
    at = GUARD + out_shift
    out = t[at:at + cap]
    ooffs = torch.full((n + 2,), -7, dtype=torch.int64, device=dev)
    cnt = torch.full((2,), -7, dtype=torch.int64, device=dev)
    oidx = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
    nvb = ((n + 31) // 32) * 4
    oval = torch.full((nvb + 8,), FILL, dtype=torch.uint8, device=dev)
    args = (batch, list(path), None if measure else out, ooffs[:n + 1], cnt[:1],
            oidx[:n] if indices else None, oval[:nvb] if validity else None)
    torch.cuda.synchronize()
    if bound:
        call = src.enc.bind_extract(*args, stream=stream)
        for _ in range(calls):
            call()
    else:
        for _ in range(calls):
            src.enc.extract_into(*args, stream=stream)
    torch.cuda.synchronize()
    assert_same(cnt.cpu().numpy(), np.array([w.count, -7], np.int64), f"{what}: out_count")
    assert_same(ooffs.cpu().numpy(), np.concatenate([w.offs, [-7]]), f"{what}: out_offsets")
    assert_same(oidx.cpu().numpy(), np.concatenate([w.idx, [-7]]) if indices
                else np.full(n + 1, -7, np.int64), f"{what}: out_indices")
    want_val = np.full(nvb + 8, FILL, np.uint8)
    if validity:
        want_val[:nvb] = w.valid
    assert_same(oval.cpu().numpy(), want_val, f"{what}: out_validity")
    want = np.full(t.numel(), FILL, np.uint8)
    if not measure:
        k = min(cap, len(w.data))
        want[at:at + k] = w.data[:k]
    assert_same(t.cpu().numpy(), want, f"{what}: output buffer")
    return w


# 1. every path x row count ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("path", FOO_PATHS, ids=".".join)
def test_extract_foo(dev, path, n):
    src = source(dev, "foo", n)
    w = check_extract(src, path, f"foo {path} n={n}")
    assert not w.bad
    if n >= 64:
        assert 0 < w.count and (path == ("f3",) or w.count < n)      # nulls and values are both there
    check_extract(src, path, f"foo {path} n={n} without indices / validity", indices=False,
                  validity=False, out_shift=8)
    src.enc.device_status()


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("path", DEEP_PATHS, ids=".".join)
def test_extract_deep(dev, path, n):
    src = source(dev, "deep", n)
    w = check_extract(src, path, f"deep {path} n={n}")
    assert not w.bad
    if n >= 64:
        assert 0 < w.count < n
    if path == ("outer", "fx"):                      # an is_fixed child: entry j at j * fixed_size
        assert src.enc.child_encoder(path).schema().is_fixed
        assert np.array_equal(w.offs[:w.count + 1], np.arange(w.count + 1) * 24)
    src.enc.device_status()


@pytest.mark.parametrize("n", [65, 257])
@pytest.mark.parametrize("mode", ["null", "valid"])
def test_extract_uniform_batches(dev, mode, n):
    for name, paths in (("foo", FOO_PATHS), ("deep", DEEP_PATHS)):
        src = source(dev, name, n, mode)
        for path in paths:
            w = check_extract(src, path, f"{name} {path} n={n} all {mode}")
            assert w.count == (0 if mode == "null" else n) and not w.bad
        src.enc.device_status()


# 2. composition with the other entry points, bit-exact -----------------------------------------------------
def _at(bean, path):
    for name in path:
        bean = None if bean is None else bean[name]
    return bean


@pytest.mark.parametrize("name,path", [("foo", ("f5",)), ("foo", ("f3",)), ("foo", ("f4",)),
                                       ("deep", ("outer", "inner")), ("deep", ("outer", "fx"))],
                         ids=lambda x: x if isinstance(x, str) else ".".join(x))
def test_extract_then_decode(dev, name, path):
    from fury_amd.beans import columns_to_beans, value_at
    from fury_amd.encoder import column_to_host
    n = 257
    src = source(dev, name, n)
    w = src.want(path)
    parent = src.enc.decode_batch(_upload(src))
    beans = columns_to_beans(src.fields, [column_to_host(c) for c in parent], n)
    values = [_at(b, path) for b in beans]
    assert [r for r, v in enumerate(values) if v is not None] == list(w.kept)
    child = src.enc.child_encoder(path)
    got, valid, idx = src.enc.extract(_upload(src), path, return_indices=True)
    assert got.nrows == w.count and got.schema_hash == child.schema_hash
    assert got.row_offsets.numel() == w.count + 1
    assert_same(got.rows.cpu().numpy(), w.data, "extract: rows")
    assert_same(got.row_offsets.cpu().numpy(), w.offs[:w.count + 1], "extract: offsets")
    assert_same(idx.cpu().numpy(), w.kept, "extract: indices")
    assert_same(valid.cpu().numpy(), w.valid[:(n + 7) // 8], "extract: validity")
    cols = [column_to_host(c) for c in child.decode_batch(got)]
    want = [values[r] for r in w.kept]
    if isinstance(want[0], dict):
        assert columns_to_beans(child.schema().fields, cols, w.count) == want
    else:
        assert [value_at(child.schema().fields[0], cols[0], j) for j in range(w.count)] == want


def test_extract_then_project_and_take(dev):
    from fury_amd.beans import value_at
    from fury_amd.encoder import column_to_host
    n = 257
    src = source(dev, "foo", n)
    for path in (("f5",), ("f3",)):
        w = src.want(path)
        child = src.enc.child_encoder(path[0])
        got, _ = src.enc.extract(_upload(src), path[0])
        if path == ("f5",):
            col = column_to_host(child.project_batch(got, ["f2"])[0])
            f2 = child.schema().fields[1]
            assert f2.name == "f2"
            assert [value_at(f2, col, j) for j in range(w.count)] == \
                [src.beans[r]["f5"]["f2"] for r in w.kept]
        back = child.take(got, torch.arange(w.count - 1, -1, -1, device=dev))
        assert_same(back.rows.cpu().numpy(), np.concatenate(w.parts[::-1]), f"{path}: reversed take")
        assert_same(np.diff(back.row_offsets.cpu().numpy()),
                    np.array([len(p) for p in w.parts[::-1]], np.int64), f"{path}: reversed sizes")


# 3. capacity, alignment, streams ----------------------------------------------------------------------------
@pytest.mark.parametrize("name,path", [("foo", ("f5",)), ("deep", ("outer", "inner", "v"))],
                         ids=lambda x: x if isinstance(x, str) else ".".join(x))
def test_extract_capacity(dev, name, path):
    src = source(dev, name, 257)
    total = len(src.want(path).data)
    assert total > 2048
    for cap in (0, 8, total - 8, total):
        for out_shift in (0, 8):
            check_extract(src, path, f"{name} {path} capacity {cap} of {total}", cap=cap,
                          out_shift=out_shift)
    check_extract(src, path, f"{name} {path} measure form", measure=True)
    src.enc.device_status()


@pytest.mark.parametrize("n", [65, 4097])
def test_extract_alignment(dev, n):
    for name, path in (("foo", ("f5",)), ("foo", ("f4",)), ("deep", ("outer",))):
        src = source(dev, name, n)
        for src_shift, out_shift in ((0, 0), (8, 0), (0, 8), (8, 8)):
            check_extract(src, path, f"{name} {path} n={n} shifts {src_shift}/{out_shift}",
                          src_shift=src_shift, out_shift=out_shift)
        src.enc.device_status()


def test_extract_on_a_side_stream_and_bound_twice(dev):
    src = source(dev, "deep", 4097)
    s = torch.cuda.Stream(device=dev)
    path = ("outer", "inner")
    check_extract(src, path, "extract_into on a side stream", stream=s, out_shift=8)
    check_extract(src, path, "bind_extract called twice", bound=True, calls=2)
    check_extract(src, path, "bind_extract twice on a side stream", bound=True, calls=2, stream=s)
    src.enc.device_status(s)
    src.enc.device_status()


# 4. malformed slots: the bounds rule ------------------------------------------------------------------------
def _slot_at(src, r, levels, level):
    """Byte position of the slot row r follows at `level`."""
    _, bases = walk(src.rows, src.offs, src.n, r, levels)
    nf, slot = levels[0][level]
    return bases[level] + ((nf + 63) // 64) * 8 + 8 * slot


def _put(rows, pos, off, size):
    rows[pos:pos + 8] = np.frombuffer(
        (((off & 0xFFFFFFFF) << 32) | (size & 0xFFFFFFFF)).to_bytes(8, "little"), np.uint8)


def _get(rows, pos):
    s = int.from_bytes(rows[pos:pos + 8].tobytes(), "little")
    return _i32(s >> 32), _i32(s)


def _victims(src, path):
    """About one row in 16, among the rows that have a value."""
    kept = [int(r) for r in src.want(path).kept if r % 16 == 5]
    assert len(kept) >= 4
    return kept


def _check_malformed(src, path, what, victims, rows=None, offs=None):
    from fury_amd.encoder import IndexOutOfBoundsException
    src.enc.device_status()
    w = check_extract(src, path, what, rows=rows, offs=offs, out_shift=8)
    assert w.bad == victims, what                         # those rows are null, every other row exact
    assert list(w.kept) == [int(r) for r in src.want(path).kept if r not in victims]
    with pytest.raises(IndexOutOfBoundsException, match=f"row ({'|'.join(map(str, victims))}) "):
        src.enc.device_status()
    src.enc.device_status()                               # raised once, then clear
    check_extract(src, path, f"{what}: the next call is clean")
    src.enc.device_status()


FINAL_EDITS = {
    "off past the batch": lambda off, size, total: (total + 64, size),
    "off + size past the batch": lambda off, size, total: (off, total),
    "negative off": lambda off, size, total: (-8, size),
    "off not a multiple of 8": lambda off, size, total: (off + 4, size),
    "size not a multiple of 8": lambda off, size, total: (off, size + 4),
    "size below the child header": lambda off, size, total: (off, 16),
}


@pytest.mark.parametrize("edit", list(FINAL_EDITS))
def test_malformed_final_slot(dev, edit):
    src = source(dev, "deep", 257)
    path = ("outer", "inner")                             # inner: 2 fields, header 24 bytes
    levels = levels_of(src.fields, path)
    victims = _victims(src, path)
    rows = src.rows.copy()
    total = len(rows)
    for r in victims:
        pos = _slot_at(src, r, levels, 1)
        _put(rows, pos, *FINAL_EDITS[edit](*_get(rows, pos), total))
    _check_malformed(src, path, edit, victims, rows=rows)


def test_malformed_intermediate_slot(dev):
    src = source(dev, "deep", 257)
    path = ("outer", "inner", "v")
    levels = levels_of(src.fields, path)
    victims = _victims(src, path)
    total = len(src.rows)
    edits = [lambda off, size: (total + 64, size), lambda off, size: (off, total),
             lambda off, size: (-8, size), lambda off, size: (off + 4, size),
             lambda off, size: (off, 16)]                 # headers: outer 40 bytes, inner 24
    for level in (0, 1):
        rows = src.rows.copy()
        for j, r in enumerate(victims):
            pos = _slot_at(src, r, levels, level)
            _put(rows, pos, *edits[j % len(edits)](*_get(rows, pos)))
        _check_malformed(src, path, f"a bad slot at level {level}", victims, rows=rows)


def test_malformed_row_offset(dev):
    src = source(dev, "deep", 257)
    path = ("outer", "inner", "v")
    victims = _victims(src, path)
    total = len(src.rows)
    offs = src.offs.copy()
    for j, r in enumerate(victims):                       # the row header is 8 + 2 * 8 = 24 bytes
        offs[r] = (total - 16, total + 64, -8, total)[j % 4]
    _check_malformed(src, path, "row offsets whose header leaves the batch", victims, offs=offs)


def test_fixed_child_of_another_size(dev):
    src = source(dev, "deep", 257)
    path = ("outer", "fx")                                # fx: is_fixed, 24 bytes
    levels = levels_of(src.fields, path)
    victims = _victims(src, path)
    rows = src.rows.copy()
    for r in victims:
        pos = _slot_at(src, r, levels, 1)
        off, size = _get(rows, pos)
        assert size == 24
        _put(rows, pos, off, 32)
    _check_malformed(src, path, "outer.fx with size != fixed_size", victims, rows=rows)


def test_a_corrupt_slot_off_the_path_is_no_error(dev):
    src = source(dev, "deep", 257)
    path = ("outer", "inner")
    levels = levels_of(src.fields, ("outer", "m"))
    rows = src.rows.copy()
    for r in _victims(src, ("outer", "m")):
        _put(rows, _slot_at(src, r, levels, 1), len(rows) + 64, -8)
    _put(rows, int(src.offs[21]) + 8, -8, 4)              # and row 21's id, a scalar slot
    src.enc.device_status()
    w = check_extract(src, path, "corrupt outer.m / id slots", rows=rows)
    assert not w.bad and np.array_equal(w.kept, src.want(path).kept)
    src.enc.device_status()


# 5. the empty batch, and a foreign batch ------------------------------------------------------------------------
def test_extract_of_no_rows(dev):
    from fury_amd.encoder import Encoders, RowBatch
    enc = Encoders.bean(SCHEMAS["foo"], device=dev)
    empty = RowBatch(torch.zeros(16, dtype=torch.uint8, device=dev)[:0],
                     torch.zeros(1, dtype=torch.int64, device=dev), 0, enc.schema_hash)
    ooffs = torch.full((2,), -7, dtype=torch.int64, device=dev)
    cnt = torch.full((2,), -7, dtype=torch.int64, device=dev)
    out = torch.full((64,), FILL, dtype=torch.uint8, device=dev)
    enc.extract_into(empty, "f5", out, ooffs[:1], cnt[:1])
    torch.cuda.synchronize()
    assert ooffs.tolist() == [0, -7] and cnt.tolist() == [0, -7] and bool((out == FILL).all())
    got, valid = enc.extract(empty, "f5")
    assert got.nrows == 0 and got.rows.numel() == 0 and valid.numel() == 0
    assert got.row_offsets.tolist() == [0] and got.schema_hash == enc.child_encoder("f5").schema_hash
    enc.device_status()


def test_foreign_schema_hash(dev):
    from fury_amd.encoder import ClassNotCompatibleException, RowBatch
    src = source(dev, "foo", 65)
    b = _upload(src)
    foreign = RowBatch(b.rows, b.row_offsets, b.nrows, b.schema_hash + 1)
    with pytest.raises(ClassNotCompatibleException, match="Schema is not consistent"):
        src.enc.extract(foreign, "f5")
