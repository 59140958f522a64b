"""List and map elements as batches on the GPU (fury_row_explode, RowEncoder.explode / explode_into /
bind_explode and the collection encoders' forms): the whole of every output -- out_list_offsets,
out_entry_validity, out_count, out_offsets, out_parents, out_ordinals, out_validity and the output
buffer with 4096 guard bytes on each side -- equals an expectation computed in numpy from the source
bytes alone, by the rules of include/fury_row.h.  Marked gpu."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from fury_amd import types as T  # noqa: E402
from tests.test_explode_abi import explode_fields  # noqa: E402
from tests.test_extract import FILL, GUARD, _i32, assert_same, levels_of, walk  # noqa: E402

COUNTS = [1, 63, 64, 65, 257, 4097]
LENGTHS = [0, 1, 2, 3, 63, 64, 65, 129]
# small lengths are drawn more often, so that 4097 rows stay a matter of seconds
WEIGHTS = [0.25, 0.2, 0.15, 0.15, 0.07, 0.07, 0.06, 0.05]
SEED = 20261019
# (field, side): everything of explode_fields() that can be exploded (m's keys are INT32)
TARGETS = [("items", "elements"), ("m", "values"), ("ll", "elements"), ("fx", "elements")]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def nested_fields():
    return [T.field("id", T.INT64), T.struct_field("outer", explode_fields())]


# -- sources: encoded once by the library, kept on the host, never modified ---------------------------
def _element(name, i, j):
    if name == "items":
        return {"a": (i * 131 + j) % 100003 - 50000, "s": None if j % 5 == 0 else "s" * (j % 7)}
    if name == "m":
        return {"x": i * 1000003 + j, "y": None if j % 4 == 1 else "y" * (j % 9)}
    if name == "ll":
        return [i + j + k if k != 1 else None for k in range(j % 4)]
    return {"p": i * 7919 - j, "q": None if j % 2 else j - i}


def _list(name, i, k):
    """k elements of field `name` of row i; nulls at ordinals 0, 63, 64 and the last one in two rows
    of three (every third row has no null element)."""
    nulls = {0: (0, 63, 64, k - 1), 1: (k - 1,), 2: ()}[i % 3]
    vals = [None if j in nulls else _element(name, i, j) for j in range(k)]
    return [(j - 7, v) for j, v in enumerate(vals)] if name == "m" else vals


def _lengths(n, seed=SEED):
    """Per row and field: a pseudo-random pick of LENGTHS."""
    rng = np.random.default_rng(seed)
    return rng.choice(LENGTHS, size=(n, 4), p=WEIGHTS)


def flat_beans(n, lengths=None, mode="mix"):
    """Null fields in a different row pattern per field (mode "valid": none)."""
    lengths = _lengths(n) if lengths is None else lengths
    beans = []
    for i in range(n):
        b = {"id": i}
        for f, (name, mod) in enumerate((("items", 11), ("m", 7), ("ll", 5), ("fx", 13))):
            null = mode == "mix" and i % mod == 3
            b[name] = None if null else _list(name, i, int(lengths[i][f]))
        beans.append(b)
    return beans


def nested_beans(n):
    return [{"id": i, "outer": None if i % 9 == 4 else dict(b, a=i)}
            for i, b in enumerate(flat_beans(n, _lengths(n, SEED + 1)))]


def _global_offsets(beans, name):
    return np.concatenate([[0], np.cumsum([len(b[name] or ()) for b in beans])])


def test_the_seed_gives_lists_that_end_and_start_on_a_tile_edge():
    """The locate pass's cases "owner changes exactly at a tile edge" and "tile starts at a row's
    first element": a non-empty list ends, and another starts, on a multiple of 64 in global
    element index, inside the batch."""
    ends = starts = 0
    for n in (257, 4097):
        beans = flat_beans(n)
        for name, _ in TARGETS:
            lo = _global_offsets(beans, name)
            size = np.diff(lo)
            ends += int(np.sum((size > 0) & (lo[1:] % 64 == 0) & (lo[1:] < lo[-1])))
            starts += int(np.sum((size > 0) & (lo[:-1] % 64 == 0) & (lo[:-1] > 0)))
    assert ends >= 1 and starts >= 1, (ends, starts)


class _Src:
    """A batch on the host and the encoder that explodes it.  path None: a collection batch."""

    def __init__(self, dev, enc, rows, offs, n, fields=None, beans=None):
        self.dev, self.enc, self.n, self.fields, self.beans = dev, enc, n, fields, beans
        self.rows, self.offs = rows, offs
        assert int(self.offs[n]) == len(self.rows)
        self._want: dict = {}

    @classmethod
    def of_beans(cls, dev, fields, beans):
        from fury_amd.beans import beans_to_columns
        from fury_amd.encoder import Encoders, column_to_device
        enc = Encoders.bean(fields, device=dev)
        host = beans_to_columns(fields, beans)
        b = enc.encode_batch([column_to_device(c, dev) for c in host], len(beans))
        return cls(dev, enc, b.rows.cpu().numpy().copy(), b.row_offsets.cpu().numpy().copy(),
                   len(beans), fields, beans)

    def spec(self, path, side):
        """(levels of the walk or None, is_map, side, least element size, exact): from the Field
        tree alone."""
        if path is None:
            node, levels = self.enc._field, None
        else:
            levels, fields = levels_of(self.fields, path), self.fields
            for name in path:
                node = fields[[f.name for f in fields].index(name)]
                fields = node.children
        s = 1 if side == "values" else 0
        e = node.children[s]
        if e.type_id == T.STRUCT:
            least = (T.fixed_size(e.children), all(T.type_width(c.type_id) > 0 for c in e.children))
        else:
            least = (8, False)
        return levels, node.type_id == T.MAP, s, least[0], least[1]

    def want(self, path, side):
        key = (path, side)
        if key not in self._want:
            self._want[key] = expect(self.rows, self.offs, self.n, self.spec(path, side))
        return self._want[key]


_CACHE: dict = {}


def source(dev, name, n) -> _Src:
    key = (name, n)
    if key not in _CACHE:
        if name == "flat":
            _CACHE[key] = _Src.of_beans(dev, explode_fields(), flat_beans(n))
        elif name == "valid":
            _CACHE[key] = _Src.of_beans(dev, explode_fields(), flat_beans(n, mode="valid"))
        elif name == "nested":
            _CACHE[key] = _Src.of_beans(dev, nested_fields(), nested_beans(n))
        elif name == "long":            # one row of 4097 elements among empty and null rows
            lengths = np.zeros((n, 4), np.int64)
            lengths[21] = 4097                                 # no field of row 21 is null
            _CACHE[key] = _Src.of_beans(dev, explode_fields(), flat_beans(n, lengths))
        else:                           # "huge": a single row with 70,000 elements
            assert n == 1
            fields = [f for f in explode_fields() if f.name in ("id", "items")]
            _CACHE[key] = _Src.of_beans(dev, fields, [{"id": 0, "items": _list("items", 1, 70000)}])
    return _CACHE[key]


# -- the expectation --------------------------------------------------------------------------------------
class Want:
    def valid_positions(self):
        return np.flatnonzero(np.unpackbits(self.valid, bitorder="little"))


def locate_row(rows, offs, n, r, spec):
    """Row r: ("array", A, count) | ("null",) | ("fail",), and the value's start V (or None)."""
    levels, is_map, side, _, _ = spec
    total = int(offs[n])
    i64 = lambda p: int.from_bytes(rows[p:p + 8].tobytes(), "little")   # noqa: E731
    if levels is None:
        V, size = int(offs[r]), int(offs[r + 1]) - int(offs[r])
        if V % 8 or size % 8 or size < 8 or V < 0 or V + size > total:
            return ("fail",), None
    else:
        res, _ = walk(rows, offs, n, r, levels)
        if res[0] != "value":
            return res, None
        V, size = res[1], res[2]
    A, asz = V, size
    if is_map:
        kb = _i32(i64(V))
        if kb < 0 or kb % 8 or 8 + kb > size:
            return ("fail",), V
        A, asz = (V + 8 + kb, size - 8 - kb) if side else (V + 8, kb)
        if asz < 8:
            return ("fail",), V
    cnt = _i32(i64(A))
    if cnt < 0 or 8 + ((cnt + 63) // 64) * 8 + 8 * cnt > asz:
        return ("fail",), V
    return ("array", A, cnt), V


def expect(rows, offs, n, spec, ecap=None) -> Want:
    """Everything fury_row_explode writes for elem_capacity ecap (None: E)."""
    _, _, _, least, exact = spec
    total = int(offs[n])
    w = Want()
    w.bad, w.V, w.A = [], [None] * n, [None] * n
    counts = np.zeros(n, np.int64)
    has = np.zeros(((n + 31) // 32) * 32, bool)
    for r in range(n):
        res, w.V[r] = locate_row(rows, offs, n, r, spec)
        if res[0] == "array":
            w.A[r], counts[r], has[r] = res[1], res[2], True
        elif res[0] == "fail":
            w.bad.append(r)
    w.lo = np.zeros(n + 1, np.int64)
    np.cumsum(counts, out=w.lo[1:])
    w.E = int(w.lo[n])
    w.entry_valid = np.packbits(has, bitorder="little")
    w.ecap = ecap = w.E if ecap is None else ecap
    seen = min(w.E, ecap)
    starts, sizes, parents, ordinals, positions, bad = [], [], [], [], [], set()
    for r in np.flatnonzero(counts > 0):
        if w.lo[r] >= seen:
            break
        A, k = w.A[r], int(min(counts[r], seen - w.lo[r]))        # the elements below the capacity
        m = int(counts[r])
        bm = ((m + 63) // 64) * 8
        null = np.unpackbits(rows[A + 8:A + 8 + bm], bitorder="little")[:k].astype(bool)
        slots = np.frombuffer(rows[A + 8 + bm:A + 8 + bm + 8 * k].tobytes(), "<u8")
        off = (slots >> np.uint64(32)).astype(np.uint32).view(np.int32).astype(np.int64)
        size = (slots & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32).astype(np.int64)
        ok = ((off >= 0) & (size >= 0) & (off % 8 == 0) & (size % 8 == 0) & (A + off + size <= total)
              & (size >= least))
        if exact:
            ok &= size == least
        if np.any(~null & ~ok):
            bad.add(int(r))
        keep = np.flatnonzero(~null & ok)
        starts.append(A + off[keep])
        sizes.append(size[keep])
        parents.append(np.full(len(keep), r, np.int64))
        ordinals.append(keep.astype(np.int32))
        positions.append(w.lo[r] + keep)
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)   # noqa: E731
    w.starts, w.sizes = cat(starts, np.int64), cat(sizes, np.int64)
    w.bad = sorted(set(w.bad) | bad)
    w.count = len(w.starts)
    w.kept_parents, w.kept_ordinals = cat(parents, np.int64), cat(ordinals, np.int32)
    w.offs = np.zeros(ecap + 1, np.int64)
    np.cumsum(w.sizes, out=w.offs[1:w.count + 1])
    w.offs[w.count + 1:] = w.offs[w.count]
    nbytes = int(w.offs[w.count])
    gather = np.repeat(w.starts - w.offs[:w.count], w.sizes) + np.arange(nbytes)
    w.data = rows[gather] if nbytes else np.zeros(0, np.uint8)
    w.parents = np.concatenate([w.kept_parents, np.full(ecap - w.count, -1, np.int64)])
    w.ordinals = np.concatenate([w.kept_ordinals, np.full(ecap - w.count, -1, np.int32)])
    bits = np.zeros(((ecap + 31) // 32) * 32, bool)
    bits[cat(positions, np.int64)] = True
    w.valid = np.packbits(bits, bitorder="little")
    return w


# -- one call into guarded buffers, everything compared ---------------------------------------------------
def _upload(src, shift=0, rows=None, offs=None):
    from fury_amd.encoder import RowBatch
    rows = src.rows if rows is None else rows
    t = torch.empty(len(rows) + 16, dtype=torch.uint8, device=src.dev)
    assert t.data_ptr() % 16 == 0
    d = t[shift:shift + len(rows)]
    d.copy_(torch.from_numpy(rows))
    o = torch.from_numpy(np.asarray(src.offs if offs is None else offs, np.int64)).to(src.dev)
    return RowBatch(d, o, src.n, src.enc.schema_hash)


def check_explode(src, path, side, what, cap=None, ecap=None, form="full", out_shift=0, src_shift=0,
                  stream=None, bound=False, calls=1, rows=None, offs=None, optional=True) -> Want:
    """form: "full", "measure" (out_rows NULL) or "count" (out_offsets NULL)."""
    dev, n = src.dev, src.n
    if rows is None and offs is None and ecap is None:
        w = src.want(path, side)
    else:
        w = expect(src.rows if rows is None else rows, src.offs if offs is None else offs, n,
                   src.spec(path, side), ecap)
    ecap = w.ecap
    cap = len(w.data) if cap is None else cap
    batch = _upload(src, src_shift, rows, offs)
    i64 = lambda k: torch.full((k,), -7, dtype=torch.int64, device=dev)   # noqa: E731
    u8 = lambda k: torch.full((k,), FILL, dtype=torch.uint8, device=dev)  # noqa: E731
    t = u8(GUARD + 16 + cap + GUARD)
    assert t.data_ptr() % 16 == 0
    at = GUARD + out_shift
    lo, ooffs, cnt, par = i64(n + 2), i64(ecap + 2), i64(2), i64(ecap + 1)
    ords = torch.full((ecap + 1,), -7, dtype=torch.int32, device=dev)
    nvb, evb = ((n + 31) // 32) * 4, ((ecap + 31) // 32) * 4
    ev, val = u8(nvb + 8), u8(evb + 8)
    count_form = form == "count"
    per_elem = optional and not count_form
    outs = (None if form != "full" else t[at:at + cap], None if count_form else ooffs[:ecap + 1],
            None if count_form else cnt[:1], par[:ecap] if per_elem and ecap else None,
            ords[:ecap] if per_elem and ecap else None, val[:evb] if per_elem and ecap else None)
    args = (lo[:n + 1], ev[:nvb] if optional and n else None) + outs
    if path is not None:
        args = (list(path),) + args
    kw = dict(side=side, elem_capacity=ecap, stream=stream)
    torch.cuda.synchronize()
    if bound:
        call = src.enc.bind_explode(batch, *args, **kw)
        for _ in range(calls):
            call()
    else:
        for _ in range(calls):
            src.enc.explode_into(batch, *args, **kw)
    torch.cuda.synchronize()
    assert_same(lo.cpu().numpy(), np.concatenate([w.lo, [-7]]), f"{what}: out_list_offsets")
    want_ev = np.full(nvb + 8, FILL, np.uint8)
    if optional and n:
        want_ev[:nvb] = w.entry_valid
    assert_same(ev.cpu().numpy(), want_ev, f"{what}: out_entry_validity")
    keep = lambda k, dt=np.int64: np.full(k, -7, dt)                      # noqa: E731
    assert_same(cnt.cpu().numpy(), keep(2) if count_form else np.array([w.count, -7], np.int64),
                f"{what}: out_count")
    assert_same(ooffs.cpu().numpy(), keep(ecap + 2) if count_form else np.concatenate([w.offs, [-7]]),
                f"{what}: out_offsets")
    assert_same(par.cpu().numpy(), np.concatenate([w.parents, [-7]]) if per_elem else keep(ecap + 1),
                f"{what}: out_parents")
    assert_same(ords.cpu().numpy(), np.concatenate([w.ordinals, np.array([-7], np.int32)]) if per_elem
                else keep(ecap + 1, np.int32), f"{what}: out_ordinals")
    want_val = np.full(evb + 8, FILL, np.uint8)
    if per_elem:
        want_val[:evb] = w.valid
    assert_same(val.cpu().numpy(), want_val, f"{what}: out_validity")
    want = np.full(t.numel(), FILL, np.uint8)
    if form == "full":
        k = min(cap, len(w.data))
        want[at:at + k] = w.data[:k]
    assert_same(t.cpu().numpy(), want, f"{what}: output buffer")
    return w


# 1. every target x row count -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("name,side", TARGETS, ids=lambda x: x)
def test_explode_flat(dev, name, side, n):
    src = source(dev, "flat", n)
    w = check_explode(src, (name,), side, f"flat {name} {side} n={n}")
    assert not w.bad
    if n >= 64:
        assert 0 < w.count < w.E                               # null elements and entries are both there
        assert 0 < int(np.unpackbits(w.entry_valid).sum()) < n    # and null fields
    if name == "fx":                                           # fixed-size elements: entry j at j * 24
        assert src.enc.element_encoder(name).schema().is_fixed
        assert np.array_equal(w.offs[:w.count + 1], np.arange(w.count + 1) * 24)
    check_explode(src, (name,), side, f"flat {name} n={n} without the optional outputs",
                  optional=False, out_shift=8)
    src.enc.device_status()


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("name,side", TARGETS, ids=lambda x: x)
def test_explode_nested(dev, name, side, n):
    src = source(dev, "nested", n)
    w = check_explode(src, ("outer", name), side, f"outer.{name} {side} n={n}")
    assert not w.bad
    if n >= 64:
        assert 0 < w.count < w.E
    src.enc.device_status()


def test_explode_one_long_list_among_empty_rows(dev):
    src = source(dev, "long", 65)
    for name, side in TARGETS:
        w = check_explode(src, (name,), side, f"4097 elements in row 21: {name}")
        assert w.E == 4097 and not w.bad and set(w.kept_parents) == {21}
    src.enc.device_status()


def test_explode_a_single_row_of_70000_elements(dev):
    src = source(dev, "huge", 1)
    w = check_explode(src, ("items",), "elements", "70000 elements in one row")
    assert w.E == 70000 and w.count == 70000 - 1 and not w.bad
    src.enc.device_status()


def test_explode_without_nulls(dev):
    src = source(dev, "valid", 65)
    for name, side in TARGETS:
        w = check_explode(src, (name,), side, f"no null fields: {name}")
        assert int(np.unpackbits(w.entry_valid).sum()) == 65 and not w.bad
    src.enc.device_status()


# 2. composition with the other entry points --------------------------------------------------------------
def _elements_of(beans, path, side):
    """The non-null elements of the field at `path` of every bean, in order."""
    out = []
    for b in beans:
        for name in path:
            b = None if b is None else b[name]
        for v in b or ():
            v = v[1] if side == "values" else v
            if v is not None:
                out.append(v)
    return out


def _decoded(child, batch):
    from fury_amd.beans import columns_to_beans, value_at
    from fury_amd.encoder import column_to_host
    cols = [column_to_host(c) for c in child.decode_batch(batch)]
    if hasattr(child, "_field"):                               # a collection encoder: one column
        return [value_at(child._field, cols[0], j) for j in range(batch.nrows)]
    return columns_to_beans(child.schema().fields, cols, batch.nrows)


def _encoded(child, values):
    from fury_amd.beans import beans_to_columns
    from fury_amd.encoder import column_to_device
    if hasattr(child, "_field"):
        cols = [child._column(values)]
    else:
        cols = [column_to_device(c, child.device)
                for c in beans_to_columns(child.schema().fields, values)]
    return child.encode_batch(cols, len(values))


@pytest.mark.parametrize("which,path,side", [("flat", ("items",), "elements"), ("flat", ("m",), "values"),
                                             ("flat", ("ll",), "elements"), ("flat", ("fx",), "elements"),
                                             ("nested", ("outer", "items"), "elements")],
                         ids=lambda x: x if isinstance(x, str) else ".".join(x))
def test_explode_then_decode_and_reencode(dev, which, path, side):
    from fury_amd.beans import columns_to_beans
    from fury_amd.encoder import column_to_host
    n = 257
    src = source(dev, which, n)
    w = src.want(path, side)
    parent = src.enc.decode_batch(_upload(src))
    beans = columns_to_beans(src.fields, [column_to_host(c) for c in parent], n)
    want = _elements_of(beans, path, side)                     # the parent's full decode
    assert want == _elements_of(src.beans, path, side) and len(want) == w.count
    child = src.enc.element_encoder(path, side)
    got, lo, ev, valid, par, ords = src.enc.explode(_upload(src), path, side)
    assert got.nrows == w.count and got.schema_hash == child.schema_hash
    assert_same(got.rows.cpu().numpy(), w.data, "explode: rows")
    assert_same(got.row_offsets.cpu().numpy(), w.offs[:w.count + 1], "explode: offsets")
    assert_same(lo.cpu().numpy(), w.lo, "explode: list offsets")
    assert_same(ev.cpu().numpy(), w.entry_valid[:(n + 7) // 8], "explode: entry validity")
    assert_same(valid.cpu().numpy(), w.valid[:(w.E + 7) // 8], "explode: element validity")
    assert_same(par.cpu().numpy(), w.kept_parents, "explode: parents")
    assert_same(ords.cpu().numpy(), w.kept_ordinals, "explode: ordinals")
    assert _decoded(child, got) == want
    again = _encoded(child, want)                              # byte for byte what the encoder writes
    assert_same(again.rows.cpu().numpy(), w.data, "encode_batch of the elements: rows")
    if child.schema().is_fixed:                                # no offsets: entry j at j * fixed_size
        assert again.row_offsets is None
        assert np.array_equal(w.offs[:w.count + 1], np.arange(w.count + 1) * child.schema().fixed_size)
    else:
        assert_same(again.row_offsets.cpu().numpy(), w.offs[:w.count + 1], "encode_batch: offsets")


def test_explode_then_project(dev):
    from fury_amd.beans import value_at
    from fury_amd.encoder import column_to_host
    src = source(dev, "flat", 257)
    got = src.enc.explode(_upload(src), "items")[0]
    child = src.enc.element_encoder("items")
    col = column_to_host(child.project_batch(got, ["s"])[0])
    want = [e["s"] for e in _elements_of(src.beans, ("items",), "elements")]
    assert [value_at(child.schema().fields[1], col, j) for j in range(got.nrows)] == want


@pytest.mark.parametrize("name,side", [("items", "elements"), ("m", "values"), ("ll", "elements")])
def test_extract_then_collection_explode(dev, name, side):
    """extract + ArrayEncoder / MapEncoder.explode = the path form, every output."""
    src = source(dev, "flat", 257)
    w = src.want((name,), side)
    values, _, idx = src.enc.extract(_upload(src), name, return_indices=True)
    coll = _Src(dev, src.enc.child_encoder(name), values.rows.cpu().numpy().copy(),
                values.row_offsets.cpu().numpy().copy(), values.nrows)
    c = check_explode(coll, None, side, f"collection form of {name}")
    assert_same(c.data, w.data, "collection form: bytes")
    assert_same(c.offs, w.offs, "collection form: offsets")
    assert_same(idx.cpu().numpy()[c.kept_parents], w.kept_parents, "collection form: parents")
    assert_same(c.kept_ordinals, w.kept_ordinals, "collection form: ordinals")
    got = coll.enc.explode(_upload(coll), side)
    assert_same(got[0].rows.cpu().numpy(), w.data, "ArrayEncoder / MapEncoder.explode: rows")
    assert got[0].schema_hash == src.enc.element_encoder(name, side).schema_hash
    coll.enc.device_status()


# 3. the reference's own bytes -----------------------------------------------------------------------------
def _fixture(dev, name):
    from fury_amd.beans import columns_to_beans
    from fury_amd.encoder import Encoders, RowBatch
    from tests import ref_fixtures as RF
    fx = RF.load(name)
    enc = Encoders.bean(fx.fields, device=dev)
    batch = RowBatch(torch.from_numpy(fx.rows).to(dev), torch.from_numpy(fx.row_offsets).to(dev),
                     fx.n, enc.schema_hash)
    return enc, batch, columns_to_beans(fx.fields, fx.columns, fx.n)


def test_reference_rows_list_list_struct(dev):
    enc, batch, beans = _fixture(dev, "list_list_struct")
    inner = enc.explode(batch, "ll")[0]                        # a batch of LIST<STRUCT> arrays
    lists = _elements_of(beans, ("ll",), "elements")
    assert inner.nrows == len(lists) > 8
    arr = enc.element_encoder("ll")
    assert _decoded(arr, inner) == lists
    structs = arr.explode(inner)[0]                            # explode again: the struct rows
    want = [s for lst in lists for s in lst if s is not None]
    assert structs.nrows == len(want) > 64
    assert _decoded(arr.element_encoder(), structs) == want
    enc.device_status()


def test_reference_rows_map_values_and_beana(dev):
    enc, batch, beans = _fixture(dev, "map_int32_struct")
    got = enc.explode(batch, "m", "values")[0]
    want = _elements_of(beans, ("m",), "values")
    assert got.nrows == len(want) > 40
    assert _decoded(enc.element_encoder("m", "values"), got) == want
    enc.device_status()
    enc, batch, beans = _fixture(dev, "beana")
    got = enc.explode(batch, "bean_b_list")[0]
    want = _elements_of(beans, ("bean_b_list",), "elements")
    assert got.nrows == len(want) > 0
    assert _decoded(enc.element_encoder("bean_b_list"), got) == want
    enc.device_status()


# 4. capacities, alignment, streams --------------------------------------------------------------------------
@pytest.mark.parametrize("name,side", [("items", "elements"), ("m", "values")])
def test_explode_capacities(dev, name, side):
    src = source(dev, "flat", 257)
    path = (name,)
    w = src.want(path, side)
    total = len(w.data)
    assert total > 4096 and w.E > 1024
    for cap in (0, 8, (total // 2) & ~7, total - 8, total):
        check_explode(src, path, side, f"{name}: out_capacity {cap} of {total}", cap=cap,
                      out_shift=8 if cap % 16 else 0)
    for ecap in (0, w.E - 1, w.E, w.E + 65, len(src.rows) // 8):
        c = check_explode(src, path, side, f"{name}: elem_capacity {ecap} of {w.E}", ecap=ecap)
        assert c.E == w.E and np.array_equal(c.lo, w.lo)       # out_list_offsets stays complete
        assert c.count == (w.count if ecap >= w.E else int(np.sum(w.valid_positions() < ecap)))
        check_explode(src, path, side, f"{name}: elem_capacity {ecap}, half the bytes", ecap=ecap,
                      cap=(len(c.data) // 2) & ~7)
    check_explode(src, path, side, f"{name}: the measure form", form="measure")
    check_explode(src, path, side, f"{name}: the count form", form="count")
    check_explode(src, path, side, f"{name}: the count form without entry validity", form="count",
                  optional=False)
    src.enc.device_status()


@pytest.mark.parametrize("n", [65, 4097])
def test_explode_alignment(dev, n):
    src = source(dev, "flat", n)
    for src_shift, out_shift in ((0, 8), (8, 0), (8, 8)):
        check_explode(src, ("items",), "elements", f"n={n} shifts {src_shift}/{out_shift}",
                      src_shift=src_shift, out_shift=out_shift)
    src.enc.device_status()


def test_explode_on_a_side_stream_and_bound_twice(dev):
    src = source(dev, "nested", 257)
    s = torch.cuda.Stream(device=dev)
    path = ("outer", "m")
    check_explode(src, path, "values", "explode_into on a side stream", stream=s, out_shift=8)
    check_explode(src, path, "values", "bind_explode called twice", bound=True, calls=2)
    check_explode(src, path, "values", "bind_explode twice on a side stream", bound=True, calls=2,
                  stream=s)
    src.enc.device_status(s)
    src.enc.device_status()


# 5. malformed input: the bounds rules -----------------------------------------------------------------------
def _put64(rows, pos, v):
    rows[pos:pos + 8] = np.frombuffer((v & 0xFFFFFFFFFFFFFFFF).to_bytes(8, "little"), np.uint8)


def _put_slot(rows, pos, off, size):
    _put64(rows, pos, ((off & 0xFFFFFFFF) << 32) | (size & 0xFFFFFFFF))


def _get_slot(rows, pos):
    s = int.from_bytes(rows[pos:pos + 8].tobytes(), "little")
    return _i32(s >> 32), _i32(s)


def _victims(w, n):
    """About one row in 16 among the rows that produce entries (never the last row)."""
    rows = [int(r) for r in np.unique(w.kept_parents) if r % 16 == 5 and r < n - 1]
    assert len(rows) >= 4
    return rows


def _check_malformed(src, path, side, what, victims, rows=None, offs=None, whole_rows=True):
    from fury_amd.encoder import IndexOutOfBoundsException
    src.enc.device_status()
    w = check_explode(src, path, side, what, rows=rows, offs=offs, out_shift=8)
    assert w.bad == victims, what
    clean = src.want(path, side)
    if whole_rows:                                             # those rows: null, zero elements
        bits = np.unpackbits(w.entry_valid, bitorder="little")
        assert not bits[victims].any() and not np.diff(w.lo)[victims].any()
        assert set(w.kept_parents) == set(clean.kept_parents) - set(victims)
    else:                                                      # those elements: null, the counts stay
        assert np.array_equal(w.lo, clean.lo) and w.count < clean.count
    with pytest.raises(IndexOutOfBoundsException, match=f"row ({'|'.join(map(str, victims))}) "):
        src.enc.device_status()
    src.enc.device_status()                                    # raised once, then clear
    check_explode(src, path, side, f"{what}: the next call is clean")
    src.enc.device_status()


def _least_bad_count(cnt, asz):
    """The smallest count whose header and slots no longer fit an array of asz bytes."""
    c = cnt
    while 8 + ((c + 63) // 64) * 8 + 8 * c <= asz:
        c += 1
    return c


COUNT_EDITS = {
    "a negative count": lambda cnt, asz: -1,
    "a huge count": lambda cnt, asz: 0x7FFFFFFF,
    "a header longer than the array": lambda cnt, asz: asz // 8,
    "one slot more than the array holds": _least_bad_count,
}


@pytest.mark.parametrize("edit", list(COUNT_EDITS))
@pytest.mark.parametrize("name,side", [("items", "elements"), ("m", "values")])
def test_malformed_element_count(dev, name, side, edit):
    src = source(dev, "flat", 257)
    w = src.want((name,), side)
    victims = _victims(w, src.n)
    rows = src.rows.copy()
    levels = levels_of(src.fields, (name,))
    for r in victims:
        res, _ = walk(src.rows, src.offs, src.n, r, levels)
        asz = res[2] if side == "elements" else res[1] + res[2] - w.A[r]
        _put64(rows, w.A[r], COUNT_EDITS[edit](int(np.diff(w.lo)[r]), asz))
    _check_malformed(src, (name,), side, f"{name}: {edit}", victims, rows=rows)


@pytest.mark.parametrize("edit", ["negative", "odd", "larger than size - 8"])
def test_malformed_key_array_bytes(dev, edit):
    src = source(dev, "flat", 257)
    w = src.want(("m",), "values")
    victims = _victims(w, src.n)
    rows = src.rows.copy()
    levels = levels_of(src.fields, ("m",))
    for r in victims:
        res, _ = walk(src.rows, src.offs, src.n, r, levels)
        kb = _i32(int.from_bytes(rows[w.V[r]:w.V[r] + 4].tobytes(), "little"))
        _put64(rows, w.V[r], {"negative": -8, "odd": kb + 4, "larger than size - 8": res[2]}[edit])
    _check_malformed(src, ("m",), "values", f"keyArrayBytes {edit}", victims, rows=rows)


SLOT_EDITS = {
    "off past the batch": lambda off, size, total: (total + 64, size),
    "off + size past the batch": lambda off, size, total: (off, total),
    "negative off": lambda off, size, total: (-8, size),
    "negative size": lambda off, size, total: (off, -8),
    "off not a multiple of 8": lambda off, size, total: (off + 4, size),
    "size not a multiple of 8": lambda off, size, total: (off, size + 4),
    "size below the element header": lambda off, size, total: (off, 16),
}


def _slot_positions(w, r):
    """Byte positions of the slots of row r's non-null elements."""
    m = int(w.lo[r + 1] - w.lo[r])
    bm = ((m + 63) // 64) * 8
    return [w.A[r] + 8 + bm + 8 * int(i) for i in w.kept_ordinals[w.kept_parents == r]]


@pytest.mark.parametrize("edit", list(SLOT_EDITS))
def test_malformed_element_slot(dev, edit):
    src = source(dev, "flat", 257)
    path, side = ("items",), "elements"                       # items' elements: 2 fields, header 24
    w = src.want(path, side)
    victims = _victims(w, src.n)
    rows = src.rows.copy()
    for r in victims:
        ps = _slot_positions(w, r)
        for pos in {ps[0], ps[-1], ps[len(ps) // 2]}:
            _put_slot(rows, pos, *SLOT_EDITS[edit](*_get_slot(rows, pos), len(rows)))
    _check_malformed(src, path, side, f"element slots: {edit}", victims, rows=rows, whole_rows=False)


def test_fixed_element_of_another_size(dev):
    src = source(dev, "flat", 257)
    path, side = ("fx",), "elements"
    w = src.want(path, side)
    victims = _victims(w, src.n)
    rows = src.rows.copy()
    for r in victims:
        pos = _slot_positions(w, r)[0]
        off, size = _get_slot(rows, pos)
        assert size == 24
        _put_slot(rows, pos, off, 32)
    _check_malformed(src, path, side, "fx element with size != fixed_size", victims, rows=rows,
                     whole_rows=False)


def test_malformed_entry_offsets_of_a_collection_batch(dev):
    src = source(dev, "flat", 257)
    values, _ = src.enc.extract(_upload(src), "items")
    coll = _Src(dev, src.enc.child_encoder("items"), values.rows.cpu().numpy().copy(),
                values.row_offsets.cpu().numpy().copy(), values.nrows)
    w = coll.want(None, "elements")
    victims = _victims(w, coll.n)
    offs = coll.offs.copy()
    total = len(coll.rows)
    for j, r in enumerate(victims):                            # misaligned, past the batch, negative
        offs[r] = (offs[r] + 4, total + 64, -8, offs[r] + 4)[j % 4]
    w2 = expect(coll.rows, offs, coll.n, coll.spec(None, "elements"))
    bad = sorted(set(w2.bad))
    assert set(victims) <= set(bad)                            # a moved start also breaks row r - 1
    _check_malformed(coll, None, "elements", "entry offsets of a collection batch", bad, offs=offs)


def test_corruption_off_the_chosen_array_is_no_error(dev):
    src = source(dev, "flat", 257)
    wk = src.want(("m",), "values")
    rows = src.rows.copy()
    for r in _victims(wk, src.n):                              # the key array: count and first slot
        _put64(rows, wk.V[r] + 8, -1)
        _put_slot(rows, wk.V[r] + 24, len(rows) + 64, -8)
    pos = int(src.offs[21]) + 8 + 8 * 1                        # and row 21's `items` slot
    _put_slot(rows, pos, -8, 4)
    src.enc.device_status()
    w = check_explode(src, ("m",), "values", "corrupt key arrays / items slot", rows=rows)
    assert not w.bad and w.count == wk.count
    src.enc.device_status()


# 6. the empty batch, and a foreign batch ------------------------------------------------------------------------
def test_explode_of_no_rows(dev):
    from fury_amd.encoder import Encoders, RowBatch
    enc = Encoders.bean(explode_fields(), device=dev)
    empty = RowBatch(torch.zeros(16, dtype=torch.uint8, device=dev)[:0],
                     torch.zeros(1, dtype=torch.int64, device=dev), 0, enc.schema_hash)
    lo = torch.full((2,), -7, dtype=torch.int64, device=dev)
    ooffs = torch.full((2,), -7, dtype=torch.int64, device=dev)
    cnt = torch.full((2,), -7, dtype=torch.int64, device=dev)
    out = torch.full((64,), FILL, dtype=torch.uint8, device=dev)
    enc.explode_into(empty, "items", lo[:1], None, out, ooffs[:1], cnt[:1])
    torch.cuda.synchronize()
    assert lo.tolist() == [0, -7] and ooffs.tolist() == [0, -7] and cnt.tolist() == [0, -7]
    assert bool((out == FILL).all())
    lo.fill_(-7)
    enc.explode_into(empty, "items", lo[:1])                   # the count form
    torch.cuda.synchronize()
    assert lo.tolist() == [0, -7]
    got, lo, ev, valid, par, ords = enc.explode(empty, "items")
    assert got.nrows == 0 and got.rows.numel() == 0 and got.row_offsets.tolist() == [0]
    assert lo.tolist() == [0] and ev.numel() == valid.numel() == par.numel() == ords.numel() == 0
    assert got.schema_hash == enc.element_encoder("items").schema_hash
    enc.device_status()


def test_foreign_schema_hash(dev):
    from fury_amd.encoder import ClassNotCompatibleException, RowBatch
    src = source(dev, "flat", 65)
    b = _upload(src)
    foreign = RowBatch(b.rows, b.row_offsets, b.nrows, b.schema_hash + 1)
    with pytest.raises(ClassNotCompatibleException, match="Schema is not consistent"):
        src.enc.explode(foreign, "items")
