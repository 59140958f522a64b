"""The numpy model of fury_row_implode and fury_row_wrap, written from the rules of include/fury_row.h
alone and pinned on the CPU in two ways.  To the oracle: applied to the numpy models of explode /
extract (tests/test_explode.py, tests/test_extract.py) of the oracle's rows it gives, byte for byte, the
oracle's rows of the one-field schema.  To the reference's own C++ writer (tests/golden/ref_cpp/):
list_list_struct exploded twice and imploded twice is the fixture again, and the value arrays of
map_int32_struct come back as the arrays an encoder writes.  tests/test_implode.py compares the GPU
against this model, which alone also covers malformed input."""
from __future__ import annotations

import numpy as np
import pytest

from fury_amd import types as T
from tests.test_explode_abi import explode_fields
from tests.test_select_model import INT32_MAX, Want, expect_select

MAX_ELEMS = (INT32_MAX - 15) // 8


def least_of(f) -> int:
    """The least size of a value of the STRUCT / LIST / MAP field f."""
    return T.fixed_size(f.children) if f.type_id == T.STRUCT else 8


def _bits(bitmap, n):
    """Bits [0, n) of an Arrow bitmap (None: all set) as bools."""
    if bitmap is None:
        return np.ones(n, bool)
    return np.unpackbits(np.asarray(bitmap, np.uint8), bitorder="little")[:n].astype(bool)


class Elements:
    """Per element e of [0, E): kept (present and well-formed), failed (present, not well-formed),
    and start / size of the value a kept one takes (size 0 otherwise)."""

    def __init__(self, vo, num_values, validity, E, least):
        vo = np.asarray(vo, np.int64)
        VT = int(vo[num_values])
        present = _bits(validity, E)
        rank = np.cumsum(present) - present                    # 1 bits before e, in the whole bitmap
        has = present & (rank < num_values)
        v = np.where(has, rank, 0)
        s0 = vo[v] if num_values else np.zeros(E, np.int64)
        s1 = vo[v + 1] if num_values else np.zeros(E, np.int64)
        ok = has & (0 <= s0) & (s0 <= s1) & (s1 <= VT) & (s0 % 8 == 0) & ((s1 - s0) % 8 == 0) & \
            (s1 - s0 >= least)
        self.kept, self.failed = ok, present & ~ok
        self.start = np.where(ok, s0, 0)
        self.size = np.where(ok, s1 - s0, 0)
        self.cs = np.concatenate([[0], np.cumsum(self.size)])  # kept bytes before element e
        self.nfail = np.concatenate([[0], np.cumsum(self.failed)])


def _array(values, el, a, n):
    """Rule 2: the BinaryArray of elements [a, a + n)."""
    bm = ((n + 63) // 64) * 8
    kept = el.kept[a:a + n]
    null = np.zeros(bm * 8, bool)
    null[:n] = ~kept
    head = 8 + bm + 8 * n
    off = head + el.cs[a:a + n] - el.cs[a]
    slots = np.where(kept, (off.astype(np.uint64) << np.uint64(32)) | el.size[a:a + n].astype(np.uint64),
                     np.uint64(0)).astype("<u8")
    parts = [np.array([n], "<i8").tobytes(), np.packbits(null, bitorder="little").tobytes(),
             slots.tobytes()]
    parts += [values[s:s + z].tobytes() for s, z, k in zip(el.start[a:a + n], el.size[a:a + n], kept) if k]
    return b"".join(parts)


NULL_ROW = (1).to_bytes(8, "little") + bytes(8)


def _finish(parts, bad) -> Want:
    w = Want()
    w.bad = bad
    w.data = np.frombuffer(b"".join(parts), np.uint8).copy()
    w.offs = np.zeros(len(parts) + 1, np.int64)
    np.cumsum([len(p) for p in parts], out=w.offs[1:])
    return w


def expect_implode(values, vo, num_values, lo, nrows, entry_validity, elem_validity, E, least,
                   rows_form) -> Want:
    """What fury_row_implode writes: ``data``, ``offs`` and the reported rows ``bad``."""
    values = np.asarray(values, np.uint8)
    el = Elements(vo, num_values, elem_validity, E, least)
    present = _bits(entry_validity, nrows)
    prefix = 16 if rows_form else 0
    parts, bad = [], []
    for r in range(nrows):
        if not present[r]:                                     # rule 5: never reported
            parts.append(NULL_ROW)
            continue
        a, b = int(lo[r]), int(lo[r + 1])
        ok = 0 <= a <= b <= E and b - a <= MAX_ELEMS           # rule 1
        if ok:
            n = b - a
            A = 8 + ((n + 63) // 64) * 8 + 8 * n + int(el.cs[b] - el.cs[a])
            ok = prefix + A <= INT32_MAX - 7                   # rule 3
        if not ok:
            bad.append(r)
            parts.append(NULL_ROW if rows_form else bytes(8))  # rules 5 and 6
            continue
        if el.nfail[b] > el.nfail[a]:
            bad.append(r)
        arr = _array(values, el, a, n)
        assert len(arr) == A
        parts.append((bytes(8) + ((16 << 32) | A).to_bytes(8, "little") if rows_form else b"") + arr)
    return _finish(parts, bad)


def expect_wrap(values, vo, num_values, validity, nrows, least) -> Want:
    """What fury_row_wrap writes."""
    values = np.asarray(values, np.uint8)
    el = Elements(vo, num_values, validity, nrows, least)
    parts, bad = [], []
    for r in range(nrows):
        s, z = int(el.start[r]), int(el.size[r])
        if el.kept[r] and 16 + z <= INT32_MAX - 7:
            parts.append(bytes(8) + ((16 << 32) | z).to_bytes(8, "little") + values[s:s + z].tobytes())
            continue
        if el.failed[r] or el.kept[r]:
            bad.append(r)
        parts.append(NULL_ROW)
    return _finish(parts, bad)


def implode_exploded(w, least, rows_form, n, entry_validity=True) -> Want:
    """The implode model applied to an explode expectation (tests.test_explode.expect)."""
    return expect_implode(w.data, w.offs, w.ecap, w.lo, n, w.entry_valid if entry_validity else None,
                          w.valid, w.E, least, rows_form)


# -- the model against the oracle --------------------------------------------------------------------
N = 65
TARGETS = [("items", "elements"), ("ll", "elements"), ("fx", "elements"), ("m", "values")]


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    return O


class Encoded:
    """The oracle's rows of `beans` under `fields`, and what explode / extract models need."""

    def __init__(self, oracle, fields, beans):
        from fury_amd.beans import beans_to_columns
        self.fields, self.beans, self.n = list(fields), beans, len(beans)
        self.cols = beans_to_columns(self.fields, beans)
        rows, offs = oracle.encode(self.fields, self.cols, self.n)
        self.rows, self.offs = np.asarray(rows, np.uint8), np.asarray(offs, np.int64)

    def field(self, path):
        fields = self.fields
        for name in path:
            node = fields[[f.name for f in fields].index(name)]
            fields = node.children
        return node

    def exploded(self, path, side="elements"):
        from tests.test_explode import _Src, expect
        spec = _Src(None, None, self.rows, self.offs, self.n, self.fields).spec(tuple(path), side)
        return expect(self.rows, self.offs, self.n, spec)

    def extracted(self, path):
        from tests.test_extract import expect, levels_of
        return expect(self.rows, self.offs, self.n, levels_of(self.fields, path))


def list_target(name, elem):
    """A fresh one-field LIST schema around the element field `elem`."""
    return [T.Field(name, T.LIST, True, (T.Field("item", elem.type_id, elem.nullable, elem.children),))]


def value_lists(beans, path):
    """Per bean the list of a MAP field's values (None: a null map)."""
    out = []
    for b in beans:
        for name in path:
            b = None if b is None else b[name]
        out.append(None if b is None else [v for _, v in b])
    return out


@pytest.fixture(scope="module")
def flat(oracle):
    from tests.test_explode import flat_beans
    return Encoded(oracle, explode_fields(), flat_beans(N))


@pytest.fixture(scope="module")
def nested(oracle):
    from tests.test_explode import nested_beans, nested_fields
    return Encoded(oracle, nested_fields(), nested_beans(N))


def _one_field_rows(oracle, src, path, side):
    """The oracle's rows of the one-field schema of the list at `path` (a map's values: as a fresh
    LIST<STRUCT>), and that schema's element field."""
    f = src.field(path)
    if side == "values":
        from fury_amd.beans import beans_to_columns
        fields = list_target("mv", f.children[1])
        cols = beans_to_columns(fields, [{"mv": v} for v in value_lists(src.beans, path)])
        rows, offs = oracle.encode(fields, cols, src.n)
        return np.asarray(rows, np.uint8), np.asarray(offs, np.int64), fields[0].children[0]
    k = [g.name for g in src.fields].index(path[0])
    rows, offs = oracle.encode([f], [src.cols[k]], src.n)
    return np.asarray(rows, np.uint8), np.asarray(offs, np.int64), f.children[0]


@pytest.mark.parametrize("name,side", TARGETS, ids=lambda x: x)
def test_rows_form_equals_the_oracle_and_select(oracle, flat, name, side):
    w = flat.exploded((name,), side)
    assert not w.bad and 0 < w.count < w.E
    want, want_offs, elem = _one_field_rows(oracle, flat, (name,), side)
    got = implode_exploded(w, least_of(elem), True, N)
    assert not got.bad
    assert np.array_equal(got.offs, want_offs) and np.array_equal(got.data, want), name
    if side == "elements":                                     # = fury_row_select of that field
        k = [f.name for f in flat.fields].index(name)
        sel = expect_select(flat.rows, flat.offs, N, flat.fields, [k])
        assert np.array_equal(got.offs, sel.offs) and np.array_equal(got.data, sel.data), name


@pytest.mark.parametrize("name,side", TARGETS, ids=lambda x: x)
def test_collection_form_equals_extract_and_the_encoder(oracle, flat, name, side):
    """Without null rows the collection form is fury_row_extract's batch; a null row is an array the
    extract does not have, so the rows are compared one by one."""
    w = flat.exploded((name,), side)
    want, want_offs, elem = _one_field_rows(oracle, flat, (name,), side)
    got = implode_exploded(w, least_of(elem), False, N, entry_validity=False)
    assert not got.bad
    has = _bits(w.entry_valid, N)
    assert 0 < has.sum() < N
    for r in range(N):
        mine = got.data[got.offs[r]:got.offs[r + 1]].tobytes()
        # the oracle's row is [bitmap][slot][array]: the array is what an ArrayEncoder writes
        assert mine == (want[want_offs[r] + 16:want_offs[r + 1]].tobytes() if has[r] else bytes(8)), r
    if side == "elements":
        ex = flat.extracted((name,))
        rows = np.flatnonzero(has)
        assert np.array_equal(ex.kept, rows)
        assert ex.data.tobytes() == b"".join(
            got.data[got.offs[r]:got.offs[r + 1]].tobytes() for r in rows)


def test_a_nested_path(oracle, nested):
    """outer.items: explode along the path, implode in both forms = the oracle's rows of a fresh
    one-field schema / the arrays inside them."""
    from fury_amd.beans import beans_to_columns
    path = ("outer", "items")
    w = nested.exploded(path)
    assert not w.bad and 0 < w.count < w.E
    f = nested.field(path)
    lists = [None if b["outer"] is None else b["outer"]["items"] for b in nested.beans]
    want, want_offs = oracle.encode([f], beans_to_columns([f], [{"items": v} for v in lists]), N)
    got = implode_exploded(w, least_of(f.children[0]), True, N)
    assert not got.bad and np.array_equal(got.offs, want_offs) and np.array_equal(got.data, want)
    ex = nested.extracted(path)
    coll = implode_exploded(w, least_of(f.children[0]), False, N, entry_validity=False)
    rows = np.flatnonzero(_bits(w.entry_valid, N))
    assert ex.data.tobytes() == b"".join(coll.data[coll.offs[r]:coll.offs[r + 1]].tobytes() for r in rows)


@pytest.mark.parametrize("path", [("items",), ("m",), ("ll",)], ids=".".join)
def test_wrap_of_extract_equals_select(oracle, flat, path):
    ex = flat.extracted(path)
    assert not ex.bad and 0 < ex.count < N
    k = [f.name for f in flat.fields].index(path[0])
    got = expect_wrap(ex.data, ex.offs, N, ex.valid, N, least_of(flat.fields[k]))
    sel = expect_select(flat.rows, flat.offs, N, flat.fields, [k])
    want, want_offs = oracle.encode([flat.fields[k]], [flat.cols[k]], N)
    assert not got.bad
    assert np.array_equal(got.offs, sel.offs) and np.array_equal(got.data, sel.data)
    assert np.array_equal(got.offs, want_offs) and np.array_equal(got.data, want)


def test_wrap_of_a_nested_struct(oracle, nested):
    ex = nested.extracted(("outer",))
    assert not ex.bad and 0 < ex.count < N
    got = expect_wrap(ex.data, ex.offs, N, ex.valid, N, least_of(nested.fields[1]))
    want, want_offs = oracle.encode([nested.fields[1]], [nested.cols[1]], N)
    assert not got.bad and np.array_equal(got.offs, want_offs) and np.array_equal(got.data, want)


# -- the model against the reference's own C++ writer ---------------------------------------------------
class Fixture:
    def __init__(self, name):
        from tests import ref_fixtures as RF
        fx = RF.load(name)
        self.fields, self.n = fx.fields, fx.n
        self.rows, self.offs = np.asarray(fx.rows, np.uint8), np.asarray(fx.row_offsets, np.int64)
        self.cols = fx.columns

    exploded = Encoded.exploded
    extracted = Encoded.extracted
    field = Encoded.field


def test_reference_list_list_struct_twice_down_and_twice_up():
    from tests.test_explode import expect
    fx = Fixture("list_list_struct")
    assert len(fx.fields) == 1                                 # already a one-field schema
    outer = fx.exploded(("ll",))                               # a batch of LIST<STRUCT> arrays
    assert not outer.bad and outer.count > 8
    inner = expect(outer.data, outer.offs, outer.count, (None, False, 0, 24, False))
    assert not inner.bad and inner.count > 64 and inner.count < inner.E
    ll = fx.fields[0]
    arrays = expect_implode(inner.data, inner.offs, inner.ecap, inner.lo, outer.count, None,
                            inner.valid, inner.E, least_of(ll.children[0].children[0]), False)
    assert not arrays.bad
    assert np.array_equal(arrays.data, outer.data)
    assert np.array_equal(arrays.offs, outer.offs[:outer.count + 1])
    rows = expect_implode(arrays.data, arrays.offs, outer.count, outer.lo, fx.n, outer.entry_valid,
                          outer.valid, outer.E, least_of(ll.children[0]), True)
    assert not rows.bad
    assert np.array_equal(rows.offs, fx.offs) and np.array_equal(rows.data, fx.rows)


def test_reference_map_values_as_arrays(oracle):
    """The value arrays of map_int32_struct: explode, implode in collection form = the array an
    encoder writes for the same elements, which for a map's value array is the array in the row."""
    from fury_amd.beans import beans_to_columns, columns_to_beans
    from tests.test_explode import locate_row
    fx = Fixture("map_int32_struct")
    w = fx.exploded(("m",), "values")
    assert not w.bad and w.count > 40 and w.count < w.E
    val = fx.field(("m",)).children[1]
    got = expect_implode(w.data, w.offs, w.ecap, w.lo, fx.n, None, w.valid, w.E, least_of(val), False)
    assert not got.bad
    fields = list_target("mv", val)
    lists = value_lists(columns_to_beans(fx.fields, fx.cols, fx.n), ("m",))
    want, want_offs = oracle.encode(fields, beans_to_columns(fields, [{"mv": v} for v in lists]), fx.n)
    want = np.asarray(want, np.uint8)
    has = _bits(w.entry_valid, fx.n)
    assert 0 < has.sum() < fx.n
    for r in range(fx.n):
        mine = got.data[got.offs[r]:got.offs[r + 1]].tobytes()
        assert mine == (want[want_offs[r] + 16:want_offs[r + 1]].tobytes() if has[r] else bytes(8)), r
        if has[r]:                                             # and the reference's own bytes
            A = w.A[r]
            assert mine == fx.rows[A:A + len(mine)].tobytes(), r


def test_reference_nested_list_wrapped(oracle):
    """The fixture `nested` (id, score, vals LIST<INT64>): extract vals, wrap = select {vals} = the
    oracle's rows of the one-field schema."""
    fx = Fixture("nested")
    k = [f.name for f in fx.fields].index("vals")
    ex = fx.extracted(("vals",))
    assert not ex.bad and ex.count > 0
    got = expect_wrap(ex.data, ex.offs, fx.n, ex.valid, fx.n, 8)
    sel = expect_select(fx.rows, fx.offs, fx.n, fx.fields, [k])
    want, want_offs = oracle.encode([fx.fields[k]], [fx.cols[k]], fx.n)
    assert not got.bad
    assert np.array_equal(got.offs, sel.offs) and np.array_equal(got.data, sel.data)
    assert np.array_equal(got.offs, want_offs) and np.array_equal(got.data, want)


# -- malformed input, by hand --------------------------------------------------------------------------
def _values(*sizes):
    """Values of the given sizes, value v filled with byte v + 1."""
    vo = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    data = np.concatenate([np.full(s, v + 1, np.uint8) for v, s in enumerate(sizes)] or
                          [np.zeros(0, np.uint8)])
    return data, vo


def _row(arr):
    return bytes(8) + ((16 << 32) | len(arr)).to_bytes(8, "little") + arr


def _arr(n, nulls, slots, payload):
    bm = ((n + 63) // 64) * 8
    bits = sum(1 << i for i in nulls)
    return (n.to_bytes(8, "little") + bits.to_bytes(bm, "little") +
            b"".join(((o << 32) | s).to_bytes(8, "little") if s else bytes(8) for o, s in slots) + payload)


def test_the_layout_by_hand():
    data, vo = _values(24, 32, 24)
    lo = np.array([0, 2, 2, 4], np.int64)
    valid = np.packbits([1, 0, 1, 1], bitorder="little")         # element 1 is null
    got = expect_implode(data, vo, 3, lo, 3, None, valid, 4, 24, True)
    r0 = _row(_arr(2, [1], [(32, 24), (0, 0)], bytes([1]) * 24))
    r1 = _row(_arr(0, [], [], b""))
    r2 = _row(_arr(2, [], [(32, 32), (64, 24)], bytes([2]) * 32 + bytes([3]) * 24))
    assert got.data.tobytes() == r0 + r1 + r2 and not got.bad
    assert list(got.offs) == [0, len(r0), len(r0) + len(r1), len(r0) + len(r1) + len(r2)]
    coll = expect_implode(data, vo, 3, lo, 3, None, valid, 4, 24, False)
    assert coll.data.tobytes() == r0[16:] + r1[16:] + r2[16:]
    ev = np.packbits([1, 0, 1], bitorder="little")               # row 1 null
    got = expect_implode(data, vo, 3, lo, 3, ev, valid, 4, 24, True)
    assert got.data.tobytes() == r0 + NULL_ROW + r2 and not got.bad
    w = expect_wrap(data, vo, 3, valid, 4, 24)
    assert w.data.tobytes() == (_row(bytes([1]) * 24) + NULL_ROW + _row(bytes([2]) * 32) +
                                _row(bytes([3]) * 24)) and not w.bad


def test_malformed_input_by_hand():
    data, vo = _values(24, 32, 24, 40)
    lo = np.array([0, 2, 4], np.int64)
    clean = expect_implode(data, vo, 4, lo, 2, None, None, 4, 24, True)
    assert not clean.bad

    def run(lo=lo, vo=vo, nv=4, ev=None, lv=None, E=4, least=24, rows_form=True):
        return expect_implode(data, vo, nv, np.asarray(lo, np.int64), 2, ev, lv, E, least, rows_form)

    got = run(lo=[2, 1, 4])                                      # decreasing: row 0 fails, row 1 = [1, 4)
    assert got.bad == [0] and got.data[:16].tobytes() == NULL_ROW
    assert got.data[16 + 16:16 + 24].tobytes() == (3).to_bytes(8, "little")
    got = run(lo=[0, 2, 5])                                      # past num_elements
    assert got.bad == [1] and got.data[-16:].tobytes() == NULL_ROW
    assert run(lo=[0, 2, 5], rows_form=False).data[-8:].tobytes() == bytes(8)
    assert run(lo=[-1, 2, 4]).bad == [0]
    odd = vo.copy()
    odd[2] += 4                                                  # values 1 and 2: sizes 36 and 20
    got = run(vo=odd)
    assert got.bad == [0, 1]
    arr = _arr(2, [1], [(32, 24), (0, 0)], bytes([1]) * 24)      # element 1 null, none of its bytes
    assert got.data[:got.offs[1]].tobytes() == _row(arr)
    got = run(least=32)                                          # values 0 and 2 are below least
    assert got.bad == [0, 1]
    dec = vo.copy()
    dec[1] = 64                                                  # value 0 [0, 64) fine, value 1 [64, 56)
    got = run(vo=dec)
    assert got.bad == [0]
    got = run(nv=3)                                              # element 3 finds no value
    assert got.bad == [1]
    ev = np.packbits([0, 1], bitorder="little")
    got = run(lo=[3, 0, 4], ev=ev)                               # a null row is never reported
    assert got.bad == [] and got.data[:16].tobytes() == NULL_ROW
    got = run(vo=odd, ev=ev)                                     # nor the failed value it would hold
    assert got.bad == [1]
    # ranks count through null and failed rows: row 1 still takes values 2 and 3
    got = run(ev=ev)
    assert got.data[16:].tobytes() == clean.data[clean.offs[1]:].tobytes()
    w = expect_wrap(data, odd, 4, None, 4, 24)
    assert w.bad == [1, 2] and list(np.diff(w.offs)) == [40, 16, 16, 56]
    w = expect_wrap(data, vo, 2, np.packbits([1, 0, 1, 1], bitorder="little"), 4, 24)
    assert w.bad == [3] and list(np.diff(w.offs)) == [40, 16, 48, 16]
