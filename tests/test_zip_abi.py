"""CPU checks of the zip's C ABI (fury_schema_zip / fury_row_zip) and of its Python surface: the zipped
schema equals a schema built directly from the picked fields, and every argument error is reported on
the host, before any device work, with its status and a message that names the function.  Host
buffers stand in for device memory and are never dereferenced: every fury_row_zip call here fails
first."""
from __future__ import annotations

import ctypes

import pytest

from fury_amd import types as T
from fury_amd.workloads import SCHEMAS
from tests.test_extract_abi import deep_fields
from tests.test_select_abi import (CAPACITY, INVALID, OK, UNSUPPORTED, _buf, _err, _info,
                                   _selected)


@pytest.fixture(scope="module")
def L():
    from fury_amd import _native as N
    return N.lib()


@pytest.fixture(scope="module")
def schemas():
    from fury_amd.encoder import Encoders, Schema
    arr = Encoders.array_encoder(T.field("item", T.INT64), device="cpu")
    return {"foo": Schema(SCHEMAS["foo"]), "deep": Schema(deep_fields()),
            "struct100": Schema(SCHEMAS["struct100"]), "array": arr.schema(), "_keep": arr}


FIELDS = {"foo": SCHEMAS["foo"], "deep": deep_fields(), "struct100": SCHEMAS["struct100"]}


def _handles(*hs):
    return (ctypes.c_void_p * max(len(hs), 1))(*hs)


def _picks(*pairs):
    flat = [w for p in pairs for w in p]
    return (ctypes.c_int32 * max(len(flat), 2))(*flat), len(pairs)


def _zipped(L, schemas, names, pairs):
    h = ctypes.c_void_p()
    p, n = _picks(*pairs)
    hs = _handles(*[schemas[x].handle for x in names])
    assert L.fury_schema_zip(hs, len(names), p, n, ctypes.byref(h)) == OK
    try:
        return _info(L, h)
    finally:
        L.fury_schema_destroy(h)


def _direct(L, names, pairs):
    from fury_amd.encoder import Schema
    return _info(L, Schema([FIELDS[names[s]][k] for s, k in pairs]).handle)


def test_symbols_are_bound(L):
    from fury_amd import _native as N
    for name in ("fury_schema_zip", "fury_row_zip"):
        assert name in N.SIGNATURES
        assert hasattr(L, name)
    assert N.ZIP_MAX_SOURCES == 4
    assert ctypes.sizeof(N.FuryZipSource) == 24


@pytest.mark.parametrize("names,pairs", [
    (("foo", "struct100"), [(0, 4), (1, 37), (0, 0), (1, 99), (0, 2)]),
    (("foo", "struct100"), [(1, k) for k in range(99, -1, -1)] + [(0, k) for k in range(5)]),
    (("foo", "struct100"), [(1, 3), (1, 13)]),                   # source 0 unused, the result fixed
    (("deep", "foo"), [(1, 3), (0, 1), (0, 0), (1, 4)]),
    (("deep", "foo", "deep", "foo"), [(3, 1), (2, 0), (1, 1), (0, 0)]),      # equal names are kept
])
def test_zipped_schema_equals_a_direct_one(L, schemas, names, pairs):
    got = _zipped(L, schemas, names, pairs)
    assert got == _direct(L, names, pairs)
    n = len(pairs)
    assert got[:3] == (n, ((n + 63) // 64) * 8, ((n + 63) // 64) * 8 + 8 * n)


def test_one_source_equals_schema_select(L, schemas):
    for name, idx in (("foo", [4, 0]), ("struct100", list(range(3, 100, 10))), ("deep", [1, 0])):
        assert _zipped(L, schemas, (name,), [(0, k) for k in idx]) == _selected(L, schemas[name], idx)


def _pick_errors(call, fn, schemas):
    """The pick rules both functions share; call(schema handles, num_sources, picks, count) -> status."""
    foo, s100, arr = schemas["foo"].handle, schemas["struct100"].handle, schemas["array"].handle
    p, n = _picks((0, 4), (1, 7))
    assert call(None, 2, p, n) == INVALID
    assert "source table is null" in _err(fn)
    for count in (0, 5, -1):
        assert call((foo, s100, foo, s100, foo), count, p, n) == INVALID, count
        assert "num_sources" in _err(fn)
    assert call((foo, None), 2, p, n) == INVALID
    assert "schema of source 1 is null" in _err(fn)
    assert call((foo, s100), 2, None, n) == INVALID
    assert "picks is null" in _err(fn)
    for count in (0, -1):
        assert call((foo, s100), 2, p, count) == INVALID, count
        assert "num_picks" in _err(fn)
    for pairs in (((-1, 0),), ((2, 0),), ((0, 1), (2, 0))):
        p, n = _picks(*pairs)
        assert call((foo, s100), 2, p, n) == INVALID, pairs
        assert "names no source" in _err(fn)
    for pairs in (((0, 5),), ((0, -1),), ((1, 100),), ((1, 99), (0, 5))):
        p, n = _picks(*pairs)
        assert call((foo, s100), 2, p, n) == INVALID, pairs
        assert "is not a field of its source" in _err(fn)
    for pairs in (((0, 1), (0, 1)), ((1, 7), (0, 3), (1, 8), (1, 7))):
        p, n = _picks(*pairs)
        assert call((foo, s100), 2, p, n) == INVALID, pairs
        assert "picked twice" in _err(fn)
    p, n = _picks((0, 0))
    assert call((foo, arr), 2, p, n) == UNSUPPORTED              # even when no pick names it
    assert "collection schema" in _err(fn)
    assert call((arr,), 1, p, n) == UNSUPPORTED
    assert "collection schema" in _err(fn)


def test_schema_zip_argument_errors(L, schemas):
    fn = "fury_schema_zip"
    h = ctypes.c_void_p(1)

    def call(hs, ns, p, n):
        return L.fury_schema_zip(None if hs is None else _handles(*hs), ns, p, n, ctypes.byref(h))
    _pick_errors(call, fn, schemas)
    assert h.value is None                                   # *out is NULL after a failure
    p, n = _picks((0, 4))
    assert L.fury_schema_zip(_handles(schemas["foo"].handle), 1, p, n, None) == INVALID
    assert "out is null" in _err(fn)


def _sources(*triples):
    from fury_amd import _native as N
    a = (N.FuryZipSource * max(len(triples), 1))()
    for i, (schema, rows, offs) in enumerate(triples):
        a[i].schema, a[i].rows, a[i].row_offsets = schema, rows, offs
    return a


def test_zip_argument_errors(L, schemas):
    zp, fn = L.fury_row_zip, "fury_row_zip"
    foo, s100 = schemas["foo"].handle, schemas["struct100"].handle
    r1, rows = _buf()
    r2, out = _buf()
    r3, aux = _buf()          # offsets

    def call(hs, ns, p, n):
        srcs = None if hs is None else _sources(*[(h, rows, aux) for h in hs])
        return zp(srcs, ns, p, n, 4, out, 4096, aux, None)
    _pick_errors(call, fn, schemas)

    def two(a=(foo, rows, aux), b=(s100, rows, None)):
        return _sources(a, b)
    p, n = _picks((0, 4), (1, 7), (0, 0))     # foo.f5, struct100.f07, foo.f1: a variable-length pick
    assert zp(two(), 2, p, n, -1, out, 4096, aux, None) == INVALID
    assert "nrows < 0" in _err(fn)
    assert zp(two(), 2, p, n, 4, out, -8, aux, None) == INVALID
    assert "out_capacity < 0" in _err(fn)
    assert zp(two(), 2, p, n, 4, out + 4, 4096, aux, None) == INVALID
    assert "out_rows must be 8-byte aligned" in _err(fn)
    assert zp(two(), 2, p, n, 4, out, 4096, aux + 4, None) == INVALID
    assert "out_offsets must be 8-byte aligned" in _err(fn)
    assert zp(two(a=(foo, rows + 4, aux)), 2, p, n, 4, out, 4096, aux, None) == INVALID
    assert "source 0: rows must be 8-byte aligned" in _err(fn)
    assert zp(two(b=(s100, rows + 4, None)), 2, p, n, 4, out, 4096, aux, None) == INVALID
    assert "source 1: rows must be 8-byte aligned" in _err(fn)
    assert zp(two(a=(foo, rows, aux + 4)), 2, p, n, 4, out, 4096, aux, None) == INVALID
    assert "source 0: row_offsets must be 8-byte aligned" in _err(fn)
    assert zp(two(a=(foo, rows, None)), 2, p, n, 4, out, 4096, aux, None) == INVALID
    assert "source 0: variable-length rows need row_offsets" in _err(fn)
    assert zp(two(b=(s100, None, None)), 2, p, n, 4, out, 4096, aux, None) == INVALID
    assert "source 1: rows is null" in _err(fn)
    assert zp(two(), 2, p, n, 4, out, 4096, None, None) == INVALID
    assert "need out_offsets" in _err(fn)
    assert zp(two(), 2, p, n, 4, None, 0, None, None) == INVALID             # the measure form too
    assert "need out_offsets" in _err(fn)
    pf, nf = _picks((1, 7), (0, 0))           # fixed-width picks: 8 + 16 bytes a row
    assert zp(two(a=(foo, rows, None)), 2, pf, nf, 4, out, 4096, None, None) == INVALID
    assert "source 0: variable-length rows need row_offsets" in _err(fn)     # foo's rows still are
    assert zp(two(), 2, pf, nf, 4, out, 4 * 24 - 8, None, None) == CAPACITY
    assert "out_capacity 88 < 4 rows of 24 bytes" in _err(fn)
    assert zp(two(), 2, pf, nf, 4, out, 4 * 24 - 1, aux, None) == CAPACITY
    assert "rows of 24 bytes" in _err(fn)


def test_an_unused_source_may_be_null(L, schemas):
    """Source 0 is named by no pick: its NULL rows and row_offsets are accepted, and the call goes on
    to the next error."""
    zp, fn = L.fury_row_zip, "fury_row_zip"
    foo, s100 = schemas["foo"].handle, schemas["struct100"].handle
    r1, rows = _buf()
    r2, out = _buf()
    srcs = _sources((foo, None, None), (s100, rows, None))
    p, n = _picks((1, 7), (1, 3))
    assert zp(srcs, 2, p, n, 4, out, 4 * 24 - 8, None, None) == CAPACITY
    assert "out_capacity 88 < 4 rows of 24 bytes" in _err(fn)
    srcs = _sources((foo, None, None), (s100, rows + 4, None))
    assert zp(srcs, 2, p, n, 4, out, 4096, None, None) == INVALID
    assert "source 1: rows must be 8-byte aligned" in _err(fn)
    srcs = _sources((None, None, None), (s100, rows, None))      # but it needs a schema
    assert zp(srcs, 2, p, n, 4, out, 4096, None, None) == INVALID
    assert "schema of source 0 is null" in _err(fn)


# -- the Python surface, as far as it goes without a device ---------------------------------------------
def test_zipped_encoder():
    from fury_amd.encoder import (Encoders, IllegalArgumentException, RowEncoder,
                                  UnsupportedOperationException)
    foo, s100 = SCHEMAS["foo"], SCHEMAS["struct100"]
    a, b = Encoders.bean(foo, device="cpu"), Encoders.bean(s100, device="cpu")
    picks = [(0, "f5"), (1, "f07"), (0, 0)]
    z = a.zipped_encoder([b], picks)
    assert type(z) is RowEncoder and tuple(z.schema().fields) == (foo[4], s100[7], foo[0])
    assert z.schema_hash == Encoders.bean([foo[4], s100[7], foo[0]], device="cpu").schema_hash
    assert str(z.device) == "cpu"
    assert a.zipped_encoder([b], [(0, 4), (1, 7), (0, "f1")]) is z          # cached per picks
    assert a.zipped_encoder([b], picks[::-1]) is not z
    r = a.zipped_encoder([b], picks, names=["x", "y", "z"])
    assert [f.name for f in r.schema().fields] == ["x", "y", "z"] and r is not z
    assert r.schema().fixed_size == z.schema().fixed_size
    assert [(f.type_id, f.children) for f in r.schema().fields] == \
        [(f.type_id, f.children) for f in z.schema().fields]
    assert a.zipped_encoder([], [(0, "f5"), (0, "f1")]).schema_hash == \
        a.selected_encoder(["f5", "f1"]).schema_hash
    many = [(1, k) for k in range(100)] + [(0, k) for k in range(5)]
    assert a.zipped_encoder([b], many).schema().num_fields == 105           # no 64-field cap
    with pytest.raises(IllegalArgumentException, match="no field named 'nope'"):
        a.zipped_encoder([b], [(1, "nope")])
    with pytest.raises(IllegalArgumentException, match="names source 2"):
        a.zipped_encoder([b], [(2, "f1")])
    with pytest.raises(IllegalArgumentException, match="names no source"):
        a.zipped_encoder([b], [(2, 0)])
    with pytest.raises(IllegalArgumentException, match="picked twice"):
        a.zipped_encoder([b], [(0, "f1"), (0, 0)])
    with pytest.raises(IllegalArgumentException, match="is not a field of its source"):
        a.zipped_encoder([b], [(0, 5)])
    with pytest.raises(IllegalArgumentException, match="num_picks"):
        a.zipped_encoder([b], [])
    with pytest.raises(IllegalArgumentException, match="num_sources"):
        a.zipped_encoder([b, b, b, b], picks)
    with pytest.raises(IllegalArgumentException, match="2 names for 3 picks"):
        a.zipped_encoder([b], picks, names=["x", "y"])
    arr = Encoders.array_encoder(T.field("item", T.INT64), device="cpu")
    with pytest.raises(UnsupportedOperationException, match="collection schema"):
        a.zipped_encoder([arr], [(0, 0), (1, 0)])


def test_with_fields_picks():
    """Replace or append, purely on the picks: every field of self in order, a field of the other
    encoder of the same name in its place, the other's remaining fields appended."""
    from fury_amd.encoder import Encoders
    mixed = Encoders.bean(SCHEMAS["mixed"], device="cpu")
    names = [f.name for f in SCHEMAS["mixed"]]
    k = names.index("s2")
    other = Encoders.bean([T.field("extra", T.INT64), T.field("s2", T.BINARY),
                           T.field("more", T.STRING)], device="cpu")
    picks = mixed._with_fields_picks(other)
    assert picks == [(0, i) if i != k else (1, 1) for i in range(len(names))] + [(1, 0), (1, 2)]
    z = mixed.zipped_encoder([other], picks)
    assert [f.name for f in z.schema().fields] == names + ["extra", "more"]
    assert z.schema().fields[k].type_id == T.BINARY              # replaced whatever its type


def test_python_surface_checks_hashes_and_row_counts():
    from fury_amd.encoder import (ClassNotCompatibleException, Encoders, IllegalArgumentException,
                                  RowBatch)
    a = Encoders.bean(SCHEMAS["foo"], device="cpu")
    b = Encoders.bean(SCHEMAS["struct100"], device="cpu")
    mine, theirs = RowBatch(None, None, 3, a.schema_hash), RowBatch(None, None, 3, b.schema_hash)
    picks = [(0, "f5"), (1, "f07")]
    calls = (lambda x, y: a.zip_fields(x, [(b, y)], picks),
             lambda x, y: a.zip_fields_into(x, [(b, y)], picks, None, None),
             lambda x, y: a.bind_zip_fields(x, [(b, y)], picks, None, None))
    for call in calls:
        with pytest.raises(ClassNotCompatibleException, match="Schema is not consistent"):
            call(RowBatch(None, None, 3, a.schema_hash + 1), theirs)
        with pytest.raises(ClassNotCompatibleException, match="Schema is not consistent"):
            call(mine, RowBatch(None, None, 3, b.schema_hash + 1))
    for call in calls:
        with pytest.raises(IllegalArgumentException, match="source 1 has 4 rows, source 0 has 3"):
            call(mine, RowBatch(None, None, 4, b.schema_hash))
    with pytest.raises(ClassNotCompatibleException):
        a.with_fields(mine, b, RowBatch(None, None, 3, b.schema_hash + 1))
