"""CPU checks of the element explosion's C ABI (fury_schema_element / fury_row_explode): the element
schema equals a schema built directly from the element's fields, and every argument error is reported
on the host, before any device work, with its status and a message that names the function.  Host
buffers stand in for device memory and are never dereferenced: every fury_row_explode call here fails
first."""
from __future__ import annotations

import ctypes

import pytest

from fury_amd import types as T
from fury_amd.workloads import SCHEMAS
from tests.test_extract_abi import _buf, _err, _info, _path, deep_fields

OK, INVALID, UNSUPPORTED = 0, 1, 2


def explode_fields():
    """id INT64, items LIST<STRUCT{a INT32, s STRING}>, m MAP<INT32, STRUCT{x INT64, y STRING}>,
    ll LIST<LIST<INT32>>, fx LIST<STRUCT{p INT64, q INT32}> -- the schema of tests/test_explode.py."""
    item = T.struct_field("item", [T.field("a", T.INT32), T.field("s", T.STRING)])
    val = T.struct_field("value", [T.field("x", T.INT64), T.field("y", T.STRING)])
    fxi = T.struct_field("item", [T.field("p", T.INT64), T.field("q", T.INT32)])
    return [T.field("id", T.INT64), T.Field("items", T.LIST, True, (item,)),
            T.map_field("m", T.field("key", T.INT32), val),
            T.Field("ll", T.LIST, True, (T.array_field("item", T.INT32),)),
            T.Field("fx", T.LIST, True, (fxi,))]


def lls_fields():
    """The schema of the reference fixture list_list_struct: ll LIST<LIST<STRUCT{a INT32, s STRING}>>."""
    st = T.struct_field("item", [T.field("a", T.INT32), T.field("s", T.STRING)])
    return [T.Field("ll", T.LIST, True, (T.Field("item", T.LIST, True, (st,)),))]


@pytest.fixture(scope="module")
def L():
    from fury_amd import _native as N
    return N.lib()


@pytest.fixture(scope="module")
def schemas():
    from fury_amd.encoder import Schema
    ex = explode_fields()
    return {"beana": Schema(SCHEMAS["beana"]), "ex": Schema(ex), "lls": Schema(lls_fields()),
            "foo": Schema(SCHEMAS["foo"]), "deep": Schema(deep_fields()),
            "c_items": Schema([ex[1]], collection=True), "c_m": Schema([ex[2]], collection=True),
            "c_ints": Schema([T.array_field("v", T.INT64)], collection=True)}


def _element(L, schema, idx, side):
    h = ctypes.c_void_p()
    p, n = _path(*idx)
    assert L.fury_schema_element(schema.handle, p, n, side, ctypes.byref(h)) == OK
    try:
        return _info(L, h)
    finally:
        L.fury_schema_destroy(h)


def _direct(L, node):
    from fury_amd.encoder import Schema
    s = Schema(node.children) if node.type_id == T.STRUCT else Schema([node], collection=True)
    return _info(L, s.handle)


def _slot(fields, name):
    return [f.name for f in fields].index(name)


def test_symbols_are_bound(L):
    from fury_amd import _native as N
    for name in ("fury_schema_element", "fury_row_explode"):
        assert name in N.SIGNATURES
        assert hasattr(L, name)


def test_element_schema_of_beana(L, schemas):
    from fury_amd.encoder import Schema
    fields = SCHEMAS["beana"]
    k = _slot(fields, "bean_b_list")
    got = _element(L, schemas["beana"], (k,), 0)
    assert got == _direct(L, fields[k].children[0])
    assert got[4] == Schema(SCHEMAS["beanb"]).schema_hash and got[0] == len(SCHEMAS["beanb"])
    k = _slot(fields, "int2_d_array")
    got = _element(L, schemas["beana"], (k,), 0)
    assert got == _direct(L, fields[k].children[0]) and got[:5] == (1, 0, 0, 0, 0)   # a collection
    k = _slot(fields, "string_bean_b_map")
    got = _element(L, schemas["beana"], (k,), 1)
    assert got == _direct(L, fields[k].children[1])
    assert got[4] == Schema(SCHEMAS["beanb"]).schema_hash


def test_element_schema_of_nested_lists_and_collections(L, schemas):
    lls = lls_fields()
    inner = lls[0].children[0]                                 # LIST<STRUCT>
    assert _element(L, schemas["lls"], (0,), 0) == _direct(L, inner)
    from fury_amd.encoder import Schema
    again = Schema([inner], collection=True)                   # the collection batch explode returns
    got = _element(L, again, (), 0)
    assert got == _direct(L, inner.children[0]) and got[:4] == (2, 8, 24, 0)
    ex = explode_fields()
    assert _element(L, schemas["c_items"], (), 0) == _direct(L, ex[1].children[0])
    assert _element(L, schemas["c_m"], (), 1) == _direct(L, ex[2].children[1])
    fx = _element(L, schemas["ex"], (4,), 0)
    assert fx[:4] == (2, 8, 24, 1)                             # fx's elements are fixed-width
    assert _element(L, schemas["ex"], (3,), 0) == _direct(L, ex[3].children[0])
    h = ctypes.c_void_p()
    assert L.fury_schema_element(schemas["c_items"].handle, None, 0, 0, ctypes.byref(h)) == OK
    L.fury_schema_destroy(h)                                   # path may be NULL with path_len 0


def _selection_errors(call, fn, schemas):
    """The rules both functions share; call(schema handle, path, path_len, side) -> status."""
    ex, foo, deep = schemas["ex"].handle, schemas["foo"].handle, schemas["deep"].handle
    p, n = _path(1)
    assert call(None, p, n, 0) == INVALID
    assert "schema is null" in _err(fn)
    assert call(ex, None, 1, 0) == INVALID
    assert "path is null" in _err(fn)
    for bad_len in (0, -1, 65):                                # a row schema needs a path
        assert call(ex, p, bad_len, 0) == INVALID
        assert "path_len" in _err(fn)
    p, n = _path(9)
    assert call(ex, p, n, 0) == INVALID
    assert "is not a slot" in _err(fn)
    for sch, idx in ((foo, (4,)), (deep, (1,)), (deep, (1, 1))):   # a path ending at a STRUCT
        p, n = _path(*idx)
        assert call(sch, p, n, 0) == UNSUPPORTED, idx
        assert "fury_row_extract" in _err(fn)
    for sch, idx in ((foo, (0,)), (foo, (1,)), (ex, (0,)), (deep, (1, 0))):   # ... at a scalar
        p, n = _path(*idx)
        assert call(sch, p, n, 0) == UNSUPPORTED, idx
        assert "fury_row_project" in _err(fn)
    p, n = _path(1, 0)                                         # through a LIST
    assert call(ex, p, n, 0) == UNSUPPORTED
    assert "only struct slots" in _err(fn)
    # scalar and STRING elements: foo.f3 LIST<STRING>, foo.f4 MAP<STRING, INT32> both sides,
    # deep.outer.inner.v LIST<INT64>, ex.m keys INT32, a collection of INT64
    for sch, idx, side in ((foo, (2,), 0), (foo, (3,), 0), (foo, (3,), 1), (deep, (1, 1, 1), 0),
                           (ex, (2,), 0)):
        p, n = _path(*idx)
        assert call(sch, p, n, side) == UNSUPPORTED, (idx, side)
        msg = _err(fn)
        assert "fury_decode_prepare" in msg and "fury_row_project" in msg
    assert call(schemas["c_ints"].handle, None, 0, 0) == UNSUPPORTED
    assert "fury_decode_prepare" in _err(fn)
    p, n = _path(1)
    assert call(ex, p, n, 1) == INVALID                        # side 1 on a LIST
    assert "side 1" in _err(fn)
    assert call(schemas["c_items"].handle, None, 0, 1) == INVALID
    assert "side 1" in _err(fn)
    for side in (2, -1):
        p, n = _path(2)
        assert call(ex, p, n, side) == INVALID
        assert "side" in _err(fn)
    p, n = _path(0)
    for sch in ("c_items", "c_m"):                             # a collection schema takes no path
        assert call(schemas[sch].handle, p, 1, 0) == INVALID
        msg = _err(fn)
        assert "collection schema" in msg and "path_len" in msg


def test_schema_element_argument_errors(L, schemas):
    fn = "fury_schema_element"
    h = ctypes.c_void_p(1)
    _selection_errors(lambda s, p, n, side: L.fury_schema_element(s, p, n, side, ctypes.byref(h)),
                      fn, schemas)
    assert h.value is None                                     # *out is NULL after a failure
    p, n = _path(1)
    assert L.fury_schema_element(schemas["ex"].handle, p, n, 0, None) == INVALID
    assert "out is null" in _err(fn)


def test_explode_argument_errors(L, schemas):
    exp, fn = L.fury_row_explode, "fury_row_explode"
    ex = schemas["ex"].handle
    r1, rows = _buf()
    r2, out = _buf()
    r3, aux = _buf()          # offsets / counts / parents / ordinals / validity
    _selection_errors(lambda s, p, n, side: exp(s, p, n, side, rows, aux, 4, aux, None, 64, out, 4096,
                                                aux, aux, None, None, None, None), fn, schemas)
    p, n = _path(1)

    def call(rows=rows, offs=aux, nrows=4, lo=aux, ev=None, ecap=64, out=out, cap=4096, oo=aux,
             cnt=aux, par=None, ords=None, val=None):
        return exp(ex, p, n, 0, rows, offs, nrows, lo, ev, ecap, out, cap, oo, cnt, par, ords, val,
                   None)
    checks = [
        (dict(nrows=-1), "nrows < 0"),
        (dict(cap=-8), "out_capacity < 0"),
        (dict(ecap=-1), "elem_capacity < 0"),
        (dict(rows=rows + 4), "rows must be 8-byte aligned"),
        (dict(out=out + 4), "out_rows must be 8-byte aligned"),
        (dict(offs=None), "row_offsets is null"),
        (dict(lo=None), "out_list_offsets is null"),
        (dict(lo=None, oo=None, cnt=None, out=None), "out_list_offsets is null"),     # the count form too
        (dict(cnt=None), "out_count is null"),
        (dict(cnt=None, nrows=0), "out_count is null"),                                 # even when empty
        (dict(offs=aux + 4), "8-byte aligned"),
        (dict(lo=aux + 4), "8-byte aligned"),
        (dict(oo=aux + 4), "8-byte aligned"),
        (dict(cnt=aux + 4), "8-byte aligned"),
        (dict(par=aux + 4), "8-byte aligned"),
        (dict(ords=aux + 2), "4-byte aligned"),
        (dict(val=aux + 2), "4-byte aligned"),
        (dict(ev=aux + 2), "out_entry_validity must be 4-byte aligned"),
        (dict(rows=None), "rows is null"),
        (dict(rows=None, out=None, cap=0), "rows is null"),       # the measure form reads rows too
        (dict(rows=None, out=None, oo=None, cnt=None), "rows is null"),   # and so does the count form
    ]
    for kw, text in checks:
        assert call(**kw) == INVALID, kw
        assert text in _err(fn), kw
    # the count form takes no per-element output
    for kw in (dict(out=out), dict(cnt=aux), dict(par=aux), dict(ords=aux), dict(val=aux)):
        full = dict(oo=None, out=None, cnt=None)
        full.update(kw)
        assert call(**full) == INVALID, kw
        assert "count form" in _err(fn), kw


def test_element_encoder():
    from fury_amd.encoder import (ArrayEncoder, Encoders, IllegalArgumentException, MapEncoder,
                                  RowEncoder, UnsupportedOperationException)
    ex = explode_fields()
    enc = Encoders.bean(ex, device="cpu")
    items = enc.element_encoder("items")
    assert type(items) is RowEncoder and tuple(items.schema().fields) == ex[1].children[0].children
    assert enc.element_encoder(["items"], "elements") is items and enc.element_encoder(1) is items
    assert str(items.device) == "cpu"
    vals = enc.element_encoder("m", "values")
    assert type(vals) is RowEncoder and [f.name for f in vals.schema().fields] == ["x", "y"]
    assert vals is not items and enc.element_encoder("m", side="values") is vals
    ll = enc.element_encoder("ll")
    assert type(ll) is ArrayEncoder and ll.field() == ex[3].children[0] and ll.schema_hash == 0
    assert enc.element_encoder("fx").schema().is_fixed
    with pytest.raises(UnsupportedOperationException, match="fury_decode_prepare"):
        enc.element_encoder("m", "keys")
    with pytest.raises(UnsupportedOperationException, match="fury_row_project"):
        enc.element_encoder("id")
    with pytest.raises(IllegalArgumentException, match="side 1"):
        enc.element_encoder("items", "values")
    with pytest.raises(IllegalArgumentException, match="is not one of"):
        enc.element_encoder("items", "both")
    with pytest.raises(IllegalArgumentException, match="no field named 'nope'"):
        enc.element_encoder("nope")
    # collection encoders: the same methods with the empty path
    arr = ArrayEncoder(ex[1], "cpu")
    e = arr.element_encoder()
    assert type(e) is RowEncoder and e.schema_hash == items.schema_hash and arr.element_encoder() is e
    mp = MapEncoder(ex[2], "cpu")
    assert mp.element_encoder("values").schema_hash == vals.schema_hash
    with pytest.raises(UnsupportedOperationException, match="fury_decode_prepare"):
        mp.element_encoder("keys")
    lle = ArrayEncoder(ex[3], "cpu").element_encoder()
    assert type(lle) is ArrayEncoder and lle.field() == ex[3].children[0]
    mm = T.map_field("mm", T.field("key", T.STRING), ex[2].children[1])
    outer = ArrayEncoder(T.Field("v", T.LIST, True, (T.Field("item", T.MAP, True, mm.children),)), "cpu")
    assert type(outer.element_encoder()) is MapEncoder


def test_python_surface_checks_the_schema_hash():
    from fury_amd.encoder import ClassNotCompatibleException, Encoders, RowBatch
    enc = Encoders.bean(explode_fields(), device="cpu")
    foreign = RowBatch(None, None, 0, enc.schema_hash + 1)
    for call in (lambda: enc.explode(foreign, "items"),
                 lambda: enc.explode_into(foreign, "items", None),
                 lambda: enc.bind_explode(foreign, "items", None)):
        with pytest.raises(ClassNotCompatibleException, match="Schema is not consistent"):
            call()
