"""CPU checks of the C ABI of fury_schema_map_side / fury_row_map_split / fury_row_map_join and of their
Python surface: the symbols are bound, the side schema equals a collection schema built directly from
the key / value field, and every path, target and argument error is reported on the host, before any
device work, with its status and a message that names the function.  Host buffers stand in for device
memory and are never dereferenced: every split / join call here fails first."""
from __future__ import annotations

import ctypes

import pytest

from fury_amd import types as T
from fury_amd.workloads import SCHEMAS
from tests.test_explode_abi import explode_fields
from tests.test_extract_abi import _buf, _err, _info, _path, deep_fields

OK, INVALID, UNSUPPORTED = 0, 1, 2


def nested_fields():
    return [T.field("id", T.INT64), T.struct_field("outer", explode_fields())]


@pytest.fixture(scope="module")
def L():
    from fury_amd import _native as N
    return N.lib()


@pytest.fixture(scope="module")
def schemas():
    from fury_amd.encoder import Encoders, Schema
    ex = explode_fields()
    arr = Encoders.array_encoder(T.field("item", T.INT64), device="cpu")
    return {"ex": Schema(ex), "nested": Schema(nested_fields()), "foo": Schema(SCHEMAS["foo"]),
            "deep": Schema(deep_fields()), "array": arr.schema(), "_keep": arr,
            "beana": Schema(SCHEMAS["beana"]),
            "m": Schema([ex[2]]), "items": Schema([ex[1]]), "id": Schema([ex[0]]),
            "c_m": Schema([ex[2]], collection=True), "c_items": Schema([ex[1]], collection=True)}


def _side(L, schema, idx, side):
    h = ctypes.c_void_p()
    p, n = _path(*idx)
    assert L.fury_schema_map_side(schema.handle, p, n, side, ctypes.byref(h)) == OK
    try:
        return _info(L, h)
    finally:
        L.fury_schema_destroy(h)


def _direct(L, m, side):
    """fury_collection_schema_create of a LIST field whose element is the map's key / value field."""
    from fury_amd.encoder import Schema
    s = Schema([T.Field(m.name, T.LIST, m.nullable, (m.children[side],))], collection=True)
    return _info(L, s.handle)


def test_symbols_are_bound(L):
    from fury_amd import _native as N
    for name, nargs in (("fury_schema_map_side", 5), ("fury_row_map_split", 16),
                        ("fury_row_map_join", 12)):
        assert name in N.SIGNATURES and len(N.SIGNATURES[name][1]) == nargs
        assert hasattr(L, name)
    assert L.fury_abi_version() == 1


def test_side_schema_equals_the_collection_schema_of_the_same_field(L, schemas):
    ex = explode_fields()
    for side in (0, 1):
        want = _direct(L, ex[2], side)
        assert want[4] == 0 and want[0] == 1                   # a collection: one field, hash 0
        assert _side(L, schemas["ex"], (2,), side) == want
        assert _side(L, schemas["nested"], (1, 2), side) == want
        assert _side(L, schemas["c_m"], (), side) == want
        assert _side(L, schemas["m"], (0,), side) == want
    assert _side(L, schemas["ex"], (2,), 0) != _side(L, schemas["ex"], (2,), 1)
    beana = SCHEMAS["beana"]
    k = [f.name for f in beana].index("string_bean_b_map")
    for side in (0, 1):                                        # STRING keys, STRUCT values
        assert _side(L, schemas["beana"], (k,), side) == _direct(L, beana[k], side)
    h = ctypes.c_void_p()
    assert L.fury_schema_map_side(schemas["c_m"].handle, None, 0, 1, ctypes.byref(h)) == OK
    L.fury_schema_destroy(h)                                   # path may be NULL with path_len 0


def _map_path_errors(call, fn, schemas):
    """The rules fury_schema_map_side and fury_row_map_split share; call(handle, path, path_len)."""
    foo, deep = schemas["foo"].handle, schemas["deep"].handle
    p, n = _path(4)
    assert call(None, p, n) == INVALID
    assert "schema is null" in _err(fn)
    assert call(foo, None, 1) == INVALID
    assert "path is null" in _err(fn)
    for bad_len in (0, -1, 65):
        assert call(foo, p, bad_len) == INVALID
        assert "path_len" in _err(fn)
    for idx in ((5,), (-1,), (1, 4), (1, -1), (1, 1, 2)):
        p, n = _path(*idx)
        assert call(deep if len(idx) > 1 else foo, p, n) == INVALID, idx
        assert "is not a slot" in _err(fn)
    for idx in ((0,), (1,)):                                   # foo.f1 INT32, foo.f2 STRING
        p, n = _path(*idx)
        assert call(foo, p, n) == UNSUPPORTED
        assert "fury_row_project" in _err(fn)
    for sch, idx in ((foo, (2, 0)), (foo, (3, 0)), (deep, (1, 3, 0))):     # through a LIST, a MAP
        p, n = _path(*idx)
        assert call(sch, p, n) == UNSUPPORTED, idx
        assert "is not a STRUCT: only struct slots" in _err(fn)
    ex = schemas["ex"].handle
    for idx, what in (((1,), "LIST"), ((3,), "LIST")):         # a path that ends at a non-MAP
        p, n = _path(*idx)
        assert call(ex, p, n) == UNSUPPORTED, idx
        assert "is not a MAP" in _err(fn) and what in _err(fn)
    p, n = _path(1)
    assert call(schemas["nested"].handle, p, n) == UNSUPPORTED     # ... at a STRUCT
    assert "is not a MAP" in _err(fn) and "STRUCT" in _err(fn)
    p, n = _path(0)
    assert call(ex, p, n) == UNSUPPORTED                       # ... at a scalar: extract's own rule
    assert call(schemas["c_items"].handle, None, 0) == UNSUPPORTED
    assert "is not a MAP" in _err(fn)
    p, n = _path(0)
    assert call(schemas["c_m"].handle, p, n) == INVALID
    assert "path_len must be 0" in _err(fn)


def test_map_side_errors(L, schemas):
    fn = "fury_schema_map_side"
    h = ctypes.c_void_p()
    _map_path_errors(lambda s, p, n: L.fury_schema_map_side(s, p, n, 0, ctypes.byref(h)), fn, schemas)
    p, n = _path(2)
    for side in (2, -1, 7):
        assert L.fury_schema_map_side(schemas["ex"].handle, p, n, side, ctypes.byref(h)) == INVALID
        assert "side" in _err(fn) and h.value is None
    assert L.fury_schema_map_side(schemas["ex"].handle, p, n, 0, None) == INVALID
    assert "out is null" in _err(fn)


def test_split_argument_errors(L, schemas):
    sp, fn = L.fury_row_map_split, "fury_row_map_split"
    r1, rows = _buf()
    r2, ko = _buf()
    r3, vo = _buf()
    r4, aux = _buf()
    _map_path_errors(lambda s, p, n: sp(s, p, n, rows, aux, 4, ko, 4096, aux, vo, 4096, aux, aux, None,
                                        None, None), fn, schemas)
    for name, idx in (("ex", (2,)), ("nested", (1, 2)), ("c_m", ())):
        s = schemas[name].handle
        p, n = _path(*idx)

        def call(rows=rows, offs=aux, nrows=4, k=ko, kc=4096, koff=aux, v=vo, vc=4096, voff=aux,
                 cnt=aux, idx_=None, val=None):
            return sp(s, p, n, rows, offs, nrows, k, kc, koff, v, vc, voff, cnt, idx_, val, None)
        assert call(nrows=-1) == INVALID
        assert "nrows < 0" in _err(fn)
        assert call(kc=-8) == INVALID
        assert "key_capacity < 0" in _err(fn)
        assert call(vc=-8) == INVALID
        assert "value_capacity < 0" in _err(fn)
        assert call(rows=rows + 4) == INVALID
        assert "rows must be 8-byte aligned" in _err(fn)
        assert call(k=ko + 4) == INVALID
        assert "out_keys / out_values must be 8-byte aligned" in _err(fn)
        assert call(v=vo + 4) == INVALID
        assert "out_keys / out_values must be 8-byte aligned" in _err(fn)
        assert call(offs=None) == INVALID
        assert "row_offsets is null" in _err(fn)
        assert call(k=None, koff=None, v=None, voff=None) == INVALID     # both sides NULL
        assert "both null" in _err(fn)
        assert call(koff=None) == INVALID                      # a skipped side has no buffer either
        assert "without its offsets" in _err(fn)
        assert call(voff=None) == INVALID
        assert "without its offsets" in _err(fn)
        assert call(cnt=None) == INVALID
        assert "out_count is null" in _err(fn)
        for kw in (dict(offs=aux + 4), dict(koff=aux + 4), dict(voff=aux + 4), dict(cnt=aux + 4),
                   dict(idx_=aux + 4)):
            assert call(**kw) == INVALID, kw
            assert "must be 8-byte aligned" in _err(fn)
        assert call(val=aux + 2) == INVALID
        assert "out_validity must be 4-byte aligned" in _err(fn)
        assert call(rows=None) == INVALID
        assert "rows is null" in _err(fn)


def test_join_targets_and_argument_errors(L, schemas):
    jn, fn = L.fury_row_map_join, "fury_row_map_join"
    r1, keys = _buf()
    r2, vals = _buf()
    r3, out = _buf()
    r4, aux = _buf()

    def target(schema, validity=None):
        h = None if schema is None else schemas[schema].handle
        return jn(h, keys, aux, vals, aux, 4, validity, 4, out, 4096, aux, None)
    assert target(None) == INVALID
    assert "schema is null" in _err(fn)
    assert target("ex") == UNSUPPORTED                         # a multi-field target
    assert "5 fields" in _err(fn) and "fury_row_zip" in _err(fn)
    for name in ("items", "id", "c_items", "array"):           # a non-MAP target
        assert target(name) == UNSUPPORTED, name
        assert "is not a MAP" in _err(fn)
    assert target("c_m", validity=aux) == INVALID              # validity in collection form
    assert "validity with a collection schema" in _err(fn)
    assert target("m", validity=aux + 2) == INVALID            # a row schema takes one
    assert "validity must be 4-byte aligned" in _err(fn)
    for name in ("m", "c_m"):
        s = schemas[name].handle

        def call(k=keys, koff=aux, v=vals, voff=aux, nv=4, nrows=4, o=out, cap=4096, ooff=aux):
            return jn(s, k, koff, v, voff, nv, None, nrows, o, cap, ooff, None)
        assert call(nrows=-1) == INVALID
        assert "nrows < 0" in _err(fn)
        assert call(nv=-1) == INVALID
        assert "num_values < 0" in _err(fn)
        assert call(cap=-8) == INVALID
        assert "out_capacity < 0" in _err(fn)
        assert call(k=keys + 4) == INVALID
        assert "keys / values must be 8-byte aligned" in _err(fn)
        assert call(v=vals + 4) == INVALID
        assert "keys / values must be 8-byte aligned" in _err(fn)
        assert call(o=out + 4) == INVALID
        assert "out_rows must be 8-byte aligned" in _err(fn)
        assert call(koff=None) == INVALID
        assert "key_offsets is null" in _err(fn)
        assert call(voff=None) == INVALID
        assert "value_offsets is null" in _err(fn)
        assert call(ooff=None) == INVALID
        assert "out_offsets is null" in _err(fn)
        assert call(o=None, cap=0, ooff=None) == INVALID       # the measure form too
        assert "out_offsets is null" in _err(fn)
        for kw in (dict(koff=aux + 4), dict(voff=aux + 4), dict(ooff=aux + 4)):
            assert call(**kw) == INVALID, kw
            assert "must be 8-byte aligned" in _err(fn)
        assert call(k=None) == INVALID
        assert "keys is null" in _err(fn)
        assert call(v=None) == INVALID
        assert "values is null" in _err(fn)


# -- the Python surface, as far as it goes without a device ---------------------------------------------
def test_array_encoders_of_a_map():
    from fury_amd.encoder import (ArrayEncoder, Encoders, IllegalArgumentException,
                                  UnsupportedOperationException)
    ex = explode_fields()
    enc = Encoders.bean(ex, device="cpu")
    k, v = enc.key_array_encoder("m"), enc.value_array_encoder("m")
    assert type(k) is ArrayEncoder and type(v) is ArrayEncoder
    assert k.field().children[0] == ex[2].children[0] and v.field().children[0] == ex[2].children[1]
    assert k.schema_hash == 0 and enc.key_array_encoder(2) is k            # cached
    nested = Encoders.bean(nested_fields(), device="cpu")
    assert nested.value_array_encoder(["outer", "m"]).field() == v.field()
    me = Encoders.map_encoder(*ex[2].children, device="cpu", name="m")
    assert me.key_array_encoder().field() == k.field()
    assert me.value_array_encoder().field() == v.field()
    assert v.element_encoder().schema_hash == enc.element_encoder("m", "values").schema_hash
    with pytest.raises(UnsupportedOperationException, match="is not a MAP"):
        enc.key_array_encoder("items")
    with pytest.raises(IllegalArgumentException, match="no field named"):
        enc.value_array_encoder("nope")


def test_python_surface_checks_its_batches():
    from fury_amd.encoder import (ClassNotCompatibleException, Encoders, IllegalArgumentException,
                                  RowBatch)
    enc = Encoders.bean(explode_fields(), device="cpu")
    bad = RowBatch(None, None, 3, enc.schema_hash + 1)
    for call in (lambda: enc.split_map(bad, "m"),
                 lambda: enc.split_map_into(bad, "m", None, None, None, None, None),
                 lambda: enc.bind_split_map(bad, "m", None, None, None, None, None)):
        with pytest.raises(ClassNotCompatibleException, match="Schema is not consistent"):
            call()
    one = enc.field_encoder("m")
    arr, rows = RowBatch(None, None, 3, 0), RowBatch(None, None, 3, enc.schema_hash)
    for call in (lambda: one.join_map(rows, arr), lambda: one.join_map_into(arr, rows, None, None),
                 lambda: one.bind_join_map(rows, arr, None, None),
                 lambda: enc.with_map(rows, "m", arr, rows)):
        with pytest.raises(ClassNotCompatibleException, match="array batches"):
            call()
    with pytest.raises(IllegalArgumentException, match="3 key arrays and 4 value arrays"):
        one.join_map(arr, RowBatch(None, None, 4, 0))
