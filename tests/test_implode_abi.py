"""CPU checks of the C ABI of fury_row_implode / fury_row_wrap and of their Python surface: the
symbols are bound, and every target and argument error is reported on the host, before any device
work, with its status and a message that names the function.  Host buffers stand in for device memory
and are never dereferenced: every call here fails first."""
from __future__ import annotations

import pytest

from fury_amd import types as T
from fury_amd.workloads import SCHEMAS
from tests.test_explode_abi import explode_fields
from tests.test_select_abi import INVALID, UNSUPPORTED, _buf, _err


@pytest.fixture(scope="module")
def L():
    from fury_amd import _native as N
    return N.lib()


def _one(fields, name):
    return [f for f in fields if f.name == name]


@pytest.fixture(scope="module")
def schemas():
    from fury_amd.encoder import Encoders, Schema
    fx = explode_fields()
    item = _one(fx, "items")[0].children[0]
    keep = {"items_arr": Encoders.array_encoder(item, device="cpu", name="items"),
            "ints_arr": Encoders.array_encoder(T.field("item", T.INT64), device="cpu"),
            "map_enc": Encoders.map_encoder(*_one(fx, "m")[0].children, device="cpu")}
    out = {name: Schema(_one(fx, name)) for name in ("id", "items", "m", "ll", "fx")}
    out.update(all=Schema(fx), f3=Schema(_one(SCHEMAS["foo"], "f3")), f5=Schema(_one(SCHEMAS["foo"], "f5")),
               strs=Schema([T.field("s", T.STRING)]),
               decs=Schema([T.Field("d", T.LIST, True, (T.field("item", T.DECIMAL),))]),
               _keep=keep)
    out.update({k: v.schema() for k, v in keep.items()})
    return out


def test_symbols_are_bound(L):
    from fury_amd import _native as N
    for name, nargs in (("fury_row_implode", 13), ("fury_row_wrap", 10)):
        assert name in N.SIGNATURES and len(N.SIGNATURES[name][1]) == nargs
        assert hasattr(L, name)
    assert L.fury_abi_version() == 1


def test_implode_targets(L, schemas):
    fn = "fury_row_implode"
    r1, vals = _buf()
    r2, out = _buf()
    r3, aux = _buf()

    def call(schema, ev=None):
        h = None if schema is None else schemas[schema].handle
        return L.fury_row_implode(h, vals, aux, 4, aux, 4, ev, None, 4, out, 4096, aux, None)
    assert call(None) == INVALID
    assert "schema is null" in _err(fn)
    assert call("all") == UNSUPPORTED
    assert "5 fields" in _err(fn) and "fury_row_zip" in _err(fn)
    for name in ("m", "map_enc"):
        assert call(name) == UNSUPPORTED, name
        assert "is a MAP" in _err(fn)
    for name in ("id", "f5", "strs"):
        assert call(name) == UNSUPPORTED, name
        assert "is not a LIST" in _err(fn)
    for name in ("f3", "decs", "ints_arr"):                    # STRING, DECIMAL and INT64 elements
        assert call(name) == UNSUPPORTED, name
        assert "are not STRUCT, LIST or MAP" in _err(fn)
    assert call("items_arr", ev=aux) == INVALID
    assert "entry_validity with a collection schema" in _err(fn)
    assert call("items", ev=aux + 2) == INVALID                # a row schema takes one
    assert "4-byte aligned" in _err(fn)


def test_implode_argument_errors(L, schemas):
    im, fn = L.fury_row_implode, "fury_row_implode"
    r1, vals = _buf()
    r2, out = _buf()
    r3, aux = _buf()
    for name in ("items", "ll", "fx", "items_arr"):
        s = schemas[name].handle
        assert im(s, vals, aux, 4, aux, -1, None, None, 4, out, 4096, aux, None) == INVALID
        assert "nrows < 0" in _err(fn)
        assert im(s, vals, aux, -1, aux, 4, None, None, 4, out, 4096, aux, None) == INVALID
        assert "num_values < 0" in _err(fn)
        assert im(s, vals, aux, 4, aux, 4, None, None, -1, out, 4096, aux, None) == INVALID
        assert "num_elements < 0" in _err(fn)
        assert im(s, vals, aux, 4, aux, 4, None, None, 4, out, -8, aux, None) == INVALID
        assert "out_capacity < 0" in _err(fn)
        assert im(s, vals + 4, aux, 4, aux, 4, None, None, 4, out, 4096, aux, None) == INVALID
        assert "values must be 8-byte aligned" in _err(fn)
        assert im(s, vals, aux, 4, aux, 4, None, None, 4, out + 4, 4096, aux, None) == INVALID
        assert "out_rows must be 8-byte aligned" in _err(fn)
        assert im(s, vals, None, 4, aux, 4, None, None, 4, out, 4096, aux, None) == INVALID
        assert "value_offsets is null" in _err(fn)
        assert im(s, vals, None, 0, aux, 4, None, None, 4, None, 0, aux, None) == INVALID
        assert "value_offsets is null" in _err(fn)             # also without values, also measuring
        assert im(s, vals, aux, 4, None, 4, None, None, 4, out, 4096, aux, None) == INVALID
        assert "list_offsets is null" in _err(fn)
        assert im(s, vals, aux, 4, aux, 4, None, None, 4, out, 4096, None, None) == INVALID
        assert "out_offsets is null" in _err(fn)
        assert im(s, vals, aux, 4, aux, 4, None, None, 4, None, 0, None, None) == INVALID
        assert "out_offsets is null" in _err(fn)               # the measure form too
        assert im(s, vals, aux + 4, 4, aux, 4, None, None, 4, out, 4096, aux, None) == INVALID
        assert "value_offsets / out_offsets must be 8-byte aligned" in _err(fn)
        assert im(s, vals, aux, 4, aux, 4, None, None, 4, out, 4096, aux + 4, None) == INVALID
        assert "value_offsets / out_offsets must be 8-byte aligned" in _err(fn)
        assert im(s, vals, aux, 4, aux + 4, 4, None, None, 4, out, 4096, aux, None) == INVALID
        assert "list_offsets must be 8-byte aligned" in _err(fn)
        assert im(s, vals, aux, 4, aux, 4, None, aux + 2, 4, out, 4096, aux, None) == INVALID
        assert "entry_validity / elem_validity must be 4-byte aligned" in _err(fn)
        assert im(s, None, aux, 4, aux, 4, None, None, 4, out, 4096, aux, None) == INVALID
        assert "values is null" in _err(fn)


def test_wrap_targets_and_argument_errors(L, schemas):
    wr, fn = L.fury_row_wrap, "fury_row_wrap"
    r1, vals = _buf()
    r2, out = _buf()
    r3, aux = _buf()

    def call(schema):
        h = None if schema is None else schemas[schema].handle
        return wr(h, vals, aux, 4, None, 4, out, 4096, aux, None)
    assert call(None) == INVALID
    assert "schema is null" in _err(fn)
    assert call("all") == UNSUPPORTED
    assert "5 fields" in _err(fn) and "fury_row_zip" in _err(fn)
    for name in ("items_arr", "map_enc"):
        assert call(name) == UNSUPPORTED, name
        assert "collection schema" in _err(fn)
    for name in ("id", "strs"):
        assert call(name) == UNSUPPORTED, name
        assert "is not a STRUCT, LIST or MAP" in _err(fn)
    for name in ("items", "m", "f5", "f3"):                    # LIST<STRUCT>, MAP, STRUCT, LIST<STRING>
        s = schemas[name].handle
        assert wr(s, vals, aux, 4, None, -1, out, 4096, aux, None) == INVALID
        assert "nrows < 0" in _err(fn)
        assert wr(s, vals, aux, -1, None, 4, out, 4096, aux, None) == INVALID
        assert "num_values < 0" in _err(fn)
        assert wr(s, vals, aux, 4, None, 4, out, -8, aux, None) == INVALID
        assert "out_capacity < 0" in _err(fn)
        assert wr(s, vals + 4, aux, 4, None, 4, out, 4096, aux, None) == INVALID
        assert "values must be 8-byte aligned" in _err(fn)
        assert wr(s, vals, aux, 4, None, 4, out + 4, 4096, aux, None) == INVALID
        assert "out_rows must be 8-byte aligned" in _err(fn)
        assert wr(s, vals, None, 4, None, 4, out, 4096, aux, None) == INVALID
        assert "value_offsets is null" in _err(fn)
        assert wr(s, vals, aux, 4, None, 4, out, 4096, None, None) == INVALID
        assert "out_offsets is null" in _err(fn)
        assert wr(s, vals, aux + 4, 4, None, 4, out, 4096, aux, None) == INVALID
        assert "must be 8-byte aligned" in _err(fn)
        assert wr(s, vals, aux, 4, aux + 2, 4, out, 4096, aux, None) == INVALID
        assert "validity must be 4-byte aligned" in _err(fn)
        assert wr(s, None, aux, 4, None, 4, out, 4096, aux, None) == INVALID
        assert "values is null" in _err(fn)


# -- the Python surface, as far as it goes without a device ---------------------------------------------
def test_field_encoder_and_value_encoders():
    from fury_amd.encoder import ArrayEncoder, Encoders, MapEncoder, RowEncoder
    fx = explode_fields()
    enc = Encoders.bean(fx, device="cpu")
    one = enc.field_encoder("items")
    assert type(one) is RowEncoder and tuple(one.schema().fields) == (fx[1],)
    assert enc.field_encoder(1) is one is enc.selected_encoder(["items"])      # cached
    assert one._value_encoder(False).schema_hash == enc.element_encoder("items").schema_hash
    assert type(one._value_encoder(True)) is ArrayEncoder
    assert type(enc.field_encoder("ll")._value_encoder(False)) is ArrayEncoder
    assert type(enc.field_encoder("m")._value_encoder(True)) is MapEncoder
    assert enc.field_encoder("m")._value_encoder(False) is None                # no target: the library says why
    assert enc._value_encoder(False) is None and enc._value_encoder(True) is None
    arr = enc.child_encoder("items")
    assert arr._value_encoder(False).schema_hash == one._value_encoder(False).schema_hash
    assert arr._value_encoder(True) is None


def test_python_surface_checks_the_values_hash():
    from fury_amd.encoder import ClassNotCompatibleException, Encoders, RowBatch
    enc = Encoders.bean(explode_fields(), device="cpu")
    one = enc.field_encoder("items")
    h = enc.element_encoder("items").schema_hash
    bad = RowBatch(None, None, 3, h + 1)
    for call in (lambda: one.implode(bad, None), lambda: one.implode_into(bad, None, None, None),
                 lambda: one.bind_implode(bad, None, None, None),
                 lambda: enc.child_encoder("items").implode(bad, None)):
        with pytest.raises(ClassNotCompatibleException, match="Schema is not consistent"):
            call()
    s = Encoders.bean(SCHEMAS["foo"], device="cpu")
    f5 = s.field_encoder("f5")
    bad = RowBatch(None, None, 3, s.child_encoder("f5").schema_hash + 1)
    for call in (lambda: f5.wrap(bad), lambda: f5.wrap_into(bad, None, None),
                 lambda: f5.bind_wrap(bad, None, None), lambda: s.with_nested(bad, "f5", bad)):
        with pytest.raises(ClassNotCompatibleException, match="Schema is not consistent"):
            call()
