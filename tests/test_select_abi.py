"""CPU checks of the field selection's C ABI (fury_schema_select / fury_row_select): the selected
schema equals a schema built directly from the same fields, and every argument error is reported on
the host, before any device work, with its status and a message that names the function.  Host
buffers stand in for device memory and are never dereferenced: every fury_row_select call here fails
first."""
from __future__ import annotations

import ctypes

import pytest

from fury_amd import types as T
from fury_amd.workloads import SCHEMAS
from tests.test_extract_abi import deep_fields

OK, INVALID, UNSUPPORTED, CAPACITY = 0, 1, 2, 7


def _buf(nbytes=8192, align=64):
    raw = ctypes.create_string_buffer(nbytes + align)
    base = (ctypes.addressof(raw) + align - 1) & ~(align - 1)
    return raw, base


def _sel(*idx):
    return (ctypes.c_int32 * max(len(idx), 1))(*idx), len(idx)


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


def _err(fn):
    from fury_amd import _native as N
    msg = N.last_error()
    assert fn in msg, msg
    return msg


def _info(L, h):
    from fury_amd import _native as N
    info = N.FurySchemaInfo()
    assert L.fury_schema_get_info(h, ctypes.byref(info)) == OK
    return (info.num_fields, info.bitmap_bytes, info.fixed_size, info.is_fixed, info.schema_hash,
            L.fury_schema_num_nodes(h))


def _selected(L, schema, idx):
    h = ctypes.c_void_p()
    p, n = _sel(*idx)
    assert L.fury_schema_select(schema.handle, p, n, ctypes.byref(h)) == OK
    try:
        return _info(L, h)
    finally:
        L.fury_schema_destroy(h)


def _direct(L, fields, idx):
    from fury_amd.encoder import Schema
    return _info(L, Schema([fields[k] for k in idx]).handle)


def test_symbols_are_bound(L):
    from fury_amd import _native as N
    for name in ("fury_schema_select", "fury_row_select"):
        assert name in N.SIGNATURES
        assert hasattr(L, name)


STRUCT100_SELECTIONS = {"one": [37], "ten spread": list(range(3, 100, 10)), "64": list(range(64)),
                        "65": list(range(30, 95)), "all reversed": list(range(99, -1, -1))}


@pytest.mark.parametrize("what", list(STRUCT100_SELECTIONS))
def test_selected_schema_of_struct100(L, schemas, what):
    idx = STRUCT100_SELECTIONS[what]
    got = _selected(L, schemas["struct100"], idx)
    assert got == _direct(L, SCHEMAS["struct100"], idx)
    assert got[:4] == (len(idx), ((len(idx) + 63) // 64) * 8, ((len(idx) + 63) // 64) * 8 + 8 * len(idx), 1)


def test_selected_schema_of_foo_and_deep(L, schemas):
    fields = SCHEMAS["foo"]
    names = [f.name for f in fields]
    for sel in (("f5", "f1"), ("f3", "f4")):
        idx = [names.index(x) for x in sel]
        got = _selected(L, schemas["foo"], idx)
        assert got == _direct(L, fields, idx), sel
        assert got[3] == 0                                           # a nested field: never is_fixed
    deep = deep_fields()
    for idx in ([0], [1], [1, 0], [0, 1]):
        assert _selected(L, schemas["deep"], idx) == _direct(L, deep, idx), idx
    assert _selected(L, schemas["deep"], [0, 1])[4] == schemas["deep"].schema_hash
    assert _selected(L, schemas["deep"], [0])[:4] == (1, 8, 16, 1)


def _selection_errors(call, fn, schemas):
    """The selection rules both functions share; call(schema handle, fields, count) -> status."""
    foo, arr = schemas["foo"].handle, schemas["array"].handle
    p, n = _sel(4, 0)
    assert call(None, p, n) == INVALID
    assert "schema is null" in _err(fn)
    assert call(foo, None, 2) == INVALID
    assert "fields is null" in _err(fn)
    for count in (0, -1, 6):
        assert call(foo, p, count) == INVALID, count
        assert "num_selected" in _err(fn)
    for idx in ((-1,), (5,), (0, 5), (2, -1)):
        p, n = _sel(*idx)
        assert call(foo, p, n) == INVALID, idx
        assert "is not a field" in _err(fn)
    for idx in ((1, 1), (0, 3, 4, 0)):
        p, n = _sel(*idx)
        assert call(foo, p, n) == INVALID, idx
        assert "selected twice" in _err(fn)
    p, n = _sel(0)
    assert call(arr, p, n) == UNSUPPORTED
    assert "collection schema" in _err(fn)


def test_schema_select_argument_errors(L, schemas):
    fn = "fury_schema_select"
    h = ctypes.c_void_p(1)
    _selection_errors(lambda s, p, n: L.fury_schema_select(s, p, n, ctypes.byref(h)), fn, schemas)
    assert h.value is None                                   # *out is NULL after a failure
    p, n = _sel(4)
    assert L.fury_schema_select(schemas["foo"].handle, p, n, None) == INVALID
    assert "out is null" in _err(fn)


def test_select_argument_errors(L, schemas):
    sel, fn = L.fury_row_select, "fury_row_select"
    foo, s100 = schemas["foo"].handle, schemas["struct100"].handle
    r1, rows = _buf()
    r2, out = _buf()
    r3, aux = _buf()          # offsets
    _selection_errors(lambda s, p, n: sel(s, p, n, rows, aux, 4, out, 4096, aux, None), fn, schemas)
    p, n = _sel(4, 0)         # foo.f5, foo.f1: a variable-length selection
    assert sel(foo, p, n, rows, aux, -1, out, 4096, aux, None) == INVALID
    assert "nrows < 0" in _err(fn)
    assert sel(foo, p, n, rows, aux, 4, out, -8, aux, None) == INVALID
    assert "out_capacity < 0" in _err(fn)
    assert sel(foo, p, n, rows + 4, aux, 4, out, 4096, aux, None) == INVALID
    assert "rows must be 8-byte aligned" in _err(fn)
    assert sel(foo, p, n, rows, aux, 4, out + 4, 4096, aux, None) == INVALID
    assert "out_rows must be 8-byte aligned" in _err(fn)
    assert sel(foo, p, n, rows, aux + 4, 4, out, 4096, aux, None) == INVALID
    assert "8-byte aligned" in _err(fn)
    assert sel(foo, p, n, rows, aux, 4, out, 4096, aux + 4, None) == INVALID
    assert "8-byte aligned" in _err(fn)
    assert sel(foo, p, n, rows, None, 4, out, 4096, aux, None) == INVALID
    assert "need row_offsets" in _err(fn)
    assert sel(foo, p, n, rows, aux, 4, out, 4096, None, None) == INVALID
    assert "needs out_offsets" in _err(fn)
    assert sel(foo, p, n, rows, aux, 4, None, 0, None, None) == INVALID      # the measure form too
    assert "needs out_offsets" in _err(fn)
    assert sel(foo, p, n, None, aux, 4, out, 4096, aux, None) == INVALID
    assert "rows is null" in _err(fn)
    p1, n1 = _sel(0)          # foo.f1 alone is fixed-width, but its source rows are not
    assert sel(foo, p1, n1, rows, None, 4, out, 4096, None, None) == INVALID
    assert "need row_offsets" in _err(fn)
    assert sel(foo, p1, n1, rows, aux, 4, out, 4 * 16 - 8, None, None) == CAPACITY
    assert "out_capacity 56 < 4 rows of 16 bytes" in _err(fn)
    p10, n10 = _sel(*range(3, 100, 10))
    assert sel(s100, p10, n10, rows, None, 4, out, 4 * 88 - 1, None, None) == CAPACITY
    assert "rows of 88 bytes" in _err(fn)
    assert sel(s100, p10, n10, None, None, 4, out, 4 * 88, None, None) == INVALID
    assert "rows is null" in _err(fn)


def test_selected_encoder():
    from fury_amd.encoder import (Encoders, IllegalArgumentException, RowEncoder,
                                  UnsupportedOperationException)
    fields = SCHEMAS["foo"]
    enc = Encoders.bean(fields, device="cpu")
    child = enc.selected_encoder(["f5", "f1"])
    assert type(child) is RowEncoder and tuple(child.schema().fields) == (fields[4], fields[0])
    assert child.schema_hash == Encoders.bean([fields[4], fields[0]], device="cpu").schema_hash
    assert str(child.device) == "cpu"
    assert enc.selected_encoder([4, 0]) is child                   # cached per selection, names or slots
    assert enc.selected_encoder([0, 4]) is not child
    wide = Encoders.bean(SCHEMAS["struct100"], device="cpu")
    assert wide.selected_encoder(range(99, -1, -1)).schema().num_fields == 100      # no 64-field cap
    with pytest.raises(IllegalArgumentException, match="no field named 'nope'"):
        enc.selected_encoder(["nope"])
    with pytest.raises(IllegalArgumentException, match="selected twice"):
        enc.selected_encoder(["f1", 0])
    with pytest.raises(IllegalArgumentException, match="is not a field"):
        enc.selected_encoder([5])
    with pytest.raises(IllegalArgumentException, match="num_selected"):
        enc.selected_encoder([])
    arr = Encoders.array_encoder(T.field("item", T.INT64), device="cpu")
    with pytest.raises(UnsupportedOperationException, match="collection schema"):
        arr.selected_encoder([0])


def test_python_surface_checks_the_schema_hash():
    from fury_amd.encoder import ClassNotCompatibleException, Encoders, RowBatch
    enc = Encoders.bean(SCHEMAS["foo"], device="cpu")
    foreign = RowBatch(None, None, 0, enc.schema_hash + 1)
    for call in (lambda: enc.select_fields(foreign, ["f5"]),
                 lambda: enc.select_fields_into(foreign, ["f5"], None, None),
                 lambda: enc.bind_select_fields(foreign, ["f5"], None, None)):
        with pytest.raises(ClassNotCompatibleException, match="Schema is not consistent"):
            call()
