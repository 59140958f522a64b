"""CPU checks of the row selection's C ABI (fury_row_take / fury_row_filter): every argument error
is reported on the host, before any device work, with its status and a message that names the
function.  Host buffers stand in for device memory and are never dereferenced: every call fails
first."""
from __future__ import annotations

import ctypes

import pytest

from fury_amd import types as T
from fury_amd.workloads import SCHEMAS

OK, INVALID, CAPACITY = 0, 1, 7


def _buf(nbytes=8192, align=64):
    raw = ctypes.create_string_buffer(nbytes + align)
    base = (ctypes.addressof(raw) + align - 1) & ~(align - 1)
    return raw, base


@pytest.fixture(scope="module")
def L():
    from fury_amd import _native as N
    return N.lib()


@pytest.fixture(scope="module")
def schemas():
    from fury_amd.encoder import Encoders, Schema
    arr = Encoders.array_encoder(T.field("item", T.INT64), device="cpu")
    return {"struct100": Schema(SCHEMAS["struct100"]), "mixed": Schema(SCHEMAS["mixed"]),
            "foo": Schema(SCHEMAS["foo"]), "array": arr.schema(), "_keep": arr}


def _err(fn):
    from fury_amd import _native as N
    msg = N.last_error()
    assert fn in msg, msg
    return msg


def test_symbols_are_bound(L):
    from fury_amd import _native as N
    for name in ("fury_row_take", "fury_row_filter"):
        assert name in N.SIGNATURES
        assert hasattr(L, name)


def test_take_argument_errors(L, schemas):
    take, fn = L.fury_row_take, "fury_row_take"
    fixed, var = schemas["struct100"].handle, schemas["mixed"].handle
    r1, rows = _buf()
    r2, out = _buf()
    r3, aux = _buf()          # offsets / indices
    assert take(None, rows, None, 4, aux, 2, out, 4096, None, None) == INVALID
    assert "schema is null" in _err(fn)
    assert take(fixed, rows, None, -1, aux, 2, out, 4096, None, None) == INVALID
    assert "nrows < 0" in _err(fn)
    assert take(fixed, rows, None, 4, aux, -1, out, 4096, None, None) == INVALID
    assert "num_selected < 0" in _err(fn)
    assert take(fixed, rows, None, 4, None, 2, out, 4096, None, None) == INVALID
    assert "indices is null" in _err(fn)
    assert take(fixed, None, None, 4, aux, 2, out, 4096, None, None) == INVALID
    assert "rows is null" in _err(fn)
    assert take(fixed, rows, None, 4, aux, 2, out, -1, None, None) == INVALID
    assert "out_capacity < 0" in _err(fn)
    assert take(fixed, rows, None, 4, aux, 2, out + 4, 4096, None, None) == INVALID
    assert "out_rows must be 8-byte aligned" in _err(fn)
    assert take(fixed, rows + 4, None, 4, aux, 2, out, 4096, None, None) == INVALID
    assert "rows must be 8-byte aligned" in _err(fn)
    # variable-length rows need both offsets arrays, whatever the schema's shape
    for s in (var, schemas["foo"].handle, schemas["array"].handle):
        assert take(s, rows, None, 4, aux, 2, out, 4096, aux, None) == INVALID
        assert "row_offsets" in _err(fn)
        assert take(s, rows, aux, 4, aux, 2, out, 4096, None, None) == INVALID
        assert "out_offsets" in _err(fn)
    assert take(var, None, aux, 4, aux, 2, out, 4096, aux, None) == INVALID
    assert "rows is null" in _err(fn)


def test_filter_argument_errors(L, schemas):
    flt, fn = L.fury_row_filter, "fury_row_filter"
    fixed, var = schemas["struct100"].handle, schemas["mixed"].handle
    r1, rows = _buf()
    r2, out = _buf()
    r3, aux = _buf()
    assert flt(None, rows, None, 4, aux, out, 4096, None, aux, None, None) == INVALID
    assert "schema is null" in _err(fn)
    assert flt(fixed, rows, None, -1, aux, out, 4096, None, aux, None, None) == INVALID
    assert "nrows < 0" in _err(fn)
    assert flt(fixed, rows, None, 4, None, out, 4096, None, aux, None, None) == INVALID
    assert "row_mask is null" in _err(fn)
    assert flt(fixed, rows, None, 4, aux + 2, out, 4096, None, aux, None, None) == INVALID
    assert "row_mask must be 4-byte aligned" in _err(fn)
    assert flt(fixed, rows, None, 4, aux, out, 4096, None, None, None, None) == INVALID
    assert "out_count is null" in _err(fn)
    assert flt(fixed, rows, None, 0, None, out, 4096, None, None, None, None) == INVALID   # even when empty
    assert "out_count is null" in _err(fn)
    assert flt(fixed, None, None, 4, aux, out, 4096, None, aux, None, None) == INVALID
    assert "rows is null" in _err(fn)
    assert flt(fixed, rows, None, 4, aux, out, -8, None, aux, None, None) == INVALID
    assert "out_capacity < 0" in _err(fn)
    assert flt(fixed, rows, None, 4, aux, out + 4, 4096, None, aux, None, None) == INVALID
    assert "out_rows must be 8-byte aligned" in _err(fn)
    assert flt(fixed, rows + 4, None, 4, aux, out, 4096, None, aux, None, None) == INVALID
    assert "rows must be 8-byte aligned" in _err(fn)
    assert flt(var, rows, None, 4, aux, out, 4096, aux, aux, None, None) == INVALID
    assert "row_offsets" in _err(fn)
    assert flt(var, rows, aux, 4, aux, out, 4096, None, aux, None, None) == INVALID
    assert "out_offsets" in _err(fn)


def test_fixed_schema_capacity_is_checked_on_the_host(L, schemas):
    fixed = schemas["struct100"].handle                     # 816-byte rows
    r1, rows = _buf()
    r2, out = _buf()
    r3, aux = _buf()
    assert L.fury_row_take(fixed, rows, None, 4, aux, 5, out, 5 * 816 - 8, None, None) == CAPACITY
    msg = _err("fury_row_take")
    assert "5 rows of 816 bytes" in msg
    assert L.fury_row_take(fixed, rows, None, 4, aux, 5, out, 0, aux, None) == CAPACITY
    # filter: the count is not known on the host, so the bound is nrows * fixed_size
    assert L.fury_row_filter(fixed, rows, None, 4, aux, out, 4 * 816 - 8, None, aux, None,
                             None) == CAPACITY
    assert "4 rows of 816 bytes" in _err("fury_row_filter")


def test_python_surface_checks_the_schema_hash():
    """take / filter and their *_into forms refuse a batch of another schema before they touch any
    buffer."""
    from fury_amd.encoder import ClassNotCompatibleException, Encoders, RowBatch
    enc = Encoders.bean(SCHEMAS["mixed"], device="cpu")
    foreign = RowBatch(None, None, 0, enc.schema_hash + 1)
    for call in (lambda: enc.take(foreign, [0]), lambda: enc.take_into(foreign, [0], None, None),
                 lambda: enc.bind_take(foreign, [0], None, None),
                 lambda: enc.filter(foreign, None),
                 lambda: enc.filter_into(foreign, None, None, None, None)):
        with pytest.raises(ClassNotCompatibleException, match="Schema is not consistent"):
            call()
