"""CPU checks of the in-place update's C ABI (fury_row_update): every argument error is reported on
the host, before any device work, with the status of the reference's exception type and a message
that names the field."""
from __future__ import annotations

import ctypes

import pytest

from fury_amd import types as T
from fury_amd.workloads import SCHEMAS

OK, INVALID, UNSUPPORTED = 0, 1, 2


def _sel(*idx):
    return (ctypes.c_int32 * max(len(idx), 1))(*idx), len(idx)


def _buf(nbytes=4096, align=64):
    """A host buffer standing in for device memory (never dereferenced: every call fails first)."""
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
    return {"struct100": Schema(SCHEMAS["struct100"]), "foo": Schema(SCHEMAS["foo"]),
            "narrow": Schema(SCHEMAS["narrow"]), "mixed": Schema(SCHEMAS["mixed"]),
            "array": arr.schema(), "_keep": arr}


def _cols(N, n, values):
    c = (N.FuryColumn * n)()
    for j in range(n):
        c[j].values = values
    return c


def test_symbol_is_bound(L):
    from fury_amd import _native as N
    assert "fury_row_update" in N.SIGNATURES
    assert hasattr(L, "fury_row_update")


def test_invalid_arguments(L, schemas):
    from fury_amd import _native as N
    s = schemas["struct100"].handle
    raw, rows = _buf()
    raw2, vals = _buf()
    cols = _cols(N, 4, vals)
    sel, k = _sel(0, 99)
    up = L.fury_row_update
    assert up(None, sel, k, rows, None, 4, cols, None, None) == INVALID            # null schema
    assert "schema is null" in N.last_error()
    assert up(s, sel, k, rows, None, -1, cols, None, None) == INVALID              # nrows < 0
    assert "nrows < 0" in N.last_error()
    assert up(s, sel, 0, rows, None, 4, cols, None, None) == INVALID               # nothing selected
    assert "num_selected <= 0" in N.last_error()
    assert up(s, sel, -3, rows, None, 4, cols, None, None) == INVALID
    assert up(s, None, k, rows, None, 4, cols, None, None) == INVALID              # null fields
    assert "fields is null" in N.last_error()
    assert up(s, sel, k, rows, None, 4, None, None, None) == INVALID               # null columns
    assert "columns is null" in N.last_error()
    assert "fury_row_update" in N.last_error()
    for bad in ((0, 100), (-1, 5), (7, 7), (3, 50, 3)):
        sb, kb = _sel(*bad)
        assert up(s, sb, kb, rows, None, 4, cols, None, None) == INVALID, bad
    sb, kb = _sel(0, 100)
    up(s, sb, kb, rows, None, 4, cols, None, None)
    assert "fields[1] = 100 is not a field of the schema" in N.last_error()
    sd, kd = _sel(7, 7)
    up(s, sd, kd, rows, None, 4, cols, None, None)
    assert "f07" in N.last_error() and "twice" in N.last_error()


def test_column_mask_and_rows_checks(L, schemas):
    from fury_amd import _native as N
    raw, rows = _buf()
    raw2, vals = _buf()
    up = L.fury_row_update
    nar = schemas["narrow"].handle
    ix = {f.name: i for i, f in enumerate(SCHEMAS["narrow"])}
    # null / misaligned values, per width (BOOL bits are read as 32-bit words)
    sel, m = _sel(ix["d_int"])
    c = (N.FuryColumn * 1)()
    assert up(nar, sel, m, rows, rows, 4, c, None, None) == INVALID
    assert "(d_int): values is null" in N.last_error()
    for name, off in (("d_int", 2), ("c_short", 1), ("g_ts", 4), ("a_bool", 2)):
        sel, m = _sel(ix[name])
        c = _cols(N, 1, vals + off)
        assert up(nar, sel, m, rows, rows, 4, c, None, None) == INVALID, name
        assert f"({name}): values misaligned" in N.last_error()
    sel, m = _sel(ix["b_byte"])                                     # INT8: any address
    c = _cols(N, 1, vals + 1)
    assert up(nar, sel, m, None, rows, 4, c, None, None) == INVALID
    assert "rows is null" in N.last_error()
    # misaligned validity / row_mask
    sel, m = _sel(ix["d_int"])
    c = _cols(N, 1, vals)
    c[0].validity = vals + 1
    assert up(nar, sel, m, rows, rows, 4, c, None, None) == INVALID
    assert "(d_int): validity must be 4-byte aligned" in N.last_error()
    c = _cols(N, 1, vals)
    assert up(nar, sel, m, rows, rows, 4, c, vals + 2, None) == INVALID
    assert "row_mask must be 4-byte aligned" in N.last_error()
    # rows / row_offsets
    assert up(nar, sel, m, None, rows, 4, c, None, None) == INVALID
    assert "rows is null" in N.last_error()
    assert up(nar, sel, m, rows + 4, rows, 4, c, None, None) == INVALID
    assert "8-byte aligned" in N.last_error()
    assert up(nar, sel, m, rows, None, 4, c, None, None) == INVALID                # var rows need offsets
    assert "row_offsets" in N.last_error()


def test_rows_messages_name_the_function(L, schemas):
    """The three checks of the row batch itself report like every other check of the call: the
    message starts with the function's name."""
    from fury_amd import _native as N
    raw, rows = _buf()
    raw2, vals = _buf()
    up = L.fury_row_update
    nar = schemas["narrow"].handle                   # variable-length rows
    sel, m = _sel({f.name: i for i, f in enumerate(SCHEMAS["narrow"])}["d_int"])
    c = _cols(N, 1, vals)
    assert up(nar, sel, m, None, rows, 4, c, None, None) == INVALID
    assert N.last_error() == "fury_row_update: rows is null"
    assert up(nar, sel, m, rows + 4, rows, 4, c, None, None) == INVALID
    assert N.last_error() == "fury_row_update: rows must be 8-byte aligned"
    assert up(nar, sel, m, rows, None, 4, c, None, None) == INVALID
    assert N.last_error() == "fury_row_update: variable-length rows need row_offsets"


def test_unsupported_selections(L, schemas):
    from fury_amd import _native as N
    raw, rows = _buf()
    raw2, vals = _buf()
    cols = _cols(N, 70, vals)
    up = L.fury_row_update
    foo = schemas["foo"].handle                      # f1 int32, f2 string, f3 list<string>, f4 map, f5 struct
    for k, name in ((1, "f2"), (2, "f3"), (3, "f4"), (4, "f5")):
        sel, m = _sel(0, k)
        assert up(foo, sel, m, rows, rows, 4, cols, None, None) == UNSUPPORTED
        msg = N.last_error()
        assert f"({name})" in msg and "variable-length" in msg and "re-encode" in msg, msg
    nar = schemas["narrow"].handle
    ix = {f.name: i for i, f in enumerate(SCHEMAS["narrow"])}
    for name in ("h_dec", "i_bin", "k_ints"):        # DECIMAL, BINARY, LIST of fixed-width elements
        sel, m = _sel(ix["d_int"], ix[name])
        assert up(nar, sel, m, rows, rows, 4, cols, None, None) == UNSUPPORTED
        assert f"({name})" in N.last_error() and "re-encode" in N.last_error()
    # a collection schema has no row fields
    sel, m = _sel(0)
    assert up(schemas["array"].handle, sel, m, rows, rows, 4, cols, None, None) == UNSUPPORTED
    assert "collection schema" in N.last_error()
    # more fields than the argument-block table
    s100 = schemas["struct100"].handle
    sel, m = _sel(*range(65))
    assert up(s100, sel, m, rows, None, 4, cols, None, None) == UNSUPPORTED
    assert "at most 64 fields" in N.last_error() and "re-encode" in N.last_error()
    sel, m = _sel(*range(64))                        # 64 are accepted (and fail later: no rows)
    assert up(s100, sel, m, None, None, 4, cols, None, None) == INVALID
    assert "rows is null" in N.last_error()


def test_empty_batch_is_ok(L, schemas):
    from fury_amd import _native as N
    sel, m = _sel(0, 99)
    cols = (N.FuryColumn * 2)()
    assert L.fury_row_update(schemas["struct100"].handle, sel, m, None, None, 0, cols, None, None) == OK
    assert L.fury_row_update(schemas["struct100"].handle, sel, m, None, None, 0, None, None, None) == OK
    sel, m = _sel(0)
    assert L.fury_row_update(schemas["mixed"].handle, sel, m, None, None, 0, cols, None, None) == OK


def test_python_update_checks_schema_hash_and_column_count():
    """update_fields refuses a batch of another schema, and a column list that does not match the
    selection, before it touches any buffer."""
    from fury_amd.encoder import (ClassNotCompatibleException, Encoders, IllegalArgumentException,
                                  RowBatch)
    enc = Encoders.bean(SCHEMAS["mixed"], device="cpu")
    with pytest.raises(ClassNotCompatibleException, match="Schema is not consistent"):
        enc.update_fields(RowBatch(None, None, 0, enc.schema_hash + 1), ["a"], [])
    with pytest.raises(IllegalArgumentException, match="1 fields selected, 0 columns"):
        enc.update_fields(RowBatch(None, None, 0, enc.schema_hash), ["a"], [])
    with pytest.raises(IllegalArgumentException, match="nope"):
        enc.update_fields(RowBatch(None, None, 0, enc.schema_hash), ["nope"], [])
