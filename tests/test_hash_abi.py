"""CPU checks of fury_row_hash: the symbols are bound and exported, and every argument error is
reported on the host, before any device work, with its status and a message that names the
function.  Host buffers stand in for device memory and are never dereferenced: every call fails
first, or has no rows."""
from __future__ import annotations

import ctypes

import pytest

from fury_amd.workloads import SCHEMAS

OK, INVALID, UNSUPPORTED = 0, 1, 2
INT32_MAX = 2 ** 31 - 1


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
    from fury_amd import types as T
    from fury_amd.encoder import Encoders, Schema
    arr = Encoders.array_encoder(T.field("item", T.INT64), device="cpu")
    return {"struct100": Schema(SCHEMAS["struct100"]), "mixed": Schema(SCHEMAS["mixed"]),
            "foo": Schema(SCHEMAS["foo"]), "narrow": Schema(SCHEMAS["narrow"]),
            "array": arr.schema(), "_keep": arr}


def _err():
    from fury_amd import _native as N
    msg = N.last_error()
    assert "fury_row_hash" in msg, msg
    return msg


def _keys(*idx):
    return (ctypes.c_int32 * max(len(idx), 1))(*idx)


def test_symbols_are_bound(L):
    from fury_amd import _native as N
    for name in ("fury_row_hash", "fury_hash_bytes", "fury_hash_null"):
        assert name in N.SIGNATURES
        assert hasattr(L, name)
    with open(N.HERE + "/../include/fury_row.h") as f:
        header = f.read()
    for rule in ("1. H(bytes, seed)", "2. For row r", "3. value_bytes", "4. part_id[r]", "5. A LIST"):
        assert rule in header, rule


def test_hash_argument_errors(L, schemas):
    fixed, var = schemas["struct100"].handle, schemas["mixed"].handle
    r1, rows = _buf()
    r2, out = _buf()
    r3, aux = _buf()

    def call(s=fixed, keys=_keys(0), nk=1, rows=rows, ro=None, n=4, seed=0, parts=3, oh=out, op=aux):
        return L.fury_row_hash(s, keys, nk, rows, ro, n, seed, parts, oh, op, None)

    assert call(s=None) == INVALID
    assert "schema is null" in _err()
    assert call(n=-1) == INVALID
    assert "nrows < 0" in _err()
    assert call(keys=None) == INVALID
    assert "fields is null" in _err()
    # the key count: 1 .. 64, with fury_row_project's codes
    assert call(nk=0) == INVALID
    assert "num_selected <= 0" in _err()
    assert call(nk=-3) == INVALID
    assert call(keys=_keys(*range(65)), nk=65) == UNSUPPORTED
    assert "at most 64 fields" in _err()
    # the key fields
    assert call(keys=_keys(100)) == INVALID
    assert "fields[0] = 100 is not a field" in _err()
    assert call(keys=_keys(0, -1), nk=2) == INVALID
    assert "fields[1] = -1" in _err()
    assert call(keys=_keys(3, 5, 3), nk=3) == INVALID
    assert "selected twice" in _err()
    assert call(s=schemas["array"].handle) == UNSUPPORTED
    assert "collection schema" in _err()
    # nested keys and lists: not canonical bytes
    foo = schemas["foo"].handle
    for k, name in ((2, "f3"), (3, "f4"), (4, "f5")):
        assert call(s=foo, keys=_keys(0, k), nk=2, ro=aux) == UNSUPPORTED
        msg = _err()
        assert f"field {k} ({name})" in msg and "LIST / STRUCT / MAP" in msg
    narrow = schemas["narrow"]
    k = [f.name for f in SCHEMAS["narrow"]].index("k_ints")
    assert call(s=narrow.handle, keys=_keys(k), ro=aux) == UNSUPPORTED
    assert "k_ints" in _err()
    # the outputs
    assert call(oh=None, op=None) == INVALID
    assert "both null" in _err()
    assert call(oh=None, op=None, n=0) == INVALID              # even when empty
    for parts in (0, -1, -2 ** 31):
        assert call(parts=parts) == INVALID
        assert "num_parts" in _err()
    assert call(oh=out + 2) == INVALID
    assert "4-byte aligned" in _err()
    assert call(op=aux + 1) == INVALID
    assert "4-byte aligned" in _err()
    # the batch
    assert call(rows=None) == INVALID
    assert "rows is null" in _err()
    assert call(rows=rows + 4) == INVALID
    assert "rows must be 8-byte aligned" in _err()
    assert call(s=var, keys=_keys(3), ro=None) == INVALID
    assert "variable-length rows need row_offsets" in _err()
    assert call(s=var, keys=_keys(3), ro=aux + 4) == INVALID
    assert "row_offsets must be 8-byte aligned" in _err()


def test_no_rows_is_a_no_op(L, schemas):
    """nrows == 0 returns FURY_OK without touching a buffer: num_parts is not looked at without
    out_part_ids, rows and row_offsets may be NULL, and the outputs keep their contents."""
    fixed, var = schemas["struct100"].handle, schemas["mixed"].handle
    raw, out = _buf(64)
    ctypes.memset(out, 0xAB, 64)
    assert L.fury_row_hash(fixed, _keys(0, 99), 2, None, None, 0, 0, 1, out, out + 32, None) == OK
    assert L.fury_row_hash(var, _keys(3, 0), 2, None, None, 0, 42, INT32_MAX, out, out + 32, None) == OK
    assert L.fury_row_hash(var, _keys(3), 1, None, None, 0, 42, 0, out, None, None) == OK
    assert L.fury_row_hash(var, _keys(3), 1, None, None, 0, 42, -5, out, None, None) == OK
    assert L.fury_row_hash(var, _keys(3), 1, None, None, 0, 0xFFFFFFFF, 1, None, out, None) == OK
    assert ctypes.string_at(out, 64) == b"\xab" * 64


def test_python_surface_checks_before_any_device_work():
    from fury_amd import types as T
    from fury_amd.encoder import (ClassNotCompatibleException, Encoders, IllegalArgumentException,
                                  RowBatch)
    import torch
    enc = Encoders.bean(SCHEMAS["mixed"], device="cpu")
    batch = RowBatch(torch.zeros(64, dtype=torch.uint8), torch.zeros(5, dtype=torch.int64), 4,
                     enc.schema_hash)
    out = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(IllegalArgumentException, match="no field named"):
        enc.hash_rows_into(batch, ["nope"], out)
    with pytest.raises(IllegalArgumentException, match="int32 or uint32"):
        enc.hash_rows_into(batch, ["a"], torch.zeros(4, dtype=torch.int64))
    with pytest.raises(IllegalArgumentException, match="3 entries for 4 rows"):
        enc.hash_rows_into(batch, ["a"], out[:3])
    with pytest.raises(IllegalArgumentException, match="seed"):
        enc.hash_rows_into(batch, ["a"], out, seed=2 ** 32)
    for parts in (None, 0, 2 ** 31):
        with pytest.raises(IllegalArgumentException, match="num_parts"):
            enc.hash_rows_into(batch, ["a"], None, out, num_parts=parts)
    other = Encoders.bean([T.field("x", T.INT64)], device="cpu")
    with pytest.raises(ClassNotCompatibleException):
        other.hash_rows_into(batch, ["x"], out)
