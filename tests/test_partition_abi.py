"""CPU checks of fury_row_partition / fury_row_concat: both symbols are bound and exported, every
argument error is reported on the host, before any device work, with its status and a message that
names the function, and the Python surface checks dtype, length and schema hash before it touches a
buffer.  Host buffers stand in for device memory and are never dereferenced: every call fails
first."""
from __future__ import annotations

import ctypes

import numpy as np
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
    for name in ("fury_row_partition", "fury_row_concat"):
        assert name in N.SIGNATURES
        assert hasattr(L, name)
    assert N.PARTITION_MAX_PARTS == 65535 and N.CONCAT_MAX_SOURCES == 32
    with open(N.HERE + "/../include/fury_row.h") as f:
        header = f.read()
    assert "#define FURY_PARTITION_MAX_PARTS 65535" in header
    assert "#define FURY_CONCAT_MAX_SOURCES 32" in header


def test_partition_argument_errors(L, schemas):
    part, fn = L.fury_row_partition, "fury_row_partition"
    fixed, var = schemas["struct100"].handle, schemas["mixed"].handle
    r1, rows = _buf()
    r2, out = _buf()
    r3, aux = _buf()          # offsets / ids / part rows / indices / positions

    def call(s=fixed, rows=rows, ro=None, n=4, ids=aux, parts=3, out=out, cap=4096, oo=None,
             pr=aux, idx=None, pos=None):
        return part(s, rows, ro, n, ids, parts, out, cap, oo, pr, idx, pos, None)

    assert call(s=None) == INVALID
    assert "schema is null" in _err(fn)
    assert call(rows=None) == INVALID
    assert "rows is null" in _err(fn)
    assert call(ids=None) == INVALID
    assert "part_ids is null" in _err(fn)
    assert call(pr=None) == INVALID
    assert "out_part_rows is null" in _err(fn)
    assert call(pr=None, n=0, rows=None, ids=None) == INVALID          # even when empty
    assert "out_part_rows is null" in _err(fn)
    assert call(n=-1) == INVALID
    assert "nrows < 0" in _err(fn)
    for parts in (0, -1, 65536, 2 ** 31 - 1):
        assert call(parts=parts) == INVALID
        assert "num_parts" in _err(fn)
    assert call(cap=-8) == INVALID
    assert "out_capacity < 0" in _err(fn)
    assert call(rows=rows + 4) == INVALID
    assert "rows must be 8-byte aligned" in _err(fn)
    assert call(out=out + 4) == INVALID
    assert "out_rows must be 8-byte aligned" in _err(fn)
    assert call(ids=aux + 2) == INVALID
    assert "part_ids must be 4-byte aligned" in _err(fn)
    assert call(idx=aux + 4) == INVALID
    assert "8-byte aligned" in _err(fn)
    assert call(pos=aux + 4) == INVALID
    assert "8-byte aligned" in _err(fn)
    # variable-length rows need both offsets arrays, whatever the schema's shape
    for s in (var, schemas["foo"].handle, schemas["array"].handle):
        assert call(s=s, ro=None, oo=aux) == INVALID
        assert "row_offsets" in _err(fn)
        assert call(s=s, ro=aux, oo=None) == INVALID
        assert "out_offsets" in _err(fn)


def test_concat_argument_errors(L, schemas):
    from fury_amd import _native as N
    cat, fn = L.fury_row_concat, "fury_row_concat"
    fixed, var = schemas["struct100"].handle, schemas["mixed"].handle
    r1, rows = _buf()
    r2, out = _buf()
    r3, aux = _buf()

    def table(*srcs, size=None):
        tab = (N.FuryConcatSource * (size or max(len(srcs), 1)))()
        for k, (r, ro, n) in enumerate(srcs):
            tab[k].rows, tab[k].row_offsets, tab[k].nrows = r, ro, n
        return tab

    good = table((rows, aux, 2), (rows, aux, 1))
    assert cat(None, good, 2, out, 4096, aux, None) == INVALID
    assert "schema is null" in _err(fn)
    assert cat(var, None, 2, out, 4096, aux, None) == INVALID
    assert "source table is null" in _err(fn)
    big = table(*[(rows, aux, 1)] * 33)
    for count in (0, -1, 33):
        assert cat(var, big, count, out, 4096, aux, None) == INVALID
        assert "num_sources" in _err(fn)
    assert cat(var, table((rows, aux, 2), (rows, aux, -1)), 2, out, 4096, aux, None) == INVALID
    assert "source 1: nrows < 0" in _err(fn)
    assert cat(var, table((rows, aux, 2), (None, aux, 1)), 2, out, 4096, aux, None) == INVALID
    assert "source 1: rows is null" in _err(fn)
    assert cat(var, table((rows + 4, aux, 2)), 1, out, 4096, aux, None) == INVALID
    assert "source 0: rows must be 8-byte aligned" in _err(fn)
    assert cat(var, table((rows, aux, 2), (rows, None, 1)), 2, out, 4096, aux, None) == INVALID
    assert "source 1" in _err(fn) and "row_offsets" in _err(fn)
    for s in (schemas["foo"].handle, schemas["array"].handle):
        assert cat(s, table((rows, None, 1)), 1, out, 4096, aux, None) == INVALID
        assert "row_offsets" in _err(fn)
    assert cat(var, good, 2, out, -1, aux, None) == INVALID
    assert "out_capacity < 0" in _err(fn)
    assert cat(var, good, 2, out + 4, 4096, aux, None) == INVALID
    assert "out_rows must be 8-byte aligned" in _err(fn)
    assert cat(var, good, 2, out, 4096, None, None) == INVALID
    assert "out_offsets" in _err(fn)
    # N too large: the sum, and a sum that would overflow
    assert cat(var, table((rows, aux, 2 ** 38 - 1), (rows, aux, 1)), 2, out, 4096, aux,
               None) == INVALID
    assert "too large" in _err(fn)
    assert cat(var, table((rows, aux, 2 ** 63 - 1), (rows, aux, 2 ** 63 - 1)), 2, out, 4096, aux,
               None) == INVALID
    assert "too large" in _err(fn)
    assert cat(fixed, table((rows, None, 2 ** 50)), 1, None, 0, None, None) == INVALID
    assert "too large" in _err(fn)


def test_fixed_schema_capacity_is_checked_on_the_host(L, schemas):
    from fury_amd import _native as N
    fixed = schemas["struct100"].handle                     # 816-byte rows
    r1, rows = _buf()
    r2, out = _buf()
    r3, aux = _buf()
    # partition: the count is not known on the host, so the bound is nrows * fixed_size
    assert L.fury_row_partition(fixed, rows, None, 4, aux, 3, out, 4 * 816 - 8, None, aux, None,
                                None, None) == CAPACITY
    assert "4 rows of 816 bytes" in _err("fury_row_partition")
    assert L.fury_row_partition(fixed, rows, None, 4, aux, 3, out, 0, aux, aux, None, None,
                                None) == CAPACITY
    tab = (N.FuryConcatSource * 3)()
    for k, n in enumerate((2, 0, 3)):
        tab[k].rows, tab[k].row_offsets, tab[k].nrows = (rows if n else None), None, n
    assert L.fury_row_concat(fixed, tab, 3, out, 5 * 816 - 8, None, None) == CAPACITY
    assert "5 rows of 816 bytes" in _err("fury_row_concat")


def test_python_surface_checks_its_arguments():
    """partition / concat and their *_into / bind_* forms refuse a batch of another schema, ids of
    a wrong dtype and ids of a wrong length before they touch any buffer."""
    import torch

    from fury_amd.encoder import (ClassNotCompatibleException, Encoders, IllegalArgumentException,
                                  IndexOutOfBoundsException, RowBatch)
    enc = Encoders.bean(SCHEMAS["mixed"], device="cpu")
    foreign = RowBatch(None, None, 0, enc.schema_hash + 1)
    mine = RowBatch(None, None, 3, enc.schema_hash)
    for call in (lambda: enc.partition(foreign, [], 2),
                 lambda: enc.partition_into(foreign, [], 2, None, None, None),
                 lambda: enc.bind_partition(foreign, [], 2, None, None, None),
                 lambda: enc.slice_rows(foreign, 0, 0),
                 lambda: enc.concat([foreign]),
                 lambda: enc.concat([mine, foreign]),
                 lambda: enc.concat_into([mine, foreign], None, None)):
        with pytest.raises(ClassNotCompatibleException, match="Schema is not consistent"):
            call()
    for ids in ([0.0, 1.0, 2.0], np.array([True, False, True]), torch.zeros(3),
                torch.zeros(3, dtype=torch.bool), torch.zeros(3, dtype=torch.bfloat16)):
        for call in (lambda: enc.partition(mine, ids, 2),
                     lambda: enc.partition_into(mine, ids, 2, None, None, None),
                     lambda: enc.bind_partition(mine, ids, 2, None, None, None)):
            with pytest.raises(IllegalArgumentException, match="part_ids must be"):
                call()
    for ids in ([0, 1], np.zeros(4, np.int32), torch.zeros(0, dtype=torch.int64)):
        with pytest.raises(IllegalArgumentException, match="entries for 3 rows"):
            enc.partition_into(mine, ids, 2, None, None, None)
    with pytest.raises(IndexOutOfBoundsException):
        enc.slice_rows(mine, 2, 4)
    with pytest.raises(IndexOutOfBoundsException):
        enc.slice_rows(mine, 2, 1)


def test_part_ids_outside_int32_drop_instead_of_wrapping():
    from fury_amd.encoder import Encoders
    enc = Encoders.bean(SCHEMAS["mixed"], device="cpu")
    wide = [0, 2 ** 32, 2 ** 32 + 1, -2 ** 32, 2 ** 31, -2 ** 31, 2 ** 31 - 1, -2 ** 31 - 1]
    want = [0, -1, -1, -1, -1, -2 ** 31, 2 ** 31 - 1, -1]
    ids = enc._part_ids(np.array(wide, np.int64), len(wide), None)
    assert str(ids.dtype) == "torch.int32" and ids.tolist() == want
    ids = enc._part_ids(np.array([0, 2 ** 31, 2 ** 64 - 1, 5], np.uint64), 4, None)
    assert ids.tolist() == [0, -1, -1, 5]
    ids = enc._part_ids(np.array([0, 2 ** 32 - 1, 7], np.uint32), 3, None)
    assert ids.tolist() == [0, -1, 7]
    ids = enc._part_ids(np.array([3, 255], np.uint8), 2, None)
    assert ids.tolist() == [3, 255]
