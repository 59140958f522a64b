"""CPU checks of fury_row_aggregate: the symbol is bound and exported, the header carries the eight
numbered rules and the constants, every argument error of rule 8 is reported on the host, before any
device work, with its status and a message that names the function, unsupported (op, type) pairs name
their route, and the call without groups returns FURY_OK.  Host buffers stand in for device memory and
are never dereferenced: every call fails first, or has no group to write."""
from __future__ import annotations

import ctypes

import pytest

from fury_amd.workloads import SCHEMAS

OK, INVALID, UNSUPPORTED = 0, 1, 2
COUNT, SUM, MIN, MAX, ARGMIN, ARGMAX = 1, 2, 3, 4, 5, 6


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
    every = [T.field("i8", T.INT8), T.field("i64", T.INT64), T.field("f32", T.FLOAT32), T.field("f64", T.FLOAT64),
             T.field("b", T.BOOL), T.field("d32", T.DATE32), T.field("ts", T.TIMESTAMP), T.field("dec", T.DECIMAL),
             T.field("s", T.STRING), T.field("bin", T.BINARY), T.field("l", T.LIST, True, [T.field("item", T.INT32)])]
    return {"struct100": Schema(SCHEMAS["struct100"]), "mixed": Schema(SCHEMAS["mixed"]),
            "every": Schema(every), "names": [f.name for f in every], "array": arr.schema(), "_keep": arr}


def _err():
    from fury_amd import _native as N
    msg = N.last_error()
    assert msg.startswith("fury_row_aggregate"), msg
    return msg


def _aggs(*recs):
    """recs: (field, op, out, out_count) tuples."""
    from fury_amd import _native as N
    arr = (N.FuryAgg * max(len(recs), 1))()
    for j, (field, op, out, cnt) in enumerate(recs):
        arr[j].field, arr[j].op, arr[j].out, arr[j].out_count = field, op, out, cnt
    return arr


def test_symbol_rules_and_constants(L):
    from fury_amd import _native as N
    assert "fury_row_aggregate" in N.SIGNATURES and len(N.SIGNATURES["fury_row_aggregate"][1]) == 9
    assert hasattr(L, "fury_row_aggregate") and hasattr(L, "fury_row_aggregate_lds_cells")
    assert L.fury_abi_version() == 1
    assert ctypes.sizeof(N.FuryAgg) == 24
    with open(N.HERE + "/../include/fury_row.h") as f:
        header = f.read()
    assert "int fury_row_aggregate(const fury_schema* schema" in header
    at = header.index("Per-group aggregates")
    doc = header[at:header.index("int fury_row_aggregate(", at)]
    for rule in ("1. Groups.", "2. Values and nulls.", "3. SUM.", "4. MIN / MAX", "5. ARGMIN / ARGMAX",
                 "6. Writes.", "7. Bounds", "8. Argument checks", "Workspace", "24 bytes per group and aggregate",
                 "(m - 1) * 2^-52", "never synchronises with the host"):
        assert rule in doc, rule
    import re
    for name, value in (("COUNT", 1), ("SUM", 2), ("MIN", 3), ("MAX", 4), ("ARGMIN", 5), ("ARGMAX", 6),
                        ("MAX_AGGS", 16)):
        assert re.search(rf"#define FURY_AGG_{name} +{value}\b", doc), name
    assert N.AGG_OPS == {"count": 1, "sum": 2, "min": 3, "max": 4, "argmin": 5, "argmax": 6}
    assert N.AGG_MAX_AGGS == 16
    for member in ("int32_t field;", "int32_t op;", "void* out;", "int64_t* out_count;"):
        assert member in doc, member


def test_argument_errors(L, schemas):
    fixed, var = schemas["struct100"].handle, schemas["mixed"].handle
    r1, rows = _buf()
    r2, out = _buf()
    r3, aux = _buf()
    one = _aggs((0, SUM, out, None))

    def call(s=fixed, rows=rows, ro=None, n=4, ids=aux, G=3, aggs=one, na=1):
        return L.fury_row_aggregate(s, rows, ro, n, ids, G, aggs, na, None)

    assert call(s=None) == INVALID
    assert "schema is null" in _err()
    assert call(n=-1) == INVALID
    assert "nrows < 0" in _err()
    assert call(aggs=None) == INVALID
    assert "aggs is null" in _err()
    assert call(s=schemas["array"].handle) == UNSUPPORTED
    assert "collection schema" in _err()
    # 1 <= num_aggs <= FURY_AGG_MAX_AGGS
    for na in (0, -1, 17):
        assert call(na=na) == INVALID
        assert f"num_aggs {na} is not in [1, 16]" in _err()
    sixteen = _aggs(*[(j, COUNT, out + 8 * j, None) for j in range(16)])
    assert call(aggs=sixteen, na=16, rows=None) == INVALID              # 16 pass
    assert "rows is null" in _err()
    # the group count and the row count
    assert call(G=-1) == INVALID
    assert "num_groups < 0" in _err()
    assert call(G=2 ** 31) == INVALID
    assert "num_groups 2147483648 > 2^31 - 1" in _err()
    for n in (2 ** 31, 2 ** 40):
        assert call(n=n) == INVALID
        assert "batch too large" in _err()
    assert call(G=2 ** 31 - 1, rows=None) == INVALID                    # the largest count passes
    assert "rows is null" in _err()
    assert call(ids=None, G=2) == INVALID
    assert "group_ids is null: num_groups must be 1, not 2" in _err()
    assert call(ids=None, G=0) == INVALID
    _err()
    assert call(ids=None, G=1, rows=None) == INVALID                    # NULL ids with one group pass
    assert "rows is null" in _err()
    # field range and op range
    for op in (0, 7, -1):
        assert call(aggs=_aggs((0, op, out, None))) == INVALID
        assert f"aggs[0]: unknown op {op}" in _err()
    assert call(aggs=_aggs((0, SUM, out, None), (100, SUM, out + 8, None)), na=2) == INVALID
    assert "aggs[1]: field 100 is not a field of the schema" in _err()
    assert call(aggs=_aggs((-2, COUNT, out, None))) == INVALID
    assert "aggs[0]: field -2 is not a field" in _err()
    assert call(aggs=_aggs((-1, SUM, out, None))) == INVALID            # -1 is COUNT(*) only
    assert "aggs[0]: field -1 is not a field" in _err()
    assert call(aggs=_aggs((-1, COUNT, out, None)), rows=None) == INVALID
    assert "rows is null" in _err()
    # required out, alignment, distinct outputs
    assert call(aggs=_aggs((0, SUM, None, aux))) == INVALID
    assert "aggs[0].out is null" in _err()
    assert call(aggs=_aggs((0, SUM, None, None)), G=0) == INVALID       # even without groups
    assert "aggs[0].out is null" in _err()
    for o, c in ((out + 4, None), (out, aux + 4)):
        assert call(aggs=_aggs((0, SUM, out + 64, None), (1, SUM, o, c)), na=2) == INVALID
        msg = _err()
        assert "aggs[1]: out / out_count must be 8-byte aligned" in msg
    for second in ((1, SUM, out, None), (1, SUM, out + 8, out), (1, COUNT, out + 8, out + 16)):
        bad = call(aggs=_aggs((0, SUM, out, out + 16), second), na=2)
        assert bad == INVALID
        assert "aggs[1]: two outputs of one call are the same pointer" in _err()
    assert call(aggs=_aggs((0, SUM, out, out))) == INVALID
    assert "same pointer" in _err()
    assert call(ids=aux + 4) == INVALID
    assert "row_offsets / group_ids must be 8-byte aligned" in _err()
    # the batch
    assert call(rows=None) == INVALID
    assert "rows is null" in _err()
    assert call(rows=rows + 4) == INVALID
    assert "rows must be 8-byte aligned" in _err()
    a = [f.name for f in SCHEMAS["mixed"]].index("a")
    assert call(s=var, aggs=_aggs((a, COUNT, out, None)), ro=None) == INVALID
    assert "variable-length rows need row_offsets" in _err()
    assert call(s=var, aggs=_aggs((a, COUNT, out, None)), ro=aux + 4) == INVALID
    assert "must be 8-byte aligned" in _err()
    assert call(n=2 ** 31, aggs=_aggs((0, SUM, None, None))) == INVALID     # the size checks come first
    assert "batch too large" in _err()


def test_unsupported_pairs_name_their_route(L, schemas):
    s, names = schemas["every"].handle, schemas["names"]
    r1, rows = _buf()
    r2, out = _buf()

    def call(field, op):
        return L.fury_row_aggregate(s, rows, rows, 4, rows, 3, _aggs((names.index(field), op, out, None)), 1, None)

    for field in ("b", "d32", "ts", "dec", "s", "bin", "l"):
        assert call(field, SUM) == UNSUPPORTED, field
        msg = _err()
        assert f"SUM of field {names.index(field)} ({field})" in msg
        assert "DECIMAL sums are out of scope" in msg and "BOOL sum is the COUNT" in msg
    for op, name in ((MIN, "MIN"), (MAX, "MAX")):
        for field in ("dec", "s", "bin", "l"):
            assert call(field, op) == UNSUPPORTED, field
            msg = _err()
            assert f"{name} of field {names.index(field)} ({field})" in msg
            assert "ARGMIN / ARGMAX" in msg and "fury_row_take" in msg
    for op in (ARGMIN, ARGMAX):
        assert call("l", op) == UNSUPPORTED
        assert "LIST / STRUCT / MAP" in _err()
    # every supported pair passes the type checks: the next check (rows) fails instead
    supported = {SUM: ("i8", "i64", "f32", "f64"), MIN: ("i8", "i64", "f32", "f64", "b", "d32", "ts"),
                 ARGMAX: ("i8", "f32", "b", "d32", "ts", "dec", "s", "bin"), COUNT: tuple(names)}
    for op, fields in supported.items():
        for field in fields:
            st = L.fury_row_aggregate(s, None, rows, 4, rows, 3, _aggs((names.index(field), op, out, None)), 1, None)
            assert st == INVALID, (op, field)
            assert "rows is null" in _err()


def test_no_groups_is_a_no_op(L, schemas):
    """num_groups == 0 returns FURY_OK without touching a buffer: rows and row_offsets may be NULL
    when there are no rows, and the outputs keep their contents."""
    fixed, var = schemas["struct100"].handle, schemas["mixed"].handle
    raw, out = _buf(64)
    ctypes.memset(out, 0xAB, 64)
    a = [f.name for f in SCHEMAS["mixed"]].index("a")
    aggs = _aggs((-1, COUNT, out, out + 8), (0, ARGMIN, out + 16, None))
    assert L.fury_row_aggregate(fixed, None, None, 0, out + 32, 0, aggs, 2, None) == OK
    assert L.fury_row_aggregate(var, None, None, 0, out + 32, 0, _aggs((a, COUNT, out, None)), 1, None) == OK
    assert L.fury_row_aggregate(fixed, out + 32, None, 4, out + 32, 0, aggs, 2, None) == OK     # rows, no groups
    assert ctypes.string_at(out, 64) == b"\xab" * 64
    assert L.fury_row_aggregate_lds_cells() == 2048
