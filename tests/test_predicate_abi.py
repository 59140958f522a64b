"""CPU checks of fury_row_predicate: the symbol is bound and exported, the header carries the eight
numbered rules and the constants, every argument error of rule 8 is reported on the host, before any
device work, with its status and a message that names the function, unsupported (op, type) pairs name
their route, the call without rows and without a count returns FURY_OK, and fury_amd.predicate turns
Python values into the literals of rule 2.  Host buffers stand in for device memory and are never
dereferenced: every call fails first, or has no row to read."""
from __future__ import annotations

import ctypes
import decimal
import re
import struct

import pytest

from fury_amd import types as T
from fury_amd.workloads import SCHEMAS

OK, INVALID, UNSUPPORTED = 0, 1, 2
IS_NULL, EQ, LT, LE, GT, GE, STARTS_WITH, ENDS_WITH, CONTAINS = range(1, 10)
NOT, OR = 1, 2


def _buf(nbytes=8192, align=64):
    raw = ctypes.create_string_buffer(nbytes + align)
    base = (ctypes.addressof(raw) + align - 1) & ~(align - 1)
    return raw, base


@pytest.fixture(scope="module")
def L():
    from fury_amd import _native as N
    return N.lib()


EVERY = [T.field("i8", T.INT8), T.field("i16", T.INT16), T.field("i32", T.INT32), T.field("i64", T.INT64),
         T.field("f32", T.FLOAT32), T.field("f64", T.FLOAT64), T.field("b", T.BOOL), T.field("d32", T.DATE32),
         T.field("ts", T.TIMESTAMP), T.field("dec", T.DECIMAL), T.field("s", T.STRING), T.field("bin", T.BINARY),
         T.field("l", T.LIST, True, [T.field("item", T.INT32)]),
         T.field("st", T.STRUCT, True, [T.field("x", T.INT32)])]
WIDTHS = {"i8": 1, "i16": 2, "i32": 4, "i64": 8, "f32": 4, "f64": 8, "b": 1, "d32": 4, "ts": 8, "dec": 16}


@pytest.fixture(scope="module")
def schemas():
    from fury_amd.encoder import Encoders, Schema
    arr = Encoders.array_encoder(T.field("item", T.INT64), device="cpu")
    return {"struct100": Schema(SCHEMAS["struct100"]), "mixed": Schema(SCHEMAS["mixed"]),
            "every": Schema(EVERY), "names": [f.name for f in EVERY], "array": arr.schema(), "_keep": arr}


def _err():
    from fury_amd import _native as N
    msg = N.last_error()
    assert msg.startswith("fury_row_predicate"), msg
    return msg


_LITS: list = []


def _terms(*recs):
    """recs: (field, op, flags, literal bytes or None[, literal_len[, reserved]]) tuples."""
    from fury_amd import _native as N
    arr = (N.FuryPredTerm * max(len(recs), 1))()
    for j, rec in enumerate(recs):
        field, op, flags, lit = rec[:4]
        arr[j].field, arr[j].op, arr[j].flags = field, op, flags
        if lit:
            buf = ctypes.create_string_buffer(lit, len(lit))
            _LITS.append(buf)
            arr[j].literal = ctypes.addressof(buf)
        arr[j].literal_len = rec[4] if len(rec) > 4 else len(lit or b"")
        arr[j].reserved = rec[5] if len(rec) > 5 else 0
    return arr


def test_symbol_rules_and_constants(L):
    from fury_amd import _native as N
    assert "fury_row_predicate" in N.SIGNATURES and len(N.SIGNATURES["fury_row_predicate"][1]) == 10
    assert hasattr(L, "fury_row_predicate")
    assert L.fury_abi_version() == 1
    assert ctypes.sizeof(N.FuryPredTerm) == 32
    with open(N.HERE + "/../include/fury_row.h") as f:
        header = f.read()
    assert "int fury_row_predicate(const fury_schema* schema" in header
    at = header.index("WHERE masks")
    doc = header[at:header.index("int fury_row_predicate(", at)]
    for rule in ("1. Shape.", "2. Fields and literals.", "3. Comparison ops.", "4. Pattern ops", "5. Nulls.",
                 "6. Outputs.", "7. Bounds", "8. Argument checks", "three-valued WHERE", "totalOrder",
                 "does not match -0.0", "a positive NaN is GT", "search_sorted", "An empty literal matches every",
                 "row_mask == out_mask", "nrows == 0 writes *out_count = 0", "does not depend on short-circuiting",
                 "never synchronises with the host", "allocates no workspace", "fury_row_project / fury_row_extract"):
        assert rule in doc, rule
    for name, value in (("IS_NULL", 1), ("EQ", 2), ("LT", 3), ("LE", 4), ("GT", 5), ("GE", 6), ("STARTS_WITH", 7),
                        ("ENDS_WITH", 8), ("CONTAINS", 9), ("NOT", 1), ("OR", 2), ("MAX_TERMS", 32),
                        ("MAX_LITERAL_BYTES", 2048)):
        assert re.search(rf"#define FURY_PRED_{name} +{value}\b", doc), name
    assert N.PRED_OPS == {"is_null": 1, "eq": 2, "lt": 3, "le": 4, "gt": 5, "ge": 6, "starts_with": 7,
                          "ends_with": 8, "contains": 9}
    assert (N.PRED_NOT, N.PRED_OR, N.PRED_MAX_TERMS, N.PRED_MAX_LITERAL_BYTES) == (1, 2, 32, 2048)
    for member in ("int32_t field;", "int32_t op;", "int32_t flags;", "int32_t reserved;", "const void* literal;",
                   "int64_t literal_len;"):
        assert member in doc, member


def test_argument_errors(L, schemas):
    fixed, var = schemas["struct100"].handle, schemas["mixed"].handle
    r1, rows = _buf()
    r2, out = _buf()
    r3, aux = _buf()
    i64 = struct.pack("<q", 7)
    one = _terms((0, EQ, 0, i64))

    def call(s=fixed, rows=rows, ro=None, n=4, terms=one, nt=1, rm=None, om=out, oc=None):
        return L.fury_row_predicate(s, rows, ro, n, terms, nt, rm, om, oc, None)

    assert call(s=None) == INVALID
    assert "schema is null" in _err()
    assert call(n=-1) == INVALID
    assert "nrows < 0" in _err()
    assert call(terms=None) == INVALID
    assert "terms is null" in _err()
    assert call(s=schemas["array"].handle) == UNSUPPORTED
    assert "collection schema" in _err()
    # 1 <= num_terms <= FURY_PRED_MAX_TERMS
    for nt in (0, -1, 33):
        assert call(nt=nt) == INVALID
        assert f"num_terms {nt} is not in [1, 32]" in _err()
    most = _terms(*[(j, EQ, OR if j else 0, i64) for j in range(32)])
    assert call(terms=most, nt=32, rows=None) == INVALID                # 32 pass
    assert "rows is null" in _err()
    # op, flags, reserved, OR on the first term, field
    for op in (0, 10, -1):
        assert call(terms=_terms((0, op, 0, i64))) == INVALID
        assert f"terms[0]: unknown op {op}" in _err()
    for flags in (4, 7, -1):
        assert call(terms=_terms((0, EQ, 0, i64), (1, EQ, flags, i64)), nt=2) == INVALID
        assert f"terms[1]: unknown flags {flags}" in _err()
    assert call(terms=_terms((0, EQ, 0, i64, 8, 5))) == INVALID
    assert "terms[0]: reserved is 5, not 0" in _err()
    for flags in (OR, OR | NOT):
        assert call(terms=_terms((0, EQ, flags, i64))) == INVALID
        assert "terms[0]: FURY_PRED_OR on the first term" in _err()
    assert call(terms=_terms((0, EQ, NOT, i64), (1, EQ, OR | NOT, i64)), nt=2, rows=None) == INVALID    # valid flags
    assert "rows is null" in _err()
    for field in (100, -1):
        assert call(terms=_terms((0, EQ, 0, i64), (field, EQ, 0, i64)), nt=2) == INVALID
        assert f"terms[1]: field {field} is not a field of the schema" in _err()
    # the literal: length, pointer, pool
    for n in (0, 4, 9):
        assert call(terms=_terms((0, EQ, 0, i64, n))) == INVALID
        assert f"literal_len {n}, 8 needed" in _err()
    assert call(terms=_terms((0, IS_NULL, 0, i64))) == INVALID
    assert "literal_len 8, 0 needed: IS_NULL takes no literal" in _err()
    assert call(terms=_terms((0, EQ, 0, None, 8))) == INVALID
    assert "terms[0]: literal is null" in _err()
    s1 = [f.name for f in SCHEMAS["mixed"]].index("s1")
    assert call(s=var, ro=aux, terms=_terms((s1, EQ, 0, b"x", -1))) == INVALID
    assert "terms[0]: literal_len < 0" in _err()
    assert call(s=var, ro=aux, terms=_terms((s1, EQ, 0, None, 3))) == INVALID
    assert "terms[0]: literal is null" in _err()
    full = _terms((s1, CONTAINS, 0, b"x" * 1000), (s1, EQ, 0, b"y" * 1033), (s1, STARTS_WITH, 0, b""))
    assert call(s=var, ro=aux, terms=full, nt=3, rows=None) == INVALID   # 1000 + 1040 + 0 <= 2048 pass
    assert "rows is null" in _err()
    over = _terms((s1, CONTAINS, 0, b"x" * 1000), (s1, EQ, 0, b"y" * 1049))
    assert call(s=var, ro=aux, terms=over, nt=2) == INVALID             # 1000 + 1056
    assert "terms[1]: the literals take more than 2048 bytes" in _err()
    assert call(s=var, ro=aux, terms=_terms((s1, EQ, 0, b"z" * 2049))) == INVALID
    assert "terms[0]: the literals take more than 2048 bytes" in _err()
    assert call(s=var, ro=aux, terms=_terms((s1, EQ, 0, b"z" * 2048)), rows=None) == INVALID    # exactly the limit
    assert "rows is null" in _err()
    # the outputs and the masks
    assert call(om=None) == INVALID
    assert "out_mask is null" in _err()
    assert call(om=None, n=0) == INVALID
    assert "out_mask is null" in _err()
    for rm, om in ((aux + 2, out), (None, out + 2)):
        assert call(rm=rm, om=om) == INVALID
        assert "row_mask / out_mask must be 4-byte aligned" in _err()
    assert call(oc=aux + 4) == INVALID
    assert "row_offsets / out_count must be 8-byte aligned" in _err()
    assert call(s=var, ro=aux + 4, terms=_terms((s1, EQ, 0, b"x"))) == INVALID
    assert "row_offsets / out_count must be 8-byte aligned" in _err()
    assert call(rm=out, om=out, rows=None) == INVALID                   # in place passes the checks
    assert "rows is null" in _err()
    # the batch
    assert call(n=2 ** 39) == INVALID
    assert "batch too large" in _err()
    assert call(n=2 ** 39 - 256, rows=None) == INVALID
    assert "rows is null" in _err()
    assert call(rows=rows + 4) == INVALID
    assert "rows must be 8-byte aligned" in _err()
    assert call(s=var, ro=None, terms=_terms((s1, EQ, 0, b"x"))) == INVALID
    assert "variable-length rows need row_offsets" in _err()
    assert call(ro=None, rows=None) == INVALID                          # a fixed schema needs no row_offsets
    assert "rows is null" in _err()


def test_unsupported_pairs_name_their_route(L, schemas):
    s, names = schemas["every"].handle, schemas["names"]
    r1, rows = _buf()
    r2, out = _buf()

    def call(field, op, lit, rows=rows):
        return L.fury_row_predicate(s, rows, out, 4, _terms((names.index(field), op, 0, lit)), 1, None, out, None, None)

    for field in ("l", "st"):
        for op, lit in ((IS_NULL, None), (EQ, b"abcd"), (CONTAINS, b"a")):
            assert call(field, op, lit) == UNSUPPORTED, (field, op)
            msg = _err()
            assert f"on field {names.index(field)} ({field})" in msg and "LIST / STRUCT / MAP" in msg
            assert "fury_row_project / fury_row_extract" in msg
    for op, name in ((STARTS_WITH, "STARTS_WITH"), (ENDS_WITH, "ENDS_WITH"), (CONTAINS, "CONTAINS")):
        for field, w in WIDTHS.items():
            assert call(field, op, b"\1" * w) == UNSUPPORTED, (field, op)
            msg = _err()
            assert f"{name} on field {names.index(field)} ({field})" in msg and "take STRING / BINARY fields" in msg
    # every supported pair passes the type checks: the next check (rows) fails instead
    for op in (EQ, LT, LE, GT, GE):
        for field, w in WIDTHS.items():
            assert call(field, op, b"\1" * w, rows=None) == INVALID, (field, op)
            assert "rows is null" in _err()
            assert call(field, op, b"\1" * (w + 1)) == INVALID
            assert f"literal_len {w + 1}, {w} needed" in _err()
    for op in range(EQ, CONTAINS + 1):
        for field in ("s", "bin"):
            for lit in (b"", b"abc", b"x" * 100):
                assert call(field, op, lit, rows=None) == INVALID, (field, op)
                assert "rows is null" in _err()
    for field in names[:12]:
        assert call(field, IS_NULL, None, rows=None) == INVALID
        assert "rows is null" in _err()


def test_no_rows(L, schemas):
    """nrows == 0 with out_count == NULL returns FURY_OK without touching a buffer: rows and row_offsets
    may be NULL, and out_mask keeps its contents."""
    fixed, var = schemas["struct100"].handle, schemas["mixed"].handle
    raw, out = _buf(64)
    ctypes.memset(out, 0xAB, 64)
    s1 = [f.name for f in SCHEMAS["mixed"]].index("s1")
    assert L.fury_row_predicate(fixed, None, None, 0, _terms((0, EQ, 0, struct.pack("<q", 1))), 1, None, out, None,
                                None) == OK
    assert L.fury_row_predicate(var, None, None, 0, _terms((s1, CONTAINS, NOT, b"abc")), 1, out + 32, out, None,
                                None) == OK
    assert ctypes.string_at(out, 64) == b"\xab" * 64


# ---- fury_amd.predicate: terms and literals ---------------------------------------------------------------------------
def _field(tid):
    return next(f for f in EVERY if f.type_id == tid)


def test_literal_conversion():
    from fury_amd.predicate import literal_bytes as lit
    assert lit(_field(T.INT8), "eq", -128) == b"\x80" and lit(_field(T.INT16), "lt", 258) == b"\x02\x01"
    assert lit(_field(T.INT32), "ge", -2) == b"\xfe\xff\xff\xff" and lit(_field(T.DATE32), "le", 1) == b"\1\0\0\0"
    assert lit(_field(T.INT64), "gt", 2 ** 63 - 1) == b"\xff" * 7 + b"\x7f"
    assert lit(_field(T.TIMESTAMP), "eq", -1) == b"\xff" * 8
    assert lit(_field(T.FLOAT32), "eq", 1.5) == struct.pack("<f", 1.5)
    assert lit(_field(T.FLOAT64), "eq", -0.0) == struct.pack("<d", -0.0) and lit(_field(T.FLOAT64), "lt", 3) == struct.pack("<d", 3.0)
    assert lit(_field(T.FLOAT32), "eq", float("inf")) == struct.pack("<f", float("inf"))
    assert lit(_field(T.BOOL), "eq", True) == b"\1" and lit(_field(T.BOOL), "eq", False) == b"\0"
    assert lit(_field(T.DECIMAL), "eq", -1) == b"\xff" * 16
    assert lit(_field(T.DECIMAL), "le", decimal.Decimal("123.45")) == (12345).to_bytes(16, "little")
    assert lit(_field(T.DECIMAL), "le", decimal.Decimal("-0.07")) == (-7).to_bytes(16, "little", signed=True)
    assert lit(_field(T.DECIMAL), "eq", 1 << 100) == (1 << 100).to_bytes(16, "little")
    # the Decimal's own digits are the unscaled value: it is written at the column's scale
    assert lit(_field(T.DECIMAL), "eq", decimal.Decimal("1.50")) == (150).to_bytes(16, "little")
    assert lit(_field(T.DECIMAL), "eq", decimal.Decimal("1.5").quantize(decimal.Decimal("0.01"))) == \
        (150).to_bytes(16, "little")
    assert lit(_field(T.DECIMAL), "eq", decimal.Decimal("100")) == (100).to_bytes(16, "little")
    assert lit(_field(T.STRING), "eq", "héllo") == "héllo".encode() and lit(_field(T.STRING), "contains", b"\xff") == b"\xff"
    assert lit(_field(T.BINARY), "starts_with", b"") == b"" and lit(_field(T.BINARY), "eq", bytearray(b"ab")) == b"ab"
    for tid in (T.INT8, T.STRING, T.DECIMAL, T.BOOL):
        assert lit(_field(tid), "is_null", None) == b""


def test_literal_conversion_errors():
    from fury_amd.encoder import IllegalArgumentException, UnsupportedOperationException
    from fury_amd.predicate import literal_bytes as lit
    bad = [(T.INT8, "eq", 128), (T.INT8, "eq", -129), (T.INT16, "eq", 1 << 15), (T.INT32, "lt", 1 << 31),
           (T.INT64, "gt", 1 << 63), (T.DATE32, "eq", -(1 << 31) - 1), (T.INT32, "eq", 1.0), (T.INT32, "eq", "1"),
           (T.INT32, "eq", True), (T.INT64, "eq", None), (T.FLOAT32, "eq", "1.0"), (T.FLOAT32, "eq", 1e39),
           (T.FLOAT64, "eq", True), (T.FLOAT64, "eq", b"x"), (T.BOOL, "eq", 1), (T.BOOL, "eq", "true"),
           (T.DECIMAL, "eq", 1.5), (T.DECIMAL, "eq", 1 << 127), (T.DECIMAL, "eq", decimal.Decimal("NaN")),
           (T.DECIMAL, "eq", decimal.Decimal("1E+2")),
           (T.DECIMAL, "eq", "1"), (T.STRING, "eq", 5), (T.STRING, "contains", None), (T.BINARY, "eq", 1.0),
           (T.STRING, "is_null", "x"), (T.INT32, "like", 1)]
    for tid, op, value in bad:
        with pytest.raises(IllegalArgumentException):
            lit(_field(tid), op, value)
    for tid, op, value in ((T.INT32, "contains", 1), (T.DECIMAL, "starts_with", 1), (T.BOOL, "ends_with", True),
                           (T.LIST, "is_null", None), (T.STRUCT, "eq", 1)):
        with pytest.raises(UnsupportedOperationException):
            lit(_field(tid), op, value)


def test_terms_and_clauses():
    from fury_amd import _native as N
    from fury_amd import predicate as P
    from fury_amd.encoder import Encoders, IllegalArgumentException
    import fury_amd
    for name in fury_amd._PREDICATE:
        assert getattr(fury_amd, name) is getattr(P, name) and name in fury_amd.__all__
    assert P.ne("a", 1) == P.Term("a", "eq", 1, True) and P.not_null("a") == P.Term("a", "is_null", None, True)
    assert [t.op for t in (P.eq(0, 1), P.lt(0, 1), P.le(0, 1), P.gt(0, 1), P.ge(0, 1), P.is_null(0),
                           P.starts_with(0, ""), P.ends_with(0, ""), P.contains(0, ""))] == list(N.PRED_OPS)[1:6] + \
        ["is_null", "starts_with", "ends_with", "contains"]
    flat = P._flatten([P.between("a", 1, 5), (P.eq("s1", "x"), P.is_null("s1")), P.ne("b", 3)])
    assert [(t.op, t.negate, j) for t, j in flat] == [("ge", False, False), ("le", False, False), ("eq", False, False),
                                                     ("is_null", False, True), ("eq", True, False)]
    assert P._flatten(P.eq("a", 1)) == [(P.eq("a", 1), False)] and len(P._flatten(P.between("a", 1, 2))) == 2
    enc = Encoders.bean(SCHEMAS["mixed"], device="cpu")
    keep: list = []
    recs, n = P._c_terms(enc, [P.between("a", 1, 5), (P.eq("s1", "xyz"), P.not_null(4))], keep)
    assert n == 4
    assert [(r.field, r.op, r.flags, r.literal_len, r.reserved) for r in recs] == \
        [(0, 5 + 1, 0, 4, 0), (0, 4, 0, 4, 0), (3, 2, 0, 3, 0), (4, 1, N.PRED_NOT | N.PRED_OR, 0, 0)]
    assert ctypes.string_at(recs[0].literal, 4) == b"\1\0\0\0" and ctypes.string_at(recs[2].literal, 3) == b"xyz"
    assert recs[3].literal is None
    for bad in ([], [()], [P.eq("nope", 1)], [P.eq(17, 1)], ["a"], [[P.between("a", 1, 2)]], [P.eq("a", 1)] * 33,
                [P.contains("s1", "x" * 1025), P.contains("s2", "y" * 1025)]):
        with pytest.raises(IllegalArgumentException):
            P._c_terms(enc, bad, [])
    P._c_terms(enc, [P.contains("s1", "x" * 1024), P.contains("s2", "y" * 1024)], [])
    P._c_terms(enc, [P.eq("a", 1)] * 32, [])
