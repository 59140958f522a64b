"""A Python model of fury_row_predicate, written from rules 1-6 of include/fury_row.h alone over
decoded values (the value bytes of a field, None for a null), and its pins without a GPU: the
comparison ops against tests/test_order_model.py's compare_model on every pair of its value table,
the pattern ops against Python's bytes.startswith / bytes.endswith / in, the null rule, and the
clause shape.  The GPU tests (tests/test_predicate.py) compare the kernel with this model applied to
the oracle's decode."""
from __future__ import annotations

import itertools
import struct

import numpy as np
import pytest

from fury_amd import types as T
from tests import test_order_model as M

IS_NULL, EQ, LT, LE, GT, GE, STARTS_WITH, ENDS_WITH, CONTAINS = range(1, 10)
NOT, OR = 1, 2
COMPARISONS = (EQ, LT, LE, GT, GE)
PATTERNS = (STARTS_WITH, ENDS_WITH, CONTAINS)
SIGNED = (T.INT8, T.INT16, T.INT32, T.INT64, T.DATE32, T.TIMESTAMP, T.DECIMAL)
FLOATS = (T.FLOAT32, T.FLOAT64)
BYTES = (T.STRING, T.BINARY)


# ---- rule 3: the order of a value against the literal ---------------------------------------------------------------
def _rank(tid, v: bytes):
    """A Python object whose own order is rule 3 of fury_row_compare for the value bytes v."""
    if tid == T.BOOL:
        return int(v[0] != 0)
    if tid in SIGNED:
        return int.from_bytes(v, "little", signed=True)
    if tid in FLOATS:                             # totalOrder: negative values all bits flipped, others the sign set
        bits, top = int.from_bytes(v, "little"), 1 << (8 * len(v) - 1)
        return (~bits & (2 * top - 1)) if bits & top else bits | top
    assert tid in BYTES, tid
    return bytes(v)                               # unsigned bytes, a proper prefix smaller


def term_true(tid, v, op, flags, literal) -> bool:
    """Rules 3-5 for one term: v = the field's value bytes or None."""
    negate = bool(flags & NOT)
    if op == IS_NULL:
        return (v is None) != negate
    if v is None:                                 # rule 5: never true, with or without NOT
        return False
    if op in COMPARISONS:
        x, y = _rank(tid, v), _rank(tid, literal)
        test = {EQ: x == y, LT: x < y, LE: x <= y, GT: x > y, GE: x >= y}[op]
    else:
        assert tid in BYTES and op in PATTERNS, (tid, op)
        v, m = bytes(v), len(literal)
        if op == STARTS_WITH:
            test = len(v) >= m and v[:m] == literal
        elif op == ENDS_WITH:
            test = len(v) >= m and v[len(v) - m:] == literal
        else:
            test = any(v[o:o + m] == literal for o in range(len(v) - m + 1))
    return test != negate


def row_passes(terms, values) -> bool:
    """Rule 1.  terms: (field, type id, op, flags, literal); values: the row's value per field."""
    clauses = []
    for j, (field, tid, op, flags, lit) in enumerate(terms):
        tv = term_true(tid, values[field], op, flags, lit)
        if flags & OR:
            assert j > 0, "FURY_PRED_OR on the first term"
            clauses[-1] = clauses[-1] or tv
        else:
            clauses.append(tv)
    return all(clauses)


def mask_model(terms, rows, examine=None):
    """(out_mask words as uint32, count) of rule 6 over the rows' value lists; `examine`: row_mask bits."""
    bits = [bool((examine is None or examine[i]) and row_passes(terms, r)) for i, r in enumerate(rows)]
    padded = np.zeros(((len(rows) + 31) // 32) * 32, np.uint8)
    padded[:len(rows)] = bits
    return np.packbits(padded, bitorder="little").view(np.uint32).copy(), int(sum(bits))


# ---- the pins ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tid", list(M.VALUE_SETS))
def test_comparisons_are_compare_model_against_the_literal(tid):
    want = {EQ: lambda c: c == 0, LT: lambda c: c < 0, LE: lambda c: c <= 0, GT: lambda c: c > 0,
            GE: lambda c: c >= 0}
    seen = set()
    for a, b in itertools.product(M.VALUE_SETS[tid], repeat=2):
        c = M.compare_model([tid], (a,), (b,))
        seen.add(c)
        for op in COMPARISONS:
            assert term_true(tid, a, op, 0, b) == want[op](c), (tid, a, op, b)
            assert term_true(tid, a, op, NOT, b) == (not want[op](c))
    assert seen == {-1, 0, 1}
    for b in M.VALUE_SETS[tid]:                   # rule 5
        for op in COMPARISONS:
            assert not term_true(tid, None, op, 0, b) and not term_true(tid, None, op, NOT, b)
    assert term_true(tid, None, IS_NULL, 0, b"") and not term_true(tid, None, IS_NULL, NOT, b"")
    v = M.VALUE_SETS[tid][0]
    assert not term_true(tid, v, IS_NULL, 0, b"") and term_true(tid, v, IS_NULL, NOT, b"")


def test_the_table_holds_what_the_rules_name():
    ints = {w: [int.from_bytes(v, "little", signed=True) for v in M.VALUE_SETS[t]]
            for w, t in ((1, T.INT8), (2, T.INT16), (4, T.INT32), (8, T.INT64))}
    for w, vals in ints.items():
        assert -(1 << (8 * w - 1)) in vals and (1 << (8 * w - 1)) - 1 in vals
    for t, fmt, w in ((T.FLOAT32, "<f", 4), (T.FLOAT64, "<d", 8)):
        have = set(M.VALUE_SETS[t])
        for x in (0.0, -0.0, float("inf"), float("-inf")):
            assert struct.pack(fmt, x) in have
        nans = [v for v in have if struct.unpack(fmt, v)[0] != struct.unpack(fmt, v)[0]]
        assert {v[-1] >> 7 for v in nans} == {0, 1}                  # NaNs of both signs
    decs = [int.from_bytes(v, "little", signed=True) for v in M.VALUE_SETS[T.DECIMAL]]
    assert (1 << 63) - 1 in decs and (1 << 63) in decs and (1 << 64) in decs and -(1 << 64) in decs
    s = M.VALUE_SETS[T.STRING]
    assert b"abcdefg" in s and b"abcdefgh" in s and b"\x7f" in s and b"\x80" in s and b"" in s


def test_floats_compare_by_total_order():
    f = lambda x: struct.pack("<d", x)           # noqa: E731
    assert not term_true(T.FLOAT64, f(-0.0), EQ, 0, f(0.0)) and term_true(T.FLOAT64, f(-0.0), LT, 0, f(0.0))
    nan, neg_nan = bytes.fromhex("000000000000f87f"), bytes.fromhex("000000000000f8ff")
    assert term_true(T.FLOAT64, nan, GT, 0, f(float("inf"))) and term_true(T.FLOAT64, nan, EQ, 0, nan)
    assert term_true(T.FLOAT64, neg_nan, LT, 0, f(float("-inf")))
    assert term_true(T.FLOAT32, struct.pack("<f", 1.5), GE, 0, struct.pack("<f", 1.5))
    assert term_true(T.INT8, b"\xff", LT, 0, b"\x00") and term_true(T.BOOL, b"\x02", EQ, 0, b"\x01")
    d = lambda x: x.to_bytes(16, "little", signed=True)              # noqa: E731
    assert term_true(T.DECIMAL, d((1 << 63) - 1), LT, 0, d(1 << 63)) and term_true(T.DECIMAL, d(-1), LT, 0, d(0))


PATTERN_VALUES = M.STRINGS + [b"aaab", b"aab", b"xxabcdefghxx", "héllo wörld \U0001f600".encode(),
                              b"\0\0", b"ab" * 150]
PATTERN_LITERALS = [b"", b"a", b"ab", b"aab", b"abcdefg", b"abcdefgh", b"defghij", b"x" * 17, b"\0", b"\x80",
                    "é".encode(), b"\xa9", b"ab" * 150, b"ba" * 150 + b"b", b"x" * 41]


def test_patterns_are_pythons():
    seen = {op: set() for op in PATTERNS}
    for v, lit in itertools.product(PATTERN_VALUES, PATTERN_LITERALS):
        want = {STARTS_WITH: v.startswith(lit), ENDS_WITH: v.endswith(lit), CONTAINS: lit in v}
        for op in PATTERNS:
            assert term_true(T.STRING, v, op, 0, lit) == want[op], (v, op, lit)
            assert term_true(T.BINARY, v, op, NOT, lit) == (not want[op])
            seen[op].add(want[op])
    assert all(s == {True, False} for s in seen.values())
    for op in PATTERNS:
        assert term_true(T.STRING, b"", op, 0, b"")                  # an empty literal: every non-null value
        assert not term_true(T.STRING, None, op, 0, b"") and not term_true(T.STRING, None, op, NOT, b"")
    assert term_true(T.STRING, b"aaab", CONTAINS, 0, b"aab")         # a false start
    assert not term_true(T.STRING, "é".encode(), CONTAINS, 0, "e".encode())


def test_clauses():
    i = lambda x: x.to_bytes(4, "little", signed=True)               # noqa: E731
    a_ge_2, a_le_5 = (0, T.INT32, GE, 0, i(2)), (0, T.INT32, LE, 0, i(5))
    s_eq_x, s_null = (1, T.STRING, EQ, 0, b"x"), (1, T.STRING, IS_NULL, 0, b"")
    orred = lambda t: t[:3] + (t[3] | OR,) + t[4:]                   # noqa: E731
    between = [a_ge_2, a_le_5]
    rows = [[i(1), b"x"], [i(2), b"x"], [i(5), None], [i(6), b"y"], [None, b"x"], [None, None]]
    assert [row_passes(between, r) for r in rows] == [False, True, True, False, False, False]
    either = [a_ge_2, orred(s_eq_x)]              # one clause: a >= 2 OR s = 'x'
    assert [row_passes(either, r) for r in rows] == [True, True, True, True, True, False]
    mixed = [a_ge_2, a_le_5, s_eq_x, orred(s_null)]
    assert [row_passes(mixed, r) for r in rows] == [False, True, True, False, False, False]
    # SQL's three-valued WHERE: NOT (a >= 2) is UNKNOWN on a null and does not pass
    assert [row_passes([(0, T.INT32, GE, NOT, i(2))], r) for r in rows] == [True, False, False, False, False, False]
    with pytest.raises(AssertionError):
        row_passes([orred(a_ge_2)], rows[0])
    words, count = mask_model(between, rows)
    assert words.tolist() == [0b000110] and count == 2
    words, count = mask_model(between, rows, examine=[1, 0, 1, 1, 1, 1])
    assert words.tolist() == [0b000100] and count == 1
    words, count = mask_model([s_null], [[None, None]] * 33)
    assert words.tolist() == [0xFFFFFFFF, 1] and count == 33
