"""The numpy model of fury_row_zip (the pick rules of include/fury_row.h: fury_row_select's rules 2-4
per picked field, rule 1 per source), pinned to the oracle on the CPU: applied to the oracle's rows of
several schemas it gives, byte for byte, the oracle's rows of the picked columns under the zipped
schema; with one source it is the model of fury_row_select.  tests/test_zip.py compares the GPU against
this model, which alone also covers malformed and non-canonical input."""
from __future__ import annotations

import numpy as np
import pytest

from fury_amd import types as T
from fury_amd.workloads import SCHEMAS
from tests.test_select_model import (INT32_MAX, Want, _i32, _value_ok, expect_select, header_size,
                                     host_columns)


class Source:
    """One source batch on the host: rows at offs (n + 1 entries, also for a fixed-width schema)."""

    def __init__(self, rows, offs, n, fields):
        self.rows, self.offs, self.n, self.fields = rows, offs, n, list(fields)


def zip_row(sources, picks, r):
    """(bytes of output row r, whether the row is reported)."""
    ns = len(picks)
    bm2 = ((ns + 63) // 64) * 8
    F2 = bm2 + 8 * ns
    ok, bad = {}, False
    for s in sorted({s for s, _ in picks}):                       # a source no pick names is never read
        src = sources[s]
        total, B, F = int(src.offs[src.n]), int(src.offs[r]), header_size(len(src.fields))
        ok[s] = not (B % 8 or not (0 <= B and B + F <= total) or int(src.offs[r + 1]) - B < F)
        bad |= not ok[s]
    head, tail, W = bytearray(F2), bytearray(), F2
    for j, (s, k) in enumerate(picks):
        src = sources[s]
        rows, f = src.rows, src.fields[k]
        u64 = lambda p: int.from_bytes(rows[p:p + 8].tobytes(), "little")   # noqa: E731
        total, B, bm = int(src.offs[src.n]), int(src.offs[r]), ((len(src.fields) + 63) // 64) * 8
        null = not ok[s] or bool((u64(B + 8 * (k >> 6)) >> (k & 63)) & 1)
        slot = 0
        if not null:
            v = u64(B + bm + 8 * k)
            w = T.type_width(f.type_id)
            if f.type_id == T.BOOL:
                slot = 1 if v & 0xFF else 0
            elif w > 0:
                slot = v & ((1 << (8 * w)) - 1)
            else:
                off, size = _i32(v >> 32), _i32(v)
                if not _value_ok(f, off, size, B, total):
                    null = bad = True
                else:
                    slot = (W << 32) | size
                    tail += rows[B + off:B + off + size].tobytes() + bytes(-size % 8)
                    W += size + (-size % 8)
                    if W > INT32_MAX - 7:                         # the whole output row is all null
                        head = bytearray(F2)
                        for i in range(ns):
                            head[i >> 3] |= 1 << (i & 7)
                        return bytes(head), True
        if null:
            head[j >> 3] |= 1 << (j & 7)
            slot = 0
        head[bm2 + 8 * j:bm2 + 8 * j + 8] = slot.to_bytes(8, "little")
    assert W == F2 + len(tail)
    return bytes(head) + bytes(tail), bad


def expect_zip(sources, picks) -> Want:
    """The batch fury_row_zip produces for ``picks`` = (source index, slot) pairs of the ``Source``s,
    computed from the source bytes alone: ``data``, ``offs`` and the reported rows ``bad``."""
    n = sources[picks[0][0]].n
    w = Want()
    parts, w.bad = [], []
    for r in range(n):
        b, bad = zip_row(sources, picks, r)
        parts.append(b)
        if bad:
            w.bad.append(r)
    w.data = np.frombuffer(b"".join(parts), np.uint8).copy()
    w.offs = np.zeros(n + 1, np.int64)
    np.cumsum([len(p) for p in parts], out=w.offs[1:])
    return w


# -- the model against the oracle --------------------------------------------------------------------
N = 65


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    return O


_ENCODED: dict = {}


def encoded(oracle, name) -> Source:
    """The oracle's rows of one of the named schemas, with their host columns (never modified)."""
    if name not in _ENCODED:
        fields = SCHEMAS[name]
        cols = host_columns(name, N)
        rows, offs = oracle.encode(fields, cols, N)
        src = Source(np.asarray(rows, np.uint8), np.asarray(offs, np.int64), N, fields)
        src.cols = cols
        _ENCODED[name] = src
    return _ENCODED[name]


def pick_patterns(a, b):
    """Interleaved, reversed and single-field-from-each picks of two sources."""
    na, nb = len(a.fields), len(b.fields)
    inter = [p for i in range(max(na, nb)) for p in ((0, i), (1, i)) if p[1] < (na, nb)[p[0]]]
    return {"interleaved": inter, "reversed": inter[::-1], "one from each": [(1, nb - 1), (0, na // 2)]}


def renamed(fields):
    """Distinct names for the oracle call; names do not enter row bytes."""
    return [T.field(f"z{j}", f.type_id, f.nullable, f.children) for j, f in enumerate(fields)]


@pytest.mark.parametrize("pair", [("struct100", "mixed"), ("foo", "narrow"), ("beana", "mixed")])
def test_model_equals_the_oracle(oracle, pair):
    srcs = [encoded(oracle, name) for name in pair]
    for what, picks in pick_patterns(*srcs).items():
        fields = renamed([srcs[s].fields[k] for s, k in picks])
        want, want_offs = oracle.encode(fields, [srcs[s].cols[k] for s, k in picks], N)
        got = expect_zip(srcs, picks)
        assert not got.bad, (pair, what)
        assert np.array_equal(got.offs, np.asarray(want_offs, np.int64)), (pair, what)
        assert np.array_equal(got.data, np.asarray(want, np.uint8)), (pair, what)


def _same(a, b):
    return np.array_equal(a.data, b.data) and np.array_equal(a.offs, b.offs) and a.bad == b.bad


@pytest.mark.parametrize("name", ["struct100", "mixed", "narrow", "foo", "beana"])
def test_one_source_is_the_select_model(oracle, name):
    src = encoded(oracle, name)
    nf = len(src.fields)
    for sel in ([nf // 2], list(range(nf - 1, -1, -2)), list(range(nf))):
        assert _same(expect_zip([src], [(0, k) for k in sel]),
                     expect_select(src.rows, src.offs, N, src.fields, sel)), (name, sel)


def test_one_source_normalises_and_rejects_like_select():
    """The hand-written row of test_select_model.test_model_normalises_and_rejects and its edits."""
    fields = [T.field("b", T.BOOL), T.field("s", T.STRING), T.field("i", T.INT32)]
    row = bytearray(8 + 24 + 8)
    row[8] = 2                                                   # BOOL byte 2
    row[16:24] = ((32 << 32) | 3).to_bytes(8, "little")          # "abc" at 32
    row[24:32] = (0xDEADBEEF_00000007).to_bytes(8, "little")     # INT32 7 under stale upper bytes
    row[32:40] = b"abc\xff\xff\xff\xff\xff"                      # non-zero padding
    rows = np.frombuffer(bytes(row) * 2, np.uint8).copy()
    offs = np.array([0, 40, 80], np.int64)

    def both(sel):
        got = expect_zip([Source(rows, offs, 2, fields)], [(0, k) for k in sel])
        assert _same(got, expect_select(rows, offs, 2, fields, sel)), sel
        return got

    one = bytes(8) + (7).to_bytes(8, "little") + ((32 << 32) | 3).to_bytes(8, "little") + \
        (1).to_bytes(8, "little") + b"abc" + bytes(5)
    assert both([2, 1, 0]).data.tobytes() == one * 2
    rows[40 + 16 + 4] = 36                                       # row 1: off 36, off % 8 == 4
    assert both([1]).bad == [1]
    offs[1] = 44                                                 # row 1 starts off an 8-byte boundary
    assert both([0, 2]).bad == [1]
    offs[1] = 40
    offs[2] = 64                                                 # row 1 shorter than its header
    assert both([0, 2]).bad == [1]


def split_picks(nf):
    """Two selections that split nf fields, and the picks that restore the field order."""
    s1, s2 = list(range(0, nf, 2)), list(range(nf - 1 - (nf % 2), 0, -2))     # evens up, odds down
    where = {k: (0, i) for i, k in enumerate(s1)}
    where.update({k: (1, i) for i, k in enumerate(s2)})
    return s1, s2, [where[k] for k in range(nf)]


@pytest.mark.parametrize("name", [name for name, fields in SCHEMAS.items() if len(fields) >= 2])
def test_split_and_rezip_returns_the_rows(oracle, name):
    if name == "row_test":                                       # no column generator: random beans
        from fury_amd.beans import beans_to_columns
        from tests.test_device import _random_value
        fields, rng = SCHEMAS[name], np.random.default_rng(12)
        cols = beans_to_columns(fields, [{f.name: _random_value(f, rng) for f in fields}
                                         for _ in range(N)])
        rows, offs = oracle.encode(fields, cols, N)
        src = Source(np.asarray(rows, np.uint8), np.asarray(offs, np.int64), N, fields)
    else:
        src = encoded(oracle, name)
    s1, s2, restore = split_picks(len(src.fields))
    halves = []
    for sel in (s1, s2):
        h = expect_select(src.rows, src.offs, N, src.fields, sel)
        assert not h.bad
        halves.append(Source(h.data, h.offs, N, [src.fields[k] for k in sel]))
    got = expect_zip(halves, restore)
    assert not got.bad
    assert np.array_equal(got.offs, src.offs) and np.array_equal(got.data, src.rows), name


def test_a_failed_row_nulls_only_its_own_source():
    """Two sources of two rows, by hand: row 1 of source 1 starts off an 8-byte boundary."""
    fa = [T.field("i", T.INT32), T.field("s", T.STRING)]
    fb = [T.field("t", T.STRING), T.field("j", T.INT64)]

    def row(slot0, slot1, tail):
        return bytes(8) + slot0.to_bytes(8, "little") + slot1.to_bytes(8, "little") + tail

    a = row(5, (24 << 32) | 2, b"hi" + bytes(6)) + row(6, (24 << 32) | 3, b"abc" + bytes(5))
    b = row((24 << 32) | 1, 77, b"x" + bytes(7)) + row((24 << 32) | 8, 78, b"12345678")
    A = Source(np.frombuffer(a, np.uint8).copy(), np.array([0, 32, 64], np.int64), 2, fa)
    offs_b = np.array([0, 32, 64], np.int64)
    B = Source(np.frombuffer(b, np.uint8).copy(), offs_b, 2, fb)
    picks = [(1, 0), (0, 0), (0, 1), (1, 1)]                     # t, i, s, j
    F2 = 8 + 32
    clean = expect_zip([A, B], picks)
    assert not clean.bad and list(clean.offs) == [0, F2 + 16, 2 * F2 + 32]
    r1 = clean.data.tobytes()[F2 + 16:]
    assert r1 == (bytes(8) + ((F2 << 32) | 8).to_bytes(8, "little") + (6).to_bytes(8, "little") +
                  (((F2 + 8) << 32) | 3).to_bytes(8, "little") + (78).to_bytes(8, "little") +
                  b"12345678" + b"abc" + bytes(5))
    offs_b[1] = 36                                               # row 1 of source 1: 36 % 8 == 4
    got = expect_zip([A, B], picks)
    assert got.bad == [1]                                        # row 0 is whole: its extent is 36 >= 24
    assert np.array_equal(got.data[:F2 + 16], clean.data[:F2 + 16])
    r1 = got.data.tobytes()[F2 + 16:]
    assert r1 == ((0b1001).to_bytes(8, "little") + bytes(8) + (6).to_bytes(8, "little") +
                  ((F2 << 32) | 3).to_bytes(8, "little") + bytes(8) + b"abc" + bytes(5))
    assert list(got.offs) == [0, F2 + 16, 2 * F2 + 24]
    only_a = expect_zip([A, B], [(0, 1), (0, 0)])                # source 1 not picked: never read
    assert not only_a.bad
