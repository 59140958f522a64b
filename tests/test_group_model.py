"""A dict model of fury_row_group, written from rules 1-3 (and 5) of include/fury_row.h alone over
decoded columns, and its pins without a GPU: the edge values rule 1 names, bad rows as their own
groups, and the two consequences of rule 3 against numpy.  The GPU tests (tests/test_group.py)
compare the kernels with this model applied to the oracle's decode."""
from __future__ import annotations

import numpy as np

from fury_amd import types as T
from fury_amd.workloads import Column
from tests.test_hash_model import fixed_column, string_column
from tests.test_keys_equal_model import key_tuples


# ---- rules 1-3 over decoded columns ----------------------------------------------------------------------
def group_model(fields, cols, n, bad_rows=()):
    """(first[n], group_ids[n], group_rows[n], G) of rules 2 and 3.  fields / cols: the key fields and
    their decoded columns, in key order; bad_rows: rows that fail rule 5 -- each a group of its own,
    never compared with another row."""
    bad = set(int(r) for r in bad_rows)
    table: dict = {}
    first = np.empty(n, np.int64)
    for r, key in enumerate(key_tuples(fields, cols, n)):
        first[r] = r if r in bad else table.setdefault(key, r)
    is_first = first == np.arange(n)
    before = np.cumsum(is_first) - is_first                       # groups whose first row is below r
    ids = before[first] if n else np.zeros(0, np.int64)
    G = int(is_first.sum())
    rows = np.full(n, -1, np.int64)
    rows[:G] = np.flatnonzero(is_first)
    return first, ids.astype(np.int64), rows, G


def _first(field, col, n):
    return group_model([field], [col], n)[0].tolist()


# ---- the pins ------------------------------------------------------------------------------------------------
def test_null_against_the_empty_string():
    s = T.field("s", T.STRING)
    col = string_column([None, b"", None, b"", b"\x00", None])
    first, ids, rows, G = group_model([s], [col], 6)
    assert first.tolist() == [0, 1, 0, 1, 4, 0]                   # null == null, null != ""
    assert ids.tolist() == [0, 1, 0, 1, 2, 0]
    assert rows.tolist() == [0, 1, 4, -1, -1, -1] and G == 3
    i64 = T.field("k", T.INT64)
    assert _first(i64, fixed_column(np.int64, [5, 5, 5, 0], nulls=[1, 3]), 4) == [0, 1, 0, 1]


def test_floats_group_by_their_raw_bits():
    for f, dt, bits_t in ((T.field("f", T.FLOAT32), np.float32, np.uint32),
                          (T.field("d", T.FLOAT64), np.float64, np.uint64)):
        assert _first(f, fixed_column(dt, [0.0, -0.0, 0.0, -0.0]), 4) == [0, 1, 0, 1]
        hi = 0x7FC00000 if dt is np.float32 else 0x7FF8000000000000
        nans = np.array([hi, hi + 1, hi, hi + 1, hi + 2], bits_t).view(dt)
        assert np.isnan(nans).all()
        assert _first(f, fixed_column(dt, nans), 5) == [0, 1, 0, 1, 4]


def test_bool_is_zero_or_one():
    b = T.field("b", T.BOOL)
    valid = np.ones(6, bool)
    valid[4] = False
    col = Column(values=np.packbits(np.array([1, 0, 1, 0, 1, 0], bool), bitorder="little"),
                 validity=np.packbits(valid, bitorder="little"))
    first, ids, rows, G = group_model([b], [col], 6)
    assert first.tolist() == [0, 1, 0, 1, 4, 1] and G == 3


def test_strings_that_differ_in_the_last_byte_or_only_in_length():
    s = T.field("s", T.STRING)
    base = bytes(range(1, 18))                                   # 17 bytes: two words and a tail
    col = string_column([base, base[:-1] + b"\xff", base[:-1], base, base[:8], base[:9], base[:8], b"a", b"ab"])
    assert _first(s, col, 9) == [0, 1, 2, 0, 4, 5, 4, 7, 8]
    assert _first(T.field("s", T.BINARY), col, 9) == [0, 1, 2, 0, 4, 5, 4, 7, 8]


def test_key_order_and_a_null_in_one_key_of_two():
    i32, j32 = T.field("i", T.INT32), T.field("j", T.INT32)
    a = fixed_column(np.int32, [7, 8, 7, 8, 7, 7], nulls=[4, 5])
    b = fixed_column(np.int32, [8, 7, 8, 7, 8, 8], nulls=[])
    # (i, j) = (7, 8), (8, 7), (7, 8), (8, 7), (null, 8), (null, 8)
    assert group_model([i32, j32], [a, b], 6)[0].tolist() == [0, 1, 0, 1, 4, 4]
    assert group_model([i32, j32], [a, b], 6)[3] == 3
    # key positions are not interchangeable: (7, 8) is not (8, 7)
    x = fixed_column(np.int32, [7, 8])
    y = fixed_column(np.int32, [8, 7])
    assert group_model([i32, j32], [x, y], 2)[3] == 2
    # a null in one key of two: equal only to the same null with the same other key
    c = fixed_column(np.int32, [1, 1, 1, 2], nulls=[])
    d = fixed_column(np.int32, [5, 5, 5, 5], nulls=[0, 2, 3])
    assert group_model([i32, j32], [c, d], 4)[0].tolist() == [0, 1, 0, 3]
    assert group_model([j32, i32], [d, c], 4)[0].tolist() == [0, 1, 0, 3]     # whatever the order


def test_bad_rows_are_groups_of_their_own():
    i64 = T.field("k", T.INT64)
    col = fixed_column(np.int64, [3, 3, 3, 4, 3, 4])
    first, ids, rows, G = group_model([i64], [col], 6, bad_rows=[0, 4])
    # row 0 is bad: rows 1 and 2 form their group without it, first row 1
    assert first.tolist() == [0, 1, 1, 3, 4, 3]
    assert ids.tolist() == [0, 1, 1, 2, 3, 2]
    assert rows.tolist() == [0, 1, 3, 4, -1, -1] and G == 4


def _random_keys(rng, n):
    ints = fixed_column(np.int32, rng.integers(0, 3, n), nulls=np.flatnonzero(rng.random(n) < 0.15))
    words = [b"", b"a", b"ab", b"abcdefgh", b"abcdefghi"]
    strs = string_column([None if rng.random() < 0.15 else words[int(rng.integers(0, len(words)))]
                          for _ in range(n)])
    return [T.field("i", T.INT32), T.field("s", T.STRING)], [ints, strs]


def test_rule_3_and_its_consequences_against_numpy():
    rng = np.random.default_rng(11)
    n = 300
    fields, cols = _random_keys(rng, n)
    first, ids, rows, G = group_model(fields, cols, n)
    keys = key_tuples(fields, cols, n)
    assert 10 < G < 30
    # rule 2 by brute force: the smallest row with the same key
    assert first.tolist() == [min(j for j in range(n) if keys[j] == keys[i]) for i in range(n)]
    # rule 3: ids count the first rows below, group_rows lists them, (c) closes the loop
    firsts = np.unique(first)
    assert len(firsts) == G and np.array_equal(rows[:G], firsts) and (rows[G:] == -1).all()
    assert np.array_equal(ids, np.searchsorted(firsts, first))
    assert np.array_equal(first, rows[ids])
    # (a) take at group_rows[0 .. G): every distinct key once, in order of first occurrence
    taken = [keys[r] for r in rows[:G]]
    assert len(set(taken)) == G == len(set(keys))
    assert taken == list(dict.fromkeys(keys))
    # (b) a stable argsort of the ids (what partition does) makes every group contiguous, groups in
    # order of first occurrence, rows in source order
    order = np.argsort(ids, kind="stable")
    sorted_ids = ids[order]
    assert (np.diff(sorted_ids) >= 0).all()
    for g in range(G):
        members = order[sorted_ids == g]
        assert members[0] == rows[g] and (np.diff(members) > 0).all()
        assert {keys[r] for r in members} == {keys[rows[g]]}
    sizes = np.bincount(ids, minlength=G)
    assert sizes.sum() == n and (sizes > 0).all()


def test_the_empty_batch():
    first, ids, rows, G = group_model([T.field("k", T.INT64)], [fixed_column(np.int64, [])], 0)
    assert len(first) == len(ids) == len(rows) == 0 and G == 0
