"""A numpy model of fury_row_keys_equal, written from rules 1-3 of include/fury_row.h alone over
decoded columns, a dict model of the equi-join, and their pins without a GPU: the edge values the
rules name, rule 4 against the hash model of tests/test_hash_model.py, and candidate_pairs (plain
torch, here on CPU tensors) against a brute-force double loop.  The GPU tests
(tests/test_keys_equal.py) compare the kernel with this model applied to the oracle's decode."""
from __future__ import annotations

import numpy as np
import pytest

from fury_amd import types as T
from fury_amd.workloads import Column
from tests.test_hash_model import fixed_column, hash_columns, string_column, value_spans


# ---- rules 1-3 over decoded columns ----------------------------------------------------------------------
def key_values(f, c, n):
    """(values, valid) of the n values of host column c of field f: value_bytes of rule 2, as an
    [n, width] byte matrix (fixed-width, BOOL, DECIMAL) or an object array of bytes (STRING /
    BINARY)."""
    data, starts, lens, valid = value_spans(f, c, n)
    if f.type_id in (T.STRING, T.BINARY):
        raw = bytes(np.ascontiguousarray(data))
        vals = np.empty(n, object)
        vals[:] = [raw[int(s):int(s) + int(k)] for s, k in zip(starts, lens)]
        return vals, valid
    w = int(lens[0]) if n else 1
    return np.ascontiguousarray(data)[:n * w].reshape(n, w), valid


def keys_equal_model(fields_l, cols_l, idx_l, fields_r, cols_r, idx_r, null_equal, n_l, n_r):
    """out_equal of rules 1-3 as a uint8 array.  fields / cols: the key fields and their decoded
    columns, in key order; idx: the row of every pair (None: pair j uses row j); n: the rows of each
    batch.  A pair with an index outside its batch is 0."""
    assert len(fields_l) == len(fields_r) == len(cols_l) == len(cols_r)
    num = len(idx_l) if idx_l is not None else len(idx_r) if idx_r is not None else min(n_l, n_r)
    L = np.arange(num, dtype=np.int64) if idx_l is None else np.asarray(idx_l, np.int64)
    R = np.arange(num, dtype=np.int64) if idx_r is None else np.asarray(idx_r, np.int64)
    assert len(L) == len(R) == num
    ok = (L >= 0) & (L < n_l) & (R >= 0) & (R < n_r)
    Lc, Rc = np.where(ok, L, 0), np.where(ok, R, 0)
    eq = ok.copy()
    if num == 0 or n_l == 0 or n_r == 0:
        return np.zeros(num, np.uint8)
    for fl, cl, fr, cr in zip(fields_l, cols_l, fields_r, cols_r):
        assert fl.type_id == fr.type_id
        vl, okl = key_values(fl, cl, n_l)
        vr, okr = key_values(fr, cr, n_r)
        a, b = vl[Lc], vr[Rc]
        same = (a == b).all(axis=1) if a.ndim == 2 else np.asarray(a == b, bool)
        nl, nr = ~okl[Lc], ~okr[Rc]
        eq &= np.where(nl | nr, nl & nr & bool(null_equal), same)
    return eq.astype(np.uint8)


def key_tuples(fields, cols, n):
    """Row r -> the tuple of its key values (bytes, None for a null)."""
    per_key = []
    for f, c in zip(fields, cols):
        vals, valid = key_values(f, c, n)
        per_key.append([bytes(vals[r]) if valid[r] else None for r in range(n)])
    return list(zip(*per_key)) if per_key else [()] * n


def join_model(fields_l, cols_l, n_l, fields_r, cols_r, n_r, null_equal):
    """Every (i, j) whose key tuples are equal under rule 2, sorted by (i, j): two int64 arrays."""
    table: dict = {}
    for j, key in enumerate(key_tuples(fields_r, cols_r, n_r)):
        if null_equal or None not in key:
            table.setdefault(key, []).append(j)
    pairs = []
    for i, key in enumerate(key_tuples(fields_l, cols_l, n_l)):
        if null_equal or None not in key:
            pairs += [(i, j) for j in table.get(key, ())]
    pairs.sort()
    out = np.asarray(pairs, np.int64).reshape(-1, 2)
    return out[:, 0].copy(), out[:, 1].copy()


def mask_words(equal):
    """out_mask of rule 3 for an out_equal array: uint32 words, LSB first, tail bits zero."""
    n = len(equal)
    padded = np.zeros((n + 31) // 32 * 32, np.uint8)
    padded[:n] = equal
    return np.packbits(padded, bitorder="little").view(np.uint32)


# ---- the pins ------------------------------------------------------------------------------------------------
def _one(field, left, right, null_equal=False):
    return keys_equal_model([field], [left], None, [field], [right], None, null_equal,
                            n_l=len(_rows(left)), n_r=len(_rows(right))).tolist()


def _rows(c):
    return c.offsets[:-1] if c.offsets is not None else c.values


def test_null_against_the_empty_string_and_both_flags():
    s = T.field("s", T.STRING)
    left = string_column([None, None, b"", b"", b"\x00"])
    right = string_column([None, b"", None, b"", b""])
    assert _one(s, left, right, False) == [0, 0, 0, 1, 0]
    assert _one(s, left, right, True) == [1, 0, 0, 1, 0]
    i64 = T.field("k", T.INT64)
    a = fixed_column(np.int64, [5, 5, 5], nulls=[0, 1])
    b = fixed_column(np.int64, [5, 5, 5], nulls=[0])
    assert _one(i64, a, b, False) == [0, 0, 1]
    assert _one(i64, a, b, True) == [1, 0, 1]


def test_floats_compare_as_raw_bits():
    for f, dt, bits_t in ((T.field("f", T.FLOAT32), np.float32, np.uint32),
                          (T.field("d", T.FLOAT64), np.float64, np.uint64)):
        assert _one(f, fixed_column(dt, [0.0, -0.0, 0.0]), fixed_column(dt, [-0.0, -0.0, 0.0])) == [0, 1, 1]
        hi = 0x7FC00000 if dt is np.float32 else 0x7FF8000000000000
        nans_l = np.array([hi, hi, hi + 1], bits_t).view(dt)
        nans_r = np.array([hi, hi + 1, hi + 1], bits_t).view(dt)
        assert np.isnan(nans_l).all() and np.isnan(nans_r).all()
        assert _one(f, fixed_column(dt, nans_l), fixed_column(dt, nans_r)) == [1, 0, 1]


def test_bool_is_one_byte():
    b = T.field("b", T.BOOL)

    def col(values, nulls=()):
        valid = np.ones(len(values), bool)
        valid[list(nulls)] = False
        return Column(values=np.packbits(np.asarray(values, bool), bitorder="little"),
                      validity=np.packbits(valid, bitorder="little"))
    assert keys_equal_model([b], [col([1, 0, 1, 0])], None, [b], [col([1, 1, 0, 0], nulls=[3])], None,
                            False, n_l=4, n_r=4).tolist() == [1, 0, 0, 0]


def test_strings_that_differ_in_the_last_byte_or_only_in_length():
    s = T.field("s", T.STRING)
    base = bytes(range(1, 18))                                   # 17 bytes: two words and a tail
    left = string_column([base, base, base, base[:8], b"a"])
    right = string_column([base, base[:-1] + b"\xff", base[:-1], base[:9], b"ab"])
    assert _one(s, left, right) == [1, 0, 0, 0, 0]
    assert _one(T.field("s", T.BINARY), left, right) == [1, 0, 0, 0, 0]


def test_key_order_pairs_positions_and_indices_pick_rows():
    i32, i64 = T.field("i", T.INT32), T.field("k", T.INT64)
    a, b = fixed_column(np.int32, [7, 8]), fixed_column(np.int64, [8, 7])
    x, y = fixed_column(np.int32, [8, 7]), fixed_column(np.int64, [7, 8])
    # left keys (i, k) = (7, 8), (8, 7); right keys, as (i, k): (8, 7), (7, 8)
    assert keys_equal_model([i32, i64], [a, b], None, [i32, i64], [x, y], None, False,
                            n_l=2, n_r=2).tolist() == [0, 0]
    assert keys_equal_model([i32, i64], [a, b], [0, 1, 0], [i32, i64], [x, y], [1, 0, 0], False,
                            n_l=2, n_r=2).tolist() == [1, 1, 0]
    # position k of the left pairs with position k of the right: the same columns in another key order
    assert keys_equal_model([i64, i32], [b, a], [0, 1], [i64, i32], [y, x], [1, 0], False,
                            n_l=2, n_r=2).tolist() == [1, 1]
    # an index outside its batch gives 0, whatever the flag
    for null_equal in (False, True):
        assert keys_equal_model([i32], [a], [0, -1, 2, 0], [i32], [a], [0, 0, 0, 2 ** 40], null_equal,
                                n_l=2, n_r=2).tolist() == [1, 0, 0, 0]


def _random_keys(rng, n, null_pct=15):
    """An (INT32, STRING, BOOL) key of few distinct values, with nulls."""
    ints = fixed_column(np.int32, rng.integers(0, 3, n), nulls=np.flatnonzero(rng.random(n) < null_pct / 100))
    words = [b"", b"a", b"ab", b"abcdefgh", b"abcdefghi"]
    strs = string_column([None if rng.random() < null_pct / 100 else words[int(rng.integers(0, len(words)))]
                          for _ in range(n)])
    bools = Column(values=np.packbits(rng.integers(0, 2, n).astype(bool), bitorder="little"),
                   validity=np.packbits(np.ones(n, bool), bitorder="little"))
    return [T.field("i", T.INT32), T.field("s", T.STRING), T.field("b", T.BOOL)], [ints, strs, bools]


def test_rule_4_equal_pairs_have_equal_hashes():
    rng = np.random.default_rng(4)
    nl, nr = 60, 45
    fields, left = _random_keys(rng, nl)
    _, right = _random_keys(rng, nr)
    L, R = np.divmod(np.arange(nl * nr), nr)
    for seed in (0, 42, 0xFFFFFFFF):
        hl, hr = hash_columns(fields, left, nl, seed), hash_columns(fields, right, nr, seed)
        for null_equal in (True, False):
            eq = keys_equal_model(fields, left, L, fields, right, R, null_equal, n_l=nl, n_r=nr)
            assert eq.sum() > 20 and (eq == 0).sum() > 20
            assert (hl[L][eq == 1] == hr[R][eq == 1]).all()
    # the flag matters on this input: pairs of null keys exist
    assert (keys_equal_model(fields, left, L, fields, right, R, True, n_l=nl, n_r=nr).sum() >
            keys_equal_model(fields, left, L, fields, right, R, False, n_l=nl, n_r=nr).sum())


def test_join_model_is_the_pairwise_model():
    rng = np.random.default_rng(5)
    nl, nr = 40, 30
    fields, left = _random_keys(rng, nl)
    _, right = _random_keys(rng, nr)
    L, R = np.divmod(np.arange(nl * nr), nr)
    for null_equal in (False, True):
        eq = keys_equal_model(fields, left, L, fields, right, R, null_equal, n_l=nl, n_r=nr) == 1
        li, ri = join_model(fields, left, nl, fields, right, nr, null_equal)
        assert np.array_equal(li, L[eq]) and np.array_equal(ri, R[eq])


def test_mask_words():
    eq = np.zeros(70, np.uint8)
    eq[[0, 31, 32, 69]] = 1
    assert mask_words(eq).tolist() == [0x80000001, 1, 1 << 5]
    assert mask_words(np.zeros(0, np.uint8)).tolist() == []


# ---- candidate_pairs: plain torch, here on the CPU ---------------------------------------------------------
def _brute(lh, rh):
    pairs = [(i, j) for i in range(len(lh)) for j in range(len(rh)) if lh[i] == rh[j]]
    out = np.asarray(pairs, np.int64).reshape(-1, 2)
    return out[:, 0], out[:, 1]


def test_candidate_pairs_against_a_double_loop():
    torch = pytest.importorskip("torch")
    from fury_amd import candidate_pairs
    rng = np.random.default_rng(6)
    values = np.array([0, 7, 0x7FFFFFFF, 0xFFFFFFF0], np.uint32)     # one of them negative as int32
    for nl, nr in ((1, 1), (37, 23), (23, 37), (64, 64)):
        lh, rh = values[rng.integers(0, 4, nl)], values[rng.integers(0, 4, nr)]
        wl, wr = _brute(lh, rh)
        for view in (np.uint32, np.int32):
            li, ri = candidate_pairs(torch.from_numpy(lh.view(view)), torch.from_numpy(rh.view(view)))
            assert li.dtype == torch.int64 and ri.dtype == torch.int64
            assert np.array_equal(li.numpy(), wl) and np.array_equal(ri.numpy(), wr), (nl, nr)
        if nl > 1:
            assert len(wl) > max(nl, nr)                             # many-to-many runs
    # no hash in common
    li, ri = candidate_pairs(torch.tensor([1, 2], dtype=torch.int32), torch.tensor([3], dtype=torch.int32))
    assert li.numel() == 0 and ri.numel() == 0


def test_candidate_pairs_empty_sides_and_max_pairs():
    torch = pytest.importorskip("torch")
    from fury_amd import candidate_pairs
    from fury_amd.encoder import IllegalArgumentException
    some = torch.tensor([1, 2, 3], dtype=torch.int32)
    none = torch.zeros(0, dtype=torch.int32)
    for lh, rh in ((none, some), (some, none), (none, none)):
        li, ri = candidate_pairs(lh, rh)
        assert li.dtype == torch.int64 and li.numel() == 0 and ri.numel() == 0
    hot = torch.full((100,), 9, dtype=torch.int32)
    with pytest.raises(IllegalArgumentException, match="10000 candidate pairs"):
        candidate_pairs(hot, hot, max_pairs=9999)
    li, ri = candidate_pairs(hot, hot, max_pairs=10000)
    assert li.numel() == 10000 and ri[:100].tolist() == list(range(100))


def test_candidates_filtered_by_the_model_are_the_join():
    """The composition join_pairs makes, on the CPU: candidates from a hash degraded to 4 values,
    so most candidates are collisions, kept where the model says the keys are equal."""
    torch = pytest.importorskip("torch")
    from fury_amd import candidate_pairs
    rng = np.random.default_rng(8)
    nl, nr = 90, 70
    fields, left = _random_keys(rng, nl)
    _, right = _random_keys(rng, nr)
    tl, tr = key_tuples(fields, left, nl), key_tuples(fields, right, nr)
    assert any(tl.count(k) >= 2 and tr.count(k) >= 2 for k in set(tl))      # a many-to-many key
    hl = hash_columns(fields, left, nl, 3) % 4
    hr = hash_columns(fields, right, nr, 3) % 4
    assert any(hl[i] == hr[j] and tl[i] != tr[j] for i in range(nl) for j in range(nr))  # a collision
    li, ri = candidate_pairs(torch.from_numpy(hl.astype(np.uint32)), torch.from_numpy(hr.astype(np.uint32)))
    li, ri = li.numpy(), ri.numpy()
    for null_equal in (True, False):
        eq = keys_equal_model(fields, left, li, fields, right, ri, null_equal, n_l=nl, n_r=nr) == 1
        assert 0 < eq.sum() < len(eq)
        wl, wr = join_model(fields, left, nl, fields, right, nr, null_equal)
        assert np.array_equal(li[eq], wl) and np.array_equal(ri[eq], wr)
