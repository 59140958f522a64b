"""A dict model of fury_row_index_build / fury_row_lookup, written from the numbered rules of
include/fury_row.h alone over decoded columns, and its pins without a GPU: the edge values the rules
name, build-side duplicates, bad rows on either side, and the torch half of lookup_join_pairs (here
on CPU tensors) against a brute-force double loop.  The GPU tests (tests/test_lookup.py) compare the
kernels with this model applied to the oracle's decode of both batches."""
from __future__ import annotations

import numpy as np
import pytest

from fury_amd import types as T
from fury_amd.workloads import Column
from tests.test_hash_model import fixed_column, string_column
from tests.test_keys_equal_model import join_model, key_tuples, mask_words


# ---- rules 2, 4, 6 over decoded columns ------------------------------------------------------------------
def lookup_model(build_cols, probe_cols, null_equal=False, bad_build=(), bad_probe=()):
    """out_rows of rule 4 as an int64 array.  build_cols / probe_cols: (fields, cols, n), the key
    fields and their decoded columns in key order and the batch's row count.  bad_build: build rows
    that fail the bounds and are never entered (rule 2); bad_probe: probe rows that fail theirs and
    find nothing (rule 6)."""
    bf, bc, nb = build_cols
    pf, pc, n = probe_cols
    assert [f.type_id for f in bf] == [f.type_id for f in pf]                 # rule 8
    skip = set(int(r) for r in bad_build)
    table: dict = {}
    for i, key in enumerate(key_tuples(bf, bc, nb)):                          # putIfAbsent: null == null
        if i not in skip:
            table.setdefault(key, i)
    lost = set(int(r) for r in bad_probe)
    out = np.full(n, -1, np.int64)
    for j, key in enumerate(key_tuples(pf, pc, n)):
        if j in lost or (not null_equal and None in key):
            continue
        out[j] = table.get(key, -1)
    return out


def lookup_mask(rows):
    """out_mask of rule 4 for an out_rows array: uint32 words, LSB first, tail bits zero."""
    return mask_words((np.asarray(rows) >= 0).astype(np.uint8))


def _n(c):
    return len(c.offsets) - 1 if c.offsets is not None else len(c.values)


def _one(field, build, probe, null_equal=False, **bad):
    return lookup_model(([field], [build], _n(build)), ([field], [probe], _n(probe)), null_equal, **bad).tolist()


# ---- the pins ------------------------------------------------------------------------------------------------
def test_null_against_null_under_both_flags_and_against_the_empty_string():
    s = T.field("s", T.STRING)
    build = string_column([b"x", None, b"", None])
    probe = string_column([None, b"", b"x", b"y", b"\x00"])
    assert _one(s, build, probe, False) == [-1, 2, 0, -1, -1]             # a null key matches nothing
    assert _one(s, build, probe, True) == [1, 2, 0, -1, -1]               # ... or the first null
    assert lookup_mask(_one(s, build, probe, True)).tolist() == [0b00111]
    only_null = string_column([None])
    assert _one(s, only_null, string_column([b"", None]), True) == [-1, 0]     # null != ""
    assert _one(s, only_null, string_column([b"", None]), False) == [-1, -1]
    i64 = T.field("k", T.INT64)
    b = fixed_column(np.int64, [5, 5, 6], nulls=[0])
    p = fixed_column(np.int64, [5, 5, 7], nulls=[1])
    assert _one(i64, b, p, False) == [1, -1, -1]
    assert _one(i64, b, p, True) == [1, 0, -1]


def test_floats_match_by_their_raw_bits():
    for f, dt in ((T.field("f", T.FLOAT32), np.float32), (T.field("d", T.FLOAT64), np.float64)):
        build = fixed_column(dt, [0.0, 1.5])
        assert _one(f, build, fixed_column(dt, [-0.0, 0.0, 1.5])) == [-1, 0, 1]
        both = fixed_column(dt, [-0.0, 0.0])
        assert _one(f, both, fixed_column(dt, [0.0, -0.0])) == [1, 0]


def test_bool_stored_as_2_is_true(oracle):
    """Any non-zero stored byte is 1 (rule 2 of fury_row_keys_equal): the model sees the oracle's
    decode, which reads the byte as BinaryRow.getBoolean does."""
    b = T.field("b", T.BOOL)
    col = Column(values=np.packbits(np.array([1, 0, 1], bool), bitorder="little"),
                 validity=np.packbits(np.ones(3, bool), bitorder="little"))
    rows, offs = oracle.encode([b], [col], 3)
    rows = np.asarray(rows, np.uint8).copy()
    fixed = 16                                                     # one bitmap word, one slot
    assert len(rows) == 3 * fixed and rows[8] == 1 and rows[fixed + 8] == 0
    rows[2 * fixed + 8] = 2                                        # row 2: true, stored as 2
    probe = oracle.decode([b], rows, offs, 3)
    build = oracle.decode([b], rows[:2 * fixed].copy(), None if offs is None else offs[:3], 2)
    assert lookup_model(([b], build, 2), ([b], probe, 3)).tolist() == [0, 1, 0]


def test_build_duplicates_the_smallest_row_wins():
    i32 = T.field("i", T.INT32)
    build = fixed_column(np.int32, [9, 7, 9, 7, 7, 3])
    probe = fixed_column(np.int32, [7, 9, 3, 4, 7])
    got = _one(i32, build, probe)
    assert got == [1, 0, 5, -1, 1]
    assert lookup_mask(got).tolist() == [0b10111]


def test_a_bad_build_row_that_is_the_first_of_its_group():
    """It is never entered: the next row of its group is the one lookups find; a bad probe row finds
    nothing under either flag."""
    i32 = T.field("i", T.INT32)
    build = fixed_column(np.int32, [7, 9, 7, 7, 9])
    probe = fixed_column(np.int32, [7, 9, 7])
    assert _one(i32, build, probe) == [0, 1, 0]
    assert _one(i32, build, probe, bad_build=[0]) == [2, 1, 2]
    assert _one(i32, build, probe, bad_build=[0, 2, 3]) == [-1, 1, -1]
    assert _one(i32, build, probe, bad_build=[2]) == [0, 1, 0]     # a later row: no change
    for null_equal in (False, True):
        assert _one(i32, build, probe, null_equal, bad_probe=[1, 2]) == [0, -1, -1]


def test_key_positions_pair_up_and_a_null_in_one_key_of_two():
    i32, i64 = T.field("i", T.INT32), T.field("k", T.INT64)
    bi, bk = fixed_column(np.int32, [7, 8, 7], nulls=[2]), fixed_column(np.int64, [8, 7, 8])
    pi, pk = fixed_column(np.int32, [8, 7, 7, 7], nulls=[3]), fixed_column(np.int64, [7, 8, 7, 8])
    build, probe = ([i32, i64], [bi, bk], 3), ([i32, i64], [pi, pk], 4)
    assert lookup_model(build, probe).tolist() == [1, 0, -1, -1]
    assert lookup_model(build, probe, True).tolist() == [1, 0, -1, 2]
    # the same columns in another key order: position k of the probe meets position k of the build
    assert lookup_model(([i64, i32], [bk, bi], 3), ([i64, i32], [pk, pi], 4), True).tolist() == [1, 0, -1, 2]


def test_empty_sides():
    i64 = T.field("k", T.INT64)
    none, some = fixed_column(np.int64, []), fixed_column(np.int64, [1, 2])
    assert _one(i64, none, some) == [-1, -1]
    assert _one(i64, some, none) == []
    assert lookup_mask([]).tolist() == []
    rows = np.full(70, -1)
    rows[[0, 31, 32, 69]] = [5, 0, 2 ** 31 - 2, 1]
    assert lookup_mask(rows).tolist() == [0x80000001, 1, 1 << 5]


def _random_keys(rng, n, null_pct=15):
    ints = fixed_column(np.int32, rng.integers(0, 3, n), nulls=np.flatnonzero(rng.random(n) < null_pct / 100))
    words = [b"", b"a", b"ab", b"abcdefgh", b"abcdefghi"]
    strs = string_column([None if rng.random() < null_pct / 100 else words[int(rng.integers(0, len(words)))]
                          for _ in range(n)])
    return [T.field("i", T.INT32), T.field("s", T.STRING)], [ints, strs]


def test_the_model_is_the_first_build_row_of_the_join():
    rng = np.random.default_rng(13)
    nb, n = 70, 90
    fields, build = _random_keys(rng, nb)
    _, probe = _random_keys(rng, n)
    for null_equal in (False, True):
        got = lookup_model((fields, build, nb), (fields, probe, n), null_equal)
        pj, bi = join_model(fields, probe, n, fields, build, nb, null_equal)
        want = np.full(n, -1, np.int64)
        for j, i in zip(pj[::-1], bi[::-1]):                        # the smallest i of every j
            want[j] = i
        assert np.array_equal(got, want)
        assert (got >= 0).sum() > 20 and (got < 0).sum() > (5 if null_equal else 20)


# ---- lookup_join_pairs' torch half, here on the CPU ------------------------------------------------------------
def test_expand_first_against_a_double_loop():
    torch = pytest.importorskip("torch")
    from fury_amd.lookup import expand_first
    rng = np.random.default_rng(14)
    for nb, n in ((1, 1), (37, 23), (23, 37), (64, 200)):
        keys_b = rng.integers(0, 5, nb)
        keys_p = rng.integers(0, 7, n)                              # 5 and 6: not in the build side
        first = np.array([np.flatnonzero(keys_b == k)[0] for k in keys_b], np.int64)
        found = np.array([np.flatnonzero(keys_b == k)[0] if (keys_b == k).any() else -1 for k in keys_p],
                         np.int64)
        want = [(j, i) for j in range(n) for i in range(nb) if keys_p[j] == keys_b[i]]
        pj, bi = expand_first(torch.from_numpy(found), torch.from_numpy(first))
        assert pj.dtype == torch.int64 and bi.dtype == torch.int64
        assert list(zip(pj.tolist(), bi.tolist())) == want, (nb, n)
        if nb > 1:
            assert len(want) > n                                     # runs of several build rows
    # no probe row finds anything; an empty side
    none = torch.full((4,), -1, dtype=torch.int64)
    pj, bi = expand_first(none, torch.zeros(3, dtype=torch.int64))
    assert pj.numel() == 0 and bi.numel() == 0
    for found, first in ((none[:0], torch.zeros(3, dtype=torch.int64)), (none, none[:0])):
        pj, bi = expand_first(found, first)
        assert pj.numel() == 0 and bi.numel() == 0 and pj.dtype == torch.int64


def test_expand_first_is_the_join_model_and_respects_max_pairs():
    torch = pytest.importorskip("torch")
    from fury_amd.encoder import IllegalArgumentException
    from fury_amd.lookup import expand_first
    from tests.test_group_model import group_model
    rng = np.random.default_rng(15)
    nb, n = 80, 60
    fields, build = _random_keys(rng, nb)
    _, probe = _random_keys(rng, n)
    first = group_model(fields, build, nb)[0]
    for null_equal in (False, True):
        found = lookup_model((fields, build, nb), (fields, probe, n), null_equal)
        pj, bi = expand_first(torch.from_numpy(found), torch.from_numpy(first))
        wj, wi = join_model(fields, probe, n, fields, build, nb, null_equal)
        assert np.array_equal(pj.numpy(), wj) and np.array_equal(bi.numpy(), wi)
        assert len(wj) > n
        with pytest.raises(IllegalArgumentException, match=f"{len(wj)} pairs exceed max_pairs"):
            expand_first(torch.from_numpy(found), torch.from_numpy(first), max_pairs=len(wj) - 1)
        assert expand_first(torch.from_numpy(found), torch.from_numpy(first), max_pairs=len(wj))[0].numel() == len(wj)
