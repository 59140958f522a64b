"""A Python model of fury_row_compare / fury_row_order_words, written from rules 1-6 of
include/fury_row.h alone over decoded key tuples (tests/test_keys_equal_model.py's key_tuples: the
value bytes of every key, None for a null), and its pins without a GPU: the order against Python's own
ordering of the decoded values, antisymmetry and transitivity, rule 5 against the equality model, the
order words against the comparison, and the two host loops of fury_amd.order (refine_order,
search_bounds) driven by the model on CPU tensors.  The GPU tests (tests/test_order.py) compare the
kernels with this model applied to the oracle's decode."""
from __future__ import annotations

import bisect
import functools
import itertools
import struct

import numpy as np
import pytest

from fury_amd import types as T
from fury_amd.workloads import Column
from tests.test_hash_model import fixed_column, string_column
from tests.test_keys_equal_model import key_tuples, keys_equal_model

DESC, NULLS_LAST = 1, 2
ALL_FLAGS = (0, DESC, NULLS_LAST, DESC | NULLS_LAST)
SIGNED = (T.INT8, T.INT16, T.INT32, T.INT64, T.DATE32, T.TIMESTAMP)
FLOATS = (T.FLOAT32, T.FLOAT64)
M64 = (1 << 64) - 1


def sign(x):
    return (x > 0) - (x < 0)


# ---- rule 3 over a decoded value: a Python object whose own order is the rule ------------------------------------
def decoded(tid, v: bytes):
    """The value bytes of rule 3 of fury_row_hash (little-endian) as a Python object that orders as
    rule 3 of fury_row_compare says."""
    if tid == T.BOOL:
        return v[0] != 0
    if tid in SIGNED or tid == T.DECIMAL:
        return int.from_bytes(v, "little", signed=True)
    if tid in FLOATS:                             # totalOrder: sign-magnitude of the raw bits
        bits = int.from_bytes(v, "little")
        top = 1 << (8 * len(v) - 1)
        return -(bits - top) - 1 if bits & top else bits
    assert tid in (T.STRING, T.BINARY)
    return bytes(v)                               # Python orders bytes unsigned, a prefix first


def compare_value(tid, a, b, flags=0):
    """Rules 2-4 for one key position; a / b: value bytes or None."""
    if a is None or b is None:
        if a is None and b is None:
            return 0
        first = (a is None) != bool(flags & NULLS_LAST)
        return -1 if first else 1
    x, y = decoded(tid, a), decoded(tid, b)
    c = sign((x > y) - (x < y))
    return -c if flags & DESC else c


def compare_model(tids, ra, rb, flags=None):
    """Rule 1: the first key position that differs decides.  ra / rb: key tuples."""
    flags = flags or [0] * len(tids)
    for t, a, b, f in zip(tids, ra, rb, flags):
        c = compare_value(t, a, b, f)
        if c:
            return c
    return 0


def compare_pairs_model(fields_l, cols_l, idx_l, fields_r, cols_r, idx_r, flags, n_l, n_r):
    """out_cmp of fury_row_compare as an int8 array, shaped like keys_equal_model.  A row outside its
    batch has every key null (rule 6)."""
    tids = [f.type_id for f in fields_l]
    tl, tr = key_tuples(fields_l, cols_l, n_l), key_tuples(fields_r, cols_r, n_r)
    num = len(idx_l) if idx_l is not None else len(idx_r) if idx_r is not None else min(n_l, n_r)
    L = range(num) if idx_l is None else [int(i) for i in idx_l]
    R = range(num) if idx_r is None else [int(i) for i in idx_r]
    nulls = (None,) * len(tids)
    return np.array([compare_model(tids, tl[i] if 0 <= i < n_l else nulls, tr[j] if 0 <= j < n_r else nulls, flags)
                     for i, j in zip(L, R)], np.int8).reshape(num)


# ---- NK and the chunk words --------------------------------------------------------------------------------------
def nk(tid, v: bytes) -> bytes:
    """The normalised key bytes: unsigned lexicographic order, prefix smaller, is rule 3."""
    if tid == T.BOOL:
        return bytes([int(v[0] != 0)])
    if tid in (T.STRING, T.BINARY):
        return bytes(v)
    be = bytearray(reversed(v))
    if tid in FLOATS and be[0] & 0x80:
        return bytes(b ^ 0xFF for b in be)
    be[0] ^= 0x80
    return bytes(be)


def word_model(tid, v, chunk, flags=0):
    """The signed 64-bit word of fury_row_order_words for one value (None: null)."""
    if v is None:
        w = M64 if flags & NULLS_LAST else 0
    else:
        k = nk(tid, v)
        part = k[7 * chunk:7 * chunk + 7]
        low = 9 if len(k) > 7 * chunk + 7 else 1 + len(part)
        w = int.from_bytes(part.ljust(7, b"\0"), "big") << 8 | low
        if flags & DESC:
            w ^= M64
    w ^= 1 << 63
    return w - (1 << 64) if w >> 63 else w


def word_more(w, flags=0):
    """The "more follows" state of a word, as fury_amd.order.word_continues reads it."""
    return ((~w if flags & DESC else w) & 0xFF) == 9


def compare_by_words(tid, a, b, flags):
    """The order of two values decided through their words alone, chunk after chunk, as the header
    says a sort may: differing words decide; equal "ended" words are equal values; equal "more" words
    pass to the next chunk."""
    for chunk in range(1 << 20):
        wa, wb = word_model(tid, a, chunk, flags), word_model(tid, b, chunk, flags)
        if wa != wb:
            return sign(wa - wb)
        if not word_more(wa, flags):
            return 0
    raise AssertionError("no end")


# ---- the value sets ------------------------------------------------------------------------------------------------
def _ints(w):
    lo, hi = -(1 << (8 * w - 1)), (1 << (8 * w - 1)) - 1
    vals = [lo, lo + 1, -257, -256, -2, -1, 0, 1, 2, 255, 256, hi - 1, hi]
    return [x.to_bytes(w, "little", signed=True) for x in vals if lo <= x <= hi]


def _floats(fmt, w, hi_nan):
    sgn = 1 << (8 * w - 1)
    bits = [hi_nan, hi_nan + 1, hi_nan | sgn, (hi_nan + 1) | sgn, 1, 2, sgn | 1, 0, sgn]       # NaNs, denormals, zeros
    out = [b.to_bytes(w, "little") for b in bits]
    for x in (float("inf"), float("-inf"), 1.0, -1.0, 1.5, -1.5, 3e38, -3e38, 1e-30):
        out.append(struct.pack(fmt, x))
    return out


def _decimals():
    vals = [0, 1, -1, (1 << 63), (1 << 63) + 1, (1 << 63) - 1, (1 << 64), (1 << 64) + (1 << 63), -(1 << 64),
            -(1 << 63), (1 << 126), -(1 << 126), (1 << 127) - 1, -(1 << 127), 5 << 64, (5 << 64) + (1 << 63)]
    return [x.to_bytes(16, "little", signed=True) for x in vals]


STRINGS = [b"", b"a", b"a\0", b"a\0\0", b"ab", b"ba", b"b", b"\x7f", b"\x80", b"\xff", b"abcdef", b"abcdefg",
           b"abcdefgh", b"abcdefg\0", b"abcdefgi", b"abcdefghijklmn", b"abcdefghijklmnz", b"abcdefghijklm\x80",
           b"x" * 31, b"x" * 32, b"x" * 33, b"x" * 32 + b"\0", b"x" * 40, b"x" * 39 + b"y"]

VALUE_SETS = {
    T.BOOL: [b"\0", b"\1"],
    T.INT8: _ints(1), T.INT16: _ints(2), T.INT32: _ints(4), T.INT64: _ints(8),
    T.DATE32: _ints(4), T.TIMESTAMP: _ints(8),
    T.FLOAT32: _floats("<f", 4, 0x7FC00000), T.FLOAT64: _floats("<d", 8, 0x7FF8000000000000),
    T.DECIMAL: _decimals(), T.STRING: STRINGS, T.BINARY: STRINGS,
}


def test_value_sets_are_what_the_rules_name():
    assert decoded(T.BOOL, b"\x02") is True and nk(T.BOOL, b"\x02") == b"\1"
    f64 = lambda x: struct.pack("<d", x)                            # noqa: E731
    order = [bytes.fromhex("010000000000f8ff"), f64(float("-inf")), f64(-1.0), f64(-0.0), f64(0.0), f64(1.0),
             f64(float("inf")), bytes.fromhex("000000000000f87f"), bytes.fromhex("010000000000f87f")]
    for a, b in zip(order, order[1:]):
        assert compare_value(T.FLOAT64, a, b) == -1 and compare_value(T.FLOAT64, b, a, DESC) == -1
    # the high payload of a negative NaN is the smallest of all
    assert compare_value(T.FLOAT64, bytes.fromhex("020000000000f8ff"), order[0]) == -1
    d = lambda x: x.to_bytes(16, "little", signed=True)             # noqa: E731
    assert compare_value(T.DECIMAL, d((1 << 63) - 1), d(1 << 63)) == -1      # the low half is unsigned
    assert compare_value(T.DECIMAL, d(-1), d(0)) == -1 and compare_value(T.DECIMAL, d(1 << 64), d(M64)) == 1
    assert compare_value(T.STRING, b"a", b"a\0") == -1 and compare_value(T.STRING, b"\x7f", b"\x80") == -1
    assert compare_value(T.STRING, b"ab", b"ba") == -1
    # rule 2: absolute, DESC does not flip it
    for f in ALL_FLAGS:
        assert compare_value(T.STRING, None, b"", f) == (1 if f & NULLS_LAST else -1)
        assert compare_value(T.STRING, None, None, f) == 0
    # UTF-8 bytes order by code point: U+FFFF before U+10000, where UTF-16 code units say the opposite
    a, b = "\uffff", "\U00010000"
    assert compare_value(T.STRING, a.encode(), b.encode()) == -1
    assert a.encode("utf-16-be") > b.encode("utf-16-be")


@pytest.mark.parametrize("tid", list(VALUE_SETS))
def test_order_is_pythons_order_of_the_decoded_values(tid):
    vals = VALUE_SETS[tid] + [None]
    for flags in ALL_FLAGS:
        cmp = lambda a, b: compare_value(tid, a, b, flags)           # noqa: E731
        got = sorted(vals, key=functools.cmp_to_key(cmp))
        real = sorted((v for v in vals if v is not None), key=lambda v: decoded(tid, v), reverse=bool(flags & DESC))
        assert got == ([None] + real if not flags & NULLS_LAST else real + [None])
        for a, b in itertools.product(vals, repeat=2):               # antisymmetry
            assert cmp(a, b) == -cmp(b, a)
        for a, b, c in itertools.product(vals, repeat=3):            # transitivity
            if cmp(a, b) <= 0 and cmp(b, c) <= 0:
                assert cmp(a, c) <= 0
        # NK: unsigned lexicographic order of the normalised bytes is rule 3
        for a, b in itertools.product(VALUE_SETS[tid], repeat=2):
            assert sign((nk(tid, a) > nk(tid, b)) - (nk(tid, a) < nk(tid, b))) == compare_value(tid, a, b)


def _column(tid, vals):
    nulls = [i for i, v in enumerate(vals) if v is None]
    if tid in (T.STRING, T.BINARY):
        return string_column(vals)
    valid = np.ones(len(vals), bool)
    valid[nulls] = False
    validity = np.packbits(valid, bitorder="little")
    if tid == T.BOOL:
        return Column(values=np.packbits([bool(v and v[0]) for v in vals], bitorder="little"), validity=validity)
    w = len(VALUE_SETS[tid][0])
    raw = b"".join(v or bytes(w) for v in vals)
    return Column(values=np.frombuffer(raw, np.uint8).copy(), validity=validity)


@pytest.mark.parametrize("tid", list(VALUE_SETS))
def test_rule_5_zero_iff_keys_equal_with_null_equal(tid):
    vals = VALUE_SETS[tid] + [None]
    n = len(vals)
    f, c = T.field("k", tid), _column(tid, vals)
    assert key_tuples([f], [c], n) == [(v,) for v in vals]
    li, ri = np.divmod(np.arange(n * n), n)
    eq = keys_equal_model([f], [c], li, [f], [c], ri, True, n_l=n, n_r=n)
    for flags in ALL_FLAGS:
        cmp = compare_pairs_model([f], [c], li, [f], [c], ri, [flags], n, n)
        assert np.array_equal(cmp == 0, eq == 1)
    assert eq.sum() == n                                              # the values are distinct


@pytest.mark.parametrize("tid", list(VALUE_SETS))
def test_word_order_agrees_with_compare(tid):
    vals = VALUE_SETS[tid] + [None]
    for flags in ALL_FLAGS:
        for a, b in itertools.product(vals, repeat=2):
            assert compare_by_words(tid, a, b, flags) == compare_value(tid, a, b, flags), (a, b, flags)
        for v in vals:
            chunks = 0 if v is None else max(len(nk(tid, v)) - 1, 0) // 7
            for c in range(chunks + 2):
                w = word_model(tid, v, c, flags)
                assert -(1 << 63) <= w < (1 << 63)
                assert word_more(w, flags) == (v is not None and c < chunks)
            if v is not None:                                          # a chunk past the end: no value bytes
                past = word_model(tid, v, chunks + 1, flags) ^ -(1 << 63)
                assert (~past if flags & DESC else past) & M64 == 1
    assert word_model(T.INT64, None, 0, 0) == -(1 << 63) and word_model(T.INT64, None, 3, NULLS_LAST) == (1 << 63) - 1
    assert word_model(T.STRING, b"ab", 0) == ((0x6162 << 48) | 3) - (1 << 63)
    assert word_model(T.INT8, b"\xff", 0) == ((0x7F << 56) | 2) - (1 << 63)


# ---- the host loops of fury_amd.order over the model ----------------------------------------------------------------
def model_source(tids, rows, flags):
    """refine_order's word source over key tuples, on CPU tensors."""
    import torch

    def source(key, chunk, idx):
        return torch.tensor([word_model(tids[key], rows[int(i)][key], chunk, flags[key]) for i in idx],
                            dtype=torch.int64)
    return source


def sorted_model(tids, rows, flags):
    """The stable permutation, by Python's sort (stable) under the model comparator."""
    cmp = lambda i, j: compare_model(tids, rows[i], rows[j], flags)  # noqa: E731
    return sorted(range(len(rows)), key=functools.cmp_to_key(cmp))


def _key_sets():
    rng = np.random.default_rng(11)
    pick = lambda tid, n, nulls=0.1: [None if rng.random() < nulls else VALUE_SETS[tid][int(i)]      # noqa: E731
                                      for i in rng.integers(0, len(VALUE_SETS[tid]), n)]
    n = 150
    sets = {}
    for tid in VALUE_SETS:
        sets[f"one key {tid}"] = ([tid], list(zip(pick(tid, n))))
    sets["all equal"] = ([T.STRING, T.INT64], [(b"abcdefghijklmnop", (5).to_bytes(8, "little"))] * 40)
    sets["all null"] = ([T.STRING], [(None,)] * 9)
    sets["all distinct"] = ([T.INT64], [(int(x).to_bytes(8, "little", signed=True),)
                                        for x in rng.permutation(200) - 100])
    hot = [(b"the hot key of the batch",) if rng.random() < 0.9 else (bytes(rng.integers(97, 100, 3).tolist()),)
           for _ in range(n)]
    sets["one hot key"] = ([T.STRING], hot)
    sets["string then int"] = ([T.STRING, T.INT32], list(zip(pick(T.STRING, n), pick(T.INT32, n))))
    sets["first key ties"] = ([T.BOOL, T.DECIMAL, T.FLOAT64],
                              list(zip(pick(T.BOOL, n, 0.0), pick(T.DECIMAL, n), pick(T.FLOAT64, n))))
    sets["long shared prefix"] = ([T.BINARY], [(b"p" * 30 + bytes([int(x)]),) for x in rng.integers(0, 4, n)])
    sets["one row"] = ([T.INT8], [(b"\x01",)])
    sets["no rows"] = ([T.INT8], [])
    return sets


KEY_SETS = _key_sets()


@pytest.mark.parametrize("name", list(KEY_SETS))
def test_refinement_loop_is_a_stable_sort(name):
    torch = pytest.importorskip("torch")
    from fury_amd.order import refine_order
    tids, rows = KEY_SETS[name]
    rng = np.random.default_rng(len(rows))
    combos = [[f] * len(tids) for f in ALL_FLAGS] + [[int(x) for x in rng.integers(0, 4, len(tids))]]
    for flags in combos:
        perm = refine_order(len(rows), len(tids), [bool(f & DESC) for f in flags],
                            model_source(tids, rows, flags), torch.device("cpu"))
        assert perm.dtype == torch.int64
        assert perm.tolist() == sorted_model(tids, rows, flags), (name, flags)


def test_refinement_reads_only_what_still_ties():
    """A key whose first chunk decides everything is read once, and the second key never."""
    torch = pytest.importorskip("torch")
    from fury_amd.order import refine_order
    tids = [T.INT32, T.STRING]
    rows = [(int(x).to_bytes(4, "little"), b"same") for x in (5, 3, 9, 1)]
    calls = []
    inner = model_source(tids, rows, [0, 0])

    def source(key, chunk, idx):
        calls.append((key, chunk, idx.numel()))
        return inner(key, chunk, idx)
    assert refine_order(4, 2, [False, False], source, torch.device("cpu")).tolist() == [3, 1, 0, 2]
    assert calls == [(0, 0, 4)]
    rows[1] = rows[0]
    calls.clear()
    assert refine_order(4, 2, [False, False], source, torch.device("cpu")).tolist() == [3, 0, 1, 2]
    assert calls == [(0, 0, 4), (1, 0, 2)]


@pytest.mark.parametrize("name", ["one key %d" % T.STRING, "one key %d" % T.FLOAT32, "string then int",
                                  "all equal", "one hot key", "no rows"])
def test_search_bounds_against_bisect(name):
    torch = pytest.importorskip("torch")
    from fury_amd.order import search_bounds
    tids, rows = KEY_SETS[name]
    probes = rows[::3] + [(None,) * len(tids)] + [tuple(VALUE_SETS[t][-1] for t in tids)]
    for f in ALL_FLAGS:
        flags = [f] * len(tids)
        srt = [rows[i] for i in sorted_model(tids, rows, flags)]
        key = functools.cmp_to_key(lambda a, b: compare_model(tids, a, b, flags))
        keyed = [key(r) for r in srt]

        def compare(mid):
            return torch.tensor([compare_model(tids, srt[int(i)], p, flags) if srt else 0
                                 for i, p in zip(mid, probes)], dtype=torch.int8)
        for right in (False, True):
            got = search_bounds(len(srt), len(probes), compare, right, torch.device("cpu")).tolist()
            want = [(bisect.bisect_right if right else bisect.bisect_left)(keyed, key(p)) for p in probes]
            assert got == want, (name, f, right)


def test_flags_per_key():
    from fury_amd.encoder import IllegalArgumentException
    from fury_amd.order import order_flags
    assert order_flags(3) == [0, 0, 0]
    assert order_flags(2, True, [False, True]) == [1, 3]
    assert order_flags(2, [True, False], True) == [3, 2]
    with pytest.raises(IllegalArgumentException, match="2 entries for 3 keys"):
        order_flags(3, [True, False])
