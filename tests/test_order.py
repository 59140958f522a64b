"""The order of rows on the GPU (fury_row_compare, fury_row_order_words; fury_amd.compare_into /
bind_compare / compare_rows / order_words_into / order_words / argsort_rows / sort_rows / is_sorted /
search_sorted).  Every output is compared in full, plus one guard entry, with the Python model of
tests/test_order_model.py (written from the header's rules alone) applied to the oracle's decode of
the batches.  Marked gpu."""
from __future__ import annotations

import bisect
import functools
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from fury_amd import types as T  # noqa: E402
from fury_amd.workloads import Column  # noqa: E402
from tests import high_offsets as H  # noqa: E402
from tests import test_keys_equal as KE  # noqa: E402
from tests import test_order_model as M  # noqa: E402
from tests.test_bounds import _corrupt  # noqa: E402
from tests.test_hash import case  # noqa: E402
from tests.test_hash_model import fixed_column  # noqa: E402
from tests.test_keys_equal_model import key_tuples  # noqa: E402
from tests.test_take import _device_src, _Src, assert_same  # noqa: E402

BYTE_GUARD = 0x5A
WORD_GUARD = 0x5A5A5A5A5A5A5A5A
MORE_GUARD = 0x5A5A5A5A
COUNTS = [1, 63, 64, 65, 257, 4097]
DESC, NULLS_LAST = M.DESC, M.NULLS_LAST
ALL_FLAGS = M.ALL_FLAGS


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


# ---- the model over a side -------------------------------------------------------------------------------------
_TUPLES: dict = {}


def tuples(b, keys):
    """(type ids, key tuples of every row) of the side `b` (a KE._Batch) for `keys`, made once."""
    k = (id(b), tuple(keys))
    if k not in _TUPLES:
        f, c = b.cols(keys)
        _TUPLES[k] = ([x.type_id for x in f], key_tuples(f, c, b.n), b)      # b: keeps the id its own
    return _TUPLES[k][:2]


def forget(b):
    """Drops the tuples of a side made for one test, and with them the side and its device memory."""
    for k in [k for k, v in _TUPLES.items() if v[2] is b]:
        del _TUPLES[k]


def at_edge(b, rows, offs):
    """The side `b` over `rows` / `offs`, the rows ending where a device allocation of their own ends:
    a read past the batch's last byte would leave the allocation.  The caching allocator serves a
    request from a cached block when one is large enough, and only a block that is a whole new segment
    ends at an allocation's end; such a block starts at a 2 MiB boundary.  Garbage is collected and the
    cache emptied first, then the request is doubled up to 1 GiB to outgrow what is cached.  Run alone,
    the first request gets a segment of its own.  In the whole suite a live tensor of an earlier module
    pins the 6 GiB segment of a high-offset arena, every request is carved out of it, and the test
    warns: it still checks every result, and only a read past the batch's end could go unnoticed."""
    import gc
    import warnings
    from fury_amd.encoder import RowBatch
    out = b.with_rows(rows, offs)
    dev = out.batch.rows.device
    assert len(rows) % 8 == 0
    size = 32 << 20
    while True:
        gc.collect()
        torch.cuda.empty_cache()
        keep = torch.empty(size, dtype=torch.uint8, device=dev)
        if keep.data_ptr() % (2 << 20) == 0 or size >= (1 << 30):
            break
        del keep
        size *= 2
    if keep.data_ptr() % (2 << 20):
        warnings.warn("the truncated batch does not end at the end of a device allocation")
    t = keep[keep.numel() - len(rows):]
    t.copy_(torch.from_numpy(np.ascontiguousarray(rows)))
    out.keep = keep
    out.batch = RowBatch(t, out.batch.row_offsets, out.n, out.enc.schema_hash)
    return out


def want_compare(tids, tl, lidx, tr, ridx, flags):
    """out_cmp over key tuples; a row outside its batch has every key null (rule 6)."""
    num = len(lidx) if lidx is not None else len(ridx) if ridx is not None else min(len(tl), len(tr))
    L = range(num) if lidx is None else [int(i) for i in lidx]
    R = range(num) if ridx is None else [int(i) for i in ridx]
    nulls = (None,) * len(tids)
    return np.array([M.compare_model(tids, tl[i] if 0 <= i < len(tl) else nulls,
                                     tr[j] if 0 <= j < len(tr) else nulls, flags) for i, j in zip(L, R)],
                    np.int8).reshape(num)


def _opts(flags):
    return [bool(f & DESC) for f in flags], [bool(f & NULLS_LAST) for f in flags]


def _dev_idx(idx, dev):
    return None if idx is None else torch.from_numpy(np.asarray(idx, np.int64)).to(dev)


def run_compare(left, lkeys, lidx, right, rkeys, ridx, flags, what, stream=None, bound=False, want=None):
    """One compare_into call into a guarded output, compared in full with the model."""
    from fury_amd import KeySide, bind_compare, compare_into
    dev = left.batch.rows.device
    if want is None:
        tids, tl = tuples(left, lkeys)
        want = want_compare(tids, tl, lidx, tuples(right, rkeys)[1], ridx, flags)
    n = len(want)
    out = torch.full((n + 1,), BYTE_GUARD, dtype=torch.int8, device=dev)
    desc, last = _opts(flags)
    args = (KeySide(left.enc, left.batch, lkeys, _dev_idx(lidx, dev)),
            KeySide(right.enc, right.batch, rkeys, _dev_idx(ridx, dev)), out[:n], desc, last)
    torch.cuda.synchronize()
    if bound:
        call = bind_compare(*args, stream=stream)
        call()
        call()
    else:
        compare_into(*args, stream=stream)
    torch.cuda.synchronize()
    assert_same(out.cpu().numpy(), np.concatenate([want, [BYTE_GUARD]]).astype(np.int8), f"{what}: out_cmp")
    return want


def want_words(tid, tup, idx, chunk, flag):
    rows = range(len(tup)) if idx is None else [int(i) for i in idx]
    vals = [tup[r][0] if 0 <= r < len(tup) else None for r in rows]
    words = [M.word_model(tid, v, chunk, flag) for v in vals]
    return np.array(words, np.int64).reshape(len(vals)), int(any(M.word_more(w, flag) for w in words))


def run_words(b, key, chunk, idx, flag, what, stream=None, want=None, more=True):
    """One order_words_into call into guarded outputs, compared in full with the model."""
    from fury_amd import order_words_into
    dev = b.batch.rows.device
    if want is None:
        (tid,), tup = tuples(b, [key])
        want = want_words(tid, tup, idx, chunk, flag)
    m = len(want[0])
    words = torch.full((m + 1,), WORD_GUARD, dtype=torch.int64, device=dev)
    flagw = torch.full((2,), MORE_GUARD, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    order_words_into(b.enc, b.batch, key, chunk, words[:m], flagw[:1] if more else None, _dev_idx(idx, dev),
                     bool(flag & DESC), bool(flag & NULLS_LAST), stream=stream)
    torch.cuda.synchronize()
    assert_same(words.cpu().numpy(), np.concatenate([want[0], [WORD_GUARD]]).astype(np.int64), f"{what}: words")
    assert flagw.cpu().tolist() == [want[1] if more else MORE_GUARD, MORE_GUARD], f"{what}: out_more"
    return want


def _make(oracle, dev, fields, host, n):
    from fury_amd.encoder import Encoders
    enc = Encoders.bean(fields, device=dev)
    return KE._Batch(oracle, enc, fields, _device_src(_Src(dev, enc, host, n), 0))


# ---- 1. the values the rules name, type by type ---------------------------------------------------------------------
def _string_values():
    """The model's strings, and for every length of the list a value, the same with another first byte
    (>= 0x80 against < 0x80) and the same with another last byte."""
    rng = np.random.default_rng(3)
    out = list(M.STRINGS)
    for n in (1, 6, 7, 8, 9, 13, 14, 15, 31, 32, 33, 40):
        v = rng.integers(1, 0x7F, n, dtype=np.uint8).tobytes()
        out += [v, bytes([v[0] | 0x80]) + v[1:], v[:-1] + bytes([v[-1] ^ 1])]
    assert len(set(out)) == len(out)
    return out


VALUES = dict(M.VALUE_SETS)
VALUES[T.STRING] = VALUES[T.BINARY] = _string_values()


_DTYPES = {T.INT8: np.int8, T.INT16: np.int16, T.INT32: np.int32, T.INT64: np.int64, T.DATE32: np.int32,
           T.TIMESTAMP: np.int64, T.FLOAT32: np.float32, T.FLOAT64: np.float64}


def _col(tid, vals):
    if tid in (T.STRING, T.BINARY):
        return KE.string_column(vals)
    c = M._column(tid, vals)
    values = np.array(c.values)
    if tid in _DTYPES:                                             # typed, as the encoder's callers pass them
        values = values.view(_DTYPES[tid])
    return Column(values=values, offsets=c.offsets, validity=np.array(c.validity))


def _type_sides(oracle, dev, tid):
    """Left: (id INT64, k) holding every value of the type and a null, fixed-size rows for a fixed-width
    k; right: (k, zz STRING), the values reversed, variable-length rows, k at another slot."""
    key = ("type", tid)
    if key not in KE._CACHE:
        vals = VALUES[tid] + [None]
        n = len(vals)
        left = _make(oracle, dev, [T.field("id", T.INT64), T.field("k", tid)],
                     [fixed_column(np.int64, np.arange(n)), _col(tid, vals)], n)
        right = _make(oracle, dev, [T.field("k", tid), T.field("zz", T.STRING)],
                      [_col(tid, vals[::-1]), KE.string_column([b"z" * (r % 5) for r in range(n)])], n)
        assert tuples(left, ["k"])[1] == [(v,) for v in vals]
        assert tuples(right, ["k"])[1] == [(v,) for v in vals[::-1]]
        assert not right.fixed and left.fixed == (tid not in (T.STRING, T.BINARY, T.DECIMAL))
        KE._CACHE[key] = (left, right)
    return KE._CACHE[key]


@pytest.mark.parametrize("tid", list(VALUES))
def test_values_of_every_type(oracle, dev, tid):
    """Every value against every value, under every DESC x NULLS_LAST combination, with indices on
    both sides, on one side and on none; each side takes each role."""
    left, right = _type_sides(oracle, dev, tid)
    n = left.n
    li, ri = np.divmod(np.arange(n * n), n)
    rev = np.arange(n)[::-1].copy()
    for flag in ALL_FLAGS:
        want = run_compare(left, ["k"], li, right, ["k"], ri, [flag], f"type {tid} flags {flag}")
        assert (want == 0).sum() == n and (want < 0).sum() == (want > 0).sum()
        run_compare(right, ["k"], ri, left, ["k"], li, [flag], f"type {tid} flags {flag}, swapped")
        same = run_compare(left, ["k"], None, right, ["k"], rev, [flag], f"type {tid} flags {flag}, left plain")
        assert not same.any()                                        # right row n - 1 - j holds left row j's value
        run_compare(left, ["k"], rev, right, ["k"], None, [flag], f"type {tid} flags {flag}, right plain")
        run_compare(left, ["k"], None, right, ["k"], None, [flag], f"type {tid} flags {flag}, no indices")
    left.enc.device_status()
    right.enc.device_status()


@pytest.mark.parametrize("tid", list(VALUES))
def test_order_words_of_every_type(oracle, dev, tid):
    """Chunks 0..3 and one past the end of the longest value, every flag combination, with and without
    indices and out_more."""
    left, right = _type_sides(oracle, dev, tid)
    longest = max(len(M.nk(tid, v)) for v in VALUES[tid])
    idx = np.random.default_rng(tid).integers(0, left.n, 100)
    for b in (left, right):
        for flag in ALL_FLAGS:
            seen = set()
            for chunk in sorted({0, 1, 2, 3, (longest - 1) // 7, (longest - 1) // 7 + 1}):
                w = run_words(b, "k", chunk, None, flag, f"type {tid} chunk {chunk} flags {flag}")
                seen.add(w[1])
                run_words(b, "k", chunk, idx, flag, f"type {tid} chunk {chunk} flags {flag}, indexed")
            assert seen == ({0, 1} if longest > 7 else {0})
            run_words(b, "k", 0, idx, flag, f"type {tid} flags {flag}, no out_more", more=False)
            run_words(b, "k", 2 ** 31 - 1, None, flag, f"type {tid} flags {flag}, the last chunk")
        b.enc.device_status()


@pytest.mark.parametrize("tid", list(VALUES))
def test_sort_of_every_type(oracle, dev, tid):
    """argsort_rows / sort_rows / is_sorted / search_sorted end to end on the values with duplicates:
    the stable permutation of the model, exactly."""
    from fury_amd import KeySide, argsort_rows, is_sorted, search_sorted, sort_rows
    left, right = _type_sides(oracle, dev, tid)
    n = left.n
    rng = np.random.default_rng(100 + tid)
    pick = torch.from_numpy(rng.integers(0, n, 3 * n)).to(dev)       # every value about three times
    for b in (left, right):
        dup = b.with_batch(b.enc.take(b.batch, pick))
        dup.ref = None
        tids, tup = tuples(b, ["k"])
        rows = [tup[int(i)] for i in pick.cpu()]
        for flag in ALL_FLAGS:
            desc, last = bool(flag & DESC), bool(flag & NULLS_LAST)
            want = M.sorted_model(tids, rows, [flag])
            perm = argsort_rows(dup.enc, dup.batch, ["k"], desc, last)
            assert perm.dtype == torch.int64 and perm.device.type == "cuda"
            assert_same(perm.cpu().numpy(), np.array(want, np.int64), f"type {tid} flags {flag}: argsort")
            srt = sort_rows(dup.enc, dup.batch, ["k"], desc, last)
            assert is_sorted(dup.enc, srt, ["k"], desc, last)
            other = all(M.compare_model(tids, rows[i], rows[j], [flag ^ DESC]) <= 0 for i, j in zip(want, want[1:]))
            assert is_sorted(dup.enc, srt, ["k"], not desc, last) == other
            key = functools.cmp_to_key(lambda x, y: M.compare_model(tids, x, y, [flag]))
            keyed = [key(rows[i]) for i in want]
            for right_bound in (False, True):
                got = search_sorted(KeySide(dup.enc, srt, ["k"]), KeySide(b.enc, b.batch, ["k"]), right_bound,
                                    desc, last)
                find = bisect.bisect_right if right_bound else bisect.bisect_left
                assert_same(got.cpu().numpy(), np.array([find(keyed, key(t)) for t in tup], np.int64),
                            f"type {tid} flags {flag}: search_sorted right={right_bound}")
        b.enc.device_status()


# ---- 2. schema shapes x pair counts x key sets x index forms ------------------------------------------------------
ORDER_KEY_SETS = {
    "pair": [["a"], ["b", "a"]],
    "struct100": [[0], [99, 0, 50], list(range(36, 100))],
    "mixed": [["s1"], ["s2", "b", "s1"], ["b", "s3", "c", "a"]],
}


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("name", list(ORDER_KEY_SETS))
def test_matrix(oracle, dev, name, n):
    c = case(oracle, dev, name, n)
    left = KE.left_of(oracle, dev, c)
    rng = np.random.default_rng(n)
    for form in ["select"] + (["variable"] if name in ("pair", "struct100") else []):
        right = KE.right_of(oracle, dev, c, form)
        for keys in ORDER_KEY_SETS[name][:2 if n > 257 else None]:      # the model is Python: 64 keys up to 257 pairs
            names = KE._names(c, keys)
            seen = set()
            for mode, lidx, ridx in KE._modes(n, left.n, right.n, np.random.default_rng(7)):
                for flags in ([[0] * len(names)] if n <= 257 else []) + [[int(x) for x in rng.integers(0, 4, len(names))]]:
                    want = run_compare(left, names, lidx, right, names, ridx, flags,
                                       f"{name}/{form} n={n} keys {names} {mode} flags {flags}")
                    seen |= set(want.tolist())
            if n >= 63:
                assert seen == {-1, 0, 1}, (name, form, names)
    c.enc.device_status()
    right.enc.device_status()


def test_many_keys(oracle, dev):
    """The 70-field schema: 2 keys where the first (a BOOL) ties, 5 keys (more than one group of header
    loads), keys in two bitmap words, and 64 keys, the most a call takes."""
    c = case(oracle, dev, "keys", 257, 30)
    a, b = KE.left_of(oracle, dev, c), KE.right_of(oracle, dev, c)
    rng = np.random.default_rng(2)
    for keys in ([0, 9], [12, 24, 0, 9, 10], [63, 64], list(range(6, 70))):
        names = KE._names(c, keys)
        for left, right in ((a, b), (b, a)):
            seen = set()
            for mode, lidx, ridx in KE._modes(257, 257, 257, rng):
                for flags in ([0] * len(keys), [int(x) for x in rng.integers(0, 4, len(keys))]):
                    seen |= set(run_compare(left, names, lidx, right, names, ridx, flags,
                                            f"keys {keys} {mode} {flags}").tolist())
            assert seen == {-1, 0, 1}, keys
    # the first key ties and the second decides in a fair share of the pairs
    tids, tl = tuples(a, KE._names(c, [0, 9]))
    tr = tuples(b, KE._names(c, [0, 9]))[1]
    decided_late = sum(x[0] == y[0] and x[1] != y[1] for x, y in zip(tl, tr))
    assert decided_late >= 5
    c.enc.device_status()


# ---- 3. ORDER BY end to end ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
def test_argsort_mixed(oracle, dev, n):
    """The mixed schema with every row about three times (duplicate keys: stability), by one string, by
    several keys with per-key flags, then sort_rows / is_sorted / search_sorted on the result."""
    from fury_amd import KeySide, argsort_rows, is_sorted, search_sorted, sort_rows
    c = case(oracle, dev, "mixed", max(n // 3, 1))
    src = KE.left_of(oracle, dev, c)
    pick = np.random.default_rng(n).integers(0, src.n, n)
    batch = src.enc.take(src.batch, torch.from_numpy(pick).to(dev))
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    for keys, flags in ((["s1"], [0]), (["b", "s1"], [DESC, NULLS_LAST]), (["s2", "c", "a"], [3, 1, 0])):
        tids, tup = tuples(src, keys)
        rows = [tup[int(i)] for i in pick]
        want = M.sorted_model(tids, rows, flags)
        desc, last = _opts(flags)
        for stream in (None, s):
            perm = argsort_rows(src.enc, batch, keys, desc, last, stream=stream)
            torch.cuda.synchronize()
            assert_same(perm.cpu().numpy(), np.array(want, np.int64), f"n={n} keys {keys} flags {flags}")
        srt = sort_rows(src.enc, batch, keys, desc, last)
        assert srt.nrows == n and is_sorted(src.enc, srt, keys, desc, last)
        again = argsort_rows(src.enc, srt, keys, desc, last)
        assert_same(again.cpu().numpy(), np.arange(n, dtype=np.int64), "a sorted batch sorts to itself")
        key = functools.cmp_to_key(lambda x, y: M.compare_model(tids, x, y, flags))
        keyed = [key(rows[i]) for i in want]
        probes = np.random.default_rng(n + 1).integers(0, src.n, 50)
        for right_bound in (False, True):
            got = search_sorted(KeySide(src.enc, srt, keys), KeySide(src.enc, src.batch, keys, _dev_idx(probes, dev)),
                                right_bound, desc, last)
            find = bisect.bisect_right if right_bound else bisect.bisect_left
            assert_same(got.cpu().numpy(), np.array([find(keyed, key(tup[int(p)])) for p in probes], np.int64),
                        f"n={n} keys {keys}: search_sorted right={right_bound}")
    src.enc.device_status(s)
    src.enc.device_status()


def test_sorted_rows_decode_in_order(oracle, dev):
    """sort_rows gives the rows themselves: the oracle's decode of the sorted batch is the decoded rows
    in the model's order."""
    from fury_amd import sort_rows
    from tests.helpers import columns_to_beans
    c = case(oracle, dev, "mixed", 257)
    src = KE.left_of(oracle, dev, c)
    keys, flags = ["s3", "b"], [DESC | NULLS_LAST, 0]
    tids, tup = tuples(src, keys)
    want = M.sorted_model(tids, tup, flags)
    srt = sort_rows(src.enc, src.batch, keys, *_opts(flags))
    got = oracle.decode(src.fields, srt.rows.cpu().numpy(), srt.row_offsets.cpu().numpy(), srt.nrows)
    beans = columns_to_beans(src.fields, src.ref, src.n)
    assert columns_to_beans(src.fields, got, srt.nrows) == [beans[i] for i in want]
    src.enc.device_status()


# ---- 4. the bound form, a side stream, compare_rows -------------------------------------------------------------------
@pytest.mark.parametrize("name,keys", [("mixed", ["s2", "a"]), ("struct100", [0, 51])])
def test_bound_and_stream(oracle, dev, name, keys):
    from fury_amd import KeySide, compare_rows
    c = case(oracle, dev, name, 4097)
    left, right = KE.left_of(oracle, dev, c), KE.right_of(oracle, dev, c)
    names = KE._names(c, keys)
    rng = np.random.default_rng(5)
    lidx = rng.integers(0, 4097, 5000)
    ridx = np.where(rng.random(5000) < 0.5, lidx, rng.integers(0, 4097, 5000))
    flags = [DESC, NULLS_LAST]
    want = run_compare(left, names, lidx, right, names, ridx, flags, f"{name} eager")
    assert set(want.tolist()) == {-1, 0, 1}
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    run_compare(left, names, lidx, right, names, ridx, flags, f"{name} side stream", stream=s, want=want)
    run_compare(left, names, lidx, right, names, ridx, flags, f"{name} bound", bound=True, want=want)
    run_compare(left, names, lidx, right, names, ridx, flags, f"{name} bound, side stream", bound=True, stream=s,
                want=want)
    (tid,), tup = tuples(left, names[:1])
    ww = want_words(tid, tup, lidx, 0, DESC)
    run_words(left, names[0], 0, lidx, DESC, f"{name} words, side stream", stream=s, want=ww)
    c.enc.device_status(s)
    c.enc.device_status()
    got = compare_rows(KeySide(left.enc, left.batch, names, _dev_idx(lidx, dev)),
                       KeySide(right.enc, right.batch, names, _dev_idx(ridx, dev)), *_opts(flags))
    assert got.dtype == torch.int8
    assert_same(got.cpu().numpy(), want, f"{name} compare_rows")


# ---- 5. bounds ----------------------------------------------------------------------------------------------------------------
BOUNDS_N = KE.BOUNDS_N


def _expect(left, right, keys, lidx, ridx, patch, bad_pairs, what):
    """compare_into over sides of which `patch` = {(side, row): {key: value}} says what rule 6 makes of
    the corrupt values: the model's result with those, and device_status names one of `bad_pairs`."""
    from fury_amd.encoder import IndexOutOfBoundsException
    tids, tl = tuples(left, keys)
    tr = tuples(right, keys)[1]
    tl, tr = list(tl), list(tr)
    for (side, row), change in patch.items():
        t = tl if side == "left" else tr
        t[row] = tuple(change.get(k, v) for k, v in zip(keys, t[row]))
    for flags in ([0] * len(keys), [NULLS_LAST | DESC] * len(keys)):
        want = want_compare(tids, tl, lidx, tr, ridx, flags)
        left.enc.device_status()
        run_compare(left, keys, lidx, right, keys, ridx, flags, f"{what} flags {flags}", want=want)
        if bad_pairs:
            with pytest.raises(IndexOutOfBoundsException) as e:
                left.enc.device_status()
            assert H.row_of(str(e.value)) in set(bad_pairs), (what, str(e.value))
        left.enc.device_status()                                   # clean (again)
    return want


@pytest.mark.parametrize("side", ["left", "right"])
def test_indices_outside_the_batch(oracle, dev, side):
    """The row has every key null: it sorts first (or last) and equals another such row."""
    left, right = KE._bounds_sides(oracle, dev)
    lidx, ridx = KE._bounds_pairs()
    for j, bad in ((3, -1), (100, BOUNDS_N), (256, 2 ** 40)):
        li, ri = lidx.copy(), ridx.copy()
        (li if side == "left" else ri)[j] = bad
        want = _expect(left, right, ["id", "s"], li, ri, {}, [j], f"{side} index {bad}")
        assert want[j] == (1 if side == "left" else -1)              # NULLS_LAST in the last run
    li, ri = lidx.copy(), ridx.copy()
    li[7], ri[7] = -5, BOUNDS_N + 5
    assert _expect(left, right, ["id", "s"], li, ri, {}, [7], "both indices")[7] == 0


@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("how", H.MALFORMED)
def test_corrupt_key_slots(oracle, dev, side, how):
    """tests/test_bounds.py's corruptions on the key field s of one row: the value is null and the pair
    is named.  huge_list_count only changes a STRING's payload: the model over the new decode."""
    from fury_amd.encoder import IndexOutOfBoundsException
    left, right = KE._bounds_sides(oracle, dev)
    lidx, ridx = KE._bounds_pairs()
    hit = left if side == "left" else right
    r, j = KE._victim(hit, lidx if side == "left" else ridx)
    k = hit.enc._select(["s"])[0]
    rows = _corrupt(hit.fields, hit.rows, hit.offs, BOUNDS_N, r, k, how)
    assert not np.array_equal(rows, hit.rows)
    bad = hit.with_rows(rows)
    if how == "huge_list_count":
        bad.ref = oracle.decode(bad.fields, rows, bad.offs, BOUNDS_N)
        patch, fails = {}, []
    else:
        patch, fails = {(side, r): {"s": None}}, [j]
    sides = (bad, right) if side == "left" else (left, bad)
    _expect(*sides, ["id", "s"], lidx, ridx, patch, fails, f"{how} on the {side}")
    # the key order does not decide whether the failure is seen: id differs first in some pairs
    _expect(*sides, ["s", "id"], lidx, ridx, patch, fails, f"{how} on the {side}, s first")
    # the order words of the corrupt value are a null's, and the output is named
    (tid,), tup = tuples(bad, ["s"])
    tup = list(tup)
    if fails:
        tup[r] = (None,)
    pos = (lidx if side == "left" else ridx)
    for flag in (0, NULLS_LAST | DESC):
        for chunk in (0, 1):
            bad.enc.device_status()
            run_words(bad, "s", chunk, pos, flag, f"{how}: words", want=want_words(tid, tup, pos, chunk, flag))
            if fails:
                with pytest.raises(IndexOutOfBoundsException) as e:
                    bad.enc.device_status()
                assert H.row_of(str(e.value)) == j
    bad.enc.device_status()
    forget(bad)


@pytest.mark.parametrize("side", ["left", "right"])
def test_corrupt_slots_of_fields_that_are_not_keys(oracle, dev, side):
    left, right = KE._bounds_sides(oracle, dev)
    lidx, ridx = KE._bounds_pairs()
    hit = left if side == "left" else right
    k = hit.enc._select(["t"])[0]
    rows = hit.rows
    for r, how in ((0, "offset_past_end"), (130, "size_past_end"), (BOUNDS_N - 1, "negative_size"),
                   (60, "huge_list_count")):
        def usable(r):                                             # not null, and 8 bytes of its own
            base = int(hit.offs[r])
            size = struct.unpack_from("<Q", hit.rows, base + 8 + 8 * k)[0] & 0xFFFFFFFF
            return not (hit.rows[base + (k >> 3)] >> (k & 7)) & 1 and size >= 1
        while not usable(r):
            r = (r + 1) % BOUNDS_N
        rows = _corrupt(hit.fields, rows, hit.offs, BOUNDS_N, r, k, how)
    assert not np.array_equal(rows, hit.rows)
    bad = hit.with_rows(rows)                                      # .ref stays: id and s are untouched
    sides = (bad, right) if side == "left" else (left, bad)
    _expect(*sides, ["id", "s"], lidx, ridx, {}, [], f"non-key corruption on the {side}")
    run_words(bad, "s", 0, None, 0, "non-key corruption: words")
    bad.enc.device_status()
    forget(bad)


@pytest.mark.parametrize("side", ["left", "right"])
def test_truncated_batch(oracle, dev, side):
    """row_offsets[n] cut 8 bytes into the last row's s payload, the rows at the very end of a device
    allocation: the last row's value leaves the batch and is null."""
    left, right = KE._bounds_sides(oracle, dev)
    lidx, ridx = KE._bounds_pairs()
    hit = left if side == "left" else right
    k = hit.enc._select(["s"])[0]
    last = BOUNDS_N - 1
    base = int(hit.offs[last])
    assert not (hit.rows[base + (k >> 3)] >> (k & 7)) & 1
    slot = struct.unpack_from("<Q", hit.rows, base + 8 + 8 * k)[0]
    assert (slot & 0xFFFFFFFF) > 8
    cut = base + (slot >> 32) + 8
    assert cut % 8 == 0 and cut < int(hit.offs[BOUNDS_N])
    offs = hit.offs.copy()
    offs[BOUNDS_N] = cut
    bad = at_edge(hit, hit.rows[:cut].copy(), offs)
    (j,) = np.flatnonzero((lidx if side == "left" else ridx) == last)
    sides = (bad, right) if side == "left" else (left, bad)
    _expect(*sides, ["id", "s"], lidx, ridx, {(side, last): {"s": None}}, [int(j)], f"truncated {side}")
    # s is not a key: the row's header is inside the batch and nothing else is looked at
    _expect(*sides, ["id"], lidx, ridx, {}, [], f"truncated {side}, key id")
    (tid,), tup = tuples(bad, ["s"])
    tup = list(tup)
    tup[last] = (None,)
    from fury_amd.encoder import IndexOutOfBoundsException
    for chunk in (0, 1, 2):                                        # the payload's first 8 bytes are inside
        run_words(bad, "s", chunk, None, 0, f"truncated {side}: words", want=want_words(tid, tup, None, chunk, 0))
        with pytest.raises(IndexOutOfBoundsException) as e:
            bad.enc.device_status()
        assert H.row_of(str(e.value)) == last
    forget(bad)
    del bad
    torch.cuda.empty_cache()


# ---- 6. batches that cross byte 2^31 and byte 2^32 of their buffer -----------------------------------------------------------
def test_high_offsets(oracle, dev):
    """The functions are not RowEncoder methods, so the placement matrix of tests/high_offsets.py does
    not reach them: its mixed batch at one placement of each boundary and kind, compared, turned into
    order words and sorted, against the same calls at base 0."""
    from fury_amd import KeySide, argsort_rows, compare_into, order_words
    from fury_amd.encoder import RowBatch
    from tests.test_high_offsets_gpu import Arena, device_batch, encoder
    ref = H.ref(oracle, "mixed")
    n, keys = ref.n, H.SPEC["mixed"]["hash"]
    enc = encoder(dev, "mixed")
    control = device_batch(dev, enc, ref.rows, ref.offs, n)
    rng = H.rng_of("order", "mixed")
    lidx = rng.integers(0, n, 3000)
    ridx = np.where(rng.random(3000) < 0.3, lidx, rng.integers(0, n, 3000))
    li, ri = torch.from_numpy(lidx).to(dev), torch.from_numpy(ridx).to(dev)
    flags = [int(x) for x in rng.integers(0, 4, len(keys))]
    desc, last = _opts(flags)

    def run(batch):
        out = torch.full((3001,), BYTE_GUARD, dtype=torch.int8, device=dev)
        compare_into(KeySide(enc, batch, keys, li), KeySide(enc, control, keys, ri), out[:3000], desc, last)
        words = [order_words(enc, batch, k, chunk, li, d, nl)[0] for k, d, nl in zip(keys, desc, last)
                 for chunk in (0, 1)]
        perm = argsort_rows(enc, batch, keys, desc, last)
        enc.device_status()
        return [out.cpu().numpy()] + [w.cpu().numpy() for w in words] + [perm.cpu().numpy()]

    base0 = run(control)
    idx = enc._select(keys)
    fields, cols = [ref.fields[k] for k in idx], [ref.cols[k] for k in idx]
    tids, tup = [f.type_id for f in fields], key_tuples(fields, cols, n)
    want = want_compare(tids, tup, lidx, tup, ridx, flags)
    assert set(want.tolist()) == {-1, 0, 1}
    assert_same(base0[0], np.concatenate([want, [BYTE_GUARD]]).astype(np.int8), "base 0: out_cmp")
    assert_same(base0[-1], np.array(M.sorted_model(tids, tup, flags), np.int64), "base 0: argsort")
    arena = Arena(dev)
    try:
        offs = control.row_offsets.cpu().numpy()
        total = int(offs[n])
        for place in ("inside_row-4g", "row_starts_at-2g", "inside_row-2g", "row_starts_at-4g"):
            X = H.BOUNDARIES[place.rsplit("-", 1)[1]]
            base = H.case_base(place, offs)
            assert base < X < base + total
            arena.clear()
            arena.place(control.rows[:total], base)
            got = run(RowBatch(arena.rows, control.row_offsets + base, n, enc.schema_hash))
            for g, w, what in zip(got, base0, ["out_cmp"] + ["words"] * (len(got) - 2) + ["argsort"]):
                assert_same(g, w, f"{place}: {what}")
            arena.assert_guard()
    finally:
        arena.rows = arena.buf = None
        del arena
        torch.cuda.empty_cache()
