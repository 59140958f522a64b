"""Key equality and the equi-join on the GPU (fury_row_keys_equal; fury_amd.keys_equal_into /
bind_keys_equal / keys_equal / join_pairs).  Every output is compared in full, plus one guard entry,
with the numpy model of tests/test_keys_equal_model.py (written from the header's rules alone)
applied to the oracle's decode of both batches.  Marked gpu."""
from __future__ import annotations

import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from fury_amd import types as T  # noqa: E402
from fury_amd.workloads import SCHEMAS, Column, gen_columns  # noqa: E402
from tests import high_offsets as H  # noqa: E402
from tests.test_bounds import _corrupt  # noqa: E402
from tests.test_hash import KEY_SETS, case  # noqa: E402
from tests.test_hash_model import fixed_column  # noqa: E402
from tests.test_hash_model import string_column as _readonly_strings  # noqa: E402
from tests.test_keys_equal_model import join_model, key_tuples, keys_equal_model, mask_words  # noqa: E402
from tests.test_take import _device_src, _Src, assert_same  # noqa: E402

BYTE_GUARD = 0x5A
WORD_GUARD = 0x5A5A5A5A
PAIR_COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 4097]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def string_column(values):
    """tests/test_hash_model.py's, over bytes of its own (torch wants writable arrays)."""
    c = _readonly_strings(values)
    return Column(values=c.values.copy(), offsets=c.offsets, validity=c.validity)


def _side(s, keys, idx=None):
    from fury_amd import KeySide
    return KeySide(s.enc, s.batch, keys, idx)


def _names(c, keys):
    return [k if isinstance(k, str) else c.fields[k].name for k in keys]


# ---- sides: a batch on the device and the oracle's decode of the same bytes, made once ----------------------
class _Batch:
    """One side of a comparison: encoder, device batch, host bytes, and the oracle's decode."""

    def __init__(self, oracle, enc, fields, batch):
        self.enc, self.fields, self.batch, self.n = enc, list(fields), batch, batch.nrows
        self.rows = batch.rows.cpu().numpy().copy()
        self.fixed = batch.row_offsets is None
        self.offs = (np.arange(self.n + 1, dtype=np.int64) * enc.schema().fixed_size if self.fixed
                     else batch.row_offsets.cpu().numpy().copy())
        self.ref = oracle.decode(self.fields, self.rows, None if self.fixed else self.offs, self.n)

    def cols(self, keys):
        idx = self.enc._select(keys)
        return [self.fields[k] for k in idx], [self.ref[k] for k in idx]

    def with_batch(self, batch):
        out = object.__new__(_Batch)
        out.__dict__.update(self.__dict__)
        out.batch, out.n = batch, batch.nrows
        return out

    def with_rows(self, rows, offs=None, edge=False):
        """The same side over other row bytes (a corrupted or truncated copy).  edge: the rows end
        where their device allocation ends."""
        from fury_amd.encoder import RowBatch
        dev = self.batch.rows.device
        out = object.__new__(_Batch)
        out.__dict__.update(self.__dict__)
        offs = self.offs if offs is None else offs
        if edge:
            # the very end of a device allocation of their own (a 32 MiB block is a segment of the
            # caching allocator by itself): a read past the batch's last byte would leave it
            torch.cuda.empty_cache()
            out.keep = torch.empty(32 << 20, dtype=torch.uint8, device=dev)
            assert len(rows) % 8 == 0 and out.keep.data_ptr() % 4096 == 0
            t = out.keep[out.keep.numel() - len(rows):]
            t.copy_(torch.from_numpy(np.ascontiguousarray(rows)))
        else:
            t = torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
        out.batch = RowBatch(t, None if self.fixed else torch.from_numpy(np.asarray(offs, np.int64)).to(dev),
                             self.n, self.enc.schema_hash)
        return out


_CACHE: dict = {}


def left_of(oracle, dev, c):
    key = ("left", id(c))
    if key not in _CACHE:
        _CACHE[key] = _Batch(oracle, c.enc, c.fields, _device_src(c.src, 0))
    return _CACHE[key]


def right_of(oracle, dev, c, form="select"):
    """The right side of a case: the left batch's rows, every third one replaced by another row (so
    that row j against row j is not always equal), through select_fields with the fields in reverse
    order: the same values at other slots.  form "variable": those fields and a STRING after them,
    encoded again, so a fixed-size schema meets variable-length rows."""
    from fury_amd.encoder import Encoders, column_to_device
    key = ("right", id(c), form)
    if key not in _CACHE:
        n = c.n
        rng = np.random.default_rng(n)
        rmap = np.arange(n, dtype=np.int64)
        swap = rng.random(n) < 1 / 3
        rmap[swap] = rng.integers(0, n, int(swap.sum()))
        rev = [f.name for f in reversed(c.fields)]
        taken = c.enc.take(left_of(oracle, dev, c).batch, torch.from_numpy(rmap).to(dev))
        batch = c.enc.select_fields(taken, rev)
        enc, fields = c.enc.selected_encoder(rev), list(reversed(c.fields))
        if form == "variable":
            cols = enc.decode_batch(batch)
            extra = T.field("zz", T.STRING)
            cols.append(column_to_device(gen_columns(None, [extra], n, seed=9)[0], dev))
            fields = fields + [extra]
            enc = Encoders.bean(fields, device=dev)
            batch = enc.encode_batch(cols, n)
            assert batch.row_offsets is not None
        _CACHE[key] = _Batch(oracle, enc, fields, batch)
    return _CACHE[key]


def run_equal(left, lkeys, lidx, right, rkeys, ridx, null_equal, what, outs="both", stream=None,
              bound=False, want=None, dtype=torch.uint8):
    """One keys_equal_into call into guarded outputs, compared in full with the model.  lidx / ridx:
    host index arrays or None."""
    from fury_amd import bind_keys_equal, keys_equal_into
    dev = left.batch.rows.device
    fl, cl = left.cols(lkeys)
    fr, cr = right.cols(rkeys)
    if want is None:
        want = keys_equal_model(fl, cl, lidx, fr, cr, ridx, null_equal, n_l=left.n, n_r=right.n)
    n = len(want)
    nw = (n + 31) // 32
    te = tm = None
    if outs in ("both", "equal"):
        te = torch.full((n + 1,), BYTE_GUARD, dtype=torch.uint8, device=dev).view(dtype)
    if outs in ("both", "mask"):
        tm = torch.full((nw + 1,), WORD_GUARD, dtype=torch.int32, device=dev)
    li = None if lidx is None else torch.from_numpy(np.asarray(lidx, np.int64)).to(dev)
    ri = None if ridx is None else torch.from_numpy(np.asarray(ridx, np.int64)).to(dev)
    torch.cuda.synchronize()
    args = (_side(left, lkeys, li), _side(right, rkeys, ri), None if te is None else te[:n],
            None if tm is None else tm[:nw], null_equal)
    if bound:
        call = bind_keys_equal(*args, stream=stream)
        call()
        call()
    else:
        keys_equal_into(*args, stream=stream)
    torch.cuda.synchronize()
    if te is not None:
        assert_same(te.view(torch.uint8).cpu().numpy(), np.concatenate([want, [BYTE_GUARD]]).astype(np.uint8),
                    f"{what}: out_equal")
    if tm is not None:
        assert_same(tm.cpu().numpy().view(np.uint32),
                    np.concatenate([mask_words(want), np.array([WORD_GUARD], np.uint32)]), f"{what}: out_mask")
    return want


def _modes(n, n_l, n_r, rng):
    """(name, left indices, right indices): NULL on both sides, NULL on one, random with repeats."""
    rand_l = rng.integers(0, n_l, n)
    rand_r = np.where(rng.random(n) < 0.5, rand_l % n_r, rng.integers(0, n_r, n))
    ident = np.arange(n, dtype=np.int64)
    out = [("no indices", None, None)] if n_l == n_r == n else []
    return out + [("left indices", rand_l, None if n == n_r else ident),
                  ("right indices", None if n == n_l else ident, rand_r),
                  ("both indices", rand_l, rand_r)]


# 1. every schema shape x pair count x key set x index form x flag ----------------------------------------------
@pytest.mark.parametrize("n", PAIR_COUNTS)
@pytest.mark.parametrize("name", list(KEY_SETS))
def test_matrix(oracle, dev, name, n):
    c = case(oracle, dev, name, max(n, 1))
    left = left_of(oracle, dev, c)
    for form in ["select"] + (["variable"] if name in ("pair", "struct100") else []):
        right = right_of(oracle, dev, c, form)
        if name in ("pair", "struct100"):
            assert left.fixed and right.fixed == (form == "select")
        for keys in KEY_SETS[name]:
            names = _names(c, keys)
            seen = set()
            for mode, lidx, ridx in _modes(n, left.n, right.n, np.random.default_rng(7)):
                for null_equal in (False, True):
                    want = run_equal(left, names, lidx, right, names, ridx, null_equal,
                                     f"{name}/{form} n={n} keys {names} {mode} null_equal={null_equal}")
                    seen |= set(want.tolist())
            if n >= 63:
                assert seen == {0, 1}, (name, form, names)        # the model: equal and unequal pairs
            if n == 0:                                            # no indices, no rows
                el = left.with_batch(left.enc.slice_rows(left.batch, 0, 0))
                er = right.with_batch(right.enc.slice_rows(right.batch, 0, 0))
                run_equal(el, names, None, er, names, None, True, f"{name}/{form} empty batches")
    c.enc.device_status()
    right.enc.device_status()


def test_two_bitmap_words_and_64_keys(oracle, dev):
    """The 70-field schema: keys 63 and 64 sit in different bitmap words on one side and in the same
    word on the other; 64 keys is the most a call takes.  Each side takes each role."""
    c = case(oracle, dev, "keys", 257, 30)
    a, b = left_of(oracle, dev, c), right_of(oracle, dev, c)
    rng = np.random.default_rng(2)
    for keys in ([63, 64], [62, 63, 64, 65], [9, 4, 10], list(range(6, 70))):
        names = _names(c, keys)
        for left, right in ((a, b), (b, a)):
            seen = set()
            for mode, lidx, ridx in _modes(257, 257, 257, rng):
                for null_equal in (False, True):
                    seen |= set(run_equal(left, names, lidx, right, names, ridx, null_equal,
                                          f"keys {keys} {mode} {null_equal}").tolist())
            assert seen == {0, 1}, keys
    c.enc.device_status()


# 2. payload edges ------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 3, 4, 7, 8, 9, 15, 16, 17, 300]
EDGE_FIELDS = [T.field("id", T.INT64), T.field("s", T.STRING)]


def _edge_values():
    """(left, right) string values, pair by pair: for every length an equal pair, a pair that differs
    in the first byte, one that differs in the last byte, and lengths n / n + 1 with a shared prefix;
    then null against empty, both ways, and null against null."""
    rng = np.random.default_rng(21)
    left, right = [], []
    for n in LENGTHS:
        v = rng.integers(1, 255, n + 1, dtype=np.uint8).tobytes()
        left += [v[:n], v[:n], v[:n], v[:n], v[:n + 1]]
        right += [v[:n],
                  bytes([v[0] ^ 0x80]) + v[1:n] if n else v[:n],
                  v[:n - 1] + bytes([v[n - 1] ^ 0x01]) if n else v[:n],
                  v[:n + 1], v[:n]]
    left += [None, b"", None]
    right += [b"", None, None]
    return left, right


def _edge_side(oracle, dev, values, key):
    from fury_amd.encoder import Encoders
    if key not in _CACHE:
        n = len(values)
        host = [fixed_column(np.int64, np.arange(n)), string_column(values)]
        enc = Encoders.bean(EDGE_FIELDS, device=dev)
        src = _Src(dev, enc, host, n)
        _CACHE[key] = _Batch(oracle, enc, EDGE_FIELDS, _device_src(src, 0))
    return _CACHE[key]


def test_payload_edges(oracle, dev):
    lv, rv = _edge_values()
    left, right = _edge_side(oracle, dev, lv, "edge-left"), _edge_side(oracle, dev, rv, "edge-right")
    n = len(lv)
    expect = []                                                   # the rules, value by value
    for a, b in zip(lv, rv):
        expect.append(int(a is not None and a == b))
    for keys in (["s"], ["id", "s"], ["s", "id"]):
        want = run_equal(left, keys, None, right, keys, None, False, f"edges {keys}")
        assert want.tolist() == expect
        want = run_equal(left, keys, None, right, keys, None, True, f"edges {keys}, null equal")
        assert want.tolist() == expect[:-1] + [1]
    assert expect[:5] == [1, 1, 1, 0, 0] and expect[5:10] == [1, 0, 0, 0, 0]     # length 0, length 1
    # padding bytes after a payload are never compared: 0xFF over the right rows' padding
    rows = right.rows.copy()
    touched = 0
    for r in range(n):
        base = int(right.offs[r])
        if rows[base] & 2:
            continue                                              # s is null
        slot = struct.unpack_from("<Q", rows, base + 8 + 8)[0]
        end = base + (slot >> 32) + (slot & 0xFFFFFFFF)
        pad = -end % 8
        rows[end:end + pad] = 0xFF
        touched += pad
        assert end + pad <= int(right.offs[r + 1])
    assert touched > 50 and not np.array_equal(rows, right.rows)
    dirty = right.with_rows(rows)
    for null_equal in (False, True):
        run_equal(left, ["id", "s"], None, dirty, ["id", "s"], None, null_equal, "edges, padding 0xFF")
        ridx = np.arange(n)[::-1].copy()
        run_equal(left, ["s"], ridx, dirty, ["s"], ridx, null_equal, "edges, padding 0xFF, indexed")
    left.enc.device_status()


# 3. the two outputs agree, alone and together ----------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 100, 257])
def test_outputs(oracle, dev, n):
    c = case(oracle, dev, "mixed", 257)
    left, right = left_of(oracle, dev, c), right_of(oracle, dev, c)
    rng = np.random.default_rng(n)
    lidx = rng.integers(0, 257, n)
    ridx = np.where(rng.random(n) < 0.7, lidx, rng.integers(0, 257, n))
    keys = ["s1", "b"]
    want = run_equal(left, keys, lidx, right, keys, ridx, True, f"outputs n={n}")
    assert n < 31 or (want.any() and not want.all())
    for outs in ("equal", "mask"):
        run_equal(left, keys, lidx, right, keys, ridx, True, f"outputs n={n} {outs} only", outs=outs,
                  want=want)
    run_equal(left, keys, lidx, right, keys, ridx, True, f"outputs n={n} bool", outs="equal", want=want,
              dtype=torch.bool)
    c.enc.device_status()


# 4. bounds -------------------------------------------------------------------------------------------------------
BOUNDS_FIELDS = [T.field("id", T.INT64), T.field("s", T.STRING), T.field("t", T.STRING)]
BOUNDS_N = 257


def _bounds_sides(oracle, dev):
    """Left: (id, s, t) with s of 9 to 40 bytes, a few nulls, 37 distinct values; right: the same rows
    rotated by one, as (t, s, id).  The last row of each has a non-null s."""
    from fury_amd.encoder import Encoders
    if "bounds" not in _CACHE:
        n = BOUNDS_N
        rng = np.random.default_rng(31)
        s = [None if r % 29 == 5 else bytes([65 + r % 37]) * (9 + r % 32) for r in range(n)]
        t = [rng.integers(0, 256, int(rng.integers(0, 20)), dtype=np.uint8).tobytes() for _ in range(n)]
        host = [fixed_column(np.int64, np.arange(n) % 37), string_column(s), string_column(t)]
        enc = Encoders.bean(BOUNDS_FIELDS, device=dev)
        left = _Batch(oracle, enc, BOUNDS_FIELDS, _device_src(_Src(dev, enc, host, n), 0))
        rot = torch.from_numpy((np.arange(n) + 1) % n).to(dev)
        rev = ["t", "s", "id"]
        right = _Batch(oracle, enc.selected_encoder(rev), list(reversed(BOUNDS_FIELDS)),
                       enc.select_fields(enc.take(left.batch, rot), rev))
        _CACHE["bounds"] = (left, right)
    return _CACHE["bounds"]


def _bounds_pairs():
    """Every left row once, in a shuffled order, against the right row that holds the same values
    (right row r = left row r + 1), two of every five against another row."""
    rng = np.random.default_rng(32)
    lidx = rng.permutation(BOUNDS_N)
    ridx = (lidx - 1) % BOUNDS_N
    for j in range(0, BOUNDS_N - 1, 5):                          # still every right row once
        ridx[j], ridx[j + 1] = ridx[j + 1], ridx[j]
    return lidx, ridx


def _expect_failure(left, right, keys, lidx, ridx, bad_pairs, what, want_by_flag=None):
    """The pairs `bad_pairs` are 0 under both flags, device_status names one of them, every other
    pair is the model's."""
    from fury_amd.encoder import IndexOutOfBoundsException
    for null_equal in (False, True):
        fl, cl = left.cols(keys)
        fr, cr = right.cols(keys)
        want = (keys_equal_model(fl, cl, lidx, fr, cr, ridx, null_equal, n_l=left.n, n_r=right.n)
                if want_by_flag is None else want_by_flag[null_equal].copy())
        want[list(bad_pairs)] = 0
        left.enc.device_status()
        run_equal(left, keys, lidx, right, keys, ridx, null_equal, f"{what} null_equal={null_equal}",
                  want=want)
        if bad_pairs:
            with pytest.raises(IndexOutOfBoundsException) as e:
                left.enc.device_status()
            assert H.row_of(str(e.value)) in set(bad_pairs), (what, str(e.value))
        left.enc.device_status()                                   # clean (again)


@pytest.mark.parametrize("side", ["left", "right"])
def test_indices_outside_the_batch(oracle, dev, side):
    left, right = _bounds_sides(oracle, dev)
    lidx, ridx = _bounds_pairs()
    keys = ["id", "s"]
    clean = {f: keys_equal_model(*left.cols(keys), lidx, *right.cols(keys), ridx, f, n_l=left.n, n_r=right.n)
             for f in (False, True)}
    assert clean[True].any() and not clean[True].all()
    for j, bad in ((3, -1), (100, BOUNDS_N), (256, 2 ** 40)):
        li, ri = lidx.copy(), ridx.copy()
        (li if side == "left" else ri)[j] = bad
        _expect_failure(left, right, keys, li, ri, [j], f"{side} index {bad}", want_by_flag=clean)


def _victim(b, lidx_or_ridx):
    """A row in the second half with a non-null s, and the pair that uses it."""
    k = b.enc._select(["s"])[0]
    for r in range(BOUNDS_N // 2, BOUNDS_N):
        if not (b.rows[int(b.offs[r]) + (k >> 3)] >> (k & 7)) & 1:
            (j,) = np.flatnonzero(lidx_or_ridx == r)
            return r, int(j)
    raise AssertionError("no victim")


@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("how", H.MALFORMED)
def test_corrupt_key_slots(oracle, dev, side, how):
    """tests/test_bounds.py's corruptions on the key field s of one row.  offset_past_end,
    size_past_end and negative_size are bounds failures.  huge_list_count overwrites the first 8
    bytes the slot points at, which for a STRING is payload: no failure, the value is another one,
    and the expectation is the model over the oracle's decode of the corrupted rows."""
    left, right = _bounds_sides(oracle, dev)
    lidx, ridx = _bounds_pairs()
    keys = ["id", "s"]
    hit = left if side == "left" else right
    r, j = _victim(hit, lidx if side == "left" else ridx)
    k = hit.enc._select(["s"])[0]
    rows = _corrupt(hit.fields, hit.rows, hit.offs, BOUNDS_N, r, k, how)
    assert not np.array_equal(rows, hit.rows)
    bad = hit.with_rows(rows)
    if how == "huge_list_count":
        bad.ref = oracle.decode(bad.fields, rows, bad.offs, BOUNDS_N)
        assert key_tuples(*bad.cols(["s"]), BOUNDS_N)[r] != key_tuples(*hit.cols(["s"]), BOUNDS_N)[r]
        fails = []
    else:
        fails = [j]
    sides = (bad, right) if side == "left" else (left, bad)
    _expect_failure(*sides, keys, lidx, ridx, fails, f"{how} on the {side}")
    # the key order does not decide whether the failure is seen: id differs first in some pairs
    _expect_failure(*sides, ["s", "id"], lidx, ridx, fails, f"{how} on the {side}, s first")


@pytest.mark.parametrize("side", ["left", "right"])
def test_corrupt_slots_of_fields_that_are_not_keys(oracle, dev, side):
    left, right = _bounds_sides(oracle, dev)
    lidx, ridx = _bounds_pairs()
    hit = left if side == "left" else right
    k = hit.enc._select(["t"])[0]
    rows = hit.rows
    assert set(H.MALFORMED) == {"offset_past_end", "size_past_end", "negative_size", "huge_list_count"}
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
    bad = hit.with_rows(rows)
    sides = (bad, right) if side == "left" else (left, bad)
    _expect_failure(*sides, ["id", "s"], lidx, ridx, [], f"non-key corruption on the {side}")


@pytest.mark.parametrize("side", ["left", "right"])
def test_truncated_batch(oracle, dev, side):
    """row_offsets[n] cut 8 bytes into the last row's s payload, the rows at the very end of a device
    allocation: the last row's value leaves the batch."""
    left, right = _bounds_sides(oracle, dev)
    lidx, ridx = _bounds_pairs()
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
    bad = hit.with_rows(hit.rows[:cut].copy(), offs, edge=True)
    (j,) = np.flatnonzero((lidx if side == "left" else ridx) == last)
    sides = (bad, right) if side == "left" else (left, bad)
    _expect_failure(*sides, ["id", "s"], lidx, ridx, [int(j)], f"truncated {side}")
    # s is not a key: the row's header is inside the batch and nothing else is looked at
    _expect_failure(*sides, ["id"], lidx, ridx, [], f"truncated {side}, key id")
    del bad


# 5. the bound form, a side stream ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,keys", [("mixed", ["s2", "a"]), ("struct100", [0, 51])])
def test_bound_and_stream(oracle, dev, name, keys):
    c = case(oracle, dev, name, 4097)
    left, right = left_of(oracle, dev, c), right_of(oracle, dev, c)
    names = _names(c, keys)
    rng = np.random.default_rng(5)
    lidx = rng.integers(0, 4097, 5000)
    ridx = np.where(rng.random(5000) < 0.5, lidx, rng.integers(0, 4097, 5000))
    want = run_equal(left, names, lidx, right, names, ridx, False, f"{name} eager")
    assert want.any() and not want.all()
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    run_equal(left, names, lidx, right, names, ridx, False, f"{name} side stream", stream=s, want=want)
    run_equal(left, names, lidx, right, names, ridx, False, f"{name} bound", bound=True, want=want)
    run_equal(left, names, lidx, right, names, ridx, False, f"{name} bound, side stream", bound=True,
              stream=s, want=want)
    c.enc.device_status(s)
    c.enc.device_status()
    from fury_amd import keys_equal
    li, ri = torch.from_numpy(lidx).to(dev), torch.from_numpy(ridx).to(dev)
    got = keys_equal(_side(left, names, li), _side(right, names, ri))
    assert got.dtype == torch.bool
    assert_same(got.cpu().numpy().astype(np.uint8), want, f"{name} keys_equal")


# 6. batches that cross byte 2^31 and byte 2^32 of their buffer ---------------------------------------------------------
def test_high_offsets(oracle, dev):
    from fury_amd import KeySide, keys_equal_into
    from fury_amd.encoder import RowBatch
    from tests.test_high_offsets_gpu import Arena, device_batch, encoder
    ref = H.ref(oracle, "mixed")
    n, keys = ref.n, H.SPEC["mixed"]["hash"]
    assert n == 1300
    enc = encoder(dev, "mixed")
    control = device_batch(dev, enc, ref.rows, ref.offs, n)
    other = enc.take(control, torch.arange(n - 1, -1, -1, device=dev))      # its reverse, at base 0
    rng = H.rng_of("keys_equal", "mixed")
    lidx = rng.integers(0, n, 3000)
    ridx = np.where(rng.random(3000) < 0.5, n - 1 - lidx, rng.integers(0, n, 3000))
    li, ri = torch.from_numpy(lidx).to(dev), torch.from_numpy(ridx).to(dev)

    def run(left, right, null_equal):
        eq = torch.full((3001,), BYTE_GUARD, dtype=torch.uint8, device=dev)
        mask = torch.full((95,), WORD_GUARD, dtype=torch.int32, device=dev)
        keys_equal_into(KeySide(enc, left, keys, li), KeySide(enc, right, keys, ri), eq[:3000], mask[:94],
                        null_equal)
        enc.device_status()
        return eq.cpu().numpy(), mask.cpu().numpy()

    fields = [ref.fields[k] for k in enc._select(keys)]
    cols = [ref.cols[k] for k in enc._select(keys)]
    base0 = {}
    for null_equal in (False, True):
        base0[null_equal] = run(control, other, null_equal)
        want = keys_equal_model(fields, cols, lidx, fields, cols, n - 1 - ridx, null_equal, n_l=n, n_r=n)
        assert want.any() and not want.all()
        assert_same(base0[null_equal][0], np.concatenate([want, [BYTE_GUARD]]).astype(np.uint8), "base 0")
    arena = Arena(dev)
    try:
        offs_l = control.row_offsets.cpu().numpy()
        offs_r = other.row_offsets.cpu().numpy()
        bl = H.case_base("inside_row-4g", offs_l)
        br = H.case_base("row_starts_at-2g", offs_r)
        assert bl < H.X32 < bl + int(offs_l[n]) and br < H.X31 < br + int(offs_r[n])
        arena.place(control.rows[:int(offs_l[n])], bl)
        arena.place(other.rows[:int(offs_r[n])], br)
        left = RowBatch(arena.rows, control.row_offsets + bl, n, enc.schema_hash)
        right = RowBatch(arena.rows, other.row_offsets + br, n, enc.schema_hash)
        for null_equal in (False, True):
            eq, mask = run(left, right, null_equal)
            assert_same(eq, base0[null_equal][0], f"high offsets, null_equal={null_equal}: out_equal")
            assert_same(mask, base0[null_equal][1], f"high offsets, null_equal={null_equal}: out_mask")
        arena.assert_guard()
    finally:
        arena.rows = arena.buf = None
        del arena
        torch.cuda.empty_cache()


# 7. the join --------------------------------------------------------------------------------------------------------
JOIN_KEYS = ["b", "s1"]


def _join_side(oracle, dev, n, seed):
    """A `mixed` batch whose keys (b, s1) are drawn from 8 x 5 = 40 combinations, 10% nulls each."""
    from fury_amd.encoder import Encoders
    key = ("join", n, seed)
    if key not in _CACHE:
        fields = SCHEMAS["mixed"]
        rng = np.random.default_rng(seed)
        host = gen_columns("mixed", fields, n, seed=seed)
        words = [b"", b"k", b"key-0001", b"key-0002", b"a longer key of thirty-two bytes"]
        host[1] = fixed_column(np.int64, rng.integers(-3, 5, n) * (1 << 40),
                               nulls=np.flatnonzero(rng.random(n) < 0.1))
        host[3] = string_column([None if rng.random() < 0.1 else words[int(rng.integers(0, 5))]
                                 for _ in range(n)])
        enc = Encoders.bean(fields, device=dev)
        _CACHE[key] = _Batch(oracle, enc, fields, _device_src(_Src(dev, enc, host, n), 0))
    return _CACHE[key]


def test_join_pairs(oracle, dev):
    from fury_amd import join_pairs
    from fury_amd.encoder import IllegalArgumentException
    left, right = _join_side(oracle, dev, 1300, 41), _join_side(oracle, dev, 700, 42)
    assert len(set(key_tuples(*left.cols(JOIN_KEYS), left.n))) > 40        # the 40 and those with nulls
    s = torch.cuda.Stream(device=dev)
    for null_equal in (False, True):
        wl, wr = join_model(*left.cols(JOIN_KEYS), left.n, *right.cols(JOIN_KEYS), right.n, null_equal)
        assert len(wl) > 10000
        for stream in (None, s):
            li, ri = join_pairs(_side(left, JOIN_KEYS), _side(right, JOIN_KEYS), null_equal=null_equal,
                                seed=5, stream=stream)
            torch.cuda.synchronize()
            assert li.dtype == torch.int64 and ri.dtype == torch.int64 and li.device.type == "cuda"
            assert_same(li.cpu().numpy(), wl, f"join null_equal={null_equal}: left rows")
            assert_same(ri.cpu().numpy(), wr, f"join null_equal={null_equal}: right rows")
    # a batch joined with itself under null-equals-null: every row finds itself (group ids, de-duplication)
    li, ri = join_pairs(_side(left, JOIN_KEYS), _side(left, JOIN_KEYS), null_equal=True)
    li, ri = li.cpu().numpy(), ri.cpu().numpy()
    wl, wr = join_model(*left.cols(JOIN_KEYS), left.n, *left.cols(JOIN_KEYS), left.n, True)
    assert_same(li, wl, "self join: left rows")
    assert_same(ri, wr, "self join: right rows")
    assert np.array_equal(li[li == ri], np.arange(left.n))
    with pytest.raises(IllegalArgumentException, match="candidate pairs exceed max_pairs 1000"):
        join_pairs(_side(left, JOIN_KEYS), _side(right, JOIN_KEYS), max_pairs=1000)
    left.enc.device_status()


def test_join_of_an_empty_side(oracle, dev):
    from fury_amd import KeySide, join_pairs
    left = _join_side(oracle, dev, 1300, 41)
    empty = left.enc.slice_rows(left.batch, 0, 0)
    for a, b in ((empty, left.batch), (left.batch, empty), (empty, empty)):
        li, ri = join_pairs(KeySide(left.enc, a, JOIN_KEYS), KeySide(left.enc, b, JOIN_KEYS))
        assert li.numel() == 0 and ri.numel() == 0 and li.dtype == torch.int64 and li.device.type == "cuda"
    left.enc.device_status()


def test_join_to_rows(oracle, dev):
    """The recipe of INTEGRATION.md: join_pairs, take on both sides, zip_fields -- decoded through the
    oracle, the rows a Python join of the decoded columns gives."""
    from fury_amd import join_pairs
    from fury_amd.encoder import Encoders
    from tests.helpers import assert_columns_equal, columns_to_beans
    left = _join_side(oracle, dev, 1300, 41)
    rfields = [T.field("rb", T.INT64), T.field("rs", T.STRING), T.field("rv", T.INT32)]
    src = _join_side(oracle, dev, 700, 42)
    renc = Encoders.bean(rfields, device=dev)
    rhost = [src.ref[1], src.ref[3], src.ref[0]]
    right = _Batch(oracle, renc, rfields, _device_src(_Src(dev, renc, rhost, 700), 0))
    li, ri = join_pairs(_side(left, ["b", "s1"]), _side(right, ["rb", "rs"]))
    picks = [(0, "a"), (0, "b"), (0, "s1"), (1, "rv"), (0, "s3"), (1, "rs")]
    joined = left.enc.zip_fields(left.enc.take(left.batch, li), [(renc, renc.take(right.batch, ri))], picks)
    jenc = left.enc.zipped_encoder([renc], picks)
    jfields = jenc.schema().fields
    n = joined.nrows
    assert n == li.numel() and n > 5000
    got = oracle.decode(jfields, joined.rows.cpu().numpy(), joined.row_offsets.cpu().numpy(), n)
    lrows = columns_to_beans(left.fields, left.ref, left.n)
    rrows = columns_to_beans(rfields, right.ref, right.n)
    table: dict = {}
    for rr in rrows:                                               # the join, in Python
        if rr["rb"] is not None and rr["rs"] is not None:
            table.setdefault((rr["rb"], rr["rs"]), []).append(rr)
    want = [{"a": lr["a"], "b": lr["b"], "s1": lr["s1"], "rv": rr["rv"], "s3": lr["s3"], "rs": rr["rs"]}
            for lr in lrows for rr in table.get((lr["b"], lr["s1"]), ())]
    assert len(want) == n
    assert columns_to_beans(jfields, got, n) == want
    left.enc.device_status()
