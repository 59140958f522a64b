"""The key index and its lookup on the GPU (fury_row_index_build / fury_row_lookup; fury_amd.build_index_into /
build_index / lookup_into / bind_lookup / lookup / semi_join / lookup_join_pairs).  Every output is
written into a guarded tensor (one guard entry past the end) and compared in full with the dict model
of tests/test_lookup_model.py (written from the header's rules alone) applied to the oracle's decode
of both batches; every case runs twice and must give identical results.  Marked gpu."""
from __future__ import annotations

import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from fury_amd import types as T  # noqa: E402
from fury_amd.workloads import Column, gen_columns  # noqa: E402
from tests import high_offsets as H  # noqa: E402
from tests.test_bounds import _corrupt  # noqa: E402
from tests.test_group import LENGTHS, MIXED_FIELDS, MIXED_KEYS, batch_of  # noqa: E402
from tests.test_group_model import group_model  # noqa: E402
from tests.test_hash import _key_fields  # noqa: E402
from tests.test_hash_model import fixed_column  # noqa: E402
from tests.test_keys_equal import _Batch, string_column  # noqa: E402
from tests.test_keys_equal_model import key_tuples, mask_words  # noqa: E402
from tests.test_lookup_model import lookup_mask, lookup_model  # noqa: E402
from tests.test_take import _device_src, _pair_fields, _Src, assert_same  # noqa: E402

GUARD = 0x5A5A5A5A5A5A5A5A
WORD_GUARD = 0x5A5A5A5A
BUILD_COUNTS = [0, 1, 63, 64, 65, 257, 4097]
PROBE_COUNTS = [0, 1, 31, 32, 33, 63, 64, 65, 257, 4097]
FORMS = [None, "seed7", "zero", "and3", "ones"]
IDS, BUILD_IDS = 96, 64                           # key numbers: a build side draws from the first 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


# ---- batches: made once, with the oracle's decode, never modified ----------------------------------------------
_CACHE: dict = {}


def _build_ids(nb):
    """The key number of every build row: duplicates among BUILD_IDS numbers; row 0 has number 0."""
    kid = np.random.default_rng(1000 + nb).integers(0, BUILD_IDS, nb)
    kid[:1] = 0
    return kid


def _probe_ids(n, build_ids):
    """The key number of every probe row, by a fixed pattern in a random order: 8 of 20 an even number of
    the build side (a key without a null: it matches under both flag values), 2 of 20 any of its
    numbers (odd ones have a null key: they match only with null_equal), 10 of 20 a number no build
    side has, one in five of those odd."""
    rng = np.random.default_rng(2000 + n + 7 * len(build_ids))
    j = np.arange(n)
    absent = BUILD_IDS + 2 * rng.integers(0, (IDS - BUILD_IDS) // 2, n) + (j % 5 == 0)
    if len(build_ids) == 0:
        return rng.permutation(np.where(j % 20 < 10, rng.integers(0, BUILD_IDS, n), absent))
    even = build_ids[build_ids % 2 == 0]
    ids = np.where(j % 20 < 8, even[rng.integers(0, len(even), n)],
                   np.where(j % 20 < 10, build_ids[rng.integers(0, len(build_ids), n)], absent))
    return rng.permutation(ids)


def _mixed_proto(dev):
    """(v, i, s, t, b), one row per key number k; the key (i, s, b) differs between any two numbers.
    Even k: no null key; k % 4 == 1: i is null; k % 4 == 3: s is null.  Number 0 has the empty
    string."""
    from fury_amd.encoder import Encoders
    k = np.arange(IDS)
    rng = np.random.default_rng(5)
    ints = fixed_column(np.int32, k * 3 - 5, nulls=np.flatnonzero(k % 4 == 1))
    strs = string_column([None if x % 4 == 3 else b"" if x == 0 else b"s%d" % x + b"x" * (x % 19) for x in k])
    bools = Column(values=np.packbits(((k >> 1) & 1).astype(bool), bitorder="little"),
                   validity=np.packbits(np.ones(IDS, bool), bitorder="little"))
    host = [fixed_column(np.int64, k), ints, strs,
            string_column([rng.integers(0, 256, int(rng.integers(0, 20)), dtype=np.uint8).tobytes() for _ in k]),
            bools]
    enc = Encoders.bean(MIXED_FIELDS, device=dev)
    return enc, MIXED_FIELDS, _device_src(_Src(dev, enc, host, IDS), 0)


def _generated_proto(dev, fields):
    """One generated row per key number, 30 % nulls in the odd numbers, none in the even ones."""
    from fury_amd.encoder import Encoders
    host = gen_columns(None, fields, IDS, seed=3, null_pct=30)
    for c in host:
        if c.validity is not None:
            valid = np.unpackbits(np.asarray(c.validity, np.uint8), bitorder="little")[:IDS].copy()
            valid[0::2] = 1
            c.validity = np.packbits(valid, bitorder="little")
    enc = Encoders.bean(fields, device=dev)
    return enc, fields, _device_src(_Src(dev, enc, host, IDS), 0)


def _proto(dev, name):
    if ("proto", name) not in _CACHE:
        _CACHE[("proto", name)] = (_mixed_proto(dev) if name == "mixed" else
                                   _generated_proto(dev, _pair_fields() if name == "pair" else _key_fields()))
    return _CACHE[("proto", name)]


def build_of(oracle, dev, name, nb):
    """nb rows of the schema `name`, drawn from the prototype rows by take."""
    key = ("build", name, nb)
    if key not in _CACHE:
        enc, fields, proto = _proto(dev, name)
        ids = _build_ids(max(nb, 1))
        b = _Batch(oracle, enc, fields, enc.take(proto, torch.from_numpy(ids).to(dev)))
        _CACHE[key] = b if nb else b.with_batch(enc.slice_rows(b.batch, 0, 0))
    return _CACHE[key]


def probe_of(oracle, dev, name, n, nb):
    """n probe rows for the build side of nb rows, through select_fields with the fields in reverse
    order: another schema, the same key values at other slots, other fields around them."""
    key = ("probe", name, n, nb)
    if key not in _CACHE:
        enc, fields, proto = _proto(dev, name)
        ids = _probe_ids(max(n, 1), _build_ids(nb) if nb else np.zeros(0, np.int64))
        rev = [f.name for f in reversed(fields)]
        batch = enc.select_fields(enc.take(proto, torch.from_numpy(ids).to(dev)), rev)
        p = _Batch(oracle, enc.selected_encoder(rev), list(reversed(fields)), batch)
        _CACHE[key] = p if n else p.with_batch(p.enc.slice_rows(p.batch, 0, 0))
    return _CACHE[key]


KEY_SETS = {
    "pair": [["a"], ["b", "a"]],                                  # fixed-size rows: row_offsets is NULL
    "mixed": [MIXED_KEYS, ["s"]],
    "keys": [[63, 64], list(range(6, 70))],                       # two bitmap words; 64 keys
}


def _names(b, keys):
    return [k if isinstance(k, str) else b.fields[k].name for k in keys]


def _side(b, keys):
    from fury_amd import KeySide
    return KeySide(b.enc, b.batch, keys)


def _cols(b, keys):
    f, c = b.cols(keys)
    return f, c, b.n


def hashes_of(b, keys, form, seed=7):
    """`hashes` in the forms rule 5 allows, the same function of the key values on both sides: none,
    hash_rows under another seed, and degraded ones -- all zero (one walk through every key), two
    bits, all ones (the walk starts at the last slot and wraps; an entry must not look EMPTY)."""
    if form is None or b.n == 0:
        return None if form is None else torch.zeros(0, dtype=torch.int32, device=b.batch.rows.device)
    if form == "zero":                            # without hash_rows: it reports a corrupt batch itself
        return torch.zeros(b.n, dtype=torch.int32, device=b.batch.rows.device)
    h = b.enc.hash_rows(b.batch, keys, seed=seed)
    if form == "seed7":
        return h
    h = h.view(torch.int32)
    return {"and3": h & 3, "ones": torch.full_like(h, -1)}[form]


def _status(b, stream, bad, what):
    """device_status is clean, or names one of the rows `bad`."""
    from fury_amd.encoder import IndexOutOfBoundsException
    if len(bad) == 0:
        b.enc.device_status(stream)
        return
    with pytest.raises(IndexOutOfBoundsException) as e:
        b.enc.device_status(stream)
    assert H.row_of(str(e.value)) in set(int(r) for r in bad), (what, str(e.value))


def run_lookup(build, bkeys, probe, pkeys, what, form=None, null_equal=False, outs=("rows", "mask"),
               stream=None, bound=False, bad_build=(), bad_probe=(), want_first=True):
    """build_index_into and lookup_into into guarded tensors, twice, compared in full with the model.
    Returns the model's out_rows."""
    from fury_amd import KeyIndex, bind_lookup, build_index_into, index_slots, lookup_into
    dev, nb, n = probe.batch.rows.device, build.n, probe.n
    want = lookup_model(_cols(build, bkeys), _cols(probe, pkeys), null_equal, bad_build, bad_probe)
    first = group_model(*build.cols(bkeys), nb, bad_build)[0]
    hb, hp = hashes_of(build, bkeys, form), hashes_of(probe, pkeys, form)
    slots, nw = index_slots(nb), (n + 31) // 32
    runs = []
    for _ in range(2):
        table = torch.full((slots + 1,), GUARD, dtype=torch.int64, device=dev)
        tf = torch.full((nb + 1,), GUARD, dtype=torch.int64, device=dev) if want_first else None
        tr = torch.full((n + 1,), GUARD, dtype=torch.int64, device=dev) if "rows" in outs else None
        tm = torch.full((nw + 1,), WORD_GUARD, dtype=torch.int32, device=dev) if "mask" in outs else None
        torch.cuda.synchronize()
        build_index_into(_side(build, bkeys), table[:slots], None if tf is None else tf[:nb], hb, stream)
        _status(build, stream, bad_build, f"{what}: build")
        index = KeyIndex(_side(build, bkeys), table[:slots], None, hb is not None)
        args = (index, _side(probe, pkeys), None if tr is None else tr[:n], None if tm is None else tm[:nw],
                null_equal, hp)
        if bound:
            bind_lookup(*args, stream=stream)()
        else:
            lookup_into(*args, stream=stream)
        _status(probe, stream, bad_probe, f"{what}: lookup")
        torch.cuda.synchronize()
        assert int(table[slots]) == GUARD, f"{what}: the table's guard"
        got = []
        if tf is not None:
            assert_same(tf.cpu().numpy(), np.concatenate([first, [GUARD]]), f"{what}: out_first")
        if tr is not None:
            got.append(tr.cpu().numpy())
            assert_same(got[-1], np.concatenate([want, [GUARD]]), f"{what}: out_rows")
        if tm is not None:
            got.append(tm.cpu().numpy().view(np.uint32))
            assert_same(got[-1], np.concatenate([lookup_mask(want), np.array([WORD_GUARD], np.uint32)]),
                        f"{what}: out_mask")
        runs.append(got)
    for x, y in zip(*runs):
        assert np.array_equal(x, y), f"{what}: the second run differs"
    return want


def _matrix_leg(oracle, dev, name, nb, n):
    build, probe = build_of(oracle, dev, name, nb), probe_of(oracle, dev, name, n, nb)
    assert build.n == nb and probe.n == n and build.fixed == probe.fixed == (name == "pair")
    assert build.enc.schema_hash != probe.enc.schema_hash
    for keys in KEY_SETS[name]:
        bkeys = _names(build, keys)
        if keys is KEY_SETS[name][0]:
            assert build.enc._select(bkeys) != probe.enc._select(bkeys)      # the key slots differ
        # at least a quarter of the probe rows match and a quarter do not, by the model, before the device
        for null_equal in (False, True):
            want = lookup_model(_cols(build, bkeys), _cols(probe, bkeys), null_equal)
            if nb > 0 and n >= 31:
                assert (want >= 0).sum() >= n / 4 and (want < 0).sum() >= n / 4, (name, keys, nb, n, null_equal)
        tuples = key_tuples(*build.cols(bkeys), nb) + key_tuples(*probe.cols(bkeys), n)
        if nb >= 63 and n >= 63:
            assert any(None in k for k in tuples[:nb]) and any(None in k for k in tuples[nb:])
        # the chain of all-equal hashes is quadratic in the keys: up to 257 rows, the 64-key set at 257 only
        if len(keys) == 64:
            forms = FORMS if nb == n == 257 else FORMS[:2]
        else:
            forms = FORMS if max(nb, n) <= 257 else FORMS[:2]
        for form in forms:
            for null_equal in (False, True):
                run_lookup(build, bkeys, probe, bkeys, f"{name} nb={nb} n={n} keys {keys} hashes {form} "
                           f"null_equal={null_equal}", form, null_equal)
    build.enc.device_status()


# 1. every schema shape x row count x key set x hash form x flag ------------------------------------------------
@pytest.mark.parametrize("nb", BUILD_COUNTS)
@pytest.mark.parametrize("name", list(KEY_SETS))
def test_build_counts(oracle, dev, name, nb):
    _matrix_leg(oracle, dev, name, nb, 257)


@pytest.mark.parametrize("n", [c for c in PROBE_COUNTS if c != 257])
@pytest.mark.parametrize("name", list(KEY_SETS))
def test_probe_counts(oracle, dev, name, n):
    _matrix_leg(oracle, dev, name, 257, n)


@pytest.mark.parametrize("name", list(KEY_SETS))
def test_mismatched_hashes(oracle, dev, name):
    """The build side hashed with seed 0 by the caller, the probe side with seed 7: a match may turn
    into -1, nothing else -- every result is -1 or the model's, the guards hold, no error."""
    from fury_amd import build_index, lookup_into
    build, probe = build_of(oracle, dev, name, 257), probe_of(oracle, dev, name, 4097, 257)
    keys = _names(build, KEY_SETS[name][0])
    for null_equal in (False, True):
        want = lookup_model(_cols(build, keys), _cols(probe, keys), null_equal)
        index = build_index(_side(build, keys), hashes=hashes_of(build, keys, "seed7", seed=0))
        out = torch.full((probe.n + 1,), GUARD, dtype=torch.int64, device=dev)
        lookup_into(index, _side(probe, keys), out[:probe.n], None, null_equal, hashes_of(probe, keys, "seed7"))
        probe.enc.device_status()
        got = out.cpu().numpy()
        assert got[-1] == GUARD
        assert ((got[:-1] == -1) | (got[:-1] == want)).all()
        assert (got[:-1] == -1).sum() > (want == -1).sum()         # the hashes did differ


# 2. payload edges ----------------------------------------------------------------------------------------------
def _dirty_padding(b, k):
    """0xFF over the padding behind field k's payload in every other row."""
    rows, touched = b.rows.copy(), 0
    bitmap = (len(b.fields) + 63) // 64 * 8
    for r in range(1, b.n, 2):
        base = int(b.offs[r])
        if (rows[base + (k >> 3)] >> (k & 7)) & 1:
            continue
        slot = struct.unpack_from("<Q", rows, base + bitmap + 8 * k)[0]
        end = base + (slot >> 32) + (slot & 0xFFFFFFFF)
        pad = -end % 8
        rows[end:end + pad] = 0xFF
        touched += pad
        assert end + pad <= int(b.offs[r + 1])
    assert touched > 40 and not np.array_equal(rows, b.rows)
    return b.with_rows(rows)


def test_string_lengths_and_padding(oracle, dev):
    """For every length around the 8-byte words the build side has the value and the value one byte
    longer; the probe side asks for the value, the value with its last byte changed, one byte
    shorter, one byte longer, and a value of the same length that is not there.  Then 0xFF over the
    padding of every other row on both sides: padding is never compared, so nothing changes."""
    from fury_amd.encoder import Encoders
    rng = np.random.default_rng(21)
    bvals, pvals = [None, b""], [None, b"", b"\x00"]
    for n in LENGTHS:
        v = rng.integers(1, 255, n + 2, dtype=np.uint8).tobytes()
        bvals += [v[:n], v[:n + 1], v[:n]]
        pvals += [v[:n], v[:n + 1], v[:n + 2]]
        if n:
            pvals += [v[:n - 1] + bytes([v[n - 1] ^ 0x01]), v[:n - 1]]
    expect = [bvals.index(v) if v is not None and v in bvals else -1 for v in pvals]    # the rules, value by value
    assert sum(e >= 0 for e in expect) >= 2 * len(LENGTHS) and sum(e < 0 for e in expect) >= 2 * len(LENGTHS)
    bf = [T.field("id", T.INT64), T.field("s", T.STRING)]
    pf = [T.field("s", T.STRING), T.field("id", T.INT64)]
    benc, penc = Encoders.bean(bf, device=dev), Encoders.bean(pf, device=dev)
    nb, n = len(bvals), len(pvals)
    build = _Batch(oracle, benc, bf, _device_src(_Src(dev, benc, [fixed_column(np.int64, np.arange(nb)),
                                                                  string_column(bvals)], nb), 0))
    probe = _Batch(oracle, penc, pf, _device_src(_Src(dev, penc, [string_column(pvals),
                                                                  fixed_column(np.int64, np.arange(n))], n), 0))
    null_found = [0 if v is None else e for v, e in zip(pvals, expect)]
    for b, p, tag in ((build, probe, "clean"), (_dirty_padding(build, 1), _dirty_padding(probe, 0), "padding 0xFF")):
        for form in FORMS:
            want = run_lookup(b, ["s"], p, ["s"], f"lengths {tag}, hashes {form}", form)
            assert want.tolist() == expect
            want = run_lookup(b, ["s"], p, ["s"], f"lengths {tag}, hashes {form}, null_equal", form, True)
            assert want.tolist() == null_found
    benc.device_status()


# 3. each output alone, the bound form, a side stream ------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "pair"])
def test_outputs_bound_and_stream(oracle, dev, name):
    build, probe = build_of(oracle, dev, name, 4097), probe_of(oracle, dev, name, 4097, 4097)
    keys = _names(build, KEY_SETS[name][0])
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    for form in (None, "seed7"):
        for null_equal in (False, True):
            what = f"{name} hashes {form} null_equal={null_equal}"
            run_lookup(build, keys, probe, keys, f"{what}: rows alone", form, null_equal, outs=("rows",))
            run_lookup(build, keys, probe, keys, f"{what}: mask alone", form, null_equal, outs=("mask",),
                       want_first=False)
            run_lookup(build, keys, probe, keys, f"{what}: bound", form, null_equal, bound=True)
            run_lookup(build, keys, probe, keys, f"{what}: side stream", form, null_equal, stream=s)
            run_lookup(build, keys, probe, keys, f"{what}: bound, side stream", form, null_equal, bound=True,
                       stream=s, outs=("mask",))
    build.enc.device_status(s)
    build.enc.device_status()


# 4. bounds -----------------------------------------------------------------------------------------------------
BOUNDS_N = 257
BUILD_FIELDS = [T.field("id", T.INT64), T.field("s", T.STRING), T.field("t", T.STRING)]
PROBE_FIELDS = [T.field("t", T.STRING), T.field("s", T.STRING), T.field("id", T.INT64)]
BOUNDS_KEYS = ["id", "s"]


def _bounds_sides(oracle, dev):
    """Build: (id, s, t) with 37 distinct (id, s), s of 9 to 45 bytes with a few nulls, t random.
    Probe: (t, s, id) with 50 key numbers, 13 of them not in the build side.  The last probe row has
    a non-null s."""
    from fury_amd.encoder import Encoders
    if "bounds" not in _CACHE:
        n = BOUNDS_N
        rng = np.random.default_rng(31)

        def cols(ids, order):
            s = [None if k % 37 == 5 and k < 37 else bytes([65 + k % 50]) * (9 + k % 37) for k in ids]
            t = [rng.integers(0, 256, int(rng.integers(1, 20)), dtype=np.uint8).tobytes() for _ in ids]
            by = {"id": fixed_column(np.int64, ids % 37), "s": string_column(s), "t": string_column(t)}
            return [by[f.name] for f in order]
        benc, penc = Encoders.bean(BUILD_FIELDS, device=dev), Encoders.bean(PROBE_FIELDS, device=dev)
        pid = (np.arange(n) * 7) % 50
        pid[n - 1] = 3
        _CACHE["bounds"] = (
            _Batch(oracle, benc, BUILD_FIELDS, _device_src(_Src(dev, benc, cols(np.arange(n) % 37, BUILD_FIELDS), n), 0)),
            _Batch(oracle, penc, PROBE_FIELDS, _device_src(_Src(dev, penc, cols(pid, PROBE_FIELDS), n), 0)))
    return _CACHE["bounds"]


def _expect(build, probe, what, bad_build=(), bad_probe=()):
    """Under the call's own hashes and under all-equal ones (every probe row would be compared with a
    bad build row if it were in the table), both flag values."""
    for form in (None, "zero"):
        for null_equal in (False, True):
            build.enc.device_status()
            probe.enc.device_status()
            want = run_lookup(build, BOUNDS_KEYS, probe, BOUNDS_KEYS, f"{what}, hashes {form}, null_equal={null_equal}",
                              form, null_equal, bad_build=bad_build, bad_probe=bad_probe)
            for r in bad_probe:
                assert want[r] == -1
            for r in bad_build:
                assert (want != r).all()
            build.enc.device_status()                              # clean (again)
    return want


def test_bounds_sides_match_and_miss(oracle, dev):
    build, probe = _bounds_sides(oracle, dev)
    want = _expect(build, probe, "clean")
    assert (want >= 0).sum() > 100 and (want < 0).sum() > 60 and want[BOUNDS_N - 1] == 3


@pytest.mark.parametrize("how", H.MALFORMED)
def test_corrupt_probe_key_slot(oracle, dev, how):
    """tests/test_bounds.py's corruptions on the key field s of one probe row that had a match.
    huge_list_count overwrites payload bytes: no failure, another value."""
    build, probe = _bounds_sides(oracle, dev)
    k = probe.enc._select(["s"])[0]
    r = 150
    assert not (probe.rows[int(probe.offs[r]) + (k >> 3)] >> (k & 7)) & 1
    assert lookup_model(_cols(build, BOUNDS_KEYS), _cols(probe, BOUNDS_KEYS))[r] >= 0
    rows = _corrupt(probe.fields, probe.rows, probe.offs, BOUNDS_N, r, k, how)
    assert not np.array_equal(rows, probe.rows)
    bad = probe.with_rows(rows)
    if how == "huge_list_count":
        bad.ref = oracle.decode(bad.fields, rows, bad.offs, BOUNDS_N)
        _expect(build, bad, how)
    else:
        _expect(build, bad, how, bad_probe=[r])


@pytest.mark.parametrize("how", H.MALFORMED)
def test_corrupt_build_key_slot(oracle, dev, how):
    """The same corruptions on the key field s of a build row: a later row of its group (nothing
    changes for the lookups), then the first row of a group (the next row of the group is found).
    The build reports the row; the lookups report nothing."""
    build, probe = _bounds_sides(oracle, dev)
    k = build.enc._select(["s"])[0]
    clean = lookup_model(_cols(build, BOUNDS_KEYS), _cols(probe, BOUNDS_KEYS), True)   # what _expect returns
    for r, moved in ((150, False), (7, True)):
        assert not (build.rows[int(build.offs[r]) + (k >> 3)] >> (k & 7)) & 1
        rows = _corrupt(build.fields, build.rows, build.offs, BOUNDS_N, r, k, how)
        assert not np.array_equal(rows, build.rows)
        bad = build.with_rows(rows)
        if how == "huge_list_count":
            bad.ref = oracle.decode(bad.fields, rows, bad.offs, BOUNDS_N)
            _expect(bad, probe, how)
            continue
        want = _expect(bad, probe, f"{how} in build row {r}", bad_build=[r])
        if moved:
            assert (clean == 7).sum() > 0 and ((clean == 7) == (want == 7 + 37)).all()
        else:
            assert np.array_equal(want, clean)


def test_corrupt_slots_of_fields_that_are_not_keys(oracle, dev):
    build, probe = _bounds_sides(oracle, dev)
    sides = []
    for b in (build, probe):
        k = b.enc._select(["t"])[0]
        rows = b.rows
        for r, how in ((0, "offset_past_end"), (130, "size_past_end"), (BOUNDS_N - 1, "negative_size"),
                       (60, "huge_list_count")):
            rows = _corrupt(b.fields, rows, b.offs, BOUNDS_N, r, k, how)
        assert not np.array_equal(rows, b.rows)
        sides.append(b.with_rows(rows))
    _expect(sides[0], sides[1], "non-key corruption")


def test_truncated_probe_batch(oracle, dev):
    """row_offsets[n] cut 8 bytes into the last probe row's s payload, the rows at the very end of a
    device allocation: the last row's value leaves the batch."""
    build, probe = _bounds_sides(oracle, dev)
    k = probe.enc._select(["s"])[0]
    last = BOUNDS_N - 1
    base = int(probe.offs[last])
    assert not (probe.rows[base + (k >> 3)] >> (k & 7)) & 1
    slot = struct.unpack_from("<Q", probe.rows, base + 8 + 8 * k)[0]
    assert (slot & 0xFFFFFFFF) > 8
    cut = base + (slot >> 32) + 8
    assert cut % 8 == 0 and cut < int(probe.offs[BOUNDS_N])
    offs = probe.offs.copy()
    offs[BOUNDS_N] = cut
    bad = probe.with_rows(probe.rows[:cut].copy(), offs, edge=True)
    _expect(build, bad, "truncated", bad_probe=[last])
    del bad


def _untrusted(build, probe, table, null_equal):
    from fury_amd import KeyIndex, lookup_into
    dev, n = probe.batch.rows.device, probe.n
    out = torch.full((n + 1,), GUARD, dtype=torch.int64, device=dev)
    mask = torch.full(((n + 31) // 32 + 1,), WORD_GUARD, dtype=torch.int32, device=dev)
    index = KeyIndex(_side(build, BOUNDS_KEYS), table, None, True)
    lookup_into(index, _side(probe, BOUNDS_KEYS), out[:n], mask[:-1], null_equal,
                torch.zeros(n, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    got, words = out.cpu().numpy(), mask.cpu().numpy().view(np.uint32)
    assert got[-1] == GUARD and words[-1] == WORD_GUARD
    assert np.array_equal(words[:-1], lookup_mask(got[:-1]))
    return got[:-1]


def test_a_table_that_no_build_made(oracle, dev):
    """The table is the caller's memory.  All-zero words (every slot: hash 0, row 0) under all-zero
    probe hashes: every result is -1 or a true match, no error.  Slots that name row nrows: all -1,
    out of bounds reported."""
    from fury_amd import index_slots
    from fury_amd.encoder import IndexOutOfBoundsException
    build, probe = _bounds_sides(oracle, dev)
    bt, pt = key_tuples(*build.cols(BOUNDS_KEYS), build.n), key_tuples(*probe.cols(BOUNDS_KEYS), probe.n)
    slots = index_slots(build.n)
    for null_equal in (False, True):
        got = _untrusted(build, probe, torch.zeros(slots, dtype=torch.int64, device=dev), null_equal)
        probe.enc.device_status()                                  # no error
        assert set(got.tolist()) == {-1, 0}
        assert [g == 0 for g in got] == [k == bt[0] and (null_equal or None not in k) for k in pt]
        got = _untrusted(build, probe, torch.full((slots,), build.n, dtype=torch.int64, device=dev), null_equal)
        assert (got == -1).all()
        with pytest.raises(IndexOutOfBoundsException) as e:
            probe.enc.device_status()
        walked = [j for j, k in enumerate(pt) if null_equal or None not in k]
        assert H.row_of(str(e.value)) in walked
    probe.enc.device_status()


# 5. joins and filters --------------------------------------------------------------------------------------------
def test_lookup_join_pairs_equals_join_pairs(oracle, dev):
    """A build side with duplicates: 4097 rows of 37 keys (tests/test_group.py's batch)."""
    from fury_amd import build_index, join_pairs, lookup, lookup_join_pairs
    build = batch_of(oracle, dev, "mixed", 4097, "37")
    source = batch_of(oracle, dev, "mixed", 257, "37")
    rev = [f.name for f in reversed(source.fields)]
    probe = _Batch(oracle, source.enc.selected_encoder(rev), list(reversed(source.fields)),
                   source.enc.select_fields(source.batch, rev))
    for stream in (None, torch.cuda.Stream(device=dev)):
        index = build_index(_side(build, MIXED_KEYS), want_first=True, stream=stream)
        assert index.first is not None and not index.caller_hashes
        for null_equal in (False, True):
            want = lookup_model(_cols(build, MIXED_KEYS), _cols(probe, MIXED_KEYS), null_equal)
            found = lookup(index, _side(probe, MIXED_KEYS), null_equal, stream=stream)
            torch.cuda.synchronize()
            assert_same(found.cpu().numpy(), want, "lookup")
            pj, bi = lookup_join_pairs(index, _side(probe, MIXED_KEYS), null_equal, stream=stream)
            wj, wi = join_pairs(_side(probe, MIXED_KEYS), _side(build, MIXED_KEYS), null_equal, stream=stream)
            torch.cuda.synchronize()
            assert pj.numel() > 4097 and torch.equal(pj, wj) and torch.equal(bi, wi)
        torch.cuda.synchronize()
        assert_same(index.first.cpu().numpy(), group_model(*build.cols(MIXED_KEYS), build.n)[0], "index.first")
    build.enc.device_status()


def test_semi_join_and_anti_join_partition_the_probe_batch(oracle, dev):
    from fury_amd import build_index, semi_join
    build, probe = build_of(oracle, dev, "mixed", 257), probe_of(oracle, dev, "mixed", 4097, 257)
    index = build_index(_side(build, MIXED_KEYS))
    sel = probe.enc._select(MIXED_KEYS)
    tuples = key_tuples(*probe.cols(MIXED_KEYS), probe.n)
    for null_equal in (False, True):
        want = lookup_model(_cols(build, MIXED_KEYS), _cols(probe, MIXED_KEYS), null_equal)
        kept = []
        for anti in (False, True):
            out, mask = semi_join(index, _side(probe, MIXED_KEYS), anti=anti, null_equal=null_equal)
            torch.cuda.synchronize()
            rows = np.flatnonzero((want < 0) if anti else (want >= 0))
            bits = np.zeros(probe.n, np.uint8)
            bits[rows] = 1
            assert_same(mask.cpu().numpy().view(np.uint32), mask_words(bits), f"mask anti={anti}")
            assert out.nrows == len(rows) and 0 < len(rows) < probe.n
            got_rows, got_offs = out.rows.cpu().numpy(), out.row_offsets.cpu().numpy()
            whole = np.concatenate([probe.rows[int(probe.offs[r]):int(probe.offs[r + 1])] for r in rows])
            assert_same(got_rows[:int(got_offs[out.nrows])], whole, f"rows anti={anti}")
            dec = oracle.decode(probe.fields, got_rows, got_offs, out.nrows)
            assert key_tuples([probe.fields[k] for k in sel], [dec[k] for k in sel], out.nrows) == \
                [tuples[r] for r in rows]
            kept.append(set(rows.tolist()))
        assert kept[0] | kept[1] == set(range(probe.n)) and not kept[0] & kept[1]
    probe.enc.device_status()


# 6. a batch that crosses byte 2^31 / 2^32 of its buffer, the other one low ------------------------------------------
def test_high_offsets(oracle, dev):
    """The functions are not RowEncoder methods, so the placement matrix of tests/high_offsets.py does
    not reach them.  Its batch, doubled, is placed across the boundary as the build side with the
    probe batch low, then as the probe side with the build batch low: one placement of each boundary
    and kind."""
    from fury_amd.encoder import RowBatch
    from tests.test_high_offsets_gpu import Arena, device_batch, encoder
    ref = H.ref(oracle, "mixed")
    n, keys = ref.n, H.SPEC["mixed"]["hash"]
    enc = encoder(dev, "mixed")
    control = device_batch(dev, enc, ref.rows, ref.offs, n)
    rng = H.rng_of("lookup", "mixed")
    idx = np.concatenate([np.arange(n), rng.permutation(n)])       # every row again, in another order
    doubled = enc.take(control, torch.from_numpy(idx).to(dev))
    big = _Batch(oracle, enc, ref.fields, doubled)
    low = _Batch(oracle, enc, ref.fields, enc.take(control, torch.from_numpy(rng.integers(0, n, n // 2)).to(dev)))
    want = run_lookup(big, keys, low, keys, "base 0, build doubled", null_equal=True)
    assert (want >= 0).all() and (want < n).all()
    want = run_lookup(low, keys, big, keys, "base 0, probe doubled", null_equal=True)
    assert (want >= 0).sum() > n // 4 and (want < 0).sum() > n // 4
    arena = Arena(dev)
    try:
        offs = doubled.row_offsets.cpu().numpy()
        total = int(offs[2 * n])
        for case, high_is_build in (("inside_row-4g", True), ("row_starts_at-2g", True),
                                    ("inside_row-2g", False), ("row_starts_at-4g", False)):
            X = H.BOUNDARIES[case.rsplit("-", 1)[1]]
            base = H.case_base(case, offs)                         # row n: the copies lie at or above X
            assert base + int(offs[n]) <= X < base + int(offs[n + 1]) and base + total > X
            arena.clear()
            arena.place(doubled.rows[:total], base)
            placed = big.with_batch(RowBatch(arena.rows, doubled.row_offsets + base, 2 * n, enc.schema_hash))
            for form in (None, "seed7", "zero"):
                if high_is_build:
                    run_lookup(placed, keys, low, keys, f"{case} build, hashes {form}", form, null_equal=True)
                else:
                    run_lookup(low, keys, placed, keys, f"{case} probe, hashes {form}", form, null_equal=True)
            enc.device_status()
            arena.assert_guard()
    finally:
        arena.rows = arena.buf = None
        del arena
        torch.cuda.empty_cache()
