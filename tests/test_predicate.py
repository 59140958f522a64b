"""WHERE masks on the GPU (fury_row_predicate; fury_amd.predicate_into / bind_predicate / predicate_mask /
where / count_where).  Every output is compared in full, plus one guard word after the mask and a guard
on both sides of the count, with the Python model of tests/test_predicate_model.py (written from the
header's rules alone) applied to the oracle's decode of the batch.  Wherever a batch has more than one
row the expected mask is asserted, from the model, to be neither all zeros nor all ones: no case passes
on a kernel that ignores its input.  Marked gpu."""
from __future__ import annotations

import ctypes
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from fury_amd import types as T  # noqa: E402
from tests import high_offsets as H  # noqa: E402
from tests import test_keys_equal as KE  # noqa: E402
from tests import test_order as TO  # noqa: E402
from tests import test_predicate_model as PM  # noqa: E402
from tests.test_bounds import _corrupt  # noqa: E402
from tests.test_hash import case  # noqa: E402
from tests.test_hash_model import fixed_column  # noqa: E402
from tests.test_keys_equal_model import key_tuples  # noqa: E402
from tests.test_take import _device_src, _Src, assert_same, expect  # noqa: E402

MASK_GUARD = 0x5A5A5A5A
COUNT_GUARD = 0x5A5A5A5A5A5A5A5A
COUNTS = [1, 31, 32, 33, 63, 64, 65, 257, 4097]
IS_NULL, EQ, LT, LE, GT, GE, STARTS_WITH, ENDS_WITH, CONTAINS = range(1, 10)
NOT, OR = PM.NOT, PM.OR


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


# ---- the model over a batch ---------------------------------------------------------------------------------------
_ROWS: dict = {}


def decoded(b):
    """The value bytes (None: null) of every field of every row of the side `b` (a KE._Batch), made once."""
    if id(b) not in _ROWS:
        _ROWS[id(b)] = (key_tuples(b.fields, b.ref, b.n), b)         # b: keeps the id its own
    return _ROWS[id(b)][0]


def forget(b):
    _ROWS.pop(id(b), None)


def term(b, name, op, lit=b"", flags=0):
    """A model term (field, type id, op, flags, literal) on the field `name` of the side `b`."""
    (k,) = b.enc._select([name])
    return (k, b.fields[k].type_id, op, flags, bytes(lit))


def nullable_term(b, name, flags=OR):
    return term(b, name, IS_NULL, b"", flags)


def mask_words(bits):
    padded = np.zeros(((len(bits) + 31) // 32) * 32, np.uint8)
    padded[:len(bits)] = np.asarray(bits, bool)
    return np.packbits(padded, bitorder="little").view(np.uint32).copy()


def c_terms(terms, keep):
    from fury_amd import _native as N
    recs = (N.FuryPredTerm * len(terms))()
    for j, (field, _, op, flags, lit) in enumerate(terms):
        recs[j].field, recs[j].op, recs[j].flags, recs[j].literal_len = field, op, flags, len(lit)
        if lit:
            buf = ctypes.create_string_buffer(lit, len(lit))
            keep.append(buf)
            recs[j].literal = ctypes.addressof(buf)
    keep.append(recs)
    return recs


def raw_call(b, terms):
    """The C entry point itself over the model terms: the literals are the model's bytes."""
    from fury_amd import _native as N
    from fury_amd.encoder import _check, _ptr, _stream_handle
    keep: list = []
    recs = c_terms(terms, keep)

    def call(out_mask, out_count, row_mask, stream):
        _check(N.lib().fury_row_predicate(b.enc._schema.handle, _ptr(b.batch.rows), _ptr(b.batch.row_offsets), b.n,
                                          recs, len(terms), _ptr(row_mask), _ptr(out_mask), _ptr(out_count),
                                          _stream_handle(stream)))
    call.keep = keep
    return call


def run(b, terms, what, examine=None, in_place=False, with_count=True, stream=None, call=None, rows=None,
        nontrivial=True):
    """One call into guarded outputs, compared in full with the model.  examine: the row_mask bits."""
    dev, n = b.batch.rows.device, b.n
    want, count = PM.mask_model(terms, decoded(b) if rows is None else rows, examine)
    if nontrivial and n > 1:
        assert 0 < count < n, f"{what}: the expected mask is trivial ({count} of {n})"
    nw = (n + 31) // 32
    out = torch.full((nw + 1,), MASK_GUARD, dtype=torch.int32, device=dev)
    cnt = torch.full((3,), COUNT_GUARD, dtype=torch.int64, device=dev)
    om, rm = out[:nw], None
    if examine is not None:
        rm = torch.from_numpy(mask_words(examine).view(np.int32)).to(dev)
        if in_place:
            om.copy_(rm)
            rm = om
    torch.cuda.synchronize()
    (call or raw_call(b, terms))(om, cnt[1:2] if with_count else None, rm, stream)
    torch.cuda.synchronize()
    assert_same(out.cpu().numpy().view(np.uint32), np.concatenate([want, [MASK_GUARD]]).astype(np.uint32),
                f"{what}: out_mask")
    assert cnt.cpu().tolist() == [COUNT_GUARD, count if with_count else COUNT_GUARD, COUNT_GUARD], f"{what}: out_count"
    assert count == sum(bin(int(w)).count("1") for w in want)
    return want, count


def run_either(b, terms, what, null_field, **kw):
    """`run`, the terms OR-ed with IS_NULL of `null_field` (which holds a null) where they alone select
    no row: the mask then says that every row with a value fails."""
    _, count = PM.mask_model(terms, decoded(b))
    if count == 0:
        assert len(terms) == 1
        terms = terms + [nullable_term(b, null_field)]
    return run(b, terms, what, **kw)


# ---- 1. every type, every comparison op, every value as the literal ----------------------------------------------
@pytest.mark.parametrize("tid", list(TO.VALUES))
def test_values_of_every_type(oracle, dev, tid):
    """Both sides of tests/test_order.py's type batches (fixed-size rows with row_offsets NULL for a
    fixed-width type; variable-length rows, k at another slot): every value of the table as the literal
    of every comparison op, plain and negated.  The batch holds a null: no mask is all ones."""
    seen = set()
    for b in TO._type_sides(oracle, dev, tid):
        rows = decoded(b)
        assert sum(r[b.enc._select(["k"])[0]] is None for r in rows) == 1
        for lit in TO.VALUES[tid]:
            for op in PM.COMPARISONS:
                for flags in (0, NOT):
                    _, count = run_either(b, [term(b, "k", op, lit, flags)], f"type {tid} op {op} flags {flags} {lit!r}",
                                          "k")
                    seen.add(count)
        for flags in (0, NOT):
            run(b, [term(b, "k", IS_NULL, b"", flags)], f"type {tid} is_null flags {flags}")
        b.enc.device_status()
    assert len(seen) > 2 or tid == T.BOOL


# ---- 2. strings: value lengths, literal lengths, where the match lies ------------------------------------------
LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 300]
NEEDLES = {1: b"N", 7: b"NEEDLE7", 8: b"NEEDLE-8", 9: b"NEEDLE--9", 17: b"NEEDLE-SEVENTEEN-!"[:17]}
STRING_FIELDS = [T.field("id", T.INT64), T.field("s", T.STRING), T.field("raw", T.BINARY)]


def _string_values():
    """For every length random bytes over {a, b}; every needle at offset 0, at the very end and across an
    8-byte word boundary of a value of every length that holds it; a false start, multibyte UTF-8, nulls."""
    rng = np.random.default_rng(17)
    vals = [None, b"", b"aaab", b"aab", b"ab", "héllo wörld".encode(), "日本語のテキスト".encode(), "é".encode(),
            b"abcdefg", b"abcdefgh", b"abcdefgh\x80", b"abcdefg\xff", None]
    for n in LENGTHS:
        vals.append(rng.choice(np.frombuffer(b"ab", np.uint8), n).tobytes())
        for m, needle in NEEDLES.items():
            for at in {0, n - m, 5, 8 - m // 2} if n >= m else ():
                if 0 <= at <= n - m:
                    v = bytearray(rng.choice(np.frombuffer(b"xy", np.uint8), n).tobytes())
                    v[at:at + m] = needle
                    vals.append(bytes(v))
    return vals


STRING_LITERALS = [b"", b"a", b"aab", b"ab", "é".encode(), "本語".encode(), b"\xa9", b"abcdefg", b"abcdefgh",
                   b"abcdefgh\x80", b"x" * 301] + list(NEEDLES.values())


def _strings(oracle, dev):
    if "predicate-strings" not in KE._CACHE:
        vals = _string_values()
        n = len(vals)
        host = [fixed_column(np.int64, np.arange(n)), KE.string_column(vals), KE.string_column(vals[::-1])]
        KE._CACHE["predicate-strings"] = TO._make(oracle, dev, STRING_FIELDS, host, n)
    return KE._CACHE["predicate-strings"]


def test_string_values_cover_the_edges():
    vals = [v for v in _string_values() if v is not None]
    assert {len(v) for v in vals} >= set(LENGTHS)
    assert sorted({len(v) for v in STRING_LITERALS}) == [0, 1, 2, 3, 6, 7, 8, 9, 17, 301]
    assert max(len(v) for v in vals) < 301
    for m, needle in NEEDLES.items():
        at = {(v.find(needle), len(v)) for v in vals if needle in v}
        assert any(o == 0 for o, n in at) and any(o == n - m and o > 0 for o, n in at)
        assert m == 1 or any(o // 8 != (o + m - 1) // 8 and o % 8 for o, n in at)      # across a word boundary
    assert b"aab" in b"aaab" and not b"aaab".startswith(b"aab")


@pytest.mark.parametrize("field", ["s", "raw"])
def test_strings(oracle, dev, field):
    b = _strings(oracle, dev)
    counts = {op: set() for op in range(EQ, CONTAINS + 1)}
    for lit in STRING_LITERALS:
        for op in range(EQ, CONTAINS + 1):
            for flags in (0, NOT):
                _, count = run_either(b, [term(b, field, op, lit, flags)], f"{field} op {op} flags {flags} {lit!r}",
                                      field)
                if not flags:
                    counts[op].add(count)
    assert all(len(c) > 1 for c in counts.values()), counts
    b.enc.device_status()


# ---- 3. row counts x term counts, NOT and OR, nulls present ----------------------------------------------------------
def _i32(x):
    return int(x).to_bytes(4, "little", signed=True)


def mixed_terms(b, rows, count):
    """Predicates of 1, 4, 5 and 32 terms over the mixed schema, their literals taken from the rows."""
    a = sorted(int.from_bytes(r[0], "little", signed=True) for r in rows if r[0] is not None) or [0]
    lo, med, hi = a[len(a) // 4], a[len(a) // 2], a[(3 * len(a)) // 4]
    if count == 1:
        return [term(b, "a", LE, _i32(med))]
    four = [term(b, "a", GE, _i32(lo)), term(b, "a", LE, _i32(hi)),
            term(b, "c", GT, struct.pack("<d", 0.3)), term(b, "s1", IS_NULL, b"", OR)]
    if count == 4:
        return four
    if count == 5:
        return four + [term(b, "s2", CONTAINS, b"a", NOT)]
    assert count == 32
    some = [r[0] for r in rows[::2] if r[0] is not None][:30] or [_i32(0)]
    some += [some[-1]] * (30 - len(some))
    return ([term(b, "a", EQ, v, OR if j else 0) for j, v in enumerate(some)] +
            [term(b, "c", IS_NULL, b"", NOT), term(b, "s3", GE, b"")])


@pytest.mark.parametrize("n", COUNTS)
def test_row_counts(oracle, dev, n):
    c = case(oracle, dev, "mixed", n)
    b = KE.left_of(oracle, dev, c)
    rows = decoded(b)
    if n >= 31:
        assert all(any(r[k] is None for r in rows) for k in range(6))        # nulls in every field
    for count in (1, 4, 5, 32):
        terms = mixed_terms(b, rows, count)
        assert len(terms) == count
        run(b, terms, f"mixed n={n}, {count} terms")
    run(b, mixed_terms(b, rows, 5), f"mixed n={n}, no count", with_count=False)
    b.enc.device_status()


def test_literal_pool_at_its_limit(oracle, dev):
    b = KE.left_of(oracle, dev, case(oracle, dev, "mixed", 257))
    terms = [term(b, "s2", LT, b"P" * 1024), term(b, "s2", CONTAINS, b"a" * 1016, OR),
             term(b, "s1", ENDS_WITH, b"z", NOT)]
    assert sum((len(t[4]) + 7) & ~7 for t in terms) == 2048
    run(b, terms, "a full literal pool")
    b.enc.device_status()


def test_fixed_schema_without_row_offsets(oracle, dev):
    c = case(oracle, dev, "struct100", 257)
    b = KE.left_of(oracle, dev, c)
    assert b.batch.row_offsets is None
    rows = decoded(b)
    med = sorted(int.from_bytes(r[0], "little", signed=True) for r in rows)[128]
    terms = [term(b, "f00", LT, med.to_bytes(8, "little", signed=True)),
             term(b, "f01", GE, struct.pack("<d", 0.5)), term(b, "f99", LT, struct.pack("<d", 0.25), OR)]
    run(b, terms, "struct100")
    run(b, terms[1:2], "struct100, one float term")
    b.enc.device_status()


# ---- 4. a second opinion: fury_row_compare against a one-row batch holding the literal ---------------------------
@pytest.mark.parametrize("field", ["a", "b", "c", "s1"])
def test_comparisons_agree_with_compare_rows(oracle, dev, field):
    from fury_amd import KeySide, compare_rows
    b = KE.left_of(oracle, dev, case(oracle, dev, "mixed", 257))
    rows = decoded(b)
    (k,) = b.enc._select([field])
    r = next(i for i in range(100, 257) if rows[i][k] is not None)
    one = b.enc.take(b.batch, torch.tensor([r], device=dev))
    cmp = compare_rows(KeySide(b.enc, b.batch, [field]),
                       KeySide(b.enc, one, [field], torch.zeros(b.n, dtype=torch.int64, device=dev))).cpu().numpy()
    valid = np.array([row[k] is not None for row in rows])
    for op, test in ((EQ, cmp == 0), (LT, cmp < 0), (LE, cmp <= 0), (GT, cmp > 0), (GE, cmp >= 0)):
        terms = [term(b, field, op, rows[r][k])]
        assert_same(PM.mask_model(terms, rows)[0], mask_words(valid & test), f"{field} op {op}: compare_rows")
        run_either(b, terms, f"{field} op {op} against row {r}", field)
    b.enc.device_status()


# ---- 5. row_mask ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 257])
def test_row_mask(oracle, dev, n):
    """Rows whose bit is 0 fail, in place too, and are not read: corrupt ones among them go unreported."""
    b = KE.left_of(oracle, dev, case(oracle, dev, "mixed", n))
    rows = decoded(b)
    examine = np.random.default_rng(n).random(n) < 0.6
    terms = mixed_terms(b, rows, 4)
    plain, count = run(b, terms, f"n={n} no row_mask")
    for in_place in (False, True):
        want, some = run(b, terms, f"n={n} row_mask, in place {in_place}", examine=examine, in_place=in_place)
        assert_same(want, plain & mask_words(examine), "the mask refines")
        assert 0 < some < count
    run(b, terms, f"n={n} row_mask, no count", examine=examine, with_count=False)
    # every row outside the mask corrupt: a string slot that points past the batch, a header past it
    k = b.enc._select(["s1"])[0]
    bad_rows, offs = b.rows.copy(), b.offs.copy()
    hit = [r for r in range(n - 1) if not examine[r] and rows[r][k] is not None]
    assert len(hit) > 3
    for r in hit:
        bad_rows = _corrupt(b.fields, bad_rows, offs, n, r, k, "offset_past_end")
    bad = b.with_rows(bad_rows)
    bad.enc.device_status()
    on_s1 = [term(b, "s1", GE, b"P"), term(b, "a", IS_NULL, b"", OR)]
    run(bad, on_s1, f"n={n} corrupt rows outside the mask", examine=examine, rows=rows)
    bad.enc.device_status()                                         # nothing was reported
    forget(bad)


# ---- 6. bounds -----------------------------------------------------------------------------------------------------------
BOUNDS_N = KE.BOUNDS_N


def _expect_bounds(bad, rows, terms, bad_rows, what):
    from fury_amd.encoder import IndexOutOfBoundsException
    bad.enc.device_status()
    run(bad, terms, what, rows=rows)
    if bad_rows:
        with pytest.raises(IndexOutOfBoundsException) as e:
            bad.enc.device_status()
        assert H.row_of(str(e.value)) in set(bad_rows), (what, str(e.value))
    bad.enc.device_status()                                         # clean (again)


@pytest.mark.parametrize("how", H.MALFORMED)
def test_corrupt_values(oracle, dev, how):
    """tests/test_bounds.py's corruptions on the field s of one row: the value is null (rule 7) and the
    row is named, whatever the terms before it gave.  huge_list_count only changes a STRING's payload:
    the model over the new decode."""
    left, _ = KE._bounds_sides(oracle, dev)
    k = left.enc._select(["s"])[0]
    r = next(i for i in range(BOUNDS_N // 2, BOUNDS_N) if decoded(left)[i][k] is not None)
    bytes_ = _corrupt(left.fields, left.rows, left.offs, BOUNDS_N, r, k, how)
    assert not np.array_equal(bytes_, left.rows)
    bad = left.with_rows(bytes_)
    rows = [list(x) for x in decoded(left)]
    if how == "huge_list_count":
        bad.ref = oracle.decode(bad.fields, bytes_, bad.offs, BOUNDS_N)
        rows, fails = decoded(bad), []
    else:
        rows[r][k] = None
        fails = [r]
    idr = int.from_bytes(rows[r][0], "little", signed=True)
    never = term(left, "id", EQ, (idr + 1).to_bytes(8, "little", signed=True))        # false on row r
    for terms in ([term(left, "s", GE, b"M")], [term(left, "s", IS_NULL)], [term(left, "s", CONTAINS, b"QQ", NOT)],
                  [never, term(left, "s", GE, b"A")],                  # decided before s is looked at
                  [term(left, "id", GE, (20).to_bytes(8, "little")), term(left, "s", ENDS_WITH, b"Z", OR)]):
        _expect_bounds(bad, rows, terms, fails, f"{how}: {[t[2] for t in terms]}")
    # t is no term's field: its slots are never looked at
    kt = left.enc._select(["t"])[0]
    rt = next(i for i in range(BOUNDS_N) if decoded(left)[i][kt])
    other = left.with_rows(_corrupt(left.fields, left.rows, left.offs, BOUNDS_N, rt, kt, "offset_past_end"))
    _expect_bounds(other, decoded(left), [term(left, "s", GE, b"M")], [], "a corrupt field no term names")
    forget(bad)


def test_row_header_outside_the_batch(oracle, dev):
    """row_offsets of the last row 8 bytes before the batch's end: its header leaves the batch, every field
    is null, the row is named."""
    from fury_amd.encoder import IndexOutOfBoundsException
    left, _ = KE._bounds_sides(oracle, dev)
    last = BOUNDS_N - 1
    offs = left.offs.copy()
    offs[last] = offs[BOUNDS_N] - 8
    bad = left.with_rows(left.rows, offs)
    rows = [list(x) for x in decoded(left)]
    rows[last] = [None] * 3
    for terms in ([term(left, "id", IS_NULL)], [term(left, "id", GE, bytes(8))], [term(left, "s", GE, b"M")]):
        want, _ = run(bad, terms, "header outside", rows=rows, nontrivial=terms[0][2] != IS_NULL)
        assert bool(want[last // 32] >> (last % 32) & 1) == (terms[0][2] == IS_NULL)
        with pytest.raises(IndexOutOfBoundsException) as e:
            bad.enc.device_status()
        assert H.row_of(str(e.value)) == last
    bad.enc.device_status()


# ---- 7. nothing past the batch is read, nothing past a value is compared ----------------------------------------------
@pytest.mark.parametrize("pad", [1, 3, 7])
@pytest.mark.parametrize("cut", [False, True])
def test_bytes_after_the_last_value(oracle, dev, pad, cut):
    """The batch is a slice of a larger device tensor and its last value ends `pad` bytes before the
    slice's end (cut: row_offsets[n] says the batch ends with the value, so its last word leaves the
    batch).  The padding and the bytes after the slice continue the value so that reading them would
    flip CONTAINS, ENDS_WITH, STARTS_WITH and EQ."""
    from fury_amd.encoder import Encoders, RowBatch
    fields = [T.field("id", T.INT64), T.field("s", T.STRING)]
    last = (b"0123456789abcdefghijklmn")[:24 - pad - 1] + b"X"           # 24 - pad bytes, ends with X
    vals = [b"XYZ", b"..XYZ..", None, b"endsXYZ", last]
    n = len(vals)
    enc = Encoders.bean(fields, device=dev)
    src = _Src(dev, enc, [fixed_column(np.int64, np.arange(n)), KE.string_column(vals)], n)
    total = int(src.offs[n])
    end = total - pad
    assert bytes(src.rows[end - len(last):end]) == last and not src.rows[end:total].any()
    after = torch.from_numpy(np.frombuffer(b"YZ" * 68, np.uint8).copy()).to(dev)      # what follows the value
    big = torch.cat([torch.from_numpy(src.rows).to(dev)[:end], after])
    offs = src.offs.copy()
    if cut:
        offs[n] = end
    batch = RowBatch(big[:int(offs[n])], torch.from_numpy(offs).to(dev), n, enc.schema_hash)
    b = object.__new__(KE._Batch)
    b.enc, b.fields, b.batch, b.n, b.fixed = enc, fields, batch, n, False
    rows = [(i.to_bytes(8, "little"), v) for i, v in enumerate(vals)]
    for op, lit in ((CONTAINS, b"XYZ"), (CONTAINS, b"XY"), (ENDS_WITH, b"XYZ"), (ENDS_WITH, b"XY"), (EQ, last + b"Y"),
                    (EQ, last), (GT, last), (STARTS_WITH, last + b"YZ"), (ENDS_WITH, b"X")):
        terms = [term(b, "s", op, lit)]
        if PM.mask_model(terms, rows)[1] == 0:
            terms.append(nullable_term(b, "s"))
        want, _ = run(b, terms, f"pad {pad} cut {cut} op {op} {lit!r}", rows=rows)
        if lit in (b"XYZ", b"XY", last + b"Y", last + b"YZ") or op == GT:
            assert not want[0] >> (n - 1) & 1                       # the last row: only with the bytes after it
    enc.device_status()


def _model_terms(b, pred):
    from fury_amd import predicate as P
    out = []
    for t, joins in P._flatten(pred):
        (k,) = b.enc._select([t.field])
        out.append((k, b.fields[k].type_id, P.N.PRED_OPS[t.op], (NOT if t.negate else 0) | (OR if joins else 0),
                    P.literal_bytes(b.fields[k], t.op, t.value)))
    return out


# ---- 8. a batch that crosses byte 2^31 and byte 2^32 of its buffer --------------------------------------------------
def test_high_offsets(oracle, dev):
    from fury_amd import predicate_mask
    from fury_amd import predicate as P
    from fury_amd.encoder import RowBatch
    from tests.test_high_offsets_gpu import Arena, device_batch, encoder
    ref = H.ref(oracle, "mixed")
    n = ref.n
    enc = encoder(dev, "mixed")
    control = device_batch(dev, enc, ref.rows, ref.offs, n)
    rows = key_tuples(ref.fields, ref.cols, n)
    a = sorted(int.from_bytes(r[0], "little", signed=True) for r in rows if r[0] is not None)
    pred = [P.between("a", a[len(a) // 8], a[-len(a) // 8]), (P.lt("s1", "P"), P.is_null("s2")),
            P.Term("s3", "contains", "e", True)]
    side = object.__new__(KE._Batch)
    side.enc, side.fields = enc, ref.fields
    terms = _model_terms(side, pred)
    want, count = PM.mask_model(terms, rows)
    assert 0 < count < n

    def run_at(batch):
        mask, cnt = predicate_mask(enc, batch, pred)
        return mask.cpu().numpy().view(np.uint32), int(cnt.item())

    got, c0 = run_at(control)
    assert_same(got, want, "base 0: mask")
    assert c0 == count
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
            got, c1 = run_at(RowBatch(arena.rows, control.row_offsets + base, n, enc.schema_hash))
            assert_same(got, want, f"{place}: mask")
            assert c1 == count
            arena.assert_guard()
    finally:
        arena.rows = arena.buf = None
        del arena
        torch.cuda.empty_cache()


# ---- 9. fury_amd.predicate end to end ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 4097])
def test_where(oracle, dev, n):
    """where = filter of the model's mask, byte for byte; count_where; the into and bound forms on a side
    stream."""
    import fury_amd as F
    b = KE.left_of(oracle, dev, case(oracle, dev, "mixed", n))
    rows = decoded(b)
    a = sorted(int.from_bytes(r[0], "little", signed=True) for r in rows if r[0] is not None)
    pred = [F.between("a", a[len(a) // 8], a[-len(a) // 8]), (F.ge("s1", "P"), F.starts_with("s2", "a"), F.is_null("s3")),
            F.ne("b", 0), F.not_null("c")]
    terms = _model_terms(b, pred)
    assert len(terms) == 7
    want, count = PM.mask_model(terms, rows)
    assert 0 < count < n
    keep = [i for i in range(n) if want[i // 32] >> (i % 32) & 1]
    data, offs, _ = expect(b.rows, b.offs, n, keep)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    for stream in (None, s):
        out, idx = F.where(b.enc, b.batch, pred, return_indices=True, stream=stream)
        torch.cuda.synchronize()
        assert out.nrows == count
        assert_same(out.rows.cpu().numpy(), data, f"n={n}: where rows")
        assert_same(out.row_offsets.cpu().numpy(), offs, f"n={n}: where offsets")
        assert_same(idx.cpu().numpy(), np.array(keep, np.int64), f"n={n}: where indices")
        assert F.count_where(b.enc, b.batch, pred, stream=stream) == count
        mask, cnt = F.predicate_mask(b.enc, b.batch, pred, stream=stream)
        torch.cuda.synchronize()
        assert mask.dtype == torch.int32 and cnt.dtype == torch.int64 and cnt.tolist() == [count]
        assert_same(mask.cpu().numpy().view(np.uint32), want, f"n={n}: predicate_mask")

        def into(om, oc, rm, st):
            F.predicate_into(b.enc, b.batch, pred, om, oc, rm, stream=st)

        def bound(om, oc, rm, st):
            call = F.bind_predicate(b.enc, b.batch, pred, om, oc, rm, stream=st)
            call()
            call()
        examine = np.random.default_rng(n).random(n) < 0.5
        for call in (into, bound):
            run(b, terms, f"n={n} {call.__name__}", stream=stream, call=call)
            run(b, terms, f"n={n} {call.__name__}, in place", stream=stream, call=call, examine=examine, in_place=True)
    b.enc.device_status(s)
    b.enc.device_status()
    refined = F.where(b.enc, b.batch, [F.not_null("a")], row_mask=torch.from_numpy(want.view(np.int32)).to(dev))
    assert_same(refined.rows.cpu().numpy(), data, "where under a row_mask")


def test_bound_call_sees_new_contents(oracle, dev):
    """bind_predicate re-issued after the batch's bytes changed in place gives the new answer."""
    import fury_amd as F
    from fury_amd.encoder import Encoders, RowBatch
    fields = [T.field("a", T.INT64), T.field("b", T.INT32)]
    enc = Encoders.bean(fields, device=dev)
    n = 257
    first = _Src(dev, enc, [fixed_column(np.int64, np.arange(n)), fixed_column(np.int32, np.arange(n) % 7)], n)
    second = _Src(dev, enc, [fixed_column(np.int64, np.arange(n)[::-1].copy()),
                             fixed_column(np.int32, np.arange(n) % 5)], n)
    assert first.fixed and len(first.rows) == len(second.rows)
    buf = torch.from_numpy(first.rows).to(dev)
    batch = RowBatch(buf, None, n, enc.schema_hash)
    pred = [F.lt("a", 100), F.ne("b", 3)]
    nw = (n + 31) // 32
    out = torch.full((nw + 1,), MASK_GUARD, dtype=torch.int32, device=dev)
    cnt = torch.full((3,), COUNT_GUARD, dtype=torch.int64, device=dev)
    call = F.bind_predicate(enc, batch, pred, out[:nw], cnt[1:2])
    for src, a_of, b_of in ((first, lambda i: i, lambda i: i % 7), (second, lambda i: n - 1 - i, lambda i: i % 5)):
        buf.copy_(torch.from_numpy(src.rows).to(dev))
        call()
        torch.cuda.synchronize()
        bits = [a_of(i) < 100 and b_of(i) != 3 for i in range(n)]
        assert 0 < sum(bits) < n
        assert_same(out.cpu().numpy().view(np.uint32), np.concatenate([mask_words(bits), [MASK_GUARD]]).astype(np.uint32),
                    "bound call")
        assert cnt.cpu().tolist() == [COUNT_GUARD, sum(bits), COUNT_GUARD]
    enc.device_status()


def test_more_tiles_than_workgroups(dev):
    """More 256-row tiles than the launch has workgroups: every workgroup walks several tiles and sums
    their counts.  The expectation is numpy's, on the columns themselves."""
    import fury_amd as F
    from fury_amd.encoder import Encoders, column_to_device
    fields = [T.field("a", T.INT64), T.field("b", T.INT32)]
    enc = Encoders.bean(fields, device=dev)
    n = 3 * 2048 * 256 + 77
    a = (np.arange(n, dtype=np.int64) * 2654435761) % 1000
    b = (np.arange(n) % 7).astype(np.int32)
    batch = enc.encode_batch([column_to_device(fixed_column(np.int64, a), dev),
                              column_to_device(fixed_column(np.int32, b), dev)], n)
    bits = (a < 300) & (b != 3)
    assert 0 < bits.sum() < n and bits[-77:].any() and not bits[-77:].all()
    nw = (n + 31) // 32
    out = torch.full((nw + 1,), MASK_GUARD, dtype=torch.int32, device=dev)
    cnt = torch.full((3,), COUNT_GUARD, dtype=torch.int64, device=dev)
    F.predicate_into(enc, batch, [F.lt("a", 300), F.ne("b", 3)], out[:nw], cnt[1:2])
    torch.cuda.synchronize()
    assert_same(out.cpu().numpy().view(np.uint32), np.concatenate([mask_words(bits), [MASK_GUARD]]).astype(np.uint32),
                "many tiles: out_mask")
    assert cnt.cpu().tolist() == [COUNT_GUARD, int(bits.sum()), COUNT_GUARD]
    enc.device_status()
