"""Per-group aggregates on the GPU (fury_row_aggregate; fury_amd.aggregate_into / bind_aggregate /
aggregate / group_by / group_by_rows).  Every output is compared in full, plus one guard entry, with the
model of tests/test_aggregate_model.py (written from the header's rules alone) applied to the oracle's
decode of the batch; the outputs are pre-filled with a garbage pattern so that rule 6 is observable,
and every case runs twice and must give identical outputs -- but for the float sums, which are checked
against math.fsum with rule 3's bound.  Marked gpu.

Dispatch thresholds this file assumes (asserted in test_thresholds): num_groups * num_aggs <= 2048
cells takes the on-chip path, more the global one; an ARGMIN / ARGMAX over a fixed-width type or BOOL
adds the row-number pass; one over STRING / BINARY / DECIMAL takes the compare-and-swap cell."""
from __future__ import annotations

import math
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from fury_amd import types as T  # noqa: E402
from fury_amd.workloads import Column  # noqa: E402
from tests import high_offsets as H  # noqa: E402
from tests import test_group as TG  # noqa: E402
from tests import test_order as TO  # noqa: E402
from tests.test_aggregate_model import FLOATS, SIGNED, SUMMABLE_INTS, aggregate_model, sum_bound  # noqa: E402
from tests.test_bounds import _corrupt  # noqa: E402
from tests.test_group_model import group_model  # noqa: E402
from tests.test_hash_model import fixed_column  # noqa: E402
from tests.test_keys_equal import _Batch, string_column  # noqa: E402
from tests.test_keys_equal_model import key_tuples, key_values  # noqa: E402
from tests.test_take import _device_src, _Src, assert_same  # noqa: E402

GUARD = 0x5A5A5A5A5A5A5A5A
ROW_COUNTS = [0, 1, 63, 64, 65, 257, 4097]
LDS_CELLS = 2048
DROPPED = [-1, None, -2 ** 63, 2 ** 40]                            # None: G itself
ISSUE_STRINGS = [b"", b"a", b"ab", b"abcdefgh", b"abcdefghi", b"\xe4\xbd\xa0\xff", b"ab", b"abcdefgh"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def Agg(op, field=None):
    from fury_amd import Agg as A
    return A(op, field)


def test_thresholds():
    import fury_amd
    assert fury_amd.aggregate.lds_cells() == LDS_CELLS


# ---- the model over a batch ---------------------------------------------------------------------------------------
_VALUES: dict = {}


def _bits(a, n):
    return np.unpackbits(np.asarray(a).view(np.uint8), bitorder="little")[:n].astype(bool)


def field_values(b, field):
    """(type id, the value bytes of every row, valid) of `field` from the oracle's decode, made once."""
    k = (id(b.ref), field)
    if k not in _VALUES:
        (f,), (c,) = b.cols([field])
        if f.type_id in (T.LIST, T.STRUCT, T.MAP):                      # COUNT: only the null bit
            vals = [b""] * b.n
            valid = np.ones(b.n, bool) if c.validity is None or b.n == 0 else _bits(c.validity, b.n)
        else:
            v, valid = key_values(f, c, b.n)
            vals = [bytes(x) for x in v]
        _VALUES[k] = (f.type_id, vals, np.asarray(valid, bool), b.ref)
    return _VALUES[k][:3]


def _f64(word):
    return struct.unpack("<d", struct.pack("<q", int(word)))[0]


def run_agg(b, ids, G, aggs, what, counts=None, stream=None, bound=False, bad_rows=(), null_cells=(),
            exact_sums=True, ids_t=None):
    """One aggregate_into call into guarded, garbage-filled outputs, twice, compared in full with the
    model.  ids: a numpy int64 array or None; counts: which aggregates get an out_count (None: all).
    bad_rows: rows whose header fails rule 7; null_cells: (aggregate, row) values that fail it;
    device_status must name one of them after each call.  exact_sums: float sums must match the exact
    sum bit for bit (integer-valued floats), else rule 3's bound decides.  Returns the model's
    [(out as int64, count)]."""
    from fury_amd import aggregate_into, bind_aggregate
    dev, n = b.batch.rows.device, b.n
    want = []
    for j, (op, field) in enumerate(aggs):
        if field is None:
            tid, vals, valid = None, [b""] * n, np.ones(n, bool)
        else:
            tid, vals, valid = field_values(b, field)
        valid = valid.copy()
        valid[list(bad_rows)] = False
        for jj, r in null_cells:
            if jj == j:
                valid[r] = False
        want.append(aggregate_model(tid, vals, valid, ids, G, op))
    if ids_t is None and ids is not None:
        ids_t = torch.from_numpy(np.asarray(ids, np.int64)).to(dev)
    given = [True] * len(aggs) if counts is None else counts
    fails = set(bad_rows) | {r for _, r in null_cells}
    runs = []
    for _ in range(2):
        outs = [torch.full((G + 1,), GUARD, dtype=torch.int64, device=dev) for _ in aggs]
        cnts = [torch.full((G + 1,), GUARD, dtype=torch.int64, device=dev) if g else None for g in given]
        torch.cuda.synchronize()
        args = (b.enc, b.batch, ids_t, G, aggs, [o[:G] for o in outs], [None if c is None else c[:G] for c in cnts])
        if bound:
            bind_aggregate(*args, stream=stream)()
        else:
            aggregate_into(*args, stream=stream)
        torch.cuda.synchronize()
        if fails:                                                   # each run reports one of them
            from fury_amd.encoder import IndexOutOfBoundsException
            with pytest.raises(IndexOutOfBoundsException) as e:
                b.enc.device_status(stream)
            assert H.row_of(str(e.value)) in fails, (what, str(e.value))
        else:
            b.enc.device_status(stream)                             # nothing was raised
        runs.append(([o.cpu().numpy() for o in outs], [None if c is None else c.cpu().numpy() for c in cnts]))
    guard = np.array([GUARD], np.int64)
    for j, (op, field) in enumerate(aggs):
        w_out, w_cnt, abs_sums, finite = want[j]
        tid = None if field is None else field_values(b, field)[0]
        got, cnt = runs[0][0][j], runs[0][1][j]
        name = f"{what}: aggs[{j}] = {op}({field})"
        assert got[G] == GUARD, name
        if cnt is not None:
            assert_same(cnt, np.concatenate([w_cnt, guard]), name + " count")
        if op == "sum" and tid in FLOATS:
            for r in range(2):                                      # each run on its own: the order may differ
                for g in range(G):
                    x, exact = _f64(runs[r][0][j][g]), _f64(w_out.view(np.int64)[g])
                    if math.isnan(exact):
                        assert math.isnan(x), (name, g)
                    elif math.isinf(exact) or exact_sums:
                        assert x == exact, (name, g, x, exact)
                    else:                                           # fsum rounds the exact sum once: half an ulp
                        assert abs(x - exact) <= sum_bound(abs_sums[g], finite[g]) + math.ulp(exact) / 2, (name, g)
            continue
        assert_same(got, np.concatenate([w_out.view(np.int64), guard]), name)
        assert np.array_equal(got, runs[1][0][j]), name + ": the second run differs"
    for x, y in zip(runs[0][1], runs[1][1]):
        assert (x is None and y is None) or np.array_equal(x, y), f"{what}: the second run's counts differ"
    return [(w[0].view(np.int64), w[1]) for w in want]


# ---- id patterns ------------------------------------------------------------------------------------------------------
def id_patterns(n):
    """name -> (ids or None, G)."""
    rng = np.random.default_rng(n + 7)
    runs = np.repeat(np.arange(n), rng.integers(1, 150, max(n, 1)))[:n]      # sorted: runs straddle wave and workgroup edges
    dropped = rng.integers(0, 37, n)
    for k, d in enumerate(DROPPED):
        dropped[k::9] = 37 if d is None else d
    return {
        "one": (np.zeros(n, np.int64), 1),
        "none": (None, 1),
        "perm": (rng.permutation(n), n),
        "37": (rng.integers(0, 37, n), 37),
        "runs": (runs, int(runs.max()) + 1 if n else 0),
        "even": (2 * rng.integers(0, 21, n), 41),                    # empty groups between the others
        "dropped": (dropped, 37),
    }


# ---- 1. every type: its edge values, 30% nulls, an all-null group, every op it takes, every id pattern ----------------
_TYPE_CACHE: dict = {}
TYPE_N = 257


def type_values(tid, n):
    pool = list(TO.VALUES[tid]) + (ISSUE_STRINGS if tid in (T.STRING, T.BINARY) else [])
    rng = np.random.default_rng(tid * 1000 + n)
    return [None if rng.random() < 0.3 else pool[int(rng.integers(0, len(pool)))] for _ in range(n)]


def type_batch(oracle, dev, tid, n=TYPE_N):
    """(id INT64, k): n values drawn from the type's edge values (tests/test_order.py's sets: integer
    extremes at every width; +-0, +-inf, both NaN signs with payloads, denormals; strings around the
    8-byte words with duplicates, prefixes and high bytes), about 30% nulls."""
    key = (tid, n)
    if key not in _TYPE_CACHE:
        vals = type_values(tid, n)
        fields = [T.field("id", T.INT64), T.field("k", tid)]
        _TYPE_CACHE[key] = TO._make(oracle, dev, fields, [fixed_column(np.int64, np.arange(n)), TO._col(tid, vals)], n)
    return _TYPE_CACHE[key]


def ops_of(tid):
    ops = ["count", "argmin", "argmax"]
    if tid in SUMMABLE_INTS:
        ops.append("sum")
    if tid in SIGNED or tid in FLOATS or tid == T.BOOL:
        ops += ["min", "max"]
    return ops


@pytest.mark.parametrize("tid", list(TO.VALUES))
def test_every_type(oracle, dev, tid):
    b = type_batch(oracle, dev, tid)
    assert b.fixed == (tid not in (T.STRING, T.BINARY, T.DECIMAL))
    aggs = [Agg(op, "k") for op in ops_of(tid)]                        # the same field under several ops
    _, vals, valid = field_values(b, "k")
    assert 0.15 < 1 - valid.mean() < 0.45
    pats = id_patterns(b.n)
    pats["nullgroup"] = (np.where(valid, 1 + np.arange(b.n) % 5, 0), 6)        # group 0: only nulls
    for name, (ids, G) in pats.items():
        want = run_agg(b, ids, G, aggs, f"type {tid} ids {name}")
        if name == "nullgroup":
            for (op, _), (out, cnt) in zip(aggs, want):
                assert cnt[0] == 0 and out[0] == (-1 if op.startswith("arg") else 0)
        if name in ("one", "none") and tid in (T.STRING, T.BINARY):
            live = [v for v, ok in zip(vals, valid) if ok]
            assert vals[want[1][0][0]] == min(live) == b"" and vals[want[2][0][0]] == max(live) >= b"\x80"
            assert live.count(b"ab") > 1                            # ties and word-boundary prefixes in one group
    b.enc.device_status()


def test_rule_5_against_compare_rows(oracle, dev):
    """compare_rows of the ARGMIN (ARGMAX) row against every non-null row of its group is <= 0 (>= 0),
    and 0 only at rows with larger numbers."""
    from fury_amd import KeySide, aggregate, compare_rows
    for tid in (T.STRING, T.DECIMAL, T.FLOAT32, T.INT8, T.BOOL):
        b = type_batch(oracle, dev, tid)
        ids, G = id_patterns(b.n)["37"]
        ids_t = torch.from_numpy(ids).to(dev)
        res = aggregate(b.enc, b.batch, ids_t, G, [Agg("argmin", "k"), Agg("argmax", "k")])
        valid = field_values(b, "k")[2]
        rows = np.flatnonzero(valid)
        for r, sign in ((res[0], 1), (res[1], -1)):
            arg = r.values.cpu().numpy()
            assert ((arg >= 0) == (r.count.cpu().numpy() > 0)).all()
            left = torch.from_numpy(arg[ids[rows]]).to(dev)
            right = torch.from_numpy(rows).to(dev)
            cmp = compare_rows(KeySide(b.enc, b.batch, ["k"], left), KeySide(b.enc, b.batch, ["k"], right))
            cmp = cmp.cpu().numpy().astype(np.int64) * sign
            assert (cmp <= 0).all(), tid
            assert (rows[cmp == 0] >= arg[ids[rows]][cmp == 0]).all(), tid


# ---- 2. row counts x id patterns, one call of mixed aggregates; both sides of the cell threshold -----------------------
MATRIX_FIELDS = [T.field("v", T.INT64), T.field("i", T.INT32), T.field("s", T.STRING), T.field("f", T.FLOAT32),
                 T.field("b", T.BOOL), T.field("d", T.FLOAT64), T.field("l", T.LIST, True, [T.field("item", T.INT32)])]
MATRIX_AGGS = [("count", None), ("sum", "v"), ("min", "i"), ("argmax", "s"), ("sum", "f"), ("max", "f"),
               ("argmin", "i"), ("count", "l"), ("max", "b"), ("sum", "d"), ("count", "s")]


def matrix_batch(oracle, dev, n):
    """v wraps around int64 in a sum; i has few values (ties); f is integer-valued (sums exact in any
    order); d is integer-valued too; l is a LIST (COUNT only); about 30% nulls in each but v."""
    from fury_amd.encoder import Encoders
    key = ("matrix", n)
    if key not in _TYPE_CACHE:
        rng = np.random.default_rng(n + 11)

        def nulls():
            return np.flatnonzero(rng.random(n) < 0.3)
        v = rng.integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64)
        strs = [None if rng.random() < 0.3 else ISSUE_STRINGS[int(rng.integers(0, len(ISSUE_STRINGS)))]
                for _ in range(n)]
        lvalid = rng.random(n) >= 0.3
        lens = np.where(lvalid, rng.integers(0, 4, n), 0)
        offs = np.zeros(n + 1, np.int32)
        np.cumsum(lens, out=offs[1:])
        items = Column(values=rng.integers(-9, 9, int(offs[n])).astype(np.int32),
                       validity=np.packbits(np.ones(int(offs[n]), bool), bitorder="little"))
        host = [fixed_column(np.int64, v), fixed_column(np.int32, rng.integers(-3, 4, n), nulls()),
                string_column(strs), fixed_column(np.float32, rng.integers(-1000, 1000, n), nulls()),
                Column(values=np.packbits(rng.random(n) < 0.5, bitorder="little"),
                       validity=np.packbits(rng.random(n) >= 0.3, bitorder="little")),
                fixed_column(np.float64, rng.integers(-2 ** 40, 2 ** 40, n), nulls()),
                Column(validity=np.packbits(lvalid, bitorder="little"), offsets=offs, child=[items])]
        enc = Encoders.bean(MATRIX_FIELDS, device=dev)
        _TYPE_CACHE[key] = _Batch(oracle, enc, MATRIX_FIELDS, _device_src(_Src(dev, enc, host, max(n, 0)), 0))
    return _TYPE_CACHE[key]


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_matrix(oracle, dev, n):
    aggs = [Agg(*a) for a in MATRIX_AGGS]
    if n == 0:
        b = matrix_batch(oracle, dev, 1)
        empty = b.with_batch(b.enc.slice_rows(b.batch, 0, 0))
        empty.ref = oracle.decode(b.fields, b.rows[:0], b.offs[:1], 0)
        none = np.zeros(0, np.int64)
        for G in (0, 1, 5):                                         # rule 6 with no rows: every entry, the empty values
            run_agg(empty, none, G, aggs, f"empty G={G}")
            run_agg(empty, none, G, aggs, f"empty G={G} bound", bound=True)
        run_agg(empty, None, 1, aggs, "empty, no ids")
        b.enc.device_status()
        return
    b = matrix_batch(oracle, dev, n)
    for name, (ids, G) in id_patterns(n).items():
        run_agg(b, ids, G, aggs, f"n={n} ids {name}")
    b.enc.device_status()


@pytest.mark.parametrize("naggs", [1, 3, 11])
def test_both_sides_of_the_cell_threshold(oracle, dev, naggs):
    """G * naggs at the last cell count of the on-chip path, and one group more: the global path."""
    n = 4097
    b = matrix_batch(oracle, dev, n)
    aggs = {1: [Agg("sum", "v")], 3: [Agg("argmax", "s"), Agg("min", "i"), Agg("sum", "f")],
            11: [Agg(*a) for a in MATRIX_AGGS]}[naggs]
    at = LDS_CELLS // naggs
    rng = np.random.default_rng(naggs)
    for G in (at, at + 1):
        assert (G * naggs <= LDS_CELLS) == (G == at)
        run_agg(b, rng.integers(0, G, n), G, aggs, f"{naggs} aggregates, G={G}, spread")
        run_agg(b, np.sort(rng.integers(0, G, n)), G, aggs, f"{naggs} aggregates, G={G}, sorted")
        run_agg(b, np.full(n, G - 1), G, aggs, f"{naggs} aggregates, G={G}, one hot group")
    b.enc.device_status()


# ---- 3. call shapes ----------------------------------------------------------------------------------------------------
SIXTEEN = [("count", None), ("count", 63), ("sum", 63), ("min", 63), ("max", 64), ("argmin", 64), ("argmax", 63),
           ("sum", 64), ("argmin", 9), ("argmax", 10), ("argmin", 11), ("min", 5), ("max", 6), ("sum", 5),
           ("count", 69), ("min", 0)]


@pytest.mark.parametrize("n", [257, 4097])
def test_sixteen_aggregates_over_two_bitmap_words(oracle, dev, n):
    """Slots 63 and 64 of the wide key schema lie in different bitmap words; all six ops; STRING,
    DECIMAL and BINARY cells beside word accumulators; 128 and 129 groups are the two paths."""
    b = TG.batch_of(oracle, dev, "keys", n, "37")
    assert [b.fields[k].type_id for k in (63, 64, 9, 10, 11, 5, 6, 0)] == [
        T.INT32, T.INT64, T.STRING, T.DECIMAL, T.BINARY, T.FLOAT32, T.FLOAT64, T.BOOL]
    aggs = [Agg(*a) for a in SIXTEEN]
    assert {a.op for a in aggs} == {"count", "sum", "min", "max", "argmin", "argmax"}
    rng = np.random.default_rng(n)
    some = [j % 3 != 1 for j in range(16)]                             # out_count for some and not for others
    for G in (1, 37, LDS_CELLS // 16, LDS_CELLS // 16 + 1):
        ids = rng.integers(0, G, n)
        run_agg(b, ids, G, aggs, f"16 aggregates n={n} G={G}", exact_sums=False)
        run_agg(b, ids, G, aggs, f"16 aggregates n={n} G={G}, some counts", counts=some, exact_sums=False)
    run_agg(b, None, 1, aggs, f"16 aggregates n={n}, no ids", counts=[False] * 16, exact_sums=False)
    b.enc.device_status()


@pytest.mark.parametrize("n", [65, 4097])
def test_fixed_size_rows(oracle, dev, n):
    """A fixed-size schema: row_offsets is None."""
    b = TG.batch_of(oracle, dev, "pair", n, "37")
    assert b.fixed and b.batch.row_offsets is None
    aggs = [Agg("sum", "a"), Agg("min", "b"), Agg("argmax", "a"), Agg("count", None), Agg("argmin", "b")]
    for name, (ids, G) in id_patterns(n).items():
        run_agg(b, ids, G, aggs, f"pair n={n} ids {name}")
    b.enc.device_status()


def test_bound_and_stream(oracle, dev):
    """bind_aggregate re-issued after the inputs' contents change; a side stream."""
    from fury_amd import bind_aggregate
    n = 4097
    b = matrix_batch(oracle, dev, n)
    aggs = [Agg(*a) for a in MATRIX_AGGS]
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    ids, G = id_patterns(n)["37"]
    for stream in (None, s):
        run_agg(b, ids, G, aggs, "side stream" if stream else "bound", stream=stream, bound=stream is None)
        run_agg(b, ids, G, aggs, "bound, side stream", stream=s, bound=True)
    # the same bound call after the ids changed in place
    ids_t = torch.from_numpy(ids).to(dev)
    outs = [torch.full((G,), GUARD, dtype=torch.int64, device=dev) for _ in aggs]
    call = bind_aggregate(b.enc, b.batch, ids_t, G, aggs, outs)
    call()
    torch.cuda.synchronize()
    first = [o.cpu().numpy().copy() for o in outs]
    other = np.random.default_rng(5).integers(-2, G + 2, n)
    ids_t.copy_(torch.from_numpy(other).to(dev))
    call()
    torch.cuda.synchronize()
    again = run_agg(b, other, G, aggs, "the bound call's second issue", ids_t=ids_t)
    changed = 0
    for j, (o, (want, _)) in enumerate(zip(outs, again)):
        assert_same(o.cpu().numpy(), want, f"bound, new ids: aggs[{j}]")
        changed += not np.array_equal(first[j], want)
    assert changed >= 6
    b.enc.device_status(s)
    b.enc.device_status()


# ---- 4. float sums: random doubles for the bound, infinities, NaN --------------------------------------------------------
def test_float_sums(oracle, dev):
    n = 4097
    rng = np.random.default_rng(17)
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, n)
    y = (rng.standard_normal(n) * 1e3).astype(np.float32)
    inf = x.copy()
    inf[100::997] = np.inf                                          # some groups +inf
    inf[200::997] = -np.inf                                         # one group both: NaN
    nan = x.copy()
    nan[7::501] = np.nan                                            # every group of "5"
    fields = [T.field("x", T.FLOAT64), T.field("y", T.FLOAT32), T.field("inf", T.FLOAT64), T.field("nan", T.FLOAT64)]
    nulls = np.flatnonzero(rng.random(n) < 0.3)
    host = [fixed_column(np.float64, x, nulls), fixed_column(np.float32, y), fixed_column(np.float64, inf),
            fixed_column(np.float64, nan)]
    b = TO._make(oracle, dev, fields, host, n)
    aggs = [Agg("sum", f.name) for f in fields]
    ids = np.arange(n) % 5
    ids[100], ids[200] = 0, 0                                       # +inf and -inf meet in group 0
    for name, (i, G) in (("one", (None, 1)), ("5", (ids, 5)), ("37", id_patterns(n)["37"]),
                         ("2049", (rng.integers(0, 2049, n), 2049))):
        want = run_agg(b, i, G, aggs, f"float sums ids {name}", exact_sums=False)
        if name == "5":
            assert math.isnan(_f64(want[2][0][0])) and _f64(want[2][0][3]) == math.inf
            assert all(math.isnan(_f64(w)) for w in want[3][0])
    b.enc.device_status()


# ---- 5. bounds -------------------------------------------------------------------------------------------------------------
BOUNDS_AGGS = [("argmin", "s"), ("argmax", "s"), ("count", "s"), ("sum", "id"), ("count", None)]


def _bounds_ids():
    return np.arange(TG.BOUNDS_N) % 7, 7


@pytest.mark.parametrize("how", H.MALFORMED)
def test_corrupt_value_slot(oracle, dev, how):
    """tests/test_bounds.py's corruptions on the value field s of one row: null for the ARG aggregates,
    still counted by COUNT (its null bit is clear), named by device_status; every other group is
    unchanged.  huge_list_count overwrites payload bytes: no failure, another value."""
    b = TG._bounds_batch(oracle, dev)
    k = b.enc._select(["s"])[0]
    aggs = [Agg(*a) for a in BOUNDS_AGGS]
    ids, G = _bounds_ids()
    clean = run_agg(b, ids, G, aggs, "clean")
    for r in (150, 185):                                            # 185: the row that wins its group's argmin
        assert not (b.rows[int(b.offs[r]) + (k >> 3)] >> (k & 7)) & 1
        rows = _corrupt(b.fields, b.rows, b.offs, TG.BOUNDS_N, r, k, how)
        assert not np.array_equal(rows, b.rows)
        bad = b.with_rows(rows)
        if how == "huge_list_count":
            bad.ref = oracle.decode(bad.fields, rows, bad.offs, TG.BOUNDS_N)
            run_agg(bad, ids, G, aggs, how)
            continue
        b.enc.device_status()
        got = run_agg(bad, ids, G, aggs, f"{how} row {r}", null_cells=[(0, r), (1, r)])
        b.enc.device_status()                                       # clean again
        for (out, cnt), (out0, cnt0) in zip(got, clean):
            keep = np.arange(G) != ids[r]
            assert np.array_equal(out[keep], out0[keep]) and np.array_equal(cnt[keep], cnt0[keep])
        assert np.array_equal(got[2][0], clean[2][0]) and np.array_equal(got[3][0], clean[3][0])
        assert got[0][1][ids[r]] == clean[0][1][ids[r]] - 1
        # without an ARG aggregate the value's slot is not looked at: nothing is raised
        run_agg(bad, ids, G, aggs[2:], f"{how} row {r}, COUNT and SUM only")
        # a dropped id: the row is not looked at at all
        dropped = ids.copy()
        dropped[r] = -1
        run_agg(bad, dropped, G, aggs, f"{how} row {r} dropped")
    b.enc.device_status()


def test_corrupt_slots_of_fields_no_aggregate_names(oracle, dev):
    b = TG._bounds_batch(oracle, dev)
    k = b.enc._select(["t"])[0]
    rows = b.rows
    for r, how in ((0, "offset_past_end"), (130, "size_past_end"), (TG.BOUNDS_N - 1, "negative_size")):
        rows = _corrupt(b.fields, rows, b.offs, TG.BOUNDS_N, r, k, how)
    assert not np.array_equal(rows, b.rows)
    ids, G = _bounds_ids()
    run_agg(b.with_rows(rows), ids, G, [Agg(*a) for a in BOUNDS_AGGS], "corruption of t")
    b.enc.device_status()


def test_row_header_past_the_end(oracle, dev):
    """row_offsets[n] cut into the last row's header, the rows at the very end of a device allocation:
    the last row takes part in nothing, COUNT(*) included."""
    b = TG._bounds_batch(oracle, dev)
    last = TG.BOUNDS_N - 1
    cut = int(b.offs[last]) + 16                                    # 8 bitmap bytes + 3 slots = 32 bytes of header
    offs = b.offs.copy()
    offs[TG.BOUNDS_N] = cut
    bad = b.with_rows(b.rows[:cut].copy(), offs, edge=True)
    ids, G = _bounds_ids()
    aggs = [Agg(*a) for a in BOUNDS_AGGS]
    clean = run_agg(b, ids, G, aggs, "clean")
    got = run_agg(bad, ids, G, aggs, "truncated header", bad_rows=[last])
    assert got[4][0][ids[last]] == clean[4][0][ids[last]] - 1
    b.enc.device_status()
    dropped = ids.copy()
    dropped[last] = G
    run_agg(bad, dropped, G, aggs, "truncated header, the row dropped")
    del bad


# ---- 6. a batch that crosses byte 2^31 / 2^32 of its buffer ------------------------------------------------------------------
def test_high_offsets(oracle, dev):
    """As tests/test_group.py's: the batch of tests/high_offsets.py placed across each boundary
    aggregates to the results of its control."""
    from fury_amd.encoder import RowBatch
    from tests.test_high_offsets_gpu import Arena, device_batch, encoder
    ref = H.ref(oracle, "mixed")
    n = ref.n
    enc = encoder(dev, "mixed")
    control = device_batch(dev, enc, ref.rows, ref.offs, n)
    b = _Batch(oracle, enc, ref.fields, control)
    aggs = [Agg("argmin", "s1"), Agg("argmax", "s2"), Agg("sum", "b"), Agg("min", "a"), Agg("sum", "c"),
            Agg("argmax", "b"), Agg("count", None)]
    rng = H.rng_of("aggregate", "mixed")
    ids = rng.integers(-1, 38, n)
    want = run_agg(b, ids, 37, aggs, "base 0", exact_sums=False)
    assert (want[6][1] > 0).all()
    arena = Arena(dev)
    try:
        offs = control.row_offsets.cpu().numpy()
        total = int(offs[n])
        for case in ("inside_row-2g", "row_starts_at-4g", "inside_row-4g"):
            X = H.BOUNDARIES[case.rsplit("-", 1)[1]]
            base = H.case_base(case, offs)
            assert base < X < base + total
            arena.clear()
            arena.place(control.rows[:total], base)
            placed = b.with_batch(RowBatch(arena.rows, control.row_offsets + base, n, enc.schema_hash))
            run_agg(placed, ids, 37, aggs, case, exact_sums=False)
            run_agg(placed, None, 1, aggs, case + ", one group", exact_sums=False)
            enc.device_status()
            arena.assert_guard()
    finally:
        arena.rows = arena.buf = None
        del arena
        torch.cuda.empty_cache()


# ---- 7. end to end: GROUP BY ------------------------------------------------------------------------------------------------------
E2E_AGGS = [("count", None), ("sum", "v"), ("argmax", "t"), ("min", "i"), ("count", "i"), ("max", "v")]


def test_group_by(oracle, dev):
    """group_by on the mixed batch of tests/test_group.py equals the model over its key tuples;
    group_by_rows decodes, through the oracle, to the same keys and values with nulls where counts are
    zero; taking the ARGMAX rows gives the per-group maximum strings."""
    from fury_amd import AggResult, Groups, group_by, group_by_rows
    b = TG.batch_of(oracle, dev, "mixed", 4097, "37")
    aggs = [Agg(*a) for a in E2E_AGGS]
    first, ids, rows, G = group_model(*b.cols(TG.MIXED_KEYS), b.n)
    want = []
    for op, field in aggs:
        tid, vals, valid = (None, [b""] * b.n, np.ones(b.n, bool)) if field is None else field_values(b, field)
        out, cnt, _, _ = aggregate_model(tid, vals, valid, ids, G, op)
        want.append((out.view(np.int64), cnt))
    for stream in (None, torch.cuda.Stream(device=dev)):
        g, res = group_by(b.enc, b.batch, TG.MIXED_KEYS, aggs, stream=stream)
        torch.cuda.synchronize()
        assert isinstance(g, Groups) and g.num_groups == G == 37 and all(isinstance(r, AggResult) for r in res)
        assert_same(g.group_ids.cpu().numpy(), ids, "group_by: ids")
        for j, (r, (out, cnt)) in enumerate(zip(res, want)):
            assert r.values.dtype == torch.int64
            assert_same(r.values.cpu().numpy(), out, f"group_by: aggs[{j}]")
            assert_same(r.count.cpu().numpy(), cnt, f"group_by: aggs[{j}] count")
    assert (want[3][1] == 0).any() and (want[3][1] > 0).any()          # min(i): some groups are all null
    # the ARGMAX rows hold the per-group maximum strings
    _, tvals, tvalid = field_values(b, "t")
    arg = res[2].values
    assert (res[2].count > 0).all()
    taken = b.enc.take(b.batch, arg)
    torch.cuda.synchronize()
    dec = oracle.decode(b.fields, taken.rows.cpu().numpy(), taken.row_offsets.cpu().numpy(), G)
    k = b.enc._select(["t"])[0]
    got = [x[0] for x in key_tuples([b.fields[k]], [dec[k]], G)]
    assert got == [max(tvals[r] for r in range(b.n) if ids[r] == gidx and tvalid[r]) for gidx in range(G)]
    # the result as rows
    names = ["n", "sum_v", "top_t", "min_i", "n_i", "max_v"]
    out, out_enc = group_by_rows(b.enc, b.batch, TG.MIXED_KEYS, aggs, names)
    torch.cuda.synchronize()
    assert out.nrows == G and out.schema_hash == out_enc.schema_hash
    fields = list(out_enc._schema.fields)
    assert [f.name for f in fields] == TG.MIXED_KEYS + names
    assert [f.type_id for f in fields][3:] == [T.INT64] * 6
    dec = oracle.decode(list(fields), out.rows.cpu().numpy(), out.row_offsets.cpu().numpy(), G)
    keys = key_tuples(list(fields)[:3], dec[:3], G)
    assert keys == list(dict.fromkeys(key_tuples(*b.cols(TG.MIXED_KEYS), b.n)))
    for j, (out_w, cnt) in enumerate(want):
        v, valid = key_values(fields[3 + j], dec[3 + j], G)
        assert np.array_equal(np.asarray(valid, bool), cnt > 0), names[j]
        got = np.ascontiguousarray(v).view(np.int64).reshape(G)
        assert np.array_equal(got[cnt > 0], out_w[cnt > 0]), names[j]
    b.enc.device_status()


def test_natural_dtypes(oracle, dev):
    """aggregate: float64 for float sums and FLOAT64 min / max, float32 from the low halves for a FLOAT32
    min / max, and aggregate_into into a float32 tensor of 2 G entries."""
    from fury_amd import aggregate, aggregate_into
    b = type_batch(oracle, dev, T.FLOAT32)
    ids, G = id_patterns(b.n)["37"]
    ids_t = torch.from_numpy(ids).to(dev)
    aggs = [Agg("min", "k"), Agg("max", "k"), Agg("sum", "k"), Agg("argmin", "k")]
    want = run_agg(b, ids, G, aggs, "float32", exact_sums=False)
    res = aggregate(b.enc, b.batch, ids_t, G, aggs)
    assert [r.values.dtype for r in res] == [torch.float32, torch.float32, torch.float64, torch.int64]
    for j in (0, 1):
        bits = res[j].values.cpu().numpy().view(np.uint32).astype(np.int64)
        assert_same(bits, want[j][0], f"float32 {aggs[j].op}: bits, NaN payloads included")
    two = torch.full((2 * G,), -7.0, dtype=torch.float32, device=dev)
    aggregate_into(b.enc, b.batch, ids_t, G, aggs[:1], [two])
    torch.cuda.synchronize()
    assert_same(two.cpu().numpy().view(np.int64), want[0][0], "float32 min into a float32 tensor")
    d = type_batch(oracle, dev, T.FLOAT64)
    res = aggregate(d.enc, d.batch, ids_t, G, [Agg("max", "k"), Agg("count", "k")])
    assert res[0].values.dtype == torch.float64 and res[1].values.dtype == torch.int64
    want = run_agg(d, ids, G, [Agg("max", "k")], "float64")
    assert_same(res[0].values.cpu().numpy().view(np.int64), want[0][0], "float64 max: bits")
    b.enc.device_status()
