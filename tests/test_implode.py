"""Elements and nested values back into rows on the GPU (fury_row_implode / fury_row_wrap, RowEncoder /
ArrayEncoder.implode*, RowEncoder.wrap*, with_elements / with_nested): out_offsets and the whole output
buffer, with 4096 guard bytes on each side, equal the numpy model of tests/test_implode_model.py; for
rows a writer made they also equal the models of fury_row_select / fury_row_extract of the source
rows.  The inputs are the numpy expectations of explode / extract (tests/test_explode.py,
tests/test_extract.py) of the sources of tests/test_explode.py.  Marked gpu."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from fury_amd import types as T  # noqa: E402
from tests.test_explode import source  # noqa: E402
from tests.test_extract import FILL, GUARD, assert_same, levels_of  # noqa: E402
from tests.test_extract import expect as expect_extract  # noqa: E402
from tests.test_implode_model import (_bits, expect_implode, expect_wrap, least_of,  # noqa: E402
                                      list_target, value_lists)
from tests.test_select_model import expect_select  # noqa: E402

COUNTS = [1, 63, 64, 65, 257, 4097]
# (source, path, side): items, ll, fx, a map's values (into a fresh LIST<STRUCT>) and a nested path
TARGETS = [("flat", ("items",), "elements"), ("flat", ("ll",), "elements"), ("flat", ("fx",), "elements"),
           ("flat", ("m",), "values"), ("nested", ("outer", "items"), "elements")]
IDS = [".".join(t[1]) for t in TARGETS]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _field_at(fields, path):
    for name in path:
        node = fields[[f.name for f in fields].index(name)]
        fields = node.children
    return node


_TARGETS: dict = {}


def targets(src, path, side):
    """(one-field row encoder, array encoder) of the list the elements go back into."""
    from fury_amd.encoder import Encoders
    key = (id(src.enc), path, side)
    if key not in _TARGETS:
        f = _field_at(src.fields, path)
        if side == "values":
            f = list_target("mv", f.children[1])[0]
        _TARGETS[key] = (Encoders.bean([f], device=src.dev), Encoders.array_encoder(
            f.children[0], device=src.dev, name=f.name))
    return _TARGETS[key]


def _bitmap(dev, bits):
    """An Arrow bitmap on the device, padded to whole 32-bit words."""
    if bits is None:
        return None
    a = np.zeros((len(bits) + 3) // 4 * 4 + 4, np.uint8)
    a[:len(bits)] = bits
    return torch.from_numpy(a).to(dev)


class Case:
    """One call: the inputs on the host, the model's expectation, and the run into guarded buffers.
    lo None: fury_row_wrap (n rows, lv their validity)."""

    def __init__(self, enc, values, vo, lo, n, ev, lv, E):
        self.enc, self.n, self.E = enc, n, E
        self.values, self.vo = np.asarray(values, np.uint8), np.asarray(vo, np.int64)
        self.lo = None if lo is None else np.asarray(lo, np.int64)
        self.ev, self.lv = ev, lv
        self.nv = len(self.vo) - 1
        self.wrap = lo is None
        f = enc.schema().fields[0]
        self.rows_form = not enc.schema().collection
        self.least = least_of(f if self.wrap else f.children[0])
        self._want = None

    @property
    def want(self):
        if self._want is None:
            if self.wrap:
                self._want = expect_wrap(self.values, self.vo, self.nv, self.lv, self.n, self.least)
            else:
                self._want = expect_implode(self.values, self.vo, self.nv, self.lo, self.n, self.ev,
                                            self.lv, self.E, self.least, self.rows_form)
        return self._want

    def run(self, what, cap=None, measure=False, out_shift=0, src_shift=0, stream=None, bound=False,
            calls=1):
        from fury_amd.encoder import RowBatch
        dev, enc, n, w = self.enc.device, self.enc, self.n, self.want
        cap = len(w.data) if cap is None else cap
        vt = torch.empty(len(self.values) + 16, dtype=torch.uint8, device=dev)
        assert vt.data_ptr() % 16 == 0
        vals = vt[src_shift:src_shift + len(self.values)]
        vals.copy_(torch.from_numpy(self.values))
        batch = RowBatch(vals, torch.from_numpy(self.vo).to(dev), self.nv,
                         enc._value_encoder(self.wrap).schema_hash)
        t = torch.full((GUARD + 16 + cap + GUARD,), FILL, dtype=torch.uint8, device=dev)
        assert t.data_ptr() % 16 == 0
        at = GUARD + out_shift
        ooffs = torch.full((n + 2,), -7, dtype=torch.int64, device=dev)
        out = None if measure else t[at:at + cap]
        lv = _bitmap(dev, self.lv)
        if self.wrap:
            fns = (enc.wrap_into, enc.bind_wrap)
            args = (batch, out, ooffs[:n + 1])
            kw = dict(validity=lv, nrows=n, stream=stream)
        else:
            fns = (enc.implode_into, enc.bind_implode)
            args = (batch, torch.from_numpy(self.lo).to(dev), out, ooffs[:n + 1])
            kw = dict(entry_validity=_bitmap(dev, self.ev), elem_validity=lv, num_elements=self.E,
                      stream=stream)
        torch.cuda.synchronize()
        if bound:
            call = fns[1](*args, **kw)
            for _ in range(calls):
                call()
        else:
            for _ in range(calls):
                fns[0](*args, **kw)
        torch.cuda.synchronize()
        assert_same(ooffs.cpu().numpy(), np.concatenate([w.offs, [-7]]), f"{what}: out_offsets")
        want = np.full(t.numel(), FILL, np.uint8)
        if not measure:
            k = min(cap & ~7, len(w.data))         # a capacity off a multiple of 8 is rounded down
            want[at:at + k] = w.data[:k]
        assert_same(t.cpu().numpy(), want, f"{what}: output buffer")
        self.status(what, stream)
        return w

    def status(self, what, stream=None):
        """The call reported one of the model's rows, or nothing; the stream is clean afterwards."""
        from fury_amd.encoder import IndexOutOfBoundsException
        bad = self.want.bad
        if bad:
            with pytest.raises(IndexOutOfBoundsException, match=f"row ({'|'.join(map(str, bad))}) "):
                self.enc.device_status(stream)
        self.enc.device_status(stream)


def exploded_case(src, path, side, rows_form=True, ecap=None, entry_validity=True) -> Case:
    from tests.test_explode import expect
    w = src.want(path, side) if ecap is None else expect(src.rows, src.offs, src.n,
                                                         src.spec(path, side), ecap)
    enc = targets(src, path, side)[0 if rows_form else 1]
    ev = w.entry_valid if rows_form and entry_validity else None
    return Case(enc, w.data, w.offs, w.lo, src.n, ev, w.valid, w.E)


def extracted_case(src, path) -> Case:
    from fury_amd.encoder import Encoders
    ex = expect_extract(src.rows, src.offs, src.n, levels_of(src.fields, path))
    enc = Encoders.bean([_field_at(src.fields, path)], device=src.dev)
    return Case(enc, ex.data, ex.offs, None, src.n, None, ex.valid, src.n)


# 1. the round-trip identities, every target x row count -----------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("which,path,side", TARGETS, ids=IDS)
def test_implode_of_explode(dev, which, path, side, n):
    src = source(dev, which, n)
    what = f"{'.'.join(path)} n={n}"
    rows = exploded_case(src, path, side)
    w = rows.run(f"{what}: rows form")
    assert not w.bad
    coll = exploded_case(src, path, side, rows_form=False)
    c = coll.run(f"{what}: collection form", out_shift=8)
    assert not c.bad
    has = _bits(src.want(path, side).entry_valid, n)
    for r in np.flatnonzero(~has)[:4]:                         # a null row: an empty array
        assert c.offs[r + 1] - c.offs[r] == 8
    if side == "elements" and len(path) == 1:                  # = select {f} of the source rows
        k = [f.name for f in src.fields].index(path[0])
        sel = expect_select(src.rows, src.offs, n, src.fields, [k])
        assert_same(w.data, sel.data, f"{what}: implode(explode) = select")
        assert_same(w.offs, sel.offs, f"{what}: implode(explode) = select, offsets")
    if side == "elements":                                     # = extract {f}, where a row has one
        ex = expect_extract(src.rows, src.offs, n, levels_of(src.fields, path))
        mine = [c.data[c.offs[r]:c.offs[r + 1]] for r in np.flatnonzero(has)]
        assert_same(np.concatenate(mine) if mine else np.zeros(0, np.uint8), ex.data,
                    f"{what}: collection form = extract")


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("which,path", [("flat", ("items",)), ("flat", ("m",)), ("nested", ("outer",)),
                                        ("nested", ("outer", "ll"))], ids=".".join)
def test_wrap_of_extract(dev, which, path, n):
    src = source(dev, which, n)
    case = extracted_case(src, path)
    w = case.run(f"wrap {'.'.join(path)} n={n}")
    assert not w.bad
    case.run(f"wrap {'.'.join(path)} n={n}: shifted", out_shift=8, src_shift=8)
    if len(path) == 1:
        k = [f.name for f in src.fields].index(path[0])
        sel = expect_select(src.rows, src.offs, n, src.fields, [k])
        assert_same(w.data, sel.data, "wrap(extract) = select")
        assert_same(w.offs, sel.offs, "wrap(extract) = select, offsets")


@pytest.mark.parametrize("which,path,side", TARGETS, ids=IDS)
def test_the_result_is_what_the_encoder_writes(dev, which, path, side):
    """implode / wrap through the allocating forms = encode_batch of the same columns under the target
    schema, and decode_batch of the result gives the lists back."""
    from fury_amd.beans import beans_to_columns, columns_to_beans
    from fury_amd.encoder import RowBatch, column_to_device, column_to_host
    n = 257
    src = source(dev, which, n)
    enc, arr = targets(src, path, side)
    f = enc.schema().fields[0]
    if side == "values":
        lists = value_lists(src.beans, path)
    else:
        lists = []
        for b in src.beans:
            for name in path:
                b = None if b is None else b[name]
            lists.append(b)
    cols = [column_to_device(c, dev) for c in beans_to_columns([f], [{f.name: v} for v in lists])]
    want = enc.encode_batch(cols, n)
    w = src.want(path, side)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    elems = RowBatch(up(w.data), up(w.offs), w.count, enc._value_encoder(False).schema_hash)
    got = enc.implode(elems, up(w.lo), up(w.entry_valid), up(w.valid[:(w.E + 7) // 8]))
    assert got.nrows == n and got.schema_hash == enc.schema_hash
    assert_same(got.rows.cpu().numpy(), want.rows.cpu().numpy(), "implode = encode_batch: rows")
    assert_same(got.row_offsets.cpu().numpy(), want.row_offsets.cpu().numpy(), "implode = encode_batch")
    back = columns_to_beans([f], [column_to_host(c) for c in enc.decode_batch(got)], n)
    assert [b[f.name] for b in back] == lists
    coll = arr.implode(elems, up(w.lo), None, up(w.valid[:(w.E + 7) // 8]))
    assert coll.schema_hash == 0 and coll.nrows == n
    null = np.flatnonzero(~_bits(w.entry_valid, n))
    assert len(null) > 0
    sel = np.flatnonzero(_bits(w.entry_valid, n))
    vo = coll.row_offsets.cpu().numpy()
    # wrap takes the next VALUE for every present row: drop the empty arrays of the null rows first
    packed = arr.take(coll, torch.from_numpy(sel).to(dev))
    wrapped = enc.wrap(packed, torch.from_numpy(_bits(w.entry_valid, n)).to(dev))
    assert_same(wrapped.rows.cpu().numpy(), want.rows.cpu().numpy(), "wrap(collection implode) = encode")
    assert np.all(np.diff(vo)[null] == 8)
    enc.device_status()


# 2. long lists: the work follows the elements ---------------------------------------------------------------
def test_a_single_row_of_70000_elements(dev):
    src = source(dev, "huge", 1)
    for rows_form in (True, False):
        case = exploded_case(src, ("items",), "elements", rows_form)
        w = case.run(f"70000 elements in one row, rows form {rows_form}")
        assert not w.bad and case.E == 70000 and len(w.data) > 70000 * 32
    sel = expect_select(src.rows, src.offs, 1, src.fields, [1])
    assert_same(exploded_case(src, ("items",), "elements").want.data, sel.data, "= select")


def test_one_long_list_among_empty_rows(dev):
    src = source(dev, "long", 65)
    for _, path, side in TARGETS[:4]:
        case = exploded_case(src, path, side)
        w = case.run(f"4097 elements in row 21: {path[0]}", out_shift=8)
        assert not w.bad and case.E == 4097
        sizes = np.diff(w.offs)
        assert sizes[21] > 4097 * 8 and sizes.max() == sizes[21] and np.all(np.delete(sizes, 21) <= 24)


# 3. degenerate batches ----------------------------------------------------------------------------------------
def test_all_null_and_empty(dev):
    src = source(dev, "flat", 257)
    path, side = ("items",), "elements"
    base = exploded_case(src, path, side)
    n, E = base.n, base.E
    none = np.zeros((n + 7) // 8, np.uint8)
    c = Case(base.enc, base.values, base.vo, base.lo, n, none, base.lv, E)
    w = c.run("every row null")
    assert list(np.diff(w.offs)) == [16] * n and not w.bad
    c = Case(base.enc, base.values[:0], [0], base.lo, n, base.ev, np.zeros((E + 7) // 8, np.uint8), E)
    w = c.run("every element null, no values")
    cnt = np.diff(base.lo)[_bits(base.ev, n)]                  # header, bitmap and zero slots only
    assert not w.bad and len(w.data) == 16 * n + int(np.sum(8 + ((cnt + 63) // 64) * 8 + 8 * cnt))
    coll = targets(src, path, side)[1]
    for enc in (base.enc, coll):
        c = Case(enc, base.values[:0], [0], np.zeros(n + 1, np.int64), n, None, None, 0)
        w = c.run("num_elements == 0")
        assert not w.bad and list(np.diff(w.offs)) == [24 if enc is base.enc else 8] * n
        c = Case(enc, base.values, base.vo, [0], 0, None, base.lv, E)
        w = c.run("nrows == 0")
        assert list(w.offs) == [0] and len(w.data) == 0
    wr = extracted_case(src, ("items",))
    c = Case(wr.enc, wr.values, wr.vo, None, 0, None, None, 0)
    assert list(c.run("wrap: nrows == 0").offs) == [0]
    c = Case(wr.enc, wr.values[:0], [0], None, wr.n, None, np.zeros((wr.n + 7) // 8, np.uint8), wr.n)
    assert list(np.diff(c.run("wrap: every row null").offs)) == [16] * wr.n


def test_num_values_may_be_a_larger_element_capacity(dev):
    src = source(dev, "flat", 257)
    for _, path, side in TARGETS[:4]:
        clean = exploded_case(src, path, side)
        case = exploded_case(src, path, side, ecap=clean.E + 65)
        assert case.nv == clean.E + 65 > clean.nv and np.all(case.vo[-66:] == case.vo[-1])
        w = case.run(f"{path[0]}: num_values = elem_capacity")
        assert not w.bad
        assert_same(w.data, clean.want.data, "the same rows")


# 4. capacities, alignment, streams ------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_form", [True, False])
def test_capacities_and_the_measure_form(dev, rows_form):
    src = source(dev, "flat", 257)
    case = exploded_case(src, ("items",), "elements", rows_form)
    total = len(case.want.data)
    assert total > 32768
    for cap in (0, 8, 16, (total // 2) & ~7, total - 8, total, total + 64):
        case.run(f"out_capacity {cap} of {total}", cap=cap, out_shift=8 if cap % 16 else 0)
    case.run("the measure form", measure=True)
    wr = extracted_case(src, ("items",))
    total = len(wr.want.data)
    for cap in (8, (total // 2) & ~7, total - 8):
        wr.run(f"wrap: out_capacity {cap} of {total}", cap=cap)
    wr.run("wrap: the measure form", measure=True)


@pytest.mark.parametrize("n", [65, 4097])
def test_alignment(dev, n):
    src = source(dev, "flat", n)
    for name in ("items", "fx"):
        case = exploded_case(src, (name,), "elements")
        for src_shift, out_shift in ((0, 8), (8, 0), (8, 8)):
            case.run(f"{name} n={n} shifts {src_shift}/{out_shift}", src_shift=src_shift,
                     out_shift=out_shift)


def test_write_pass_rounds_and_end_words(dev):
    """tests.test_select.test_write_pass_rounds_and_end_words for implode_write (implode and wrap), which
    stages 512 rows a round: one present row of 24 bytes -- an empty list -- ahead of 2049 null rows of
    16, so the rows start at 8 mod 16, the second 16 KB span is three rounds and the 32,808 bytes are 8
    mod 16; capacities inside a row, on and off a multiple of 8.  (A list across several spans among
    short rows: test_one_long_list_among_empty_rows.)"""
    src = source(dev, "flat", 257)
    n = 2050
    first = np.zeros((n + 7) // 8, np.uint8)
    first[0] = 1
    empty_list = np.zeros(8, np.uint8)                         # [int64 numElements = 0]
    cases = {"implode": Case(targets(src, ("items",), "elements")[0], empty_list[:0], [0],
                             np.zeros(n + 1, np.int64), n, first, None, 0),
             "wrap": Case(extracted_case(src, ("items",)).enc, empty_list, [0, 8], None, n, None, first, n)}
    for name, case in cases.items():
        total = len(case.want.data)
        assert list(np.diff(case.want.offs)) == [24] + [16] * 2049 and total % 16 == 8
        for out_shift in (0, 8):
            for cap in (None, total - 24, total - 20):
                w = case.run(f"{name}: shift {out_shift} capacity {cap}", cap=cap, out_shift=out_shift)
                assert not w.bad


def test_on_a_side_stream_and_bound_twice(dev):
    src = source(dev, "nested", 257)
    s = torch.cuda.Stream(device=dev)
    case = exploded_case(src, ("outer", "items"), "elements")
    case.run("implode_into on a side stream", stream=s, out_shift=8)
    case.run("bind_implode called twice", bound=True, calls=2)
    case.run("bind_implode twice on a side stream", bound=True, calls=2, stream=s)
    wr = extracted_case(src, ("outer",))
    wr.run("wrap_into on a side stream", stream=s)
    wr.run("bind_wrap twice on a side stream", bound=True, calls=2, stream=s, out_shift=8)


# 5. malformed input -----------------------------------------------------------------------------------------------
def _base(dev, rows_form=True):
    return exploded_case(source(dev, "flat", 257), ("items",), "elements", rows_form)


def _rows_with_elements(case, k=4):
    """k rows that are present and hold at least two kept elements, spread over the batch."""
    from tests.test_implode_model import Elements
    el = Elements(case.vo, case.nv, case.lv, case.E, case.least)
    kept = el.cs[case.lo[1:]] - el.cs[case.lo[:-1]] >= 2 * case.least
    rows = np.flatnonzero(kept & _bits(case.ev, case.n))
    assert len(rows) >= 4 * k
    return [int(r) for r in rows[::len(rows) // k][:k]], el


def _edited(case, **kw) -> Case:
    a = dict(values=case.values, vo=case.vo, lo=case.lo, n=case.n, ev=case.ev, lv=case.lv, E=case.E)
    a.update(kw)
    return Case(case.enc, **a)


@pytest.mark.parametrize("rows_form", [True, False])
def test_malformed_list_offsets(dev, rows_form):
    base = _base(dev, rows_form)
    victims, _ = _rows_with_elements(base)
    lo = base.lo.copy()
    for r in victims:                                          # row r - 1 decreases, row r grows
        lo[r] -= 1 if r % 2 else -1
    lo[victims[0]] = lo[victims[0] + 1] + 3                    # row victims[0]: decreasing
    c = _edited(base, lo=lo)
    w = c.run("decreasing list_offsets", out_shift=8)
    assert victims[0] in w.bad
    lo = base.lo.copy()
    lo[victims[1] + 1] = base.E + 1                            # past num_elements: rows v and v + 1
    lo[victims[2]] = -8
    c = _edited(base, lo=lo)
    w = c.run("list_offsets outside [0, num_elements]")
    assert {victims[1], victims[2]} <= set(w.bad)              # (a neighbour fails too unless it is null)
    c = _edited(base, E=int(base.lo[victims[3]]))              # a smaller num_elements
    w = c.run("list_offsets past a smaller num_elements")
    assert w.bad[0] >= victims[3] - 1 and len(w.bad) > 1
    if rows_form:                                              # a null row with a broken range
        ev = base.ev.copy()
        r = victims[0]
        ev[r >> 3] &= ~(1 << (r & 7)) & 0xFF
        lo = base.lo.copy()
        lo[r] = lo[r + 1] + 3
        c = _edited(base, lo=lo, ev=ev)
        w = c.run("a null row with a decreasing range")
        assert w.bad == [r - 1] or w.bad == []                 # only its neighbour's range can fail
        c = _edited(base, ev=ev)
        w = c.run("a null row with a non-empty range")
        assert not w.bad and w.offs[r + 1] - w.offs[r] == 16
    base.run("the next call is clean")


@pytest.mark.parametrize("rows_form", [True, False])
def test_malformed_values(dev, rows_form):
    base = _base(dev, rows_form)
    victims, el = _rows_with_elements(base)
    firsts = [int(np.flatnonzero(el.kept[base.lo[r]:base.lo[r + 1]])[0] + base.lo[r]) for r in victims]
    rank = np.cumsum(_bits(base.lv, base.E)) - _bits(base.lv, base.E)
    vs = [int(rank[e]) for e in firsts]                        # the values those elements take
    vo = base.vo.copy()
    for v in vs:
        vo[v + 1] -= 4                                         # value v: size % 8 == 4; v + 1: start
    c = _edited(base, vo=vo)
    w = c.run("value sizes that are no multiple of 8", out_shift=8)
    assert w.bad == victims
    vo = base.vo.copy()
    for v in vs:
        vo[v + 1] = vo[v] + 16                                 # value v: 16 < 24; v + 1 grows
    c = _edited(base, vo=vo)
    w = c.run("value sizes below least")
    assert w.bad == victims
    vo = base.vo.copy()
    for v in vs:
        vo[v + 1] = vo[v] - 8                                  # decreasing
    vo[vs[-1] + 1] = vo[-1] + 64                               # and one end past VT
    c = _edited(base, vo=vo)
    w = c.run("decreasing value_offsets, an end past the total")
    assert set(victims) <= set(w.bad)
    vo = base.vo.copy()
    vo[vs[0]] = -8
    c = _edited(base, vo=vo)
    w = c.run("a negative value offset")
    assert victims[0] in w.bad
    nv = vs[2]                                                 # fewer values than valid bits
    c = _edited(base, vo=base.vo[:nv + 1].copy(), values=base.values[:base.vo[nv]])
    w = c.run("more valid bits than values")
    assert w.bad and w.bad[0] == victims[2]
    base.run("the next call is clean")
    wr = extracted_case(source(dev, "flat", 257), ("items",))
    vo = wr.vo.copy()
    vo[5] += 4
    vo[9] = vo[10] + 8
    c = Case(wr.enc, wr.values, vo, None, wr.n, None, wr.lv, wr.n)
    w = c.run("wrap: malformed value offsets")
    assert len(w.bad) >= 3
    c = Case(wr.enc, wr.values[:wr.vo[7]], wr.vo[:8].copy(), None, wr.n, None, wr.lv, wr.n)
    w = c.run("wrap: more valid bits than values")
    assert len(w.bad) > 1
    wr.run("wrap: the next call is clean")


# 6. end to end: explode, process the elements, put them back --------------------------------------------
def test_explode_update_and_put_back(dev):
    from fury_amd.beans import columns_to_beans
    from fury_amd.encoder import RowBatch, column_to_host
    from fury_amd.workloads import Column
    n = 257
    src = source(dev, "flat", n)
    enc = src.enc
    batch = RowBatch(torch.from_numpy(src.rows).to(dev), torch.from_numpy(src.offs).to(dev), n,
                     enc.schema_hash)
    elems, lo, ev, valid, par, ords = enc.explode(batch, "items")
    child = enc.element_encoder("items")
    new_a = (par * 1000 + ords.to(torch.int64)).to(torch.int32)
    child.update_fields(elems, ["a"], [Column(values=new_a)])
    enc2, out = enc.with_elements(batch, "items", elems, lo, ev, valid)
    assert enc2.schema_hash == enc.schema_hash and out.nrows == n
    got = columns_to_beans(src.fields, [column_to_host(c) for c in enc2.decode_batch(out)], n)
    want = []
    for i, b in enumerate(src.beans):
        b = dict(b)
        if b["items"] is not None:
            b["items"] = [None if e is None else dict(e, a=i * 1000 + j) for j, e in enumerate(b["items"])]
        want.append(b)
    assert got == want
    vals, vvalid = enc.extract(batch, "m")                     # and a nested value: out and back in
    enc3, same = enc.with_nested(batch, "m", vals, vvalid)
    assert enc3.schema_hash == enc.schema_hash
    assert_same(same.rows.cpu().numpy(), src.rows, "with_nested(extract) returns the rows")
    enc.device_status()
