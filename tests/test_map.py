"""Maps as key / value arrays and back on the GPU (fury_row_map_split / fury_row_map_join, RowEncoder /
MapEncoder.split* and join*, with_map): every output -- both offsets arrays, count, indices, validity
and both output buffers of split, out_offsets and the output buffer of join, each buffer with 4096 guard
bytes on each side -- equals the numpy model of tests/test_map_model.py; for rows a writer made the
results also equal the models of fury_row_select / fury_row_extract of the source rows.  The sources are
those of tests/test_explode.py.  Marked gpu."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.test_explode import _list, _Src, _upload, source  # noqa: E402
from tests.test_explode_abi import explode_fields  # noqa: E402
from tests.test_extract import FILL, GUARD, assert_same, levels_of  # noqa: E402
from tests.test_extract import expect as expect_extract  # noqa: E402
from tests.test_map_model import (EMPTY_MAP, expect_join, expect_split, locate_map,  # noqa: E402
                                  widths_of)
from tests.test_select_model import expect_select  # noqa: E402

COUNTS = [1, 63, 64, 65, 257, 4097]
SOURCES = [("flat", ("m",)), ("nested", ("outer", "m")), ("coll", None)]
IDS = ["m", "outer.m", "collection"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _field_at(fields, path):
    for name in path:
        node = fields[[f.name for f in fields].index(name)]
        fields = node.children
    return node


_CACHE: dict = {}


def map_source(dev, which, n) -> _Src:
    """The sources of tests/test_explode.py, a MAP collection batch (the maps of `flat`, extracted by
    the model) and `huge`: one single 70,000-entry map built the way test_explode's `huge` list is."""
    if which in ("flat", "nested", "long"):
        return source(dev, which, n)
    key = (which, n)
    if key not in _CACHE:
        if which == "coll":
            from fury_amd.encoder import Encoders
            src = source(dev, "flat", n)
            m = _field_at(src.fields, ("m",))
            ex = expect_extract(src.rows, src.offs, n, levels_of(src.fields, ("m",)))
            enc = Encoders.map_encoder(*m.children, device=dev, name="m")
            _CACHE[key] = _Src(dev, enc, ex.data, ex.offs[:ex.count + 1].copy(), ex.count, [m])
        else:
            assert which == "huge" and n == 1
            fields = [f for f in explode_fields() if f.name in ("id", "m")]
            _CACHE[key] = _Src.of_beans(dev, fields, [{"id": 0, "m": _list("m", 1, 70000)}])
    return _CACHE[key]


def spec_of(src, path):
    """(levels of the walk or None, slot widths of the two arrays): from the Field tree alone."""
    if path is None:
        return None, widths_of(src.fields[0])
    return levels_of(src.fields, path), widths_of(_field_at(src.fields, path))


def want_split(src, path, rows=None, offs=None):
    if rows is None and offs is None:
        key = (path, "split")
        if key not in src._want:
            src._want[key] = expect_split(src.rows, src.offs, src.n, *spec_of(src, path))
        return src._want[key]
    return expect_split(src.rows if rows is None else rows, src.offs if offs is None else offs, src.n,
                        *spec_of(src, path))


def check_status(enc, bad, counts, what, stream=None):
    """The call reported one of the model's rows (saying so when it can only be a counts mismatch), or
    nothing; the stream is clean afterwards."""
    from fury_amd.encoder import IndexOutOfBoundsException
    if bad:
        with pytest.raises(IndexOutOfBoundsException, match=f"row ({'|'.join(map(str, bad))}) ") as e:
            enc.device_status(stream)
        if set(bad) <= set(counts):
            assert "different element counts" in str(e.value), what
        if not counts:
            assert "different element counts" not in str(e.value), what
    enc.device_status(stream)


# -- one split call into guarded buffers, everything compared ---------------------------------------------
def check_split(src, path, what, kcap=None, vcap=None, kform="full", vform="full", out_shift=0,
                src_shift=0, stream=None, bound=False, calls=1, rows=None, offs=None, optional=True):
    """kform / vform: "full", "measure" (buffer None) or "skip" (buffer and offsets None)."""
    from fury_amd.encoder import RowEncoder
    dev, n = src.dev, src.n
    w = want_split(src, path, rows, offs)
    batch = _upload(src, src_shift, rows, offs)
    i64 = lambda k: torch.full((k,), -7, dtype=torch.int64, device=dev)   # noqa: E731
    u8 = lambda k: torch.full((k,), FILL, dtype=torch.uint8, device=dev)  # noqa: E731
    at = GUARD + out_shift
    sides = []
    for side, cap, form in ((w.keys, kcap, kform), (w.vals, vcap, vform)):
        cap = len(side.data) if cap is None else cap
        t = u8(GUARD + 16 + cap + GUARD)
        assert t.data_ptr() % 16 == 0
        sides.append((side, cap, form, t, i64(n + 2)))
    cnt, idx = i64(2), i64(n + 1)
    nvb = ((n + 31) // 32) * 4
    val = u8(nvb + 8)
    args = []
    for side, cap, form, t, oo in sides:
        args += [t[at:at + cap] if form == "full" else None, None if form == "skip" else oo[:n + 1]]
    args += [cnt[:1], idx[:n] if optional and n else None, val[:nvb] if optional and n else None]
    fns = ((src.enc.split_into, src.enc.bind_split) if path is None else
           (lambda *a, **k: RowEncoder.split_map_into(src.enc, batch, list(path), *a[1:], **k),
            lambda *a, **k: RowEncoder.bind_split_map(src.enc, batch, list(path), *a[1:], **k)))
    torch.cuda.synchronize()
    if bound:
        call = fns[1](batch, *args, stream=stream)
        for _ in range(calls):
            call()
    else:
        for _ in range(calls):
            fns[0](batch, *args, stream=stream)
    torch.cuda.synchronize()
    for name, (side, cap, form, t, oo) in zip(("keys", "values"), sides):
        keep = np.full(n + 2, -7, np.int64)
        assert_same(oo.cpu().numpy(), keep if form == "skip" else np.concatenate([side.offs, [-7]]),
                    f"{what}: {name} offsets")
        want = np.full(t.numel(), FILL, np.uint8)
        if form == "full":
            k = min(cap, len(side.data))
            want[at:at + k] = side.data[:k]
        assert_same(t.cpu().numpy(), want, f"{what}: {name} buffer")
    assert_same(cnt.cpu().numpy(), np.array([w.count, -7], np.int64), f"{what}: out_count")
    assert_same(idx.cpu().numpy(), np.concatenate([w.idx, [-7]]) if optional and n else
                np.full(n + 1, -7, np.int64), f"{what}: out_indices")
    want_val = np.full(nvb + 8, FILL, np.uint8)
    if optional and n:
        want_val[:nvb] = w.valid
    assert_same(val.cpu().numpy(), want_val, f"{what}: out_validity")
    check_status(src.enc, w.bad, w.bad_counts, what, stream)
    return w


# -- one join call into guarded buffers ---------------------------------------------------------------------
def _bitmap(dev, bits):
    """An Arrow bitmap on the device, padded to whole 32-bit words."""
    if bits is None:
        return None
    a = np.zeros((len(bits) + 3) // 4 * 4 + 4, np.uint8)
    a[:len(bits)] = bits
    return torch.from_numpy(a).to(dev)


class JoinCase:
    """One join: the inputs on the host, the model's expectation, and the run into guarded buffers."""

    def __init__(self, enc, keys, ko, vals, vo, validity, n):
        self.enc, self.n, self.validity = enc, n, validity
        self.keys, self.ko = np.asarray(keys, np.uint8), np.asarray(ko, np.int64)
        self.vals, self.vo = np.asarray(vals, np.uint8), np.asarray(vo, np.int64)
        assert len(self.ko) == len(self.vo)
        self.nv = len(self.ko) - 1
        self.rows_form = not enc.schema().collection
        self._want = None

    @property
    def want(self):
        if self._want is None:
            self._want = expect_join(self.keys, self.ko, self.vals, self.vo, self.nv, self.validity,
                                     self.n, self.rows_form)
        return self._want

    def run(self, what, cap=None, measure=False, out_shift=0, src_shift=0, stream=None, bound=False,
            calls=1):
        from fury_amd.encoder import RowBatch, RowEncoder
        dev, enc, n, w = self.enc.device, self.enc, self.n, self.want
        cap = len(w.data) if cap is None else cap
        batches = []
        for data, oo in ((self.keys, self.ko), (self.vals, self.vo)):
            t = torch.empty(len(data) + 16, dtype=torch.uint8, device=dev)
            assert t.data_ptr() % 16 == 0
            d = t[src_shift:src_shift + len(data)]
            d.copy_(torch.from_numpy(data))
            batches.append(RowBatch(d, torch.from_numpy(oo).to(dev), self.nv, 0))
        t = torch.full((GUARD + 16 + cap + GUARD,), FILL, dtype=torch.uint8, device=dev)
        assert t.data_ptr() % 16 == 0
        at = GUARD + out_shift
        ooffs = torch.full((n + 2,), -7, dtype=torch.int64, device=dev)
        out = None if measure else t[at:at + cap]
        if self.rows_form:
            fns = (enc.join_map_into, enc.bind_join_map)
            kw = dict(validity=_bitmap(dev, self.validity), nrows=n, stream=stream)
        else:                                                  # MapEncoder: n = the entries
            assert n == self.nv
            fns = (enc.join_into, enc.bind_join)
            kw = dict(stream=stream)
        args = (*batches, out, ooffs[:n + 1])
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
        check_status(enc, w.bad, w.bad_counts, what, stream)
        return w


_TARGETS: dict = {}


def targets(src, path):
    """(one-field row encoder, map encoder) of the map the arrays go back into."""
    from fury_amd.encoder import Encoders
    key = (id(src.enc), path)
    if key not in _TARGETS:
        m = src.fields[0] if path is None else _field_at(src.fields, path)
        _TARGETS[key] = (Encoders.bean([m], device=src.dev),
                         Encoders.map_encoder(*m.children, device=src.dev, name=m.name))
    return _TARGETS[key]


def joined_case(src, path, rows_form=True) -> JoinCase:
    """The join of the model's split of `src`: rows form over the source rows (path given), collection
    form over the entries."""
    w = want_split(src, path)
    enc = targets(src, path)[0 if rows_form else 1]
    c = w.count
    if rows_form:
        return JoinCase(enc, w.keys.data, w.keys.offs, w.vals.data, w.vals.offs, w.valid, src.n)
    return JoinCase(enc, w.keys.data, w.keys.offs[:c + 1], w.vals.data, w.vals.offs[:c + 1], None, c)


# 1. split and the round-trip identities, every source x row count ------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("which,path", SOURCES, ids=IDS)
def test_split_and_join_of_split(dev, which, path, n):
    src = map_source(dev, which, n)
    what = f"{which} n={n}"
    w = check_split(src, path, f"{what}: split")
    assert not w.bad
    if path is not None:
        assert 0 < w.count <= n and (n < 8 or w.count < n)     # null rows have no entry
        rows = joined_case(src, path).run(f"{what}: join, rows form")
        assert not rows.bad
        if len(path) == 1:                                     # = select {m} of the source rows
            k = [f.name for f in src.fields].index(path[0])
            sel = expect_select(src.rows, src.offs, n, src.fields, [k])
            assert_same(rows.data, sel.data, f"{what}: join(split) = select")
            assert_same(rows.offs, sel.offs, f"{what}: join(split) = select, offsets")
        ex = expect_extract(src.rows, src.offs, n, levels_of(src.fields, path))
        want_data, want_offs = ex.data, ex.offs[:ex.count + 1]
    else:
        want_data, want_offs = src.rows, src.offs              # the collection batch itself
    coll = joined_case(src, path, rows_form=False).run(f"{what}: join, collection form", out_shift=8)
    assert not coll.bad
    assert_same(coll.data, want_data, f"{what}: collection form = extract")
    assert_same(coll.offs, want_offs, f"{what}: collection form = extract, offsets")


def test_each_side_is_what_the_array_encoder_writes_and_explodes_alike(dev):
    """Through the allocating forms: each side of split = encode_batch, under that side's array
    encoder, of the map column's key / value child with the map's offsets; explode of the value batch =
    explode of the source."""
    from fury_amd.beans import beans_to_columns
    from fury_amd.encoder import RowBatch, column_to_device
    n = 257
    src = map_source(dev, "flat", n)
    enc = src.enc
    batch = RowBatch(torch.from_numpy(src.rows).to(dev), torch.from_numpy(src.offs).to(dev), n,
                     enc.schema_hash)
    keys, vals, idx, valid = enc.split_map(batch, "m")
    w = want_split(src, ("m",))
    assert keys.nrows == vals.nrows == w.count and keys.schema_hash == 0
    assert_same(idx.cpu().numpy(), w.kept, "split_map: indices")
    assert_same(valid.cpu().numpy(), w.valid[:(n + 7) // 8], "split_map: validity")
    maps = [b["m"] for b in src.beans if b["m"] is not None]
    for side, got, arr in ((0, keys, enc.key_array_encoder("m")), (1, vals, enc.value_array_encoder("m"))):
        f = arr.field()
        col = beans_to_columns([f], [{f.name: [kv[side] for kv in p]} for p in maps])[0]
        col.validity = None
        want = arr.encode_batch([column_to_device(col, dev)], len(maps))
        assert_same(got.rows.cpu().numpy(), want.rows.cpu().numpy(), f"side {side} = encode_batch")
        assert_same(got.row_offsets.cpu().numpy(), want.row_offsets.cpu().numpy(), f"side {side}: offsets")
    direct = enc.explode(batch, "m", "values")
    mine = enc.value_array_encoder("m").explode(vals)
    assert_same(mine[0].rows.cpu().numpy(), direct[0].rows.cpu().numpy(), "explode(split) = explode")
    assert_same(mine[0].row_offsets.cpu().numpy(), direct[0].row_offsets.cpu().numpy(), "its offsets")
    assert_same(mine[3].cpu().numpy(), direct[3].cpu().numpy(), "its element validity")
    assert_same(idx[mine[4]].cpu().numpy(), direct[4].cpu().numpy(), "its parents")
    back = enc.field_encoder("m").join_map(keys, vals, valid, n)
    sel = expect_select(src.rows, src.offs, n, src.fields, [2])
    assert_same(back.rows.cpu().numpy(), sel.data, "join_map(split_map) = select")
    me = targets(src, ("m",))[1]
    again = me.split(me.join(keys, vals))
    assert_same(again[0].rows.cpu().numpy(), keys.rows.cpu().numpy(), "MapEncoder.split(join): keys")
    assert_same(again[1].rows.cpu().numpy(), vals.rows.cpu().numpy(), "MapEncoder.split(join): values")
    enc.device_status()


# 2. long maps: the work follows the bytes -------------------------------------------------------------------
def test_a_single_map_of_70000_entries(dev):
    src = map_source(dev, "huge", 1)
    w = check_split(src, ("m",), "70000 entries in one row: split", out_shift=8)
    assert not w.bad and w.count == 1
    assert len(w.keys.data) > 70000 * 4 and len(w.vals.data) > 70000 * 32      # many 16 KB spans each
    for rows_form in (True, False):
        j = joined_case(src, ("m",), rows_form).run(f"70000 entries: join, rows form {rows_form}")
        assert not j.bad
    sel = expect_select(src.rows, src.offs, 1, src.fields, [1])
    assert_same(joined_case(src, ("m",)).want.data, sel.data, "= select")


def test_one_long_map_among_empty_rows(dev):
    src = map_source(dev, "long", 65)
    w = check_split(src, ("m",), "4097 entries in row 21: split", out_shift=8)
    assert not w.bad
    sizes = np.diff(w.vals.offs)[:w.count]
    at = int(np.flatnonzero(w.kept == 21)[0])
    assert sizes[at] > 4097 * 8 and np.all(np.delete(sizes, at) == 8)
    j = joined_case(src, ("m",)).run("4097 entries in row 21: join", out_shift=8)
    sizes = np.diff(j.offs)
    assert not j.bad and sizes.max() == sizes[21] and np.all(np.delete(sizes, 21) <= 40)


# 3. degenerate batches ----------------------------------------------------------------------------------------
def test_no_rows_all_null_and_no_entries(dev):
    src = map_source(dev, "flat", 257)
    base = joined_case(src, ("m",))
    none = np.zeros((src.n + 7) // 8, np.uint8)
    c = JoinCase(base.enc, base.keys[:0], [0], base.vals[:0], [0], none, src.n)
    assert list(np.diff(c.run("every row null, no entries").offs)) == [16] * src.n
    c = JoinCase(base.enc, base.keys, base.ko, base.vals, base.vo, None, 0)
    assert list(c.run("join: nrows == 0").offs) == [0]
    me = targets(src, ("m",))[1]
    c = JoinCase(me, base.keys[:0], [0], base.vals[:0], [0], None, 0)
    assert list(c.run("join, collection form: nrows == 0").offs) == [0]
    empty = _Src(dev, src.enc, src.rows[:0], src.offs[:1].copy(), 0, src.fields)
    w = check_split(empty, ("m",), "split: nrows == 0")
    assert w.count == 0 and list(w.keys.offs) == [0] and list(w.vals.offs) == [0]
    nulls = _Src.of_beans(dev, src.fields, [dict(b, m=None) for b in src.beans[:65]])
    w = check_split(nulls, ("m",), "split: every map null")
    assert w.count == 0 and not w.bad and np.all(w.idx == -1)


# 4. capacities, the measure form, a skipped side, alignment, streams -------------------------------------
def test_capacities_the_measure_form_and_a_skipped_side(dev):
    src = map_source(dev, "flat", 257)
    w = want_split(src, ("m",))
    kt, vt = len(w.keys.data), len(w.vals.data)
    assert kt > 16384 and vt > 32768
    # capacities that cut inside a header word's chunk, inside the key run and inside the value run
    for kcap, vcap in ((0, 0), (8, 8), (16, 24), ((kt // 2) & ~7, (vt // 2) & ~7), (kt - 8, vt - 8),
                       (kt + 64, vt + 64)):
        check_split(src, ("m",), f"capacities {kcap}/{vcap} of {kt}/{vt}", kcap=kcap, vcap=vcap,
                    out_shift=8 if kcap % 16 else 0)
    check_split(src, ("m",), "the measure form", kform="measure", vform="measure")
    check_split(src, ("m",), "keys measured, values written", kform="measure")
    check_split(src, ("m",), "keys skipped", kform="skip", out_shift=8)
    check_split(src, ("m",), "values skipped", vform="skip")
    check_split(src, ("m",), "values skipped, keys measured, no optional outputs", kform="measure",
                vform="skip", optional=False)
    for rows_form in (True, False):
        case = joined_case(src, ("m",), rows_form)
        total = len(case.want.data)
        w = case.want
        r = int(np.flatnonzero(np.diff(w.offs) > 256)[0])      # a row whose map has entries
        o = int(w.offs[r]) + (16 if rows_form else 0)          # its key-size word
        ksz = int.from_bytes(w.data[o:o + 8].tobytes(), "little")
        assert 32 < ksz < w.offs[r + 1] - o - 40
        # ... and cuts at the key-size word, inside the key run and inside the value run
        cuts = [0, 8, 16, 24, o, o + 8, o + 8 + ((ksz // 2) & ~7), o + 8 + ksz + 8,
                (total // 2) & ~7, total - 8, total, total + 64]
        for cap in cuts:
            case.run(f"join rows form {rows_form}: out_capacity {cap} of {total}", cap=cap,
                     out_shift=8 if cap % 16 else 0)
        case.run("join: the measure form", measure=True)


@pytest.mark.parametrize("n", [65, 4097])
def test_alignment(dev, n):
    for which, path in SOURCES[:2]:
        src = map_source(dev, which, n)
        for src_shift, out_shift in ((0, 8), (8, 0), (8, 8)):
            what = f"{which} n={n} shifts {src_shift}/{out_shift}"
            check_split(src, path, f"{what}: split", src_shift=src_shift, out_shift=out_shift)
            joined_case(src, path).run(f"{what}: join", src_shift=src_shift, out_shift=out_shift)
    coll = map_source(dev, "coll", n)
    joined_case(coll, None, rows_form=False).run(f"collection n={n}: join", src_shift=8)


def test_write_pass_rounds_and_end_words(dev):
    """tests.test_select.test_write_pass_rounds_and_end_words for map_join_write, which stages 512 rows a
    round: one present row of 40 bytes -- a map without entries -- ahead of 2049 null rows of 16, so the
    rows start at 8 mod 16, a 16 KB span is three rounds and the 32,824 bytes are 8 mod 16;
    capacities inside a row, on and off a multiple of 8.  (A map across several spans among short rows:
    test_one_long_map_among_empty_rows.)"""
    enc = targets(map_source(dev, "flat", 257), ("m",))[0]
    n = 2050
    first = np.zeros((n + 7) // 8, np.uint8)
    first[0] = 1
    no_entries = np.zeros(8, np.uint8)                         # [int64 numElements = 0]
    case = JoinCase(enc, no_entries, [0, 8], no_entries, [0, 8], first, n)
    total = len(case.want.data)
    assert list(np.diff(case.want.offs)) == [40] + [16] * 2049 and total % 16 == 8
    for out_shift in (0, 8):
        for cap in (None, total - 24, total - 20):
            w = case.run(f"shift {out_shift} capacity {cap}", cap=cap, out_shift=out_shift)
            assert not w.bad


def test_on_a_side_stream_and_bound_twice(dev):
    s = torch.cuda.Stream(device=dev)
    for which, path in SOURCES:
        src = map_source(dev, which, 257)
        check_split(src, path, f"{which}: split on a side stream", stream=s, out_shift=8)
        check_split(src, path, f"{which}: bound split called twice", bound=True, calls=2)
        check_split(src, path, f"{which}: bound split twice on a side stream", bound=True, calls=2,
                    stream=s)
        for rows_form in ((True, False) if path is not None else (False,)):
            case = joined_case(src, path, rows_form)
            case.run(f"{which}: join on a side stream", stream=s, out_shift=8)
            case.run(f"{which}: bound join called twice", bound=True, calls=2)
            case.run(f"{which}: bound join twice on a side stream", bound=True, calls=2, stream=s)


# 5. malformed input -----------------------------------------------------------------------------------------------
def _put(rows, pos, value):
    rows[pos:pos + 8] = np.frombuffer(int(value).to_bytes(8, "little", signed=True), np.uint8)


def _victims(src, path, k=6):
    """k rows, spread over the batch, whose map has at least two entries, with (K, kb, A, asz) each."""
    spec = spec_of(src, path)
    found = []
    for r in range(src.n):
        res = locate_map(src.rows, src.offs, src.n, r, *spec)
        if res[0] == "map" and int.from_bytes(src.rows[res[1]:res[1] + 8].tobytes(), "little") >= 2:
            found.append((r,) + res[1:])
    assert len(found) >= 4 * k
    return found[::len(found) // k][:k]


def _neighbours_intact(src, path, w, victims):
    """Every entry of a row that is no victim is what the clean split has."""
    clean = want_split(src, path)
    bad = {v[0] for v in victims}
    assert list(w.kept) == [r for r in clean.kept if r not in bad]
    for side, ref in ((w.keys, clean.keys), (w.vals, clean.vals)):
        mine = {int(r): side.data[side.offs[j]:side.offs[j + 1]].tobytes() for j, r in enumerate(w.kept)}
        for j, r in enumerate(clean.kept):
            if int(r) not in bad:
                assert mine[int(r)] == ref.data[ref.offs[j]:ref.offs[j + 1]].tobytes(), r


@pytest.mark.parametrize("which,path", SOURCES, ids=IDS)
def test_malformed_maps(dev, which, path):
    src = map_source(dev, which, 257)
    victims = _victims(src, path)
    rows = src.rows.copy()
    (r0, K0, kb0, A0, z0), (r1, K1, kb1, A1, z1), (r2, K2, kb2, A2, z2) = victims[:3]
    _put(rows, K0 - 8, -8)                                     # kb negative
    _put(rows, K1 - 8, kb1 + 4)                                # kb odd
    _put(rows, K2 - 8, kb2 + z2 + 8)                           # kb past size
    w = check_split(src, path, "kb negative, odd, past size", rows=rows, out_shift=8)
    assert w.bad == [r0, r1, r2] and not w.bad_counts
    _neighbours_intact(src, path, w, victims[:3])
    rows = src.rows.copy()
    _put(rows, K0 - 8, 0)                                      # a key array shorter than 8 bytes
    _put(rows, K1 - 8, kb1 + z1)                               # a value array shorter than 8 bytes
    w = check_split(src, path, "an array shorter than 8 bytes", rows=rows)
    assert w.bad == [r0, r1] and not w.bad_counts
    _neighbours_intact(src, path, w, victims[:2])
    rows = src.rows.copy()
    for r, K, kb, A, z in victims:                             # n_k != n_v, on either side
        nk = int.from_bytes(rows[K:K + 8].tobytes(), "little")
        _put(rows, K if r % 2 else A, nk - 1)
    w = check_split(src, path, "n_k != n_v", rows=rows, out_shift=8)
    assert w.bad == [v[0] for v in victims] and w.bad_counts == w.bad
    _neighbours_intact(src, path, w, victims)
    rows = src.rows.copy()
    for (r, K, kb, A, z), grow in zip(victims[:4], (1 << 20, 1 << 20, 1, -1)):
        nk = int.from_bytes(rows[K:K + 8].tobytes(), "little")
        n2 = -5 if grow < 0 else max(nk + grow, (z - 8) // 8 + 1)      # both headers: the counts stay equal
        _put(rows, K, n2)
        _put(rows, A, n2)
    w = check_split(src, path, "a header longer than its array, a negative count", rows=rows)
    assert w.bad == [v[0] for v in victims[:4]] and not w.bad_counts
    _neighbours_intact(src, path, w, victims[:4])
    check_split(src, path, "the next call is clean")


def test_a_misaligned_row_start(dev):
    for which, path in SOURCES[::2]:
        src = map_source(dev, which, 257)
        victims = _victims(src, path, 2)
        offs = src.offs.copy()
        for v in victims:
            offs[v[0]] += 4
        w = check_split(src, path, f"{which}: misaligned row starts", offs=offs)
        bad = {v[0] for v in victims}
        assert bad <= set(w.bad) and not w.bad_counts
        if path is not None:                                   # (a collection entry ends where the next starts)
            assert set(w.bad) == bad
            _neighbours_intact(src, path, w, victims)
        check_split(src, path, f"{which}: the next call is clean")


@pytest.mark.parametrize("rows_form", [True, False])
def test_malformed_join_offsets_and_counts(dev, rows_form):
    src = map_source(dev, "flat", 257)
    base = joined_case(src, ("m",), rows_form)

    def edited(**kw):
        a = dict(keys=base.keys, ko=base.ko, vals=base.vals, vo=base.vo, validity=base.validity, n=base.n)
        a.update(kw)
        return JoinCase(base.enc, **a)
    present = (np.unpackbits(base.validity, bitorder="little")[:base.n].astype(bool) if rows_form
               else np.ones(base.n, bool))
    row_of = np.flatnonzero(present)                           # entry v goes to row row_of[v]
    big = np.flatnonzero(np.diff(base.ko[:len(row_of) + 1]) > 16)      # entries with keys
    vs = [int(v) for v in big[::len(big) // 4][:4]]
    ko = base.ko.copy()
    ko[vs[0] + 1] = ko[vs[0]] - 8                              # decreasing
    ko[vs[1] + 1] += 4                                         # unaligned: entries v and v + 1
    w = edited(ko=ko).run("key offsets that decrease and are unaligned", out_shift=8)
    assert {int(row_of[vs[0]]), int(row_of[vs[1]]), int(row_of[vs[1] + 1])} <= set(w.bad)
    for r in (int(row_of[vs[2]]), int(row_of[vs[3]])):         # untouched rows are what they were
        assert_same(w.data[w.offs[r]:w.offs[r + 1]], base.want.data[base.want.offs[r]:base.want.offs[r + 1]],
                    f"row {r} is intact")
    vo = base.vo.copy()
    vo[vs[2] + 1] = vo[-1] + 64                                # past the total
    vo[vs[3]] = -8
    w = edited(vo=vo).run("value offsets past the total and negative")
    assert {int(row_of[vs[2]]), int(row_of[vs[3]])} <= set(w.bad)
    failed = w.data[w.offs[row_of[vs[2]]]:w.offs[row_of[vs[2]] + 1]].tobytes()
    assert failed == ((1).to_bytes(8, "little") + bytes(8) if rows_form else EMPTY_MAP)
    keys = base.keys.copy()
    for v in vs:                                               # n_k != n_v
        _put(keys, base.ko[v], int.from_bytes(keys[base.ko[v]:base.ko[v] + 8].tobytes(), "little") + 1)
    w = edited(keys=keys).run("n_k != n_v", out_shift=8)
    assert w.bad == [int(row_of[v]) for v in vs] and w.bad_counts == w.bad
    keys, vals = base.keys.copy(), base.vals.copy()
    _put(keys, base.ko[vs[0]], (2**31 - 15) // 8 + 1)          # equal counts past the array limit
    _put(vals, base.vo[vs[0]], (2**31 - 15) // 8 + 1)
    _put(keys, base.ko[vs[1]], -1)
    _put(vals, base.vo[vs[1]], -1)
    w = edited(keys=keys, vals=vals).run("counts outside [0, (INT32_MAX - 15) / 8]")
    assert w.bad == [int(row_of[vs[0]]), int(row_of[vs[1]])] and not w.bad_counts
    if rows_form:                                              # num_values below the bitmap's popcount
        nv = vs[2]
        c = edited(ko=base.ko[:nv + 1].copy(), vo=base.vo[:nv + 1].copy(), keys=base.keys[:base.ko[nv]],
                   vals=base.vals[:base.vo[nv]])
        w = c.run("more valid bits than entries")
        assert w.bad == [int(r) for r in row_of[nv:]] and len(w.bad) > 8
        for r in w.bad[:4]:
            assert w.offs[r + 1] - w.offs[r] == 16
    base.run("the next call is clean")


def test_validity_patterns_at_word_edges(dev):
    """The first and the last set bit at bits 31 / 32 and 63 / 64: ranks across 32-bit words and
    64-row tiles."""
    src = map_source(dev, "flat", 257)
    base = joined_case(src, ("m",))
    n = 129
    for first, last, dense in ((31, 32, False), (32, 63, False), (63, 64, False), (31, 64, False),
                               (31, 64, True), (0, 128, True)):
        bits = np.zeros(((n + 31) // 32) * 32, bool)
        bits[[first, last]] = True
        if dense:
            bits[first:last + 1] = True
        nv = int(bits.sum())
        c = JoinCase(base.enc, base.keys[:base.ko[nv]], base.ko[:nv + 1].copy(),
                     base.vals[:base.vo[nv]], base.vo[:nv + 1].copy(),
                     np.packbits(bits, bitorder="little")[:(n + 7) // 8], n)
        w = c.run(f"set bits {first} .. {last}, dense {dense}")
        sizes = np.diff(w.offs)
        assert not w.bad and list(np.flatnonzero(sizes > 16)) == list(np.flatnonzero(bits))
        r = last                                               # the last present row takes the last entry
        assert w.data[w.offs[r] + 24:w.offs[r + 1]].tobytes() == (
            base.keys[base.ko[nv - 1]:base.ko[nv]].tobytes() + base.vals[base.vo[nv - 1]:base.vo[nv]].tobytes())


# 6. the use itself: re-key a map on the device ------------------------------------------------------------------
def test_rekey_a_map_and_put_it_back(dev):
    """Keys re-encoded through the ArrayEncoder with every key + 1, joined with the untouched value
    batch and zipped back by with_map = encode_batch of the modified beans, byte for byte."""
    from fury_amd.beans import beans_to_columns
    from fury_amd.encoder import RowBatch, column_to_device
    n = 257
    src = map_source(dev, "flat", n)
    enc = src.enc
    batch = RowBatch(torch.from_numpy(src.rows).to(dev), torch.from_numpy(src.offs).to(dev), n,
                     enc.schema_hash)
    keys, vals, idx, valid = enc.split_map(batch, "m")
    karr = enc.key_array_encoder("m")
    cols = karr.decode_batch(keys)
    cols[0].validity = None
    cols[0].child[0].values.view(torch.int32).add_(1)          # (decoded values are a byte buffer)
    keys2 = karr.encode_batch(cols, keys.nrows)
    assert_same(keys2.row_offsets.cpu().numpy(), keys.row_offsets.cpu().numpy(), "re-encoded key offsets")
    enc2, out = enc.with_map(batch, "m", keys2, vals, valid)
    assert enc2.schema_hash == enc.schema_hash and out.nrows == n
    beans = [dict(b, m=None if b["m"] is None else [(k + 1, v) for k, v in b["m"]]) for b in src.beans]
    want = enc.encode_batch([column_to_device(c, dev) for c in beans_to_columns(src.fields, beans)], n)
    assert_same(out.rows.cpu().numpy(), want.rows.cpu().numpy(), "with_map = encode_batch: rows")
    assert_same(out.row_offsets.cpu().numpy(), want.row_offsets.cpu().numpy(), "with_map: offsets")
    _, same = enc.with_map(batch, "m", keys, vals, valid)      # untouched: the rows again
    assert_same(same.rows.cpu().numpy(), src.rows, "with_map(split_map) returns the rows")
    enc.device_status()
