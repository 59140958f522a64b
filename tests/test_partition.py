"""Partition and concat on the GPU (fury_row_partition / fury_row_concat and their RowEncoder
surface).  Every comparison covers the whole output buffer with 4096 guard bytes on each side, and
every output array in full plus one guard entry, against the numpy model of
tests/test_partition_model.py, which is written from the header's rules alone.  Marked gpu."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from fury_amd.workloads import SCHEMAS  # noqa: E402
from tests.helpers import assert_columns_equal  # noqa: E402
from tests.test_partition_model import (concat_model, id_shapes, model_slices,  # noqa: E402
                                        partition_model)
from tests.test_take import (COUNTS, FILL, _device_src, _filled, _index_columns,  # noqa: E402
                             _out_buffer, _pack, assert_same, expect, source)

SENTINEL = -7
PARTS = [1, 2, 7, 255, 256, 257, 65535]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _guarded(dev, n):
    """An int64 array of n entries followed by one guard entry: (whole tensor, the n entries)."""
    t = torch.full((n + 1,), SENTINEL, dtype=torch.int64, device=dev)
    return t, t[:n]


def _with_guard(a):
    return np.concatenate([np.asarray(a, np.int64), [SENTINEL]])


def _fs(src):
    return src.enc.schema().fixed_size if src.fixed else None


def run_partition(src, ids, num_parts, what, cap=None, src_shift=0, out_shift=0, measure=False,
                  optional=True, stream=None, bound=False, offs=None, with_offsets=True,
                  model=None):
    """One partition_into call into guarded buffers, compared in full with the model.  Returns
    (model, the buffers as numpy arrays)."""
    dev, n = src.dev, src.n
    ids = np.asarray(ids, np.int64)
    if model is None:
        model = partition_model(src.rows, src.offs if offs is None else offs, n, ids, num_parts,
                                _fs(src))
    data, eoffs, eparts, eidx, epos, _ = model
    if cap is None:
        cap = n * _fs(src) if src.fixed else len(data)      # fixed: the host cannot know the count
    batch = _device_src(src, src_shift, offs)
    t, out, at = _out_buffer(dev, cap, out_shift)
    tids = torch.from_numpy(ids.astype(np.int32)).to(dev)
    toffs, ooffs = _guarded(dev, n + 1) if with_offsets else (None, None)
    tparts, oparts = _guarded(dev, num_parts + 1)
    tidx, oidx = _guarded(dev, n) if optional else (None, None)
    tpos, opos = _guarded(dev, n) if optional else (None, None)
    torch.cuda.synchronize()
    args = (batch, tids, num_parts, None if measure else out, ooffs, oparts, oidx, opos)
    if bound:
        src.enc.bind_partition(*args, stream=stream)()
    else:
        src.enc.partition_into(*args, stream=stream)
    torch.cuda.synchronize()
    got = {"rows": t.cpu().numpy(), "parts": tparts.cpu().numpy()}
    assert_same(got["parts"], _with_guard(eparts), f"{what}: out_part_rows")
    if with_offsets:
        got["offs"] = toffs.cpu().numpy()
        assert_same(got["offs"], _with_guard(eoffs), f"{what}: out_offsets")
    if optional:
        got["idx"], got["pos"] = tidx.cpu().numpy(), tpos.cpu().numpy()
        assert_same(got["idx"], _with_guard(eidx), f"{what}: out_indices")
        assert_same(got["pos"], _with_guard(epos), f"{what}: out_positions")
    want = np.full(t.numel(), FILL, np.uint8) if measure else _filled(t.numel(), at, data, cap)
    assert_same(got["rows"], want, f"{what}: output buffer")
    return model, got


# 1. every schema shape x row count x partition count -----------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("name", ["pair", "struct100", "mixed", "foo", "array"])
def test_partition_matrix(dev, name, n):
    src = source(dev, name, n)
    if name == "pair":
        assert src.enc.schema().fixed_size == 24 and src.fixed
    for num_parts in PARTS:
        ids = np.random.default_rng(1000 * num_parts + n).integers(-1, num_parts + 1, n)
        what = f"{name} n={n} parts={num_parts}"
        model, _ = run_partition(src, ids, num_parts, what)
        assert not model[5]
        run_partition(src, ids, num_parts, what + " without the optional outputs", optional=False,
                      model=model)
    if src.fixed:                                   # out_offsets is optional for fixed-width schemas
        run_partition(src, ids, num_parts, f"{name} n={n} no out_offsets", with_offsets=False,
                      model=model)
    src.enc.device_status()


# 2. shapes that break a ranking pass ------------------------------------------------------------------
@pytest.mark.parametrize("num_parts", [3, 65535])
@pytest.mark.parametrize("name,n", [("mixed", 4097), ("pair", 70_001)])
def test_partition_id_shapes(dev, name, n, num_parts):
    src = source(dev, name, n)
    shapes = id_shapes(n, num_parts, 7)
    shapes.pop("uniform")
    assert (np.diff(shapes["descending"]) < 0).all()
    assert set(np.unique(shapes["extremes"])) == {-2 ** 31, -1, 0, 2 ** 31 - 1}
    for what, ids in shapes.items():
        what = f"{name} n={n} parts={num_parts} ids {what}"
        model, first = run_partition(src, ids, num_parts, what)
        _, second = run_partition(src, ids, num_parts, what + " (second run)", model=model)
        for k in first:                              # two runs into fresh buffers: identical
            assert_same(second[k], first[k], f"{what}: {k} of the second run")
    count = int(partition_model(src.rows, src.offs, n, shapes["all dropped"], num_parts,
                                _fs(src))[2][-1])
    assert count == 0
    src.enc.device_status()


# 3. one partition is filter, byte for byte ------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "struct100"])
def test_one_partition_equals_filter(dev, name):
    n = 4097
    src = source(dev, name, n)
    fs = _fs(src)
    m = np.random.default_rng(12).random(n) < 0.5
    cap = n * fs if src.fixed else len(expect(src.rows, src.offs, n, np.flatnonzero(m), fs)[0])
    batch = _device_src(src, 0)
    t, out, at = _out_buffer(dev, cap, 8)
    toffs, ooffs = _guarded(dev, n + 1)
    tidx, oidx = _guarded(dev, n)
    cnt = torch.full((1,), SENTINEL, dtype=torch.int64, device=dev)
    src.enc.filter_into(batch, torch.from_numpy(_pack(m)).to(dev), out, ooffs, cnt, oidx)
    torch.cuda.synchronize()
    _, got = run_partition(src, m.astype(np.int64) - 1, 1, f"{name} as a filter", out_shift=8)
    assert_same(got["rows"], t.cpu().numpy(), "out_rows against fury_row_filter's")
    assert_same(got["offs"], toffs.cpu().numpy(), "out_offsets against fury_row_filter's")
    assert_same(got["idx"], tidx.cpu().numpy(), "out_indices against fury_row_filter's")
    assert got["parts"].tolist() == [0, int(cnt.item()), SENTINEL] and int(cnt.item()) == m.sum()
    src.enc.device_status()


# 4. out_positions is the inverse permutation -----------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "struct100"])
def test_positions_restore_source_order(dev, name):
    from fury_amd.encoder import RowBatch
    n = 4097
    src = source(dev, name, n)
    ids = np.random.default_rng(13).integers(-1, 8, n)
    kept = np.flatnonzero((ids >= 0) & (ids < 7))
    batch = _device_src(src, 0)
    total = n * _fs(src) if src.fixed else len(src.rows)
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    offs = None if src.fixed else torch.empty(n + 1, dtype=torch.int64, device=dev)
    parts = torch.empty(8, dtype=torch.int64, device=dev)
    pos = torch.empty(n, dtype=torch.int64, device=dev)
    src.enc.partition_into(batch, ids, 7, out, offs, parts, None, pos)
    count = int(parts[7].item())
    assert count == len(kept)
    parted = RowBatch(out, None if src.fixed else offs[:count + 1], count, src.enc.schema_hash)
    back = src.enc.take(parted, pos[torch.from_numpy(kept).to(dev)])
    want = src.enc.take(batch, kept)
    assert_same(back.rows.cpu().numpy(), want.rows.cpu().numpy(), "rows in source order")
    assert_same(back.rows.cpu().numpy(), expect(src.rows, src.offs, n, kept, _fs(src))[0],
                "rows against the source bytes")
    if not src.fixed:
        assert_same(back.row_offsets.cpu().numpy(), want.row_offsets.cpu().numpy(), "offsets")


# 5. capacity, the measure form, alignment, streams --------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "foo"])
def test_partition_capacity_and_measure_form(dev, name):
    src = source(dev, name, 257)
    ids = np.random.default_rng(14).integers(-1, 8, src.n)
    model = partition_model(src.rows, src.offs, src.n, ids, 7)
    needed = len(model[0])
    assert needed > 4096
    for cap in (0, 8, needed - 8, needed):
        for out_shift in (0, 8):
            # bytes before the capacity are the full result's, bytes at or past it still hold the
            # fill, every array is complete: run_partition compares everything
            run_partition(src, ids, 7, f"{name} capacity {cap} of {needed}", cap=cap,
                          out_shift=out_shift, model=model)
    run_partition(src, ids, 7, f"{name} measure form", measure=True, model=model)
    run_partition(src, ids, 7, f"{name} measure form, no optional outputs", measure=True,
                  optional=False, model=model)
    src.enc.device_status()


def test_partition_fixed_schema_capacity(dev):
    from fury_amd.encoder import CapacityError
    src = source(dev, "struct100", 65)
    batch = _device_src(src, 0)
    out = torch.full((65 * 816 - 8,), FILL, dtype=torch.uint8, device=dev)
    parts = torch.full((4,), SENTINEL, dtype=torch.int64, device=dev)
    with pytest.raises(CapacityError, match="fury_row_partition"):
        src.enc.partition_into(batch, np.zeros(65, np.int32), 3, out, None, parts)
    torch.cuda.synchronize()
    assert bool((out == FILL).all()) and bool((parts == SENTINEL).all())
    ids = np.arange(65) % 4
    run_partition(src, ids, 3, "struct100 measure form", measure=True)
    run_partition(src, ids, 3, "struct100 measure form, nothing optional", measure=True,
                  optional=False, with_offsets=False)


@pytest.mark.parametrize("name", ["mixed", "pair", "struct100"])
def test_partition_alignment(dev, name):
    src = source(dev, name, 257)
    ids = np.random.default_rng(15).integers(-1, 4, src.n)
    model = partition_model(src.rows, src.offs, src.n, ids, 3, _fs(src))
    for src_shift, out_shift in ((8, 0), (0, 8), (8, 8)):
        run_partition(src, ids, 3, f"{name} shifts {src_shift}/{out_shift}", src_shift=src_shift,
                      out_shift=out_shift, model=model)
    src.enc.device_status()


@pytest.mark.parametrize("num_parts", [5, 300])
def test_partition_on_a_side_stream(dev, num_parts):
    src = source(dev, "mixed", 4097)
    ids = np.random.default_rng(16).integers(-1, num_parts + 1, src.n)
    s = torch.cuda.Stream(device=dev)
    model, plain = run_partition(src, ids, num_parts, "default stream")
    _, side = run_partition(src, ids, num_parts, "bind_partition on a side stream", stream=s,
                            bound=True, model=model)
    src.enc.device_status(s)
    for k in plain:
        assert_same(side[k], plain[k], f"side stream: {k}")


def test_partition_of_an_empty_batch(dev):
    from fury_amd.encoder import RowBatch
    for name in ("mixed", "struct100"):
        src = source(dev, name, 65)
        empty = RowBatch(torch.empty(0, dtype=torch.uint8, device=dev),
                         None if src.fixed else torch.zeros(1, dtype=torch.int64, device=dev), 0,
                         src.enc.schema_hash)
        for num_parts in (1, 300):
            t, out, at = _out_buffer(dev, 64, 0)
            toffs, ooffs = _guarded(dev, 1)
            tparts, oparts = _guarded(dev, num_parts + 1)
            src.enc.partition_into(empty, np.zeros(0, np.int32), num_parts, out, ooffs, oparts)
            torch.cuda.synchronize()
            assert toffs.tolist() == [0, SENTINEL]
            assert tparts.tolist() == [0] * (num_parts + 1) + [SENTINEL]
            assert bool((t == FILL).all())
        b, part_rows = src.enc.partition(empty, [], 4)
        assert b.nrows == 0 and b.rows.numel() == 0 and part_rows.tolist() == [0] * 5
        src.enc.device_status()


# 6. malformed source offsets: values the bounds rule rejects before any read ---------------------------
def test_partition_malformed_source_offsets(dev):
    from fury_amd.encoder import IndexOutOfBoundsException
    src = source(dev, "mixed", 257)
    n = src.n
    total = int(src.offs[n])
    base_ids = np.arange(n) % 5

    def case(entry, value, bad_row, drop):
        offs = src.offs.copy()
        if value is None:
            offs[entry], offs[entry + 1] = offs[entry + 1], offs[entry]
        else:
            offs[entry] = value
        ids = base_ids.copy()
        ids[drop] = -1                               # the other rows the entry spoils: dropped
        return offs, ids, bad_row

    cases = {"extent past the total": case(100, total + 64, 99, [100]),
             "unaligned start": case(150, int(src.offs[150]) + 4, 150, [149]),
             "negative size": case(201, None, 201, [])}
    src.enc.device_status()
    for what, (offs, ids, bad_row) in cases.items():
        for num_parts in (5, 300):
            model, _ = run_partition(src, ids, num_parts, what, offs=offs)
            assert model[5] == [bad_row]
            assert model[1][model[4][bad_row] + 1] == model[1][model[4][bad_row]]    # 0 bytes
            with pytest.raises(IndexOutOfBoundsException, match=f"row {bad_row} "):
                src.enc.device_status()
            src.enc.device_status()                  # raised once, then clear
            run_partition(src, base_ids, num_parts, "the next call is clean")
            src.enc.device_status()
        for dropping in (-1, 5):                     # the same bad row, dropped: nothing raised
            ids2 = ids.copy()
            ids2[bad_row] = dropping
            model, _ = run_partition(src, ids2, 5, what + ", dropped", offs=offs)
            assert not model[5]
            src.enc.device_status()


# 7. concat -----------------------------------------------------------------------------------------------
def _concat_sources(dev, name, counts, shifts=True):
    """(model sources, device batches) of one source per count; source k sits at 8 * (k % 2) mod 16."""
    from fury_amd.encoder import RowBatch
    msrc, batches = [], []
    enc = source(dev, name, 1).enc
    for k, c in enumerate(counts):
        if c == 0:
            msrc.append((np.zeros(0, np.uint8), np.zeros(1, np.int64), 0))
            # an empty source: rows may be NULL, and so may the offsets
            batches.append(RowBatch(None, None, 0, enc.schema_hash))
            continue
        s = source(dev, name, c)
        msrc.append((s.rows, s.offs, c))
        b = _device_src(s, 8 * (k % 2) if shifts else 0)
        batches.append(RowBatch(b.rows, b.row_offsets, c, enc.schema_hash))
    return enc, msrc, batches


def run_concat(enc, msrc, batches, what, cap=None, out_shift=0, measure=False, with_offsets=True,
               stream=None):
    dev = enc.device
    fs = enc.schema().fixed_size if enc.schema().is_fixed else None
    data, eoffs, bad = concat_model(msrc, fs)
    n = len(eoffs) - 1
    cap = len(data) if cap is None else cap
    t, out, at = _out_buffer(dev, cap, out_shift)
    toffs, ooffs = _guarded(dev, n + 1) if with_offsets else (None, None)
    torch.cuda.synchronize()
    enc.concat_into(batches, None if measure else out, ooffs, stream=stream)
    torch.cuda.synchronize()
    if with_offsets:
        assert_same(toffs.cpu().numpy(), _with_guard(eoffs), f"{what}: out_offsets")
    want = np.full(t.numel(), FILL, np.uint8) if measure else _filled(t.numel(), at, data, cap)
    assert_same(t.cpu().numpy(), want, f"{what}: output buffer")
    return data, eoffs, bad


CONCAT_COUNTS = {1: [[257], [1]], 2: [[63, 0], [0, 65]], 3: [[65, 0, 257], [1, 63, 0]],
                 32: [[(0, 1, 63, 65, 257)[(3 * k + 1) % 5] for k in range(32)]]}


@pytest.mark.parametrize("k", [1, 2, 3, 32])
@pytest.mark.parametrize("name", ["mixed", "foo", "struct100", "array"])
def test_concat_sources(dev, name, k):
    for counts in CONCAT_COUNTS[k]:
        assert len(counts) == k and (k == 1 or 0 in counts)
        enc, msrc, batches = _concat_sources(dev, name, counts)
        for out_shift in (0, 8):
            _, _, bad = run_concat(enc, msrc, batches, f"{name} {counts} shift {out_shift}",
                                   out_shift=out_shift)
            assert not bad
        if enc.schema().is_fixed:
            run_concat(enc, msrc, batches, f"{name} {counts} no out_offsets", with_offsets=False)
    enc.device_status()


def test_concat_of_one_source_is_take_with_arange(dev):
    for name in ("mixed", "struct100"):
        src = source(dev, name, 257)
        enc, msrc, batches = _concat_sources(dev, name, [257])
        data, eoffs, _ = run_concat(enc, msrc, batches, f"{name}: one source")
        want, woffs, _ = expect(src.rows, src.offs, 257, np.arange(257), _fs(src))
        assert_same(data, want, "bytes")
        assert_same(eoffs, woffs, "offsets")
        got = enc.take(batches[0], torch.arange(257, device=dev))
        assert_same(got.rows.cpu().numpy(), data, "take with arange")


def test_concat_interior_slices_and_aliased_sources(dev):
    from fury_amd.encoder import RowBatch
    src = source(dev, "mixed", 257)
    enc = src.enc
    whole = _device_src(src, 0)
    cut = int(src.offs[100])
    assert src.offs[60] != 0
    # rows [60, 100) with the offsets as they are (the source's bytes end at offs[100]), the whole
    # batch, the same slice again and the whole batch again: aliased sources
    inner = RowBatch(whole.rows[:cut], whole.row_offsets[60:101], 40, enc.schema_hash)
    msrc = [(src.rows[:cut], src.offs[60:101], 40), (src.rows, src.offs, 257)] * 2
    batches = [inner, whole] * 2
    data, eoffs, bad = run_concat(enc, msrc, batches, "interior slices, aliased", out_shift=8)
    order = (list(range(60, 100)) + list(range(257))) * 2
    want, woffs, _ = expect(src.rows, src.offs, 257, order)
    assert not bad
    assert_same(data, want, "bytes")
    assert_same(eoffs, woffs, "offsets")
    enc.device_status()


@pytest.mark.parametrize("name", ["mixed", "foo"])
def test_concat_capacity_and_measure_form(dev, name):
    enc, msrc, batches = _concat_sources(dev, name, [65, 0, 257, 63])
    needed = len(concat_model(msrc)[0])
    assert needed > 4096
    for cap in (0, 8, needed - 8, needed):
        for out_shift in (0, 8):
            run_concat(enc, msrc, batches, f"{name} capacity {cap} of {needed}", cap=cap,
                       out_shift=out_shift)
    run_concat(enc, msrc, batches, f"{name} measure form", measure=True)
    enc.device_status()


def test_concat_fixed_schema_capacity(dev):
    from fury_amd.encoder import CapacityError
    enc, msrc, batches = _concat_sources(dev, "struct100", [63, 0, 65])
    out = torch.full((128 * 816 - 8,), FILL, dtype=torch.uint8, device=dev)
    with pytest.raises(CapacityError, match="fury_row_concat"):
        enc.concat_into(batches, out)
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    run_concat(enc, msrc, batches, "struct100 measure form", measure=True)


def test_concat_malformed_row_names_its_output_position(dev):
    from fury_amd.encoder import IndexOutOfBoundsException
    src = source(dev, "mixed", 257)
    enc = src.enc
    offs = src.offs.copy()
    offs[201], offs[202] = offs[202], offs[201]       # row 201 of source 2: a negative size
    good = _device_src(src, 0)
    badb = _device_src(src, 8, offs)
    short = source(dev, "mixed", 65)
    msrc = [(short.rows, short.offs, 65), (src.rows, src.offs, 257), (src.rows, offs, 257)]
    batches = [_device_src(short, 0), good, badb]
    enc.device_status()
    _, _, bad = run_concat(enc, msrc, batches, "one malformed row in source 2")
    assert bad == [65 + 257 + 201]
    with pytest.raises(IndexOutOfBoundsException, match=f"row {65 + 257 + 201} "):
        enc.device_status()
    enc.device_status()
    run_concat(enc, msrc[:2], batches[:2], "the next call is clean")
    enc.device_status()


def test_concat_on_a_side_stream(dev):
    enc, msrc, batches = _concat_sources(dev, "mixed", [257, 65, 0, 63])
    s = torch.cuda.Stream(device=dev)
    run_concat(enc, msrc, batches, "side stream", stream=s, out_shift=8)
    enc.device_status(s)


# 8. partition -> slices -> concat, and the Python surface ---------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "struct100"])
def test_high_level_partition_slice_concat(dev, name):
    n = 4097
    src = source(dev, name, n)
    enc, fs = src.enc, _fs(src)
    batch = _device_src(src, 0)
    for num_parts in (6, 300):
        ids = np.random.default_rng(17).integers(-1, num_parts + 1, n)
        model = partition_model(src.rows, src.offs, n, ids, num_parts, fs)
        data, eoffs, eparts, eidx, _, _ = model
        count = int(eparts[-1])
        for given in (torch.from_numpy(ids).to(dev), ids.astype(np.int32), [int(i) for i in ids]):
            out, part_rows, kept = enc.partition(batch, given, num_parts, return_indices=True)
            assert out.nrows == count and out.schema_hash == enc.schema_hash
            assert_same(part_rows.cpu().numpy(), eparts, "partition: part_rows")
            assert_same(kept.cpu().numpy(), eidx[:count], "partition: indices")
            assert_same(out.rows.cpu().numpy(), data, "partition: rows")
            if fs is None:
                assert_same(out.row_offsets.cpu().numpy(), eoffs[:count + 1], "partition: offsets")
            else:
                assert out.row_offsets is None
        pr = part_rows.cpu().tolist()
        picks = range(num_parts) if num_parts <= 32 else range(100, 132)
        slices = [enc.slice_rows(out, pr[p], pr[p + 1]) for p in picks]
        mslices = model_slices(model)
        for p, s in zip(picks, slices):
            assert s.nrows == mslices[p][2]
            assert_same(s.rows.cpu().numpy(), mslices[p][0], f"slice {p}: rows")
            if fs is None:
                assert_same(s.row_offsets.cpu().numpy(), mslices[p][1], f"slice {p}: offsets")
            else:
                assert s.row_offsets is None
        glued = enc.concat(slices)
        a, b = pr[picks[0]], pr[picks[-1] + 1]
        lo, hi = (a * fs, b * fs) if fs else (int(eoffs[a]), int(eoffs[b]))
        assert glued.nrows == b - a
        assert_same(glued.rows.cpu().numpy(), data[lo:hi], "concat of the slices: rows")
        if fs is None:
            assert_same(glued.row_offsets.cpu().numpy(), eoffs[a:b + 1] - eoffs[a],
                        "concat of the slices: offsets")
    enc.device_status()


def test_concat_of_a_partition_decodes_to_the_reordered_columns(dev):
    from fury_amd.encoder import column_to_host
    n = 257
    src = source(dev, "mixed", n)
    enc = src.enc
    fields = SCHEMAS["mixed"]
    ids = np.random.default_rng(18).integers(-1, 5, n)
    out, part_rows, kept = enc.partition(_device_src(src, 0), ids, 4, return_indices=True)
    pr = part_rows.cpu().tolist()
    glued = enc.concat([enc.slice_rows(out, pr[p], pr[p + 1]) for p in range(4)])
    assert glued.nrows == out.nrows == pr[4]
    assert_same(glued.rows.cpu().numpy(), out.rows.cpu().numpy(), "round trip: rows")
    assert_same(glued.row_offsets.cpu().numpy(), out.row_offsets.cpu().numpy(), "round trip: offsets")
    got = [column_to_host(c) for c in enc.decode_batch(glued)]
    order = kept.cpu().numpy()
    assert_same(order, partition_model(src.rows, src.offs, n, ids, 4)[3][:pr[4]], "indices")
    assert_columns_equal(fields, got, _index_columns(fields, src.host, order, n), glued.nrows)


@pytest.mark.parametrize("name", ["mixed", "struct100"])
def test_shuffle_recipe_partition_frame_unframe_concat(dev, name):
    """INTEGRATION's recipe: partition by destination, frame each slice, unframe, concat -- with an
    empty partition among them -- returns the partitioned batch byte for byte."""
    n = 257
    src = source(dev, name, n)
    enc = src.enc
    ids = np.random.default_rng(19).integers(-1, 5, n)
    ids[ids == 2] = 3                                 # partition 2 is empty
    out, part_rows = enc.partition(_device_src(src, 0), ids, 5)
    pr = part_rows.cpu().tolist()
    assert pr[2] == pr[3] and pr[5] == int(((ids >= 0) & (ids < 5)).sum())
    frames = [enc.frame(enc.slice_rows(out, pr[w], pr[w + 1]))[0] for w in range(5)]
    counts = [pr[w + 1] - pr[w] for w in range(5)]
    glued = enc.concat([enc.unframe(f.clone(), c) for f, c in zip(frames, counts)])
    enc.device_status()
    assert glued.nrows == out.nrows
    assert_same(glued.rows.cpu().numpy(), out.rows.cpu().numpy(), "shuffle: rows")
    assert_same(glued.rows.cpu().numpy(), partition_model(src.rows, src.offs, n, ids, 5, _fs(src))[0],
                "shuffle: rows against the model")
    if not src.fixed:
        assert_same(glued.row_offsets.cpu().numpy(), out.row_offsets.cpu().numpy(), "shuffle: offsets")


def test_foreign_schema_hash(dev):
    from fury_amd.encoder import ClassNotCompatibleException, RowBatch
    src = source(dev, "mixed", 65)
    b = _device_src(src, 0)
    foreign = RowBatch(b.rows, b.row_offsets, b.nrows, b.schema_hash + 1)
    with pytest.raises(ClassNotCompatibleException, match="Schema is not consistent"):
        src.enc.partition(foreign, np.zeros(65, np.int32), 2)
    with pytest.raises(ClassNotCompatibleException, match="Schema is not consistent"):
        src.enc.concat([b, foreign])
