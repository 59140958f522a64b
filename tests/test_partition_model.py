"""A numpy model of fury_row_partition / fury_row_concat, written from the rules of include/
fury_row.h alone -- bytes, offsets with the repeated tail, part rows, indices, positions and the list
of rows that fail the extent rule -- and pinned here, without a GPU, on oracle-encoded batches:
against `expect` of tests/test_take.py on the stable argsort of the kept ids, against a filter model
for num_parts == 1, positions against indices, concat of the slices against the whole, and on
malformed offsets.  The GPU tests (tests/test_partition.py) compare the kernels with this model."""
from __future__ import annotations

import numpy as np
import pytest

from fury_amd import types as T
from fury_amd.workloads import SCHEMAS, gen_columns
from oracle import oracle as O
from tests.test_take import expect

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def _row(rows, offs, n, i, fixed_size):
    """The bytes of source row i, or None when its extent fails the rule of fury_row_take."""
    if fixed_size is not None:
        return rows[i * fixed_size:(i + 1) * fixed_size]
    total = int(offs[n])
    b, e = int(offs[i]), int(offs[i + 1])
    if b < 0 or e < b or e > total or b % 8 or e % 8:
        return None
    return rows[b:e]


def partition_model(rows, offs, n, ids, num_parts, fixed_size=None):
    """What fury_row_partition writes: (data, out_offsets[n + 1], part_rows[num_parts + 1],
    out_indices[n], out_positions[n], bad) with bad = the kept SOURCE rows of 0 bytes, in output
    order.  fixed_size: the rows of an is_fixed schema (offs is not used)."""
    ids = [int(x) for x in ids]
    assert len(ids) == n and 1 <= num_parts <= 65535
    kept = [i for i in range(n) if 0 <= ids[i] < num_parts]
    kept.sort(key=lambda i: (ids[i], i))              # by (partition id, source row number)
    count = len(kept)
    part_rows = np.zeros(num_parts + 1, np.int64)
    for i in kept:                                     # part_rows[p] = kept rows with id < p
        part_rows[ids[i] + 1] += 1
    part_rows = np.cumsum(part_rows)
    parts, bad = [], []
    out_offsets = np.zeros(n + 1, np.int64)
    indices = np.full(n, -1, np.int64)
    positions = np.full(n, -1, np.int64)
    for j, i in enumerate(kept):
        r = _row(rows, offs, n, i, fixed_size)
        if r is None:
            bad.append(i)
            r = rows[:0]
        parts.append(r)
        out_offsets[j + 1] = out_offsets[j] + len(r)
        indices[j] = i
        positions[i] = j
    out_offsets[count + 1:] = out_offsets[count]
    data = np.concatenate(parts).astype(np.uint8) if parts else np.zeros(0, np.uint8)
    return data, out_offsets, part_rows, indices, positions, bad


def concat_model(sources, fixed_size=None):
    """What fury_row_concat writes: (data, out_offsets[N + 1], bad output positions).  sources:
    (rows, offs, nrows) per source; a row is checked against its own source's [0, offs[nrows])."""
    parts, bad = [], []
    for rows, offs, n in sources:
        for i in range(n):
            r = _row(rows, offs, n, i, fixed_size)
            if r is None:
                bad.append(len(parts))
                r = rows[:0]
            parts.append(r)
    out_offsets = np.zeros(len(parts) + 1, np.int64)
    np.cumsum(np.asarray([len(p) for p in parts], np.int64), out=out_offsets[1:])
    data = np.concatenate(parts).astype(np.uint8) if parts else np.zeros(0, np.uint8)
    return data, out_offsets, bad


def filter_model(rows, offs, n, mask, fixed_size=None):
    """fury_row_filter by its own header rule: (data, out_offsets[n + 1], count, out_indices[n])."""
    sel = [i for i in range(n) if mask[i]]
    data, eoffs, _ = expect(rows, offs, n, sel, fixed_size)
    out_offsets = np.concatenate([eoffs, np.full(n - len(sel), eoffs[-1], np.int64)])
    indices = np.concatenate([np.asarray(sel, np.int64), np.full(n - len(sel), -1, np.int64)])
    return data, out_offsets, len(sel), indices


def model_slices(model):
    """The partitions of a partition_model result as concat sources with rebased offsets."""
    data, offs, part_rows = model[0], model[1], model[2]
    out = []
    for p in range(len(part_rows) - 1):
        a, b = int(part_rows[p]), int(part_rows[p + 1])
        o = offs[a:b + 1]
        out.append((data[int(o[0]):int(o[-1])], o - o[0], b - a))
    return out


def id_shapes(n, num_parts, seed):
    """The id patterns the ranking has to survive, by name."""
    rng = np.random.default_rng(seed)
    return {
        "uniform": rng.integers(-1, num_parts + 1, n),
        "last partition": np.full(n, num_parts - 1),
        "all dropped": np.full(n, num_parts),
        "descending": n - 1 - np.arange(n),             # strictly; ids >= num_parts drop
        "alternating": np.arange(n) % 2,
        "row number": np.arange(n) % 65535,
        "extremes": rng.choice(np.array([INT32_MIN, -1, 0, INT32_MAX]), n),
    }


# ---- oracle-encoded batches ---------------------------------------------------------------------
def _pair_fields():
    return [T.field("a", T.INT64), T.field("b", T.INT32)]


_CACHE: dict = {}


def oracle_batch(name, n):
    """(rows, offs, fixed_size or None) of n rows encoded by the oracle."""
    if (name, n) not in _CACHE:
        if name == "foo":
            from fury_amd.beans import beans_to_columns
            fields = SCHEMAS["foo"]
            host = beans_to_columns(fields, [
                {"f1": i, "f2": None if i % 3 == 0 else f"s{i}" * (i % 5),
                 "f3": [f"x{j}" for j in range(i % 4)],
                 "f4": [(f"k{j}", j) for j in range(i % 3)] if i % 5 else None,
                 "f5": None if i % 7 == 0 else {"f1": i, "f2": "b" * (i % 11)}} for i in range(n)])
        else:
            fields = _pair_fields() if name == "pair" else SCHEMAS[name]
            host = gen_columns(name if name != "pair" else None, fields, n, seed=3)
        rows, offs = O.encode(fields, host, n)
        rows = np.asarray(rows, np.uint8)
        fixed = 24 if name == "pair" else None
        if offs is None:
            offs = np.arange(n + 1, dtype=np.int64) * fixed
        offs = np.asarray(offs, np.int64)
        assert int(offs[n]) == len(rows)
        if fixed:
            assert np.array_equal(np.diff(offs), np.full(n, fixed))
        _CACHE[(name, n)] = (rows, offs, fixed)
    return _CACHE[(name, n)]


NAMES = ["mixed", "foo", "pair"]


@pytest.mark.parametrize("num_parts", [1, 2, 7, 256, 65535])
@pytest.mark.parametrize("name", NAMES)
def test_model_is_take_of_the_stable_argsort(name, num_parts):
    n = 300
    rows, offs, fixed = oracle_batch(name, n)
    for what, ids in id_shapes(n, num_parts, 11).items():
        ids = np.asarray(ids, np.int64)
        data, ooffs, part_rows, idx, pos, bad = partition_model(rows, offs, n, ids, num_parts, fixed)
        keep = np.flatnonzero((ids >= 0) & (ids < num_parts))
        order = keep[np.argsort(ids[keep], kind="stable")]
        count = len(order)
        want, woffs, wbad = expect(rows, offs, n, order, fixed)
        assert not bad and not wbad, what
        assert np.array_equal(data, want), what
        assert np.array_equal(ooffs[:count + 1], woffs) and (ooffs[count:] == woffs[-1]).all(), what
        assert np.array_equal(idx[:count], order) and (idx[count:] == -1).all(), what
        assert part_rows[0] == 0 and part_rows[-1] == count, what
        assert np.array_equal(part_rows, np.searchsorted(ids[order], np.arange(num_parts + 1))), what
        for p in {0, num_parts // 2, num_parts - 1}:       # a partition's rows are those of its id
            assert np.array_equal(idx[part_rows[p]:part_rows[p + 1]], np.flatnonzero(ids == p)), what


@pytest.mark.parametrize("name", NAMES)
def test_one_partition_is_filter(name):
    n = 257
    rows, offs, fixed = oracle_batch(name, n)
    rng = np.random.default_rng(4)
    for mask in (rng.random(n) < 0.5, np.zeros(n, bool), np.ones(n, bool), np.arange(n) % 2 == 1):
        data, ooffs, part_rows, idx, pos, _ = partition_model(rows, offs, n, mask.astype(np.int64) - 1,
                                                              1, fixed)
        fdata, foffs, count, fidx = filter_model(rows, offs, n, mask, fixed)
        assert np.array_equal(data, fdata) and np.array_equal(ooffs, foffs)
        assert part_rows.tolist() == [0, count] and np.array_equal(idx, fidx)


@pytest.mark.parametrize("name", NAMES)
def test_positions_invert_indices(name):
    n = 257
    rows, offs, fixed = oracle_batch(name, n)
    for num_parts in (1, 7, 300):
        ids = id_shapes(n, num_parts, 5)["uniform"]
        data, ooffs, part_rows, idx, pos, _ = partition_model(rows, offs, n, ids, num_parts, fixed)
        count = int(part_rows[-1])
        kept = np.flatnonzero(pos >= 0)
        assert len(kept) == count and sorted(pos[kept].tolist()) == list(range(count))
        assert np.array_equal(idx[pos[kept]], kept)
        assert np.array_equal(pos[idx[:count]], np.arange(count))
        assert ((ids[pos < 0] < 0) | (ids[pos < 0] >= num_parts)).all()
        # take of the partitioned batch at the positions of the kept rows restores source order
        back, boffs, _ = expect(data, ooffs, n, pos[kept], fixed)
        want, woffs, _ = expect(rows, offs, n, kept, fixed)
        assert np.array_equal(back, want) and np.array_equal(boffs, woffs)


@pytest.mark.parametrize("name", NAMES)
def test_concat_of_the_slices_is_the_whole(name):
    n = 257
    rows, offs, fixed = oracle_batch(name, n)
    for num_parts in (1, 3, 32):
        ids = id_shapes(n, num_parts, 6)["uniform"]
        m = partition_model(rows, offs, n, ids, num_parts, fixed)
        count = int(m[2][-1])
        data, coffs, bad = concat_model(model_slices(m), fixed)
        assert not bad and np.array_equal(data, m[0]) and np.array_equal(coffs, m[1][:count + 1])
    # one source = take with arange; a source given as an interior slice, offsets as they are
    data, coffs, bad = concat_model([(rows, offs, n)], fixed)
    want, woffs, _ = expect(rows, offs, n, np.arange(n), fixed)
    assert not bad and np.array_equal(data, want) and np.array_equal(coffs, woffs)
    if fixed is None:
        cut = int(offs[100])
        data, coffs, bad = concat_model([(rows[:cut], offs[60:101], 40), (rows, offs, 0),
                                         (rows, offs[:11], 10)])
        want, woffs, _ = expect(rows, offs, n, list(range(60, 100)) + list(range(10)))
        assert not bad and np.array_equal(data, want) and np.array_equal(coffs, woffs)


def malformed(offs, n):
    """Offsets with one bad row per kind, and the rows that fail: an entry past the total (the rows
    on both sides of it), a decreasing pair (a negative size), an unaligned entry (both sides)."""
    total = int(offs[n])
    bad = offs.copy()
    bad[100] = total + 64
    bad[201], bad[202] = bad[202], bad[201]
    bad[150] += 4
    assert bad[202] < bad[201]
    return bad, [99, 100, 149, 150, 201]


def test_malformed_offsets_give_empty_rows_at_the_right_positions():
    n = 257
    rows, offs, _ = oracle_batch("mixed", n)
    boffs, failing = malformed(offs, n)
    ids = np.arange(n) % 3
    ids[149] = -1                                       # a dropped row's extent is never examined
    ids[100] = 3
    data, ooffs, part_rows, idx, pos, bad = partition_model(rows, boffs, n, ids, 3)
    assert sorted(bad) == [99, 150, 201]
    assert bad == sorted(bad, key=lambda i: (ids[i], i))
    for i in bad:
        assert ooffs[pos[i] + 1] == ooffs[pos[i]]        # 0 bytes, and it keeps its position
    good = [i for i in range(n) if pos[i] >= 0 and i not in bad]
    for i in good[::17]:
        assert np.array_equal(data[ooffs[pos[i]]:ooffs[pos[i] + 1]], rows[boffs[i]:boffs[i + 1]])
    assert ooffs[int(part_rows[-1])] == sum(int(boffs[i + 1] - boffs[i]) for i in good)
    # concat: positions, not source rows; each row against its own source
    data, coffs, cbad = concat_model([(rows, offs, 5), (rows, boffs, n), (rows, offs, 2)])
    assert cbad == [5 + i for i in failing]
    assert len(coffs) == 5 + n + 2 + 1 and coffs[-1] == len(data)
