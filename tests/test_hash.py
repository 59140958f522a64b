"""Key hash on the GPU (fury_row_hash and RowEncoder.hash_rows / hash_rows_into / bind_hash /
partition_by).  Every output is compared in full, plus one guard entry, with the numpy model of
tests/test_hash_model.py (written from the header's rules alone) applied to the oracle's decode of
the same rows; malformed rows with a second model that reads the key slots from the row bytes under
the "Decode bounds" rules.  Marked gpu."""
from __future__ import annotations

import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from fury_amd import types as T  # noqa: E402
from fury_amd.workloads import SCHEMAS, Column, gen_columns  # noqa: E402
from tests.test_hash_model import hash_columns, mm3, mm3_null, part_ids  # noqa: E402
from tests.test_partition_model import partition_model  # noqa: E402
from tests.test_take import COUNTS, _device_src, _pair_fields, _Src, assert_same, source  # noqa: E402

SENTINEL = 0x5A5A5A5A
ROW_COUNTS = sorted(set(COUNTS) | {255, 256})
# hash.hip: a tile is the 256 rows of a workgroup (fewer when the keys need more than 24 header
# words); when the tile's rows, [row_offsets[r0], row_offsets[r0 + nr]), are at most this many bytes they are staged in LDS and the
# variable-length keys are hashed from there, otherwise from global memory
STAGE_BYTES = 32 * 1024
TILE_ROWS = 256


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


# ---- sources: one encoded batch and the oracle's decode of it, computed once and never modified --------
_CACHE: dict = {}


def _key_fields():
    """70 nullable fields of every hashable kind: bits 63 and 64 lie in different bitmap words."""
    kinds = [T.BOOL, T.INT8, T.INT16, T.INT32, T.INT64, T.FLOAT32, T.FLOAT64, T.DATE32, T.TIMESTAMP,
             T.STRING, T.DECIMAL, T.BINARY]
    return [T.field(f"c{k:02d}", kinds[k % len(kinds)]) for k in range(70)]


def _fields_of(name):
    return {"pair": _pair_fields(), "keys": _key_fields()}.get(name) or SCHEMAS[name]


class _Case:
    def __init__(self, oracle, src, fields):
        self.src, self.fields, self.n = src, list(fields), src.n
        self.enc = src.enc
        self.ref = oracle.decode(self.fields, src.rows, None if src.fixed else src.offs, src.n)
        assert len(src.rows) % 8 == 0

    def idx(self, keys):
        return self.enc._select(keys)

    def want(self, keys, seed=0, null_rows=()):
        idx = self.idx(keys)
        return hash_columns([self.fields[k] for k in idx], [self.ref[k] for k in idx], self.n, seed,
                            null_rows)


def case(oracle, dev, name, n, null_pct=None):
    from fury_amd.encoder import Encoders
    key = (name, n, null_pct)
    if key not in _CACHE:
        fields = _fields_of(name)
        if name == "row_test":                       # a map and a struct: from row values
            from fury_amd.beans import beans_to_columns
            from tests.test_device import _random_value
            rng = np.random.default_rng(12)
            host = beans_to_columns(fields, [{f.name: _random_value(f, rng) for f in fields}
                                             for _ in range(n)])
            src = _Src(dev, Encoders.bean(fields, device=dev), host, n)
        elif null_pct is None and name != "keys":
            src = source(dev, name, n)
        else:
            host = gen_columns(name if name in SCHEMAS else None, fields, n, seed=3,
                               null_pct=30 if null_pct is None else null_pct)
            src = _Src(dev, Encoders.bean(fields, device=dev), host, n)
        _CACHE[key] = _Case(oracle, src, fields)
    return _CACHE[key]


def _guarded(dev, n, dtype):
    t = torch.full((n + 1,), SENTINEL, dtype=torch.int32, device=dev).view(dtype)
    return t, t[:n]


def run_hash(c, keys, what, seed=0, num_parts=7, hashes=True, ids=True, shift=0, stream=None,
             bound=False, batch=None, want=None):
    """One hash_rows_into call into guarded outputs, compared in full with the model."""
    dev, n = c.src.dev, c.n
    want = c.want(keys, seed) if want is None else want
    batch = _device_src(c.src, shift) if batch is None else batch
    th, oh = _guarded(dev, n, torch.uint32) if hashes else (None, None)
    tp, op = _guarded(dev, n, torch.int32) if ids else (None, None)
    torch.cuda.synchronize()
    args = (batch, keys, oh, op, seed, num_parts if ids else None)
    if bound:
        c.enc.bind_hash(*args, stream=stream)()
    else:
        c.enc.hash_rows_into(*args, stream=stream)
    torch.cuda.synchronize()
    guard = np.array([SENTINEL], np.uint32)
    if hashes:
        assert_same(th.cpu().numpy(), np.concatenate([want, guard]), f"{what}: hashes")
    if ids:
        assert_same(tp.cpu().numpy(), np.concatenate([part_ids(want, num_parts),
                                                      guard.view(np.int32)]), f"{what}: part ids")
    return want


KEY_SETS = {
    "pair": [["a"], ["b", "a"]],
    "struct100": [[0], [99, 0, 50], [63, 64], list(range(36, 100))],
    "mixed": [["a"], ["s1"], ["s2", "b", "s1"], ["b", "s3", "c", "a"]],
    "foo": [["f1"], ["f2"], ["f2", "f1"]],
    "row_test": [["f2"], ["f1"], ["f1", "f2"]],
}


# 1. every schema shape x row count x key set ---------------------------------------------------------------
@pytest.mark.parametrize("n", ROW_COUNTS)
@pytest.mark.parametrize("name", list(KEY_SETS))
def test_hash_matrix(oracle, dev, name, n):
    c = case(oracle, dev, name, n)
    if name in ("pair", "struct100"):
        assert c.src.fixed                          # row_offsets is NULL in these calls
    for keys in KEY_SETS[name]:
        assert len(keys) <= 64
        run_hash(c, keys, f"{name} n={n} keys {keys}")
    c.enc.device_status()


# 2. every key kind, nulls, bitmap-word boundaries -------------------------------------------------------------
@pytest.mark.parametrize("null_pct", [0, 30, 100])
@pytest.mark.parametrize("name", ["keys", "mixed"])
def test_key_kinds_and_nulls(oracle, dev, name, null_pct):
    n = 257
    c = case(oracle, dev, name, n, null_pct)
    if name == "keys":
        sets = [[4], list(range(9)), [9], [9, 4, 10], [10, 4, 9], [62, 63, 64, 65], [11, 0],
                list(range(6, 70))]
    else:
        sets = [["b"], ["s1"], ["s1", "b", "s2"], ["c", "s3", "a"]]
    for keys in sets:
        want = run_hash(c, keys, f"{name} nulls {null_pct}% keys {keys}", seed=42)
        if null_pct == 100:                          # a chain of nulls, whatever the kinds
            h = 42
            for _ in keys:
                h = mm3_null(h)
            assert (want == h).all()
    c.enc.device_status()


# 3. every tail length, a value longer than a tile's stage, both paths ----------------------------------------------
LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 300, 8191]


def _string_case(oracle, dev, lens, key):
    from fury_amd.encoder import Encoders
    if key not in _CACHE:
        rng = np.random.default_rng(11)
        offs = np.zeros(len(lens) + 1, np.int32)
        np.cumsum(lens, out=offs[1:])
        col = Column(values=rng.integers(0, 256, int(offs[-1]), dtype=np.uint8), offsets=offs)
        fields = [T.field("s", T.STRING)]
        src = _Src(dev, Encoders.bean(fields, device=dev), [col], len(lens))
        _CACHE[key] = _Case(oracle, src, fields)
    return _CACHE[key]


def _tile_bytes(src):
    return [int(src.offs[min(r0 + TILE_ROWS, src.n)] - src.offs[r0])
            for r0 in range(0, src.n, TILE_ROWS)]


def test_string_lengths_staged_and_fallback(oracle, dev):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "fury_amd", "csrc", "hash.hip")) as f:
        assert "kHashStage = 32 * 1024;" in f.read()           # STAGE_BYTES above is the kernel's
    # one tile of 14 rows, 8.9 KB: staged, the 8191-byte value included
    small = _string_case(oracle, dev, LENGTHS, "lens")
    assert _tile_bytes(small.src) == [int(small.src.offs[-1])] and _tile_bytes(small.src)[0] <= STAGE_BYTES
    # the same lengths six times over in one tile, 53 KB: every value from global memory
    big = _string_case(oracle, dev, LENGTHS * 6, "lens6")
    assert len(_tile_bytes(big.src)) == 1 and _tile_bytes(big.src)[0] > STAGE_BYTES
    # two tiles in one launch: 256 short rows (staged), then the long ones (not staged)
    both = _string_case(oracle, dev, (LENGTHS[:12] * 22)[:256] + LENGTHS * 6, "lens2")
    tb = _tile_bytes(both.src)
    assert len(tb) == 2 and tb[0] <= STAGE_BYTES < tb[1]
    for what, c in (("staged", small), ("fallback", big), ("staged + fallback", both)):
        for seed in (0, 0xFFFFFFFF):
            want = run_hash(c, ["s"], f"string lengths, {what}, seed {seed}", seed=seed)
            vals, o = c.ref[0].values, np.asarray(c.ref[0].offsets).view(np.int32)
            for r in range(min(c.n, 14)):             # the model itself, value by value
                assert want[r] == mm3(bytes(vals[o[r]:o[r + 1]]), seed)
        run_hash(c, ["s"], f"string lengths, {what}, shifted", shift=8)
        c.enc.device_status()


# 4. the outputs, the partition counts, the seeds -------------------------------------------------------------------
@pytest.mark.parametrize("name,keys", [("mixed", ["s1", "b"]), ("struct100", [2, 3])])
def test_outputs_parts_and_seeds(oracle, dev, name, keys):
    c = case(oracle, dev, name, 4097)
    for seed in (0, 42, 0xFFFFFFFF):
        want = c.want(keys, seed)
        for num_parts in (1, 2, 7, 65535, 2 ** 31 - 1):
            run_hash(c, keys, f"{name} seed {seed} parts {num_parts}", seed, num_parts, want=want)
        run_hash(c, keys, f"{name} seed {seed} hashes only", seed, ids=False, want=want)
        run_hash(c, keys, f"{name} seed {seed} ids only", seed, 65535, hashes=False, want=want)
    assert len(np.unique(c.want(keys, 0))) > 4000               # a hash, not a constant
    c.enc.device_status()


# 5. a side stream, the bound form, a shifted source ----------------------------------------------------------------
@pytest.mark.parametrize("name,keys", [("mixed", ["s2", "a"]), ("pair", ["a", "b"]),
                                       ("struct100", list(range(64)))])
def test_stream_bound_and_shift(oracle, dev, name, keys):
    c = case(oracle, dev, name, 4097)
    want = c.want(keys, 5)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    run_hash(c, keys, f"{name} side stream", 5, stream=s, want=want)
    c.enc.device_status(s)
    run_hash(c, keys, f"{name} bound", 5, bound=True, want=want)
    run_hash(c, keys, f"{name} bound, side stream, shifted", 5, bound=True, stream=s, shift=8,
             want=want)
    run_hash(c, keys, f"{name} shifted by 8", 5, shift=8, want=want)
    c.enc.device_status(s)
    c.enc.device_status()


# 6. hash_rows == model(project_batch) on the same batch ---------------------------------------------------------------
@pytest.mark.parametrize("name,keys", [("mixed", ["s3", "a", "s1"]), ("keys", [9, 4, 10, 0, 11]),
                                       ("struct100", [1, 98])])
def test_hash_rows_is_the_model_of_project_batch(oracle, dev, name, keys):
    from fury_amd.encoder import column_to_host
    n = 4097 if name != "keys" else 257
    c = case(oracle, dev, name, n, 30 if name == "keys" else None)
    batch = _device_src(c.src, 0)
    cols = [column_to_host(x) for x in c.enc.project_batch(batch, keys)]
    idx = c.idx(keys)
    want = hash_columns([c.fields[k] for k in idx], cols, n, seed=9)
    hashes = c.enc.hash_rows(batch, keys, seed=9)
    assert hashes.dtype == torch.uint32 and hashes.shape == (n,)
    assert_same(hashes.cpu().numpy(), want, f"{name}: hash_rows")
    h2, ids = c.enc.hash_rows(batch, keys, seed=9, num_parts=11)
    assert ids.dtype == torch.int32
    assert_same(h2.cpu().numpy(), want, f"{name}: hash_rows with ids")
    assert_same(ids.cpu().numpy(), part_ids(want, 11), f"{name}: part ids")
    assert_same(want, c.want(keys, 9), f"{name}: the two references")


# 7. partition_by == partition with the model's ids, byte for byte ---------------------------------------------------------
@pytest.mark.parametrize("num_parts", [1, 7, 300])
@pytest.mark.parametrize("name,keys", [("mixed", ["s1", "b"]), ("struct100", [0]), ("foo", ["f2"])])
def test_partition_by(oracle, dev, name, keys, num_parts):
    n = 4097
    c = case(oracle, dev, name, n)
    ids = part_ids(c.want(keys, 3), num_parts)
    fs = c.enc.schema().fixed_size if c.src.fixed else None
    data, eoffs, eparts, _, _, bad = partition_model(c.src.rows, c.src.offs, n, ids, num_parts, fs)
    assert not bad and int(eparts[-1]) == n
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    for stream in (None, s):
        out, part_rows = c.enc.partition_by(_device_src(c.src, 0), keys, num_parts, seed=3,
                                            stream=stream)
        torch.cuda.synchronize()
        what = f"{name} partition_by {num_parts}"
        assert out.nrows == n
        assert_same(part_rows.cpu().numpy(), eparts, f"{what}: part_rows")
        assert_same(out.rows.cpu().numpy(), data, f"{what}: rows")
        if not c.src.fixed:
            assert_same(out.row_offsets.cpu().numpy(), eoffs, f"{what}: offsets")
    if num_parts > 1:
        assert (np.diff(eparts) > 0).sum() > 1                  # the rows do spread


# 8. malformed rows ----------------------------------------------------------------------------------------------------------
def rows_model(fields, rows, offs, n, keys, seed):
    """hash[r] from the row bytes under the "Decode bounds" rules: (hashes, rows that raise).  A row
    whose header leaves [0, offs[n]) has every key null; a variable-length value whose bytes leave it,
    or whose size is negative, is null."""
    nf = len(fields)
    bm = (nf + 63) // 64 * 8
    total = int(offs[n])
    out, bad = np.zeros(n, np.uint32), []
    for r in range(n):
        base = int(offs[r])
        ok = 0 <= base and base + bm + 8 * nf <= total
        if not ok:
            bad.append(r)
        h = seed
        for k in keys:
            value = None
            if ok and not (rows[base + (k >> 3)] >> (k & 7)) & 1:
                slot = struct.unpack_from("<Q", rows, base + bm + 8 * k)[0]
                t = fields[k].type_id
                if t == T.BOOL:
                    value = bytes([(slot & 0xFF) != 0])
                elif T.type_width(t) > 0:
                    value = struct.pack("<Q", slot)[:T.type_width(t)]
                else:
                    p = base + struct.unpack("<i", struct.pack("<I", slot >> 32))[0]
                    size = 16 if t == T.DECIMAL else struct.unpack("<i", struct.pack("<I", slot & 0xFFFFFFFF))[0]
                    if p >= 0 and size >= 0 and p + size <= total:
                        value = bytes(rows[p:p + size])
                    else:
                        bad.append(r)
            h = mm3_null(h) if value is None else mm3(value, h)
        out[r] = h
    return out, sorted(set(bad))


def _edge_batch(c, rows, offs):
    """The rows at the very end of a device allocation of their own (a 32 MiB block is a segment of
    the caching allocator by itself): a read past the batch's last byte leaves the allocation."""
    from fury_amd.encoder import RowBatch
    torch.cuda.empty_cache()
    big = torch.empty(32 << 20, dtype=torch.uint8, device=c.src.dev)
    assert len(rows) % 8 == 0 and big.data_ptr() % 4096 == 0
    view = big[big.numel() - len(rows):]
    view.copy_(torch.from_numpy(np.ascontiguousarray(rows)))
    return RowBatch(view, torch.from_numpy(np.asarray(offs, np.int64)).to(c.src.dev), c.n,
                    c.enc.schema_hash), big


def _set_slot(c, rows, r, k, off, size):
    base = int(c.src.offs[r])
    rows[base + (k >> 3)] &= ~(1 << (k & 7)) & 0xFF                     # not null
    struct.pack_into("<Q", rows, base + c.enc.schema().bitmap_bytes + 8 * k,
                     ((off & 0xFFFFFFFF) << 32) | (size & 0xFFFFFFFF))


def test_rows_model_is_the_column_model_on_clean_rows(oracle, dev):
    for name, keys in (("mixed", ["s1", "b", "s3"]), ("keys", [9, 0, 10, 2, 11, 6])):
        c = case(oracle, dev, name, 257, 30 if name == "keys" else None)
        got, bad = rows_model(c.fields, c.src.rows, c.src.offs, c.n, c.idx(keys), 42)
        assert not bad
        assert_same(got, c.want(keys, 42), name)


MALFORMED = ["negative size", "span past the total", "span ending exactly at the total",
             "unaligned in-bounds offset", "unaligned long value", "truncated last row",
             "last row without its header", "corrupt slots of fields that are not keys"]


@pytest.mark.parametrize("what", MALFORMED)
def test_malformed_rows(oracle, dev, what):
    from fury_amd.encoder import IndexOutOfBoundsException
    n, victim = 257, 100
    c = case(oracle, dev, "mixed", n)
    fields, keys = c.fields, c.idx(["a", "s1", "b"])
    k = c.idx(["s1"])[0]
    rows, offs = c.src.rows.copy(), c.src.offs.copy()
    total, base = int(offs[n]), int(offs[victim])
    expect_bad = [victim]
    if what == "negative size":
        _set_slot(c, rows, victim, k, 32, -5)
    elif what == "span past the total":
        _set_slot(c, rows, victim, k, total - base - 8, 9)
    elif what == "span ending exactly at the total":
        _set_slot(c, rows, victim, k, total - base - 13, 13)
        expect_bad = []
    elif what == "unaligned in-bounds offset":
        assert _tile_bytes(c.src)[0] <= STAGE_BYTES                   # hashed from the staged rows
        _set_slot(c, rows, victim, k, 19, 21)                         # inside its own tile
        expect_bad = []
    elif what == "unaligned long value":
        _set_slot(c, rows, victim, k, 5 - base, total - 5)            # almost the whole batch
        expect_bad = []
    elif what == "truncated last row":
        last = c.idx(["s3"])[0]
        rows, offs[n] = rows[:total - 8], total - 8
        keys = c.idx(["a", "s3", "s1", "s2"])
        assert not (rows[int(offs[n - 1]) + (last >> 3)] >> (last & 7)) & 1     # s3 is there
        expect_bad = [n - 1]
    elif what == "last row without its header":
        cut = int(offs[n - 1]) + 16
        rows, offs[n] = rows[:cut], cut
        expect_bad = [n - 1]
    else:
        for r in (0, victim, n - 1):
            for name in ("s2", "s3", "c"):
                _set_slot(c, rows, r, c.idx([name])[0], 2 ** 31 - 1, 2 ** 31 - 1)
        expect_bad = []
    want, bad = rows_model(fields, rows, offs, n, keys, 42)
    assert bad == expect_bad
    if what == "span ending exactly at the total":
        assert want[victim] != c.want(keys, 42)[victim]
    batch, keep = _edge_batch(c, rows, offs)
    th, oh = _guarded(c.src.dev, n, torch.uint32)
    tp, op = _guarded(c.src.dev, n, torch.int32)
    c.enc.device_status()
    c.enc.hash_rows_into(batch, keys, oh, op, 42, 7)
    torch.cuda.synchronize()
    guard = np.array([SENTINEL], np.uint32)
    assert_same(th.cpu().numpy(), np.concatenate([want, guard]), f"{what}: hashes")
    assert_same(tp.cpu().numpy(), np.concatenate([part_ids(want, 7), guard.view(np.int32)]),
                f"{what}: part ids")
    if expect_bad:
        with pytest.raises(IndexOutOfBoundsException, match=f"row {expect_bad[0]} "):
            c.enc.device_status()
    c.enc.device_status()                                              # clean (again)
    del keep


def test_foreign_schema_hash_and_nested_keys(oracle, dev):
    from fury_amd.encoder import ClassNotCompatibleException, UnsupportedOperationException
    c, other = case(oracle, dev, "foo", 65), case(oracle, dev, "mixed", 257)
    batch = _device_src(c.src, 0)
    with pytest.raises(UnsupportedOperationException, match="f5"):
        c.enc.hash_rows(batch, ["f1", "f5"])
    with pytest.raises(ClassNotCompatibleException):
        other.enc.hash_rows(batch, ["a"])
    run_hash(c, ["f2"], "foo after the errors")                       # they left no state behind
    empty = c.enc.hash_rows(c.enc.slice_rows(batch, 0, 0), ["f2"], num_parts=3)
    assert empty[0].numel() == 0 and empty[1].numel() == 0
