"""A plain-Python model of fury_row_aggregate, written from rules 1-6 of include/fury_row.h alone over
decoded values, and its pins without a GPU: hand-computed cases of every rule, then the Python layer's
host-side argument checks on CPU tensors (nothing reaches the library there).  The GPU tests
(tests/test_aggregate.py) compare the kernels with this model applied to the oracle's decode."""
from __future__ import annotations

import math
import struct

import numpy as np
import pytest

from fury_amd import types as T

M64 = (1 << 64) - 1
SIGNED = (T.INT8, T.INT16, T.INT32, T.INT64, T.DATE32, T.TIMESTAMP)
SUMMABLE_INTS = (T.INT8, T.INT16, T.INT32, T.INT64)
FLOATS = (T.FLOAT32, T.FLOAT64)
OPS = ("count", "sum", "min", "max", "argmin", "argmax")


def order_key(tid, v: bytes):
    """A Python value that ranks as rule 3 of fury_row_compare ranks the value bytes v."""
    if tid in SIGNED or tid == T.DECIMAL:
        return int.from_bytes(v, "little", signed=True)
    if tid in FLOATS:
        bits, top = int.from_bytes(v, "little"), 1 << (8 * len(v) - 1)
        return (bits ^ (2 * top - 1)) if bits & top else bits | top      # IEEE-754 totalOrder
    if tid == T.BOOL:
        return int(v[0] != 0)
    assert tid in (T.STRING, T.BINARY), tid
    return bytes(v)                                                     # unsigned bytes, a prefix first


def stored(tid, v: bytes) -> int:
    """The 8 bytes rule 4 stores for the winning value v, as an unsigned word."""
    if tid in SIGNED:
        return int.from_bytes(v, "little", signed=True) & M64               # sign-extended
    if tid == T.BOOL:
        return int(v[0] != 0)
    assert tid in FLOATS, tid
    return int.from_bytes(v, "little")                                  # FLOAT32: low half, high half zero


def widen(tid, v: bytes) -> float:
    return struct.unpack("<f" if tid == T.FLOAT32 else "<d", v)[0]


def aggregate_model(tid, values, valid, ids, G, op):
    """(out, count, abs_sums, finite) of one aggregate.  tid: the field's type id (None: COUNT(*));
    values[r]: the value bytes of row r (fixed-width little-endian, BOOL one byte, DECIMAL 16 bytes,
    STRING / BINARY the payload); valid[r]: not null (and the row takes part); ids[r]: the group, None:
    all 0.  out: uint64 words as rule 2-5 store them, count: int64.  For a float SUM, abs_sums[g] is the
    sum of |x| and finite[g] the number m of finite values of rule 3's bound, and out[g] holds the bits
    of the correctly rounded exact sum (math.fsum) -- or of the IEEE sum when a value is not finite."""
    assert op in OPS
    n = len(valid)
    groups = [[] for _ in range(G)]
    for r in range(n):
        g = 0 if ids is None else int(ids[r])
        if 0 <= g < G and valid[r]:                                     # rule 1: other ids take no part
            groups[g].append(r)
    out, count = np.zeros(G, np.uint64), np.zeros(G, np.int64)
    abs_sums, finite = [0.0] * G, [0] * G
    for g, rows in enumerate(groups):
        count[g] = len(rows)
        if op == "count":
            out[g] = len(rows)
        elif op == "sum" and tid in SUMMABLE_INTS:
            out[g] = sum(int.from_bytes(values[r], "little", signed=True) for r in rows) & M64
        elif op == "sum":
            assert tid in FLOATS, tid
            xs = [widen(tid, values[r]) for r in rows]
            fin = [x for x in xs if math.isfinite(x)]
            abs_sums[g], finite[g] = math.fsum(abs(x) for x in fin), len(fin)
            total = math.fsum(fin) + 0.0                                # an empty sum is +0.0
            for x in xs:                                                # IEEE: inf - inf and NaN give NaN in any order
                if not math.isfinite(x):
                    total = total + x
            out[g] = struct.unpack("<Q", struct.pack("<d", total))[0]
        elif not rows:
            out[g] = M64 if op.startswith("arg") else 0                 # rule 2: -1 / 0
        else:
            keys = [order_key(tid, values[r]) for r in rows]
            best = min(keys) if op in ("min", "argmin") else max(keys)
            first = rows[keys.index(best)]                              # rows ascend: the smallest row number
            out[g] = first if op.startswith("arg") else stored(tid, values[first])
    return out, count, abs_sums, finite


def sum_bound(abs_sum, m):
    """Rule 3: |float sum - exact sum| <= (m - 1) * 2^-52 * sum |x|."""
    return max(m - 1, 0) * 2.0 ** -52 * abs_sum


# ---- pins -------------------------------------------------------------------------------------------------------
def _i(width, *xs):
    return [int(x).to_bytes(width, "little", signed=True) for x in xs]


def _f32(*bits):
    return [struct.pack("<I", b) for b in bits]


def _run(tid, values, ids, G, op, nulls=()):
    valid = np.ones(len(values), bool)
    valid[list(nulls)] = False
    out, count, _, _ = aggregate_model(tid, values, valid, ids, G, op)
    return [int(x) for x in out], count.tolist()


def test_int64_sum_wraps():
    vals = _i(8, 2 ** 63 - 1, 1, 5)
    assert _run(T.INT64, vals, None, 1, "sum") == ([(2 ** 63 + 5) & M64], [3])       # = -2^63 + 5 as int64
    assert np.array([(2 ** 63 + 5)], np.uint64).view(np.int64)[0] == -2 ** 63 + 5
    assert _run(T.INT64, _i(8, -2 ** 63, -1), None, 1, "sum") == ([2 ** 63 - 1], [2])
    assert _run(T.INT8, _i(1, -128, -128, 127), None, 1, "sum") == ([(-129) & M64], [3])  # widened, no wrap at 8 bits


def test_int8_min_is_sign_extended():
    vals = _i(1, 5, -3, 127, -128)
    assert _run(T.INT8, vals, [0, 0, 1, 1], 2, "min") == ([(-3) & M64, (-128) & M64], [2, 2])
    assert _run(T.INT8, vals, [0, 0, 1, 1], 2, "max") == ([5, 127], [2, 2])
    assert vals[1] == b"\xfd"                                           # unsigned it would be the maximum


def test_float32_total_order_and_payloads():
    NZ, PZ, NINF, PINF = 0x80000000, 0x00000000, 0xFF800000, 0x7F800000
    NNAN, PNAN = 0xFFC00123, 0x7FC00456
    vals = _f32(PZ, NZ)
    assert _run(T.FLOAT32, vals, None, 1, "min") == ([NZ], [2])         # -0.0 < +0.0
    assert _run(T.FLOAT32, vals, None, 1, "max") == ([PZ], [2])
    assert _run(T.FLOAT32, vals, None, 1, "argmin") == ([1], [2])
    vals = _f32(NINF, NNAN, PINF, PNAN, 0x3F800000)
    assert _run(T.FLOAT32, vals, None, 1, "min") == ([NNAN], [5])       # a negative NaN below -inf, payload kept
    assert _run(T.FLOAT32, vals, None, 1, "max") == ([PNAN], [5])       # a positive NaN above +inf; high half zero
    assert _run(T.FLOAT32, vals, None, 1, "argmax") == ([3], [5])
    d = [struct.pack("<Q", b) for b in (0xFFF8000000000001, 0xFFF0000000000000, 0x7FF8000000000002)]
    assert _run(T.FLOAT64, d, None, 1, "min") == ([0xFFF8000000000001], [3])
    assert _run(T.FLOAT64, d, None, 1, "max") == ([0x7FF8000000000002], [3])


def test_empty_groups_and_nulls():
    vals = _i(4, 7, 8, 9)
    for op, empty in (("count", 0), ("sum", 0), ("min", 0), ("max", 0), ("argmin", M64), ("argmax", M64)):
        out, count = _run(T.INT32, vals, [0, 2, 2], 4, op, nulls=[0])
        assert count == [0, 0, 2, 0], op
        assert out[0] == out[1] == out[3] == empty, op                  # an all-null group, two unused ids
    assert _run(T.INT32, vals, [0, 2, 2], 4, "sum", nulls=[0])[0][2] == 17
    assert _run(None, [b""] * 3, [0, 2, 2], 4, "count") == ([1, 0, 2, 0], [1, 0, 2, 0])      # COUNT(*)
    assert np.array([M64], np.uint64).view(np.int64)[0] == -1


def test_dropped_ids():
    vals = _i(8, 1, 2, 4, 8, 16, 32)
    ids = [-1, 3, -2 ** 63, 2 ** 40, 0, 2]
    assert _run(T.INT64, vals, ids, 3, "sum") == ([16, 0, 32], [1, 0, 1])
    assert _run(T.INT64, vals, ids, 3, "argmax") == ([4, M64, 5], [1, 0, 1])


def test_argmin_ties_go_to_the_smallest_row():
    vals = _i(2, 9, 3, 3, 9, 3)
    assert _run(T.INT16, vals, None, 1, "argmin") == ([1], [5])
    assert _run(T.INT16, vals, None, 1, "argmax") == ([0], [5])
    assert _run(T.INT16, vals, None, 1, "argmin", nulls=[1]) == ([2], [4])
    assert _run(T.INT16, vals, [1, 1, 0, 0, 0], 2, "argmin") == ([2, 1], [3, 2])


def test_byte_string_order():
    vals = [b"ab", b"a", b"abc", b"", b"a", b"\x80", b"z", b"\xff\x00"]
    assert _run(T.STRING, vals, None, 1, "argmin") == ([3], [8])        # the empty string: a prefix of all
    assert _run(T.STRING, vals, None, 1, "argmin", nulls=[3]) == ([1], [7])     # "a" before "ab" before "abc"
    assert _run(T.BINARY, vals, None, 1, "argmax") == ([7], [8])        # bytes >= 0x80 after ASCII
    assert _run(T.BINARY, vals[:7], None, 1, "argmax") == ([5], [7])
    assert _run(T.STRING, [None, b""], None, 1, "argmin", nulls=[0]) == ([1], [1])   # null is not the empty string


def test_decimal_is_a_signed_128_bit_integer():
    vals = [int(x).to_bytes(16, "little", signed=True) for x in (1, -1, 2 ** 100, -2 ** 127, 2 ** 127 - 1, 2 ** 64)]
    assert _run(T.DECIMAL, vals, None, 1, "argmin") == ([3], [6])
    assert _run(T.DECIMAL, vals, None, 1, "argmax") == ([4], [6])
    assert _run(T.DECIMAL, vals[:3] + vals[5:], None, 1, "argmin") == ([1], [4])   # -1 = 0xFF..FF is not the largest
    assert _run(T.DECIMAL, vals[:3] + vals[5:], None, 1, "argmax") == ([2], [4])


def test_float_sum_reports_the_bound_terms():
    xs = [1.5, -2.25, 1e300, -1e300, 3.0]
    vals = [struct.pack("<d", x) for x in xs]
    out, count, abs_sums, finite = aggregate_model(T.FLOAT64, vals, np.ones(5, bool), None, 1, "sum")
    assert struct.unpack("<d", struct.pack("<Q", int(out[0])))[0] == 2.25 and count.tolist() == [5]
    assert finite == [5] and abs_sums[0] == math.fsum(abs(x) for x in xs)
    assert sum_bound(abs_sums[0], 5) == 4 * 2.0 ** -52 * abs_sums[0]
    f = [struct.pack("<f", x) for x in (0.1, 0.2)]                     # widened exactly, then added in double
    out, _, _, _ = aggregate_model(T.FLOAT32, f, np.ones(2, bool), None, 1, "sum")
    want = float(np.float32(0.1)) + float(np.float32(0.2))
    assert struct.unpack("<d", struct.pack("<Q", int(out[0])))[0] == want != 0.1 + 0.2
    inf = [struct.pack("<d", x) for x in (1.0, math.inf, 2.0)]
    out, _, abs_sums, finite = aggregate_model(T.FLOAT64, inf, np.ones(3, bool), None, 1, "sum")
    assert struct.unpack("<d", struct.pack("<Q", int(out[0])))[0] == math.inf and finite == [2]
    both = inf + [struct.pack("<d", -math.inf)]
    out, _, _, _ = aggregate_model(T.FLOAT64, both, np.ones(4, bool), None, 1, "sum")
    assert math.isnan(struct.unpack("<d", struct.pack("<Q", int(out[0])))[0])


# ---- the Python layer's host-side checks: CPU tensors, nothing reaches the library ------------------------------------
def test_python_surface_checks_before_any_device_work():
    import torch
    import fury_amd
    from fury_amd import Agg, AggResult, aggregate_into, bind_aggregate, group_by, group_by_rows
    from fury_amd.encoder import ClassNotCompatibleException, Encoders, IllegalArgumentException, RowBatch
    from fury_amd.workloads import SCHEMAS
    enc = Encoders.bean(SCHEMAS["mixed"], device="cpu")

    def batch(n):
        return RowBatch(torch.zeros(64, dtype=torch.uint8), torch.zeros(n + 1, dtype=torch.int64), n,
                        enc.schema_hash)
    four = batch(4)
    ids = torch.zeros(4, dtype=torch.int64)
    out = torch.zeros(8, dtype=torch.int64)
    assert Agg("count") == ("count", None) and Agg("sum", "a").field == "a"
    assert AggResult._fields == ("values", "count")
    one = [Agg("count", None)]
    with pytest.raises(IllegalArgumentException, match="0 aggregates: 1 to 16"):
        aggregate_into(enc, four, ids, 2, [], [])
    with pytest.raises(IllegalArgumentException, match="17 aggregates: 1 to 16"):
        aggregate_into(enc, four, ids, 2, one * 17, [out] * 17)
    with pytest.raises(IllegalArgumentException, match="unknown aggregate op 'avg'"):
        aggregate_into(enc, four, ids, 2, [Agg("avg", "a")], [out])
    with pytest.raises(IllegalArgumentException, match="sum needs a field"):
        aggregate_into(enc, four, ids, 2, [Agg("sum", None)], [out])
    with pytest.raises(IllegalArgumentException, match="no field named"):
        aggregate_into(enc, four, ids, 2, [Agg("sum", "nope")], [out])
    with pytest.raises(IllegalArgumentException, match="num_groups < 0"):
        aggregate_into(enc, four, ids, -1, one, [out])
    with pytest.raises(IllegalArgumentException, match="group_ids is None: num_groups must be 1, not 2"):
        aggregate_into(enc, four, None, 2, one, [out])
    with pytest.raises(IllegalArgumentException, match="group_ids must be an int64 tensor"):
        aggregate_into(enc, four, ids.to(torch.int32), 2, one, [out])
    with pytest.raises(IllegalArgumentException, match="group_ids has 3 entries for 4 rows"):
        aggregate_into(enc, four, ids[:3], 2, one, [out])
    with pytest.raises(IllegalArgumentException, match="2 outputs for 1 aggregates"):
        aggregate_into(enc, four, ids, 2, one, [out, out])
    with pytest.raises(IllegalArgumentException, match="2 counts for 1 aggregates"):
        aggregate_into(enc, four, ids, 2, one, [out], [out, out])
    with pytest.raises(IllegalArgumentException, match=r"outs\[0\] must be an int64 or float64 tensor"):
        aggregate_into(enc, four, ids, 2, one, [out.to(torch.int32)])
    with pytest.raises(IllegalArgumentException, match=r"outs\[0\] must be an int64 or float64 tensor"):
        aggregate_into(enc, four, ids, 2, one, [out.to(torch.float32)])       # float32: a FLOAT32 min / max only
    with pytest.raises(IllegalArgumentException, match=r"outs\[0\] has 8 entries, 9 needed"):
        aggregate_into(enc, four, ids, 9, one, [out])
    with pytest.raises(IllegalArgumentException, match=r"counts\[0\] must be an int64 tensor"):
        aggregate_into(enc, four, ids, 2, one, [out], [out.to(torch.float64)])
    with pytest.raises(IllegalArgumentException, match=r"counts\[0\] has 1 entries, 2 needed"):
        aggregate_into(enc, four, ids, 2, one, [out], [out[:1]])
    other = Encoders.bean([T.field("x", T.INT64)], device="cpu")
    with pytest.raises(ClassNotCompatibleException):
        aggregate_into(other, four, ids, 2, [Agg("sum", "x")], [out])
    with pytest.raises(ClassNotCompatibleException):
        bind_aggregate(other, four, ids, 2, [Agg("sum", "x")], [out])
    f32 = Encoders.bean([T.field("x", T.FLOAT32)], device="cpu")
    fb = RowBatch(torch.zeros(64, dtype=torch.uint8), None, 4, f32.schema_hash)
    with pytest.raises(IllegalArgumentException, match=r"outs\[0\] has 3 entries, 4 needed"):
        aggregate_into(f32, fb, ids, 2, [Agg("min", "x")], [torch.zeros(3, dtype=torch.float32)])
    with pytest.raises(IllegalArgumentException, match=r"outs\[0\] must be an int64 or float64"):
        aggregate_into(f32, fb, ids, 2, [Agg("sum", "x")], [torch.zeros(4, dtype=torch.float32)])
    # no groups: rule 6 has nothing to write, nothing is launched (there is no GPU here)
    aggregate_into(enc, four, ids, 0, [Agg("count", None), Agg("sum", "a")], [out[:0], out[:0]])
    bind_aggregate(enc, four, ids, 0, one, [out[:0]], [out[:0]])()
    res = fury_amd.aggregate(enc, four, ids, 0, [Agg("count", None), Agg("max", "a")])
    assert len(res) == 2 and all(isinstance(r, AggResult) and r.values.numel() == r.count.numel() == 0 for r in res)
    g, res = group_by(enc, batch(0), ["a"], one)                        # an empty batch has no groups
    assert g.num_groups == 0 and res[0].values.numel() == 0
    with pytest.raises(IllegalArgumentException, match="2 names for 1 aggregates"):
        group_by_rows(enc, four, ["a"], one, ["n", "m"])
    with pytest.raises(IllegalArgumentException, match="unknown aggregate op"):
        group_by(enc, batch(0), ["a"], [Agg("median", "a")])
