"""The numpy model of fury_row_select (rules 1-5 of include/fury_row.h), pinned to the oracle on the
CPU: applied to the oracle's rows of all columns it gives, byte for byte, the oracle's rows of the
selected columns under the selected schema.  tests/test_select.py compares the GPU against this
model, which alone also covers malformed and non-canonical input."""
from __future__ import annotations

import numpy as np
import pytest

from fury_amd import types as T
from fury_amd.workloads import SCHEMAS, gen_columns

INT32_MAX = 2 ** 31 - 1


def _i32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >> 31 else x


def header_size(nf):
    return ((nf + 63) // 64) * 8 + 8 * nf


class Want:
    """data / offs: the output batch; bad: the rows the call reports (a failed row or value)."""


def _value_ok(f, off, size, B, total):
    if off < 0 or size < 0 or off % 8 or not (0 <= B + off and B + off + size <= total):
        return False
    if f.type_id == T.DECIMAL:
        return size == 16
    if f.type_id == T.STRUCT:
        return size % 8 == 0 and size >= header_size(len(f.children))
    if f.type_id in (T.LIST, T.MAP):
        return size % 8 == 0 and size >= 8
    return True


def select_row(rows, offs, n, fields, sel, r):
    """(bytes of output row r, whether the row is reported)."""
    total = int(offs[n])
    nf, ns = len(fields), len(sel)
    bm, bm2 = ((nf + 63) // 64) * 8, ((ns + 63) // 64) * 8
    F, F2 = bm + 8 * nf, bm2 + 8 * ns
    u64 = lambda p: int.from_bytes(rows[p:p + 8].tobytes(), "little")   # noqa: E731

    def all_null():
        head = bytearray(F2)
        for j in range(ns):
            head[j >> 3] |= 1 << (j & 7)
        return bytes(head)

    B = int(offs[r])
    if B % 8 or not (0 <= B and B + F <= total) or int(offs[r + 1]) - B < F:
        return all_null(), True
    head, tail, W, bad = bytearray(F2), bytearray(), F2, False
    for j, k in enumerate(sel):
        f = fields[k]
        null = bool((u64(B + 8 * (k >> 6)) >> (k & 63)) & 1)
        slot = 0
        if not null:
            s = u64(B + bm + 8 * k)
            w = T.type_width(f.type_id)
            if f.type_id == T.BOOL:
                slot = 1 if s & 0xFF else 0
            elif w > 0:
                slot = s & ((1 << (8 * w)) - 1)
            else:
                off, size = _i32(s >> 32), _i32(s)
                if not _value_ok(f, off, size, B, total):
                    null = bad = True
                else:
                    slot = (W << 32) | size
                    tail += rows[B + off:B + off + size].tobytes() + bytes(-size % 8)
                    W += size + (-size % 8)
                    if W > INT32_MAX - 7:
                        return all_null(), True
        if null:
            head[j >> 3] |= 1 << (j & 7)
            slot = 0
        head[bm2 + 8 * j:bm2 + 8 * j + 8] = slot.to_bytes(8, "little")
    assert W == F2 + len(tail)
    return bytes(head) + bytes(tail), bad


def expect_select(rows, offs, n, fields, sel) -> Want:
    """The batch fury_row_select produces for the slot indices ``sel`` of the rows at ``offs`` (n + 1
    entries, also for a fixed-width schema), computed from the source bytes alone."""
    w = Want()
    parts, w.bad = [], []
    for r in range(n):
        b, bad = select_row(rows, offs, n, fields, sel, r)
        parts.append(b)
        if bad:
            w.bad.append(r)
    w.data = np.frombuffer(b"".join(parts), np.uint8).copy()
    w.offs = np.zeros(n + 1, np.int64)
    np.cumsum([len(p) for p in parts], out=w.offs[1:])
    return w


# -- the model against the oracle --------------------------------------------------------------------
N = 65


def host_columns(name, n):
    """Host columns of one of the named schemas: the generator where it has one, else beans."""
    fields = SCHEMAS[name]
    if name == "foo":
        from fury_amd.beans import beans_to_columns
        return beans_to_columns(fields, [
            {"f1": i, "f2": None if i % 3 == 0 else f"s{i}" * (i % 5),
             "f3": [f"x{j}" for j in range(i % 4)],
             "f4": [(f"k{j}", j) for j in range(i % 3)] if i % 5 else None,
             "f5": None if i % 7 == 0 else {"f1": i, "f2": "b" * (i % 11)}} for i in range(n)])
    if name == "beana":
        from fury_amd.beans import beans_to_columns
        from tests.test_reference_beans import beana_batch
        return beans_to_columns(*beana_batch(n))
    return gen_columns(name, fields, n, seed=3)


def selections(fields, one):
    nf = len(fields)
    return {"one": [[f.name for f in fields].index(one)], "half": list(range(nf - 1, -1, -2)),
            "all": list(range(nf))}


ONE = {"struct100": "f37", "mixed": "s2", "narrow": "h_dec", "foo": "f4", "beana": "f16"}


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    return O


@pytest.mark.parametrize("name", list(ONE))
def test_model_equals_the_oracle(oracle, name):
    fields = SCHEMAS[name]
    cols = host_columns(name, N)
    rows, offs = oracle.encode(fields, cols, N)
    rows, offs = np.asarray(rows, np.uint8), np.asarray(offs, np.int64)
    for what, sel in selections(fields, ONE[name]).items():
        want, want_offs = oracle.encode([fields[k] for k in sel], [cols[k] for k in sel], N)
        got = expect_select(rows, offs, N, fields, sel)
        assert not got.bad, (name, what)
        assert np.array_equal(got.offs, np.asarray(want_offs, np.int64)), (name, what)
        assert np.array_equal(got.data, np.asarray(want, np.uint8)), (name, what)
        if what == "all":
            assert np.array_equal(got.data, rows), name


def test_model_normalises_and_rejects():
    """The rules the oracle's own rows never exercise, on a two-field row written by hand."""
    fields = [T.field("b", T.BOOL), T.field("s", T.STRING), T.field("i", T.INT32)]
    row = bytearray(8 + 24 + 8)
    row[8] = 2                                                   # BOOL byte 2
    row[16:24] = ((32 << 32) | 3).to_bytes(8, "little")          # "abc" at 32
    row[24:32] = (0xDEADBEEF_00000007).to_bytes(8, "little")     # INT32 7 under stale upper bytes
    row[32:40] = b"abc\xff\xff\xff\xff\xff"                      # non-zero padding
    rows = np.frombuffer(bytes(row) * 2, np.uint8).copy()
    offs = np.array([0, 40, 80], np.int64)
    got = expect_select(rows, offs, 2, fields, [2, 1, 0])
    one = bytes(8) + (7).to_bytes(8, "little") + ((32 << 32) | 3).to_bytes(8, "little") + \
        (1).to_bytes(8, "little") + b"abc" + bytes(5)
    assert got.data.tobytes() == one * 2 and not got.bad and list(got.offs) == [0, 40, 80]
    rows[40 + 16 + 4] = 36                                       # row 1: off 36, off % 8 == 4
    got = expect_select(rows, offs, 2, fields, [1])
    assert got.bad == [1] and got.data.tobytes()[24:] == (1).to_bytes(8, "little") + bytes(8)
    offs[1] = 44                                                 # row 1 starts off an 8-byte boundary
    got = expect_select(rows, offs, 2, fields, [0, 2])
    assert got.bad == [1] and got.data.tobytes()[24:] == (3).to_bytes(8, "little") + bytes(16)
