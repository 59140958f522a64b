"""CPU checks of the projected decode's C ABI (fury_row_project / fury_row_project_measure): every
argument error is reported on the host, before any device work, with the status of the reference's
exception type and a message that names the field."""
from __future__ import annotations

import ctypes

import pytest

from fury_amd import types as T
from fury_amd.workloads import SCHEMAS

INVALID, UNSUPPORTED = 1, 2


def _sel(*idx):
    return (ctypes.c_int32 * max(len(idx), 1))(*idx), len(idx)


def _buf(nbytes=4096, align=64):
    """A host buffer standing in for device memory (never dereferenced: every call fails first)."""
    raw = ctypes.create_string_buffer(nbytes + align)
    base = (ctypes.addressof(raw) + align - 1) & ~(align - 1)
    return raw, base


@pytest.fixture(scope="module")
def L():
    from fury_amd import _native as N
    return N.lib()


@pytest.fixture(scope="module")
def schemas():
    from fury_amd.encoder import Encoders, Schema
    arr = Encoders.array_encoder(T.field("item", T.INT64), device="cpu")
    return {"struct100": Schema(SCHEMAS["struct100"]), "foo": Schema(SCHEMAS["foo"]),
            "narrow": Schema(SCHEMAS["narrow"]), "mixed": Schema(SCHEMAS["mixed"]),
            "array": arr.schema(), "_keep": arr}


def _both(L, s, sel, nsel, rows, offs, n, cols, arrow=0):
    """Status of fury_row_project and of fury_row_project_measure for the same arguments."""
    return (L.fury_row_project(s, sel, nsel, rows, offs, n, cols, arrow, None),
            L.fury_row_project_measure(s, sel, nsel, rows, offs, n, cols, None))


def test_symbols_are_bound(L):
    from fury_amd import _native as N
    assert "fury_row_project" in N.SIGNATURES and "fury_row_project_measure" in N.SIGNATURES
    assert hasattr(L, "fury_row_project") and hasattr(L, "fury_row_project_measure")


def test_invalid_arguments(L, schemas):
    from fury_amd import _native as N
    s = schemas["struct100"].handle
    raw, rows = _buf()
    cols = (N.FuryColumn * 4)()
    sel, k = _sel(0, 99)
    assert _both(L, None, sel, k, rows, None, 4, cols) == (INVALID, INVALID)       # null schema
    assert "schema is null" in N.last_error()
    assert _both(L, s, sel, k, rows, None, -1, cols) == (INVALID, INVALID)         # nrows < 0
    assert _both(L, s, sel, 0, rows, None, 4, cols) == (INVALID, INVALID)          # nothing selected
    assert _both(L, s, sel, -3, rows, None, 4, cols) == (INVALID, INVALID)
    assert _both(L, s, None, k, rows, None, 4, cols) == (INVALID, INVALID)         # null fields
    assert "fields is null" in N.last_error()
    assert _both(L, s, sel, k, rows, None, 4, None) == (INVALID, INVALID)          # null columns
    assert "columns is null" in N.last_error()
    for bad in ((0, 100), (-1, 5), (7, 7), (3, 50, 3)):
        sb, kb = _sel(*bad)
        assert _both(L, s, sb, kb, rows, None, 4, cols) == (INVALID, INVALID), bad
    sd, kd = _sel(7, 7)
    L.fury_row_project(s, sd, kd, rows, None, 4, cols, 0, None)
    assert "f07" in N.last_error() and "twice" in N.last_error()


def test_unsupported_selections(L, schemas):
    from fury_amd import _native as N
    raw, rows = _buf()
    cols = (N.FuryColumn * 70)()
    foo = schemas["foo"].handle                      # f1 int32, f2 string, f3 list<string>, f4 map, f5 struct
    for k, name in ((2, "f3"), (3, "f4"), (4, "f5")):
        sel, m = _sel(0, k)
        assert _both(L, foo, sel, m, rows, rows, 4, cols) == (UNSUPPORTED, UNSUPPORTED)
        msg = N.last_error()
        assert f"({name})" in msg and "fury_decode_prepare" in msg, msg
    # a collection schema has no row fields
    sel, m = _sel(0)
    assert _both(L, schemas["array"].handle, sel, m, rows, rows, 4, cols) == (UNSUPPORTED, UNSUPPORTED)
    # more fields than the argument-block table: the message names the full decode
    sel, m = _sel(*range(65))
    assert _both(L, schemas["struct100"].handle, sel, m, rows, None, 4, cols) == (UNSUPPORTED, UNSUPPORTED)
    assert "fury_row_decode" in N.last_error()
    sel, m = _sel(*range(64))                        # 64 are accepted (and fail later: no buffers)
    assert L.fury_row_project(schemas["struct100"].handle, sel, m, rows, None, 4, cols, 0, None) == INVALID
    assert "values is null" in N.last_error()


def test_column_checks_use_the_decode_wording(L, schemas):
    from fury_amd import _native as N
    raw, rows = _buf()
    raw2, out = _buf()
    nar = schemas["narrow"].handle
    names = [f.name for f in SCHEMAS["narrow"]]
    ix = {n: i for i, n in enumerate(names)}

    def cols_for(*kinds):
        c = (N.FuryColumn * len(kinds))()
        for j, kind in enumerate(kinds):
            if kind == "fixed":
                c[j].values = out
            elif kind == "bytes":
                c[j].offsets = out
            elif kind == "list":
                c[j].offsets = out
        return c

    # null values / offsets / list child
    sel, m = _sel(ix["d_int"])
    c = (N.FuryColumn * 1)()
    assert L.fury_row_project(nar, sel, m, rows, rows, 4, c, 0, None) == INVALID
    assert "(d_int): values is null" in N.last_error()
    sel, m = _sel(ix["h_dec"])
    assert L.fury_row_project(nar, sel, m, rows, rows, 4, c, 0, None) == INVALID
    assert "(h_dec): values is null" in N.last_error()
    sel, m = _sel(ix["i_bin"])
    assert _both(L, nar, sel, m, rows, rows, 4, c) == (INVALID, INVALID)
    assert "(i_bin): offsets is null" in N.last_error()
    sel, m = _sel(ix["k_ints"])
    assert _both(L, nar, sel, m, rows, rows, 4, c) == (INVALID, INVALID)
    assert "(k_ints): offsets is null" in N.last_error()
    c = cols_for("list")
    assert L.fury_row_project(nar, sel, m, rows, rows, 4, c, 0, None) == INVALID
    assert "(k_ints): list needs a child column" in N.last_error()
    # misalignment: values, validity, element bitmaps
    sel, m = _sel(ix["d_int"])
    c = cols_for("fixed")
    c[0].values = out + 2
    assert L.fury_row_project(nar, sel, m, rows, rows, 4, c, 0, None) == INVALID
    assert "(d_int): values misaligned" in N.last_error()
    c = cols_for("fixed")
    c[0].validity = out + 1
    assert L.fury_row_project(nar, sel, m, rows, rows, 4, c, 0, None) == INVALID
    assert "validity must be 4-byte aligned" in N.last_error()
    sel, m = _sel(ix["k_ints"])
    c = cols_for("list")
    child = (N.FuryColumn * 1)()
    child[0].values = out
    child[0].validity = out + 2
    c[0].child = child
    assert L.fury_row_project(nar, sel, m, rows, rows, 4, c, 0, None) == INVALID
    assert "element bitmaps must be 4-byte aligned" in N.last_error()
    # arrow output needs validity buffers (field and list elements)
    sel, m = _sel(ix["d_int"])
    c = cols_for("fixed")
    assert L.fury_row_project(nar, sel, m, rows, rows, 4, c, 1, None) == INVALID
    assert "(d_int): Arrow output needs a validity buffer" in N.last_error()
    sel, m = _sel(ix["k_ints"])
    c = cols_for("list")
    c[0].validity = out
    child = (N.FuryColumn * 1)()
    child[0].values = out
    c[0].child = child
    assert L.fury_row_project(nar, sel, m, rows, rows, 4, c, 1, None) == INVALID
    assert "Arrow output needs element validity" in N.last_error()
    # rows / row_offsets
    sel, m = _sel(ix["d_int"])
    c = cols_for("fixed")
    assert _both(L, nar, sel, m, None, rows, 4, c) == (INVALID, INVALID)
    assert "rows is null" in N.last_error()
    assert _both(L, nar, sel, m, rows, None, 4, c) == (INVALID, INVALID)           # var rows need offsets
    assert "row_offsets" in N.last_error()
    assert _both(L, nar, sel, m, rows + 4, rows, 4, c) == (INVALID, INVALID)
    assert "8-byte aligned" in N.last_error()


def test_empty_batch_of_fixed_outputs_is_ok(L, schemas):
    """nrows = 0 with no offsets buffers: nothing to launch, nothing to zero."""
    from fury_amd import _native as N
    sel, m = _sel(0, 99)
    cols = (N.FuryColumn * 2)()
    assert _both(L, schemas["struct100"].handle, sel, m, None, None, 0, cols) == (0, 0)


def test_python_select_rejects_unknown_names(schemas):
    from fury_amd.encoder import Encoders, IllegalArgumentException
    enc = Encoders.bean(SCHEMAS["mixed"], device="cpu")
    assert enc._select(["s2", 0, "a"]) == [4, 0, 0]
    with pytest.raises(IllegalArgumentException, match="nope"):
        enc._select(["a", "nope"])
