"""CPU checks of fury_row_compare and fury_row_order_words: the symbols are bound and exported, the
header carries the six numbered rules and both flag macros, and every argument error is reported on the
host, before any device work, with its status and a message that names the function.  Host buffers
stand in for device memory and are never dereferenced: every call fails first, or has nothing to do."""
from __future__ import annotations

import ctypes

import pytest

from fury_amd.workloads import SCHEMAS
from tests.test_keys_equal_abi import _buf, _keys, _side

OK, INVALID, UNSUPPORTED = 0, 1, 2
DESC, NULLS_LAST = 1, 2


@pytest.fixture(scope="module")
def L():
    from fury_amd import _native as N
    return N.lib()


@pytest.fixture(scope="module")
def schemas():
    from fury_amd import types as T
    from fury_amd.encoder import Encoders, Schema
    arr = Encoders.array_encoder(T.field("item", T.INT64), device="cpu")
    return {"struct100": Schema(SCHEMAS["struct100"]), "mixed": Schema(SCHEMAS["mixed"]),
            "foo": Schema(SCHEMAS["foo"]), "narrow": Schema(SCHEMAS["narrow"]),
            "array": arr.schema(), "_keep": arr}


def _err(fn):
    from fury_amd import _native as N
    msg = N.last_error()
    assert msg.startswith(fn), msg
    return msg


def _flags(*f):
    return (ctypes.c_int32 * max(len(f), 1))(*f)


def test_symbols_rules_and_macros(L):
    import fury_amd
    from fury_amd import _native as N
    assert len(N.SIGNATURES["fury_row_compare"][1]) == 7
    assert len(N.SIGNATURES["fury_row_order_words"][1]) == 12
    assert hasattr(L, "fury_row_compare") and hasattr(L, "fury_row_order_words")
    assert L.fury_abi_version() == 1
    assert (N.ORDER_DESC, N.ORDER_NULLS_LAST) == (DESC, NULLS_LAST)
    with open(N.HERE + "/../include/fury_row.h") as f:
        header = f.read()
    assert "#define FURY_ORDER_DESC 1" in header and "#define FURY_ORDER_NULLS_LAST 2" in header
    for rule in ("1. Keys.", "2. Nulls.", "3. Value order, ascending.", "4. Direction.", "5. Consistency.",
                 "6. Bounds"):
        assert rule in header, rule
    assert "code-point order" in header and "String.compareTo" in header
    for name in ("compare_into", "bind_compare", "compare_rows", "order_words_into", "order_words",
                 "argsort_rows", "sort_rows", "is_sorted", "search_sorted"):
        assert name in fury_amd.__all__ and callable(getattr(fury_amd, name)), name
    from fury_amd.encoder import RowEncoder
    assert not hasattr(RowEncoder, "argsort_rows")


def test_compare_argument_errors(L, schemas):
    fixed, var = schemas["struct100"].handle, schemas["mixed"].handle
    r1, rows = _buf()
    r2, out = _buf()
    r3, aux = _buf()
    fn = "fury_row_compare"

    def call(left=None, right=None, nk=1, kf=None, pairs=4, oc=out, **kw):
        left = _side(fixed, _keys(0), rows, **kw) if left is None else left
        right = _side(fixed, _keys(2), rows) if right is None else right
        return L.fury_row_compare(left if left != "null" else None, right if right != "null" else None, nk,
                                  kf, pairs, oc, None)

    def both(make):
        res = []
        for name in ("left", "right"):
            st = call(**{name: make()})
            res.append((st, _err(fn)))
            assert name in res[-1][1], res[-1]
        return res

    assert call(left="null") == INVALID
    assert "left is null" in _err(fn)
    assert call(right="null") == INVALID
    assert "right is null" in _err(fn)
    for st, msg in both(lambda: _side(None, _keys(0), rows)):
        assert st == INVALID and "schema is null" in msg
    for st, msg in both(lambda: _side(schemas["array"].handle, _keys(0), rows)):
        assert st == UNSUPPORTED and "collection schema" in msg
    # the key count and the key fields: as fury_row_keys_equal
    assert call(nk=0) == INVALID
    assert "num_selected <= 0" in _err(fn)
    many = _keys(*range(65))
    assert call(left=_side(fixed, many, rows), right=_side(fixed, many, rows), nk=65) == UNSUPPORTED
    assert "at most 64 fields" in _err(fn)
    for st, msg in both(lambda: _side(fixed, None, rows)):
        assert st == INVALID and "fields is null" in msg
    for st, msg in both(lambda: _side(fixed, _keys(100), rows)):
        assert st == INVALID and "fields[0] = 100 is not a field" in msg
    assert call(left=_side(fixed, _keys(3, 5, 3), rows), right=_side(fixed, _keys(1, 2, 3), rows), nk=3) == INVALID
    assert "left" in _err(fn) and "selected twice" in _err(fn)
    assert call(left=_side(fixed, _keys(1, 2, 3), rows), right=_side(fixed, _keys(3, 5, 3), rows), nk=3) == INVALID
    assert "right" in _err(fn) and "selected twice" in _err(fn)
    foo = schemas["foo"].handle
    for k, name in ((2, "f3"), (3, "f4"), (4, "f5")):
        for st, msg in both(lambda: _side(foo, _keys(k), rows, aux)):
            assert st == UNSUPPORTED and f"field {k} ({name})" in msg and "LIST / STRUCT / MAP" in msg
    k = [f.name for f in SCHEMAS["narrow"]].index("k_ints")
    for st, msg in both(lambda: _side(schemas["narrow"].handle, _keys(k), rows, aux)):
        assert st == UNSUPPORTED and "k_ints" in msg
    # the type ids of a key position agree
    names = [f.name for f in SCHEMAS["mixed"]]
    a, b, s1 = names.index("a"), names.index("b"), names.index("s1")
    assert call(left=_side(var, _keys(b, a), rows, aux), right=_side(var, _keys(b, s1), rows, aux), nk=2) == INVALID
    msg = _err(fn)
    assert "key 1" in msg and f"left field {a} (a)" in msg and f"right field {s1} (s1)" in msg
    # the flags: one entry per key, only the two known bits
    for bad in (4, 7, -1, 1 << 30):
        assert call(kf=_flags(bad)) == INVALID
        assert "key 0" in _err(fn) and "unknown flags" in _err(fn)
    assert call(left=_side(fixed, _keys(0, 1), rows), right=_side(fixed, _keys(2, 3), rows), nk=2,
                kf=_flags(3, 8)) == INVALID
    assert "key 1" in _err(fn)
    # the counts, the output, the batches
    assert call(pairs=-1) == INVALID
    assert "num_pairs < 0" in _err(fn)
    for st, msg in both(lambda: _side(fixed, _keys(0), rows, n=-1)):
        assert st == INVALID and "nrows < 0" in msg
    for st, msg in both(lambda: _side(fixed, _keys(0), rows, n=3)):
        assert st == INVALID and "nrows 3 < num_pairs 4" in msg
    assert call(oc=None) == INVALID
    assert "out_cmp is null" in _err(fn)
    assert call(oc=None, pairs=0) == INVALID                     # even when empty
    for st, msg in both(lambda: _side(fixed, _keys(0), None)):
        assert st == INVALID and "rows is null" in msg
    for st, msg in both(lambda: _side(fixed, _keys(0), rows + 4)):
        assert st == INVALID and "rows must be 8-byte aligned" in msg
    for st, msg in both(lambda: _side(var, _keys(b), rows, None)):
        assert st == INVALID and "variable-length rows need row_offsets" in msg
    for st, msg in both(lambda: _side(var, _keys(b), rows, aux + 4)):
        assert st == INVALID and "8-byte aligned" in msg and "row_offsets" in msg
    for st, msg in both(lambda: _side(fixed, _keys(0), rows, idx=aux + 4)):
        assert st == INVALID and "8-byte aligned" in msg and "indices" in msg
    big = 2 ** 31 * 256
    assert call(left=_side(fixed, _keys(0), rows, n=big), right=_side(fixed, _keys(2), rows, n=big),
                pairs=big) == INVALID
    assert "batch too large" in _err(fn)


def test_order_words_argument_errors(L, schemas):
    fixed, var = schemas["struct100"].handle, schemas["mixed"].handle
    r1, rows = _buf()
    r2, out = _buf()
    r3, aux = _buf()
    fn = "fury_row_order_words"
    names = [f.name for f in SCHEMAS["mixed"]]
    b = names.index("b")

    def call(schema=fixed, field=0, flags=0, chunk=0, rows=rows, ro=None, n=4, idx=None, num=4, ow=out, om=None):
        return L.fury_row_order_words(schema, field, flags, chunk, rows, ro, n, idx, num, ow, om, None)

    assert call(schema=None) == INVALID
    assert "schema is null" in _err(fn)
    assert call(schema=schemas["array"].handle) == UNSUPPORTED
    assert "collection schema" in _err(fn)
    for field in (-1, 100):
        assert call(field=field) == INVALID
        assert f"fields[0] = {field} is not a field" in _err(fn)
    assert call(schema=schemas["foo"].handle, field=2, ro=aux) == UNSUPPORTED
    assert "field 2 (f3)" in _err(fn) and "LIST / STRUCT / MAP" in _err(fn)
    for flags in (4, -1, 1 << 20):
        assert call(flags=flags) == INVALID
        assert "unknown flags" in _err(fn)
    assert call(chunk=-1) == INVALID
    assert "chunk < 0" in _err(fn)
    assert call(n=-1) == INVALID
    assert "nrows < 0" in _err(fn)
    assert call(num=-1) == INVALID
    assert "num_out < 0" in _err(fn)
    assert call(num=5) == INVALID
    assert "nrows 4 < num_out 5" in _err(fn)
    assert call(ow=None) == INVALID
    assert "out_words is null" in _err(fn)
    assert call(ow=None, num=0) == INVALID                        # even when empty
    assert call(ow=out + 4) == INVALID
    assert "8-byte aligned" in _err(fn) and "out_words" in _err(fn)
    assert call(idx=aux + 4) == INVALID
    assert "8-byte aligned" in _err(fn) and "indices" in _err(fn)
    assert call(om=aux + 2) == INVALID
    assert "out_more must be 4-byte aligned" in _err(fn)
    assert call(rows=None) == INVALID
    assert "rows is null" in _err(fn)
    assert call(rows=rows + 4) == INVALID
    assert "rows must be 8-byte aligned" in _err(fn)
    assert call(schema=var, field=b) == INVALID
    assert "variable-length rows need row_offsets" in _err(fn)
    assert call(schema=var, field=b, ro=aux + 4) == INVALID
    assert "row_offsets" in _err(fn)
    assert call(idx=aux, num=2 ** 62) == INVALID
    assert "batch too large" in _err(fn)


def test_nothing_to_do_is_a_no_op(L, schemas):
    """Zero pairs, zero outputs and zero rows return FURY_OK without touching a buffer."""
    fixed, var = schemas["struct100"].handle, schemas["mixed"].handle
    raw, out = _buf(64)
    ctypes.memset(out, 0xAB, 64)
    s1 = [f.name for f in SCHEMAS["mixed"]].index("s1")
    for kf in (None, _flags(DESC | NULLS_LAST, DESC)):
        assert L.fury_row_compare(_side(fixed, _keys(0, 99), None, n=0), _side(fixed, _keys(2, 97), None, n=0),
                                  2, kf, 0, out, None) == OK
        assert L.fury_row_compare(_side(var, _keys(s1, 0), None, n=0), _side(var, _keys(s1, 0), None, n=7),
                                  2, kf, 0, out, None) == OK
    for flags in (0, DESC, NULLS_LAST, 3):
        assert L.fury_row_order_words(fixed, 5, flags, 0, None, None, 0, None, 0, out, None, None) == OK
        assert L.fury_row_order_words(var, s1, flags, 7, None, None, 9, None, 0, out, None, None) == OK
    assert ctypes.string_at(out, 64) == b"\xab" * 64


def test_python_surface_checks_before_any_device_work():
    import torch
    from fury_amd import (KeySide, argsort_rows, compare_into, is_sorted, order_words_into, search_sorted)
    from fury_amd.encoder import (ClassNotCompatibleException, Encoders, IllegalArgumentException, RowBatch)
    from fury_amd import types as T
    enc = Encoders.bean(SCHEMAS["mixed"], device="cpu")

    def batch(n):
        return RowBatch(torch.zeros(64, dtype=torch.uint8), torch.zeros(n + 1, dtype=torch.int64), n,
                        enc.schema_hash)
    four, five = batch(4), batch(5)
    out = torch.zeros(8, dtype=torch.int8)
    with pytest.raises(IllegalArgumentException, match="4 rows against 5"):
        compare_into(KeySide(enc, four, ["a"]), KeySide(enc, five, ["a"]), out)
    with pytest.raises(IllegalArgumentException, match="2 left keys against 1"):
        compare_into(KeySide(enc, four, ["a", "b"]), KeySide(enc, four, ["a"]), out)
    with pytest.raises(IllegalArgumentException, match="int8"):
        compare_into(KeySide(enc, four, ["a"]), KeySide(enc, four, ["a"]), out.to(torch.uint8))
    with pytest.raises(IllegalArgumentException, match="3 entries for 4 pairs"):
        compare_into(KeySide(enc, four, ["a"]), KeySide(enc, four, ["a"]), out[:3])
    with pytest.raises(IllegalArgumentException, match="2 entries for 1 keys"):
        compare_into(KeySide(enc, four, ["a"]), KeySide(enc, four, ["a"]), out, descending=[True, False])
    words = torch.zeros(8, dtype=torch.int64)
    with pytest.raises(IllegalArgumentException, match="no field named"):
        order_words_into(enc, four, "nope", 0, words)
    with pytest.raises(IllegalArgumentException, match="int64 tensor"):
        order_words_into(enc, four, "a", 0, words.to(torch.int32))
    with pytest.raises(IllegalArgumentException, match="3 entries for 4 rows"):
        order_words_into(enc, four, "a", 0, words[:3])
    with pytest.raises(IllegalArgumentException, match="out_more"):
        order_words_into(enc, four, "a", 0, words, torch.zeros(1, dtype=torch.int64))
    other = Encoders.bean([T.field("x", T.INT64)], device="cpu")
    with pytest.raises(ClassNotCompatibleException):
        argsort_rows(other, four, ["x"])
    with pytest.raises(IllegalArgumentException, match="indices must be None"):
        search_sorted(KeySide(enc, four, ["a"], torch.zeros(2, dtype=torch.int64)), KeySide(enc, four, ["a"]))
    # nothing to sort, nothing to search: no launch (there is no GPU here)
    assert argsort_rows(enc, batch(0), ["a"]).tolist() == []
    assert argsort_rows(enc, batch(1), ["a", "s1"], descending=[True, False]).tolist() == [0]
    assert is_sorted(enc, batch(1), ["a"]) is True
    assert search_sorted(KeySide(enc, batch(0), ["a"]), KeySide(enc, four, ["a"])).tolist() == [0, 0, 0, 0]
    assert search_sorted(KeySide(enc, four, ["a"]), KeySide(enc, batch(0), ["a"])).tolist() == []
