"""CPU checks of fury_row_keys_equal: the symbol is bound and exported, the header carries the six
numbered rules, and every argument error is reported on the host, before any device work, with its
status and a message that names the function.  Host buffers stand in for device memory and are
never dereferenced: every call fails first, or has no pairs."""
from __future__ import annotations

import ctypes

import pytest

from fury_amd.workloads import SCHEMAS

OK, INVALID, UNSUPPORTED = 0, 1, 2
NULL_EQUAL = 1


def _buf(nbytes=8192, align=64):
    raw = ctypes.create_string_buffer(nbytes + align)
    base = (ctypes.addressof(raw) + align - 1) & ~(align - 1)
    return raw, base


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


def _err():
    from fury_amd import _native as N
    msg = N.last_error()
    assert msg.startswith("fury_row_keys_equal"), msg
    return msg


def _keys(*idx):
    return (ctypes.c_int32 * max(len(idx), 1))(*idx)


def _side(schema, keys, rows, ro=None, n=4, idx=None):
    from fury_amd import _native as N
    s = N.FuryKeySide()
    s.schema, s.fields, s.rows, s.row_offsets, s.nrows, s.indices = schema, keys, rows, ro, n, idx
    s.keep = keys
    return s


def test_symbol_rules_and_version(L):
    from fury_amd import _native as N
    assert "fury_row_keys_equal" in N.SIGNATURES and len(N.SIGNATURES["fury_row_keys_equal"][1]) == 8
    assert hasattr(L, "fury_row_keys_equal")
    assert L.fury_abi_version() == 1
    assert N.KEYS_NULL_EQUAL == NULL_EQUAL
    with open(N.HERE + "/../include/fury_row.h") as f:
        header = f.read()
    assert "#define FURY_KEYS_NULL_EQUAL 1" in header and "typedef struct fury_key_side" in header
    for rule in ("1. Pairs.", "2. Key positions.", "3. Outputs.", "4. Consequence.", "5. Bounds",
                 "6. Key types"):
        assert rule in header, rule
    assert ctypes.sizeof(N.FuryKeySide) == 48


def test_argument_errors(L, schemas):
    fixed, var = schemas["struct100"].handle, schemas["mixed"].handle
    r1, rows = _buf()
    r2, out = _buf()
    r3, aux = _buf()

    def call(left=None, right=None, nk=1, pairs=4, flags=0, oe=out, om=aux, **kw):
        left = _side(fixed, _keys(0), rows, **kw) if left is None else left
        right = _side(fixed, _keys(2), rows) if right is None else right
        return L.fury_row_keys_equal(left if left != "null" else None,
                                     right if right != "null" else None, nk, pairs, flags, oe, om, None)

    def both(make):
        """The same mistake on the left and on the right: (status, message) of each."""
        res = []
        for name in ("left", "right"):
            st = call(**{name: make()})
            res.append((st, _err()))
            assert name in res[-1][1], res[-1]
        return res

    # the sides and their schemas
    assert call(left="null") == INVALID
    assert "left is null" in _err()
    assert call(right="null") == INVALID
    assert "right is null" in _err()
    for st, msg in both(lambda: _side(None, _keys(0), rows)):
        assert st == INVALID and "schema is null" in msg
    for st, msg in both(lambda: _side(schemas["array"].handle, _keys(0), rows)):
        assert st == UNSUPPORTED and "collection schema" in msg
    # the key count and the key fields: as fury_row_hash
    assert call(nk=0) == INVALID
    assert "num_selected <= 0" in _err()
    assert call(nk=-3) == INVALID
    _err()
    many = _keys(*range(65))
    assert call(left=_side(fixed, many, rows), right=_side(fixed, many, rows), nk=65) == UNSUPPORTED
    assert "at most 64 fields" in _err()
    for st, msg in both(lambda: _side(fixed, None, rows)):
        assert st == INVALID and "fields is null" in msg
    for st, msg in both(lambda: _side(fixed, _keys(100), rows)):
        assert st == INVALID and "fields[0] = 100 is not a field" in msg
    assert call(left=_side(fixed, _keys(0, -1), rows), right=_side(fixed, _keys(0, 1), rows), nk=2) == INVALID
    assert "fields[1] = -1" in _err()
    assert call(left=_side(fixed, _keys(3, 5, 3), rows), right=_side(fixed, _keys(1, 2, 3), rows),
                nk=3) == INVALID
    assert "left" in _err() and "selected twice" in _err()
    assert call(left=_side(fixed, _keys(1, 2, 3), rows), right=_side(fixed, _keys(3, 5, 3), rows),
                nk=3) == INVALID
    assert "right" in _err() and "selected twice" in _err()
    # nested keys and lists: not canonical bytes (hash rule 5)
    foo = schemas["foo"].handle
    for k, name in ((2, "f3"), (3, "f4"), (4, "f5")):
        for st, msg in both(lambda: _side(foo, _keys(k), rows, aux)):
            assert st == UNSUPPORTED and f"field {k} ({name})" in msg and "LIST / STRUCT / MAP" in msg
    k = [f.name for f in SCHEMAS["narrow"]].index("k_ints")
    for st, msg in both(lambda: _side(schemas["narrow"].handle, _keys(k), rows, aux)):
        assert st == UNSUPPORTED and "k_ints" in msg
    # rule 6: the type ids of a key position agree; mixed is a INT32, b INT64, c FLOAT64, s1.. STRING
    names = [f.name for f in SCHEMAS["mixed"]]
    a, b, s1 = names.index("a"), names.index("b"), names.index("s1")
    assert call(left=_side(var, _keys(b, a), rows, aux), right=_side(var, _keys(b, s1), rows, aux),
                nk=2) == INVALID
    msg = _err()
    assert "key 1" in msg and f"left field {a} (a)" in msg and f"right field {s1} (s1)" in msg
    assert call(left=_side(var, _keys(a), rows, aux), right=_side(var, _keys(b), rows, aux)) == INVALID
    assert "key 0" in _err()
    # the counts
    assert call(pairs=-1) == INVALID
    assert "num_pairs < 0" in _err()
    for st, msg in both(lambda: _side(fixed, _keys(0), rows, n=-1)):
        assert st == INVALID and "nrows < 0" in msg
    for st, msg in both(lambda: _side(fixed, _keys(0), rows, n=3)):
        assert st == INVALID and "nrows 3 < num_pairs 4" in msg
    # the flags and the outputs
    for flags in (2, 3, -1, 1 << 30):
        assert call(flags=flags) == INVALID
        assert "flags" in _err()
    assert call(oe=None, om=None) == INVALID
    assert "both null" in _err()
    assert call(oe=None, om=None, pairs=0) == INVALID          # even when empty
    assert call(om=aux + 2) == INVALID
    assert "out_mask must be 4-byte aligned" in _err()
    # the batches
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
    # a pair count the grid cannot index
    big = 2 ** 31 * 256
    assert call(left=_side(fixed, _keys(0), rows, n=big), right=_side(fixed, _keys(2), rows, n=big),
                pairs=big) == INVALID
    assert "batch too large" in _err()
    assert call(left=_side(fixed, _keys(0), rows, idx=aux), right=_side(fixed, _keys(2), rows, idx=aux),
                pairs=2 ** 62) == INVALID
    assert "batch too large" in _err()


def test_no_pairs_is_a_no_op(L, schemas):
    """num_pairs == 0 returns FURY_OK without touching a buffer: rows, row_offsets and indices may be
    NULL, and the outputs keep their contents."""
    fixed, var = schemas["struct100"].handle, schemas["mixed"].handle
    raw, out = _buf(64)
    ctypes.memset(out, 0xAB, 64)
    names = [f.name for f in SCHEMAS["mixed"]]
    s1 = names.index("s1")
    for flags in (0, NULL_EQUAL):
        assert L.fury_row_keys_equal(_side(fixed, _keys(0, 99), None, n=0), _side(fixed, _keys(2, 97), None, n=0),
                                     2, 0, flags, out, out + 32, None) == OK
        assert L.fury_row_keys_equal(_side(var, _keys(s1), None, n=0), _side(var, _keys(s1), None, n=7),
                                     1, 0, flags, out, None, None) == OK
        assert L.fury_row_keys_equal(_side(var, _keys(s1), None, n=5), _side(var, _keys(s1), None, n=0),
                                     1, 0, flags, None, out, None) == OK
    assert ctypes.string_at(out, 64) == b"\xab" * 64


def test_python_surface_checks_before_any_device_work():
    import torch
    from fury_amd import KeySide, candidate_pairs, join_pairs, keys_equal, keys_equal_into  # noqa: F401
    from fury_amd import types as T
    from fury_amd.encoder import (ClassNotCompatibleException, Encoders, IllegalArgumentException,
                                  RowBatch)
    enc = Encoders.bean(SCHEMAS["mixed"], device="cpu")

    def batch(n):
        return RowBatch(torch.zeros(64, dtype=torch.uint8), torch.zeros(n + 1, dtype=torch.int64), n,
                        enc.schema_hash)
    four, five = batch(4), batch(5)
    out = torch.zeros(8, dtype=torch.uint8)
    with pytest.raises(IllegalArgumentException, match="4 rows against 5"):
        keys_equal_into(KeySide(enc, four, ["a"]), KeySide(enc, five, ["a"]), out)
    idx = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(IllegalArgumentException, match="3 entries, right.indices has 2"):
        keys_equal_into(KeySide(enc, four, ["a"], idx), KeySide(enc, five, ["a"], idx[:2]), out)
    with pytest.raises(IllegalArgumentException, match="int64"):
        keys_equal_into(KeySide(enc, four, ["a"], idx.to(torch.int32)), KeySide(enc, five, ["a"]), out)
    with pytest.raises(IllegalArgumentException, match="no field named"):
        keys_equal_into(KeySide(enc, four, ["nope"]), KeySide(enc, four, ["a"]), out)
    with pytest.raises(IllegalArgumentException, match="2 left keys against 1"):
        keys_equal_into(KeySide(enc, four, ["a", "b"]), KeySide(enc, four, ["a"]), out)
    with pytest.raises(IllegalArgumentException, match="uint8 or bool"):
        keys_equal_into(KeySide(enc, four, ["a"]), KeySide(enc, four, ["a"]), out.to(torch.int32))
    with pytest.raises(IllegalArgumentException, match="3 entries for 4 pairs"):
        keys_equal_into(KeySide(enc, four, ["a"]), KeySide(enc, four, ["a"]), out[:3])
    with pytest.raises(IllegalArgumentException, match="int32 or uint32"):
        keys_equal_into(KeySide(enc, four, ["a"]), KeySide(enc, four, ["a"]), None, out)
    with pytest.raises(IllegalArgumentException, match="0 words for 4 pairs"):
        keys_equal_into(KeySide(enc, four, ["a"]), KeySide(enc, four, ["a"]), None,
                        torch.zeros(0, dtype=torch.int32))
    other = Encoders.bean([T.field("x", T.INT64)], device="cpu")
    with pytest.raises(ClassNotCompatibleException):
        keys_equal_into(KeySide(other, four, ["x"]), KeySide(enc, four, ["b"]), out)
    with pytest.raises(IllegalArgumentException, match="indices must be None"):
        join_pairs(KeySide(enc, four, ["a"], idx), KeySide(enc, four, ["a"]))
    # an empty side joins to nothing and launches nothing (there is no GPU here)
    li, ri = join_pairs(KeySide(enc, batch(0), ["a"]), KeySide(enc, four, ["a"]))
    assert li.numel() == 0 and ri.numel() == 0 and li.dtype == torch.int64
