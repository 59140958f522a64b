"""CPU checks of fury_row_group: the symbol is bound and exported, the header carries the six
numbered rules, and every argument error is reported on the host, before any device work, with its
status and a message that names the function.  Host buffers stand in for device memory and are
never dereferenced: every call fails first, or has no rows and no count to write."""
from __future__ import annotations

import ctypes

import pytest

from fury_amd.workloads import SCHEMAS

OK, INVALID, UNSUPPORTED = 0, 1, 2


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
    assert msg.startswith("fury_row_group"), msg
    return msg


def _keys(*idx):
    return (ctypes.c_int32 * max(len(idx), 1))(*idx)


def test_symbol_and_rules(L):
    from fury_amd import _native as N
    assert "fury_row_group" in N.SIGNATURES and len(N.SIGNATURES["fury_row_group"][1]) == 12
    assert hasattr(L, "fury_row_group")
    assert L.fury_abi_version() == 1
    with open(N.HERE + "/../include/fury_row.h") as f:
        header = f.read()
    assert "int fury_row_group(const fury_schema* schema" in header
    at = header.index("Group ids and distinct rows")
    doc = header[at:header.index("int fury_row_group(", at)]
    for rule in ("1. Groups.", "2. First rows.", "3. Numbering.", "4. Hashes.", "5. Bounds", "6. Key types",
                 "Workspace", "48 bytes per row"):
        assert rule in doc, rule


def test_argument_errors(L, schemas):
    fixed, var = schemas["struct100"].handle, schemas["mixed"].handle
    r1, rows = _buf()
    r2, out = _buf()
    r3, aux = _buf()

    def call(s=fixed, keys=_keys(0), nk=1, rows=rows, ro=None, n=4, hashes=None, first=out, ids=None,
             grows=None, num=None):
        return L.fury_row_group(s, keys, nk, rows, ro, n, hashes, first, ids, grows, num, None)

    # the schema, the key count and the key fields: as fury_row_hash
    assert call(s=None) == INVALID
    assert "schema is null" in _err()
    assert call(s=schemas["array"].handle) == UNSUPPORTED
    assert "collection schema" in _err()
    assert call(nk=0) == INVALID
    assert "num_selected <= 0" in _err()
    assert call(nk=-3) == INVALID
    _err()
    assert call(keys=_keys(*range(65)), nk=65) == UNSUPPORTED
    assert "at most 64 fields" in _err()
    assert call(keys=_keys(*range(64)), nk=64, first=None) == INVALID      # 64 keys pass the selection
    assert "out_first is null" in _err()
    assert call(keys=None) == INVALID
    assert "fields is null" in _err()
    assert call(keys=_keys(100)) == INVALID
    assert "fields[0] = 100 is not a field" in _err()
    assert call(keys=_keys(0, -1), nk=2) == INVALID
    assert "fields[1] = -1" in _err()
    assert call(keys=_keys(3, 5, 3), nk=3) == INVALID
    assert "selected twice" in _err()
    assert call(n=-1) == INVALID
    assert "nrows < 0" in _err()
    # nested keys and lists: not canonical bytes (hash rule 5)
    foo = schemas["foo"].handle
    for k, name in ((2, "f3"), (3, "f4"), (4, "f5")):
        assert call(s=foo, keys=_keys(k), ro=aux) == UNSUPPORTED
        msg = _err()
        assert f"field {k} ({name})" in msg and "LIST / STRUCT / MAP" in msg
    k = [f.name for f in SCHEMAS["narrow"]].index("k_ints")
    assert call(s=schemas["narrow"].handle, keys=_keys(k), ro=aux) == UNSUPPORTED
    assert "k_ints" in _err()
    # the outputs and the hashes
    assert call(first=None) == INVALID
    assert "out_first is null" in _err()
    assert call(first=None, n=0) == INVALID                    # even when empty
    for name in ("first", "ids", "grows", "num"):
        assert call(**{name: out + 4}) == INVALID
        msg = _err()
        assert "must be 8-byte aligned" in msg and "out_first / out_group_ids / out_group_rows" in msg
    assert call(hashes=aux + 2) == INVALID
    assert "hashes must be 4-byte aligned" in _err()
    assert call(hashes=aux + 4, rows=None) == INVALID          # 4-byte alignment is enough
    assert "rows is null" in _err()
    # the batch
    assert call(rows=None) == INVALID
    assert "rows is null" in _err()
    assert call(rows=rows + 4) == INVALID
    assert "rows must be 8-byte aligned" in _err()
    names = [f.name for f in SCHEMAS["mixed"]]
    b = names.index("b")
    assert call(s=var, keys=_keys(b), ro=None) == INVALID
    assert "variable-length rows need row_offsets" in _err()
    assert call(s=var, keys=_keys(b), ro=aux + 4) == INVALID
    assert "row_offsets must be 8-byte aligned" in _err()
    # more rows than a table slot can name
    for n in (2 ** 31, 2 ** 40):
        assert call(n=n, ids=aux, grows=aux, num=aux) == INVALID
        assert "batch too large" in _err()
    assert call(n=2 ** 31, first=None) == INVALID              # the other argument checks still come first
    assert "out_first is null" in _err()


def test_no_rows_and_no_count_is_a_no_op(L, schemas):
    """nrows == 0 without out_num_groups returns FURY_OK without touching a buffer: rows, row_offsets
    and hashes may be NULL, and the outputs keep their contents."""
    fixed, var = schemas["struct100"].handle, schemas["mixed"].handle
    raw, out = _buf(64)
    ctypes.memset(out, 0xAB, 64)
    s1 = [f.name for f in SCHEMAS["mixed"]].index("s1")
    assert L.fury_row_group(fixed, _keys(0, 99), 2, None, None, 0, None, out, out + 8, out + 16, None, None) == OK
    assert L.fury_row_group(var, _keys(s1), 1, None, None, 0, None, out, None, None, None, None) == OK
    assert L.fury_row_group(var, _keys(s1), 1, None, None, 0, out + 32, out, None, out + 8, None, None) == OK
    assert ctypes.string_at(out, 64) == b"\xab" * 64


def test_python_surface_checks_before_any_device_work():
    import torch
    from fury_amd import types as T
    from fury_amd import Groups, bind_group, group_rows, group_rows_into, group_sizes
    from fury_amd.encoder import ClassNotCompatibleException, Encoders, IllegalArgumentException, RowBatch
    enc = Encoders.bean(SCHEMAS["mixed"], device="cpu")

    def batch(n):
        return RowBatch(torch.zeros(64, dtype=torch.uint8), torch.zeros(n + 1, dtype=torch.int64), n,
                        enc.schema_hash)
    four = batch(4)
    out = torch.zeros(8, dtype=torch.int64)
    with pytest.raises(IllegalArgumentException, match="out_first is required"):
        group_rows_into(enc, four, ["a"], None)
    with pytest.raises(IllegalArgumentException, match="no field named"):
        group_rows_into(enc, four, ["nope"], out)
    with pytest.raises(IllegalArgumentException, match="out_first must be an int64 tensor"):
        group_rows_into(enc, four, ["a"], out.to(torch.int32))
    with pytest.raises(IllegalArgumentException, match="out_group_ids has 3 entries, 4 needed"):
        group_rows_into(enc, four, ["a"], out, out[:3])
    with pytest.raises(IllegalArgumentException, match="out_group_rows has 2 entries, 4 needed"):
        group_rows_into(enc, four, ["a"], out, None, out[:2])
    with pytest.raises(IllegalArgumentException, match="out_num_groups has 0 entries, 1 needed"):
        group_rows_into(enc, four, ["a"], out, None, None, out[:0])
    with pytest.raises(IllegalArgumentException, match="hashes must be an int32 or uint32"):
        group_rows_into(enc, four, ["a"], out, hashes=out)
    with pytest.raises(IllegalArgumentException, match="hashes has 3 entries for 4 rows"):
        group_rows_into(enc, four, ["a"], out, hashes=torch.zeros(3, dtype=torch.int32))
    other = Encoders.bean([T.field("x", T.INT64)], device="cpu")
    with pytest.raises(ClassNotCompatibleException):
        group_rows_into(other, four, ["x"], out)
    with pytest.raises(ClassNotCompatibleException):
        bind_group(other, four, ["x"], out)
    # an empty batch has no groups and launches nothing (there is no GPU here)
    group_rows_into(enc, batch(0), ["a", "s1"], out)
    g = group_rows(enc, batch(0), ["a", "s1"])
    assert isinstance(g, Groups) and g.num_groups == 0
    assert g.first.numel() == g.group_ids.numel() == g.group_rows.numel() == 0 and g.first.dtype == torch.int64
    assert group_sizes(g).numel() == 0
    with pytest.raises(IllegalArgumentException, match="no field named"):
        group_rows(enc, batch(0), ["nope"])
