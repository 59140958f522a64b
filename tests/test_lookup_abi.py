"""CPU checks of fury_row_index_slots / fury_row_index_build / fury_row_lookup: the symbols are bound
and exported, the header carries the eight numbered rules and declares what the library exports, and
every argument error is reported on the host, before any device work, with its status and a message
that names the function.  Host buffers stand in for device memory and are never dereferenced: every
call fails first, or has no probe rows."""
from __future__ import annotations

import ctypes
import re

import pytest

from fury_amd.workloads import SCHEMAS
from tests.test_keys_equal_abi import _buf, _keys, _side

OK, INVALID, UNSUPPORTED = 0, 1, 2
NULL_EQUAL = 1


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


def test_index_slots(L):
    """The smallest power of two >= max(2, 2 * nrows); -1 outside [0, 2^31 - 1]."""
    from fury_amd import index_slots
    from fury_amd.encoder import IllegalArgumentException
    want = {-1: -1, 0: 2, 1: 2, 2: 4, 3: 8, 2 ** 31 - 1: 2 ** 32, 2 ** 31: -1}
    for n, slots in want.items():
        assert L.fury_row_index_slots(n) == slots, n
        if slots < 0:
            with pytest.raises(IllegalArgumentException, match="is not in"):
                index_slots(n)
        else:
            assert index_slots(n) == slots
    for n in (4, 5, 63, 64, 65, 4097, 2 ** 30, 2 ** 30 + 1):
        slots = L.fury_row_index_slots(n)
        assert slots == index_slots(n) and slots & (slots - 1) == 0 and slots >= 2 * n > slots // 2
    assert L.fury_row_index_slots(-2 ** 40) == -1 and L.fury_row_index_slots(2 ** 62) == -1


def test_symbols_rules_and_header(L):
    from fury_amd import _native as N
    for name, nargs in (("fury_row_index_slots", 1), ("fury_row_index_build", 11), ("fury_row_lookup", 10)):
        assert name in N.SIGNATURES and len(N.SIGNATURES[name][1]) == nargs
        assert hasattr(L, name)
    assert N.SIGNATURES["fury_row_index_slots"][0] is ctypes.c_int64
    assert L.fury_abi_version() == 1
    with open(N.HERE + "/../include/fury_row.h") as f:
        header = f.read()
    assert "int64_t fury_row_index_slots(int64_t nrows);" in header
    assert "int fury_row_index_build(const fury_schema* schema, const int32_t* fields, int32_t num_keys," in header
    assert "int fury_row_lookup(const fury_key_side* probe, const fury_key_side* build, int32_t num_keys," in header
    at = header.index("Key index and lookup")
    doc = header[at:header.index("int64_t fury_row_index_slots(", at)]
    for rule in ("1. Slots.", "2. Build.", "3. The table.", "4. Lookup.", "5. Hashes.", "6. Probe-side bounds",
                 "7. Table robustness.", "8. Key types.", "Workspace", "4 bytes per row", "Limits"):
        assert rule in doc, rule
    # the declarations' parameter counts are the bound signatures'
    for name in ("fury_row_index_build", "fury_row_lookup"):
        decl = header[header.index(f"int {name}("):]
        decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(");")], flags=re.S)
        assert decl.count(",") + 1 == len(N.SIGNATURES[name][1]), name


def test_build_argument_errors(L, schemas):
    fixed, var = schemas["struct100"].handle, schemas["mixed"].handle
    r1, rows = _buf()
    r2, table = _buf()
    r3, aux = _buf()
    fn = "fury_row_index_build"

    def call(s=fixed, keys=_keys(0), nk=1, rows=rows, ro=None, n=4, hashes=None, table=table, slots=8,
             first=None):
        return L.fury_row_index_build(s, keys, nk, rows, ro, n, hashes, table, slots, first, None)

    # the schema, the key count and the key fields: as fury_row_group
    assert call(s=None) == INVALID
    assert "schema is null" in _err(fn)
    assert call(s=schemas["array"].handle) == UNSUPPORTED
    assert "collection schema" in _err(fn)
    assert call(nk=0) == INVALID
    assert "num_selected <= 0" in _err(fn)
    assert call(keys=_keys(*range(65)), nk=65) == UNSUPPORTED
    assert "at most 64 fields" in _err(fn)
    assert call(keys=_keys(*range(64)), nk=64, table=None) == INVALID       # 64 keys pass the selection
    assert "table is null" in _err(fn)
    assert call(keys=None) == INVALID
    assert "fields is null" in _err(fn)
    assert call(keys=_keys(100)) == INVALID
    assert "fields[0] = 100 is not a field" in _err(fn)
    assert call(keys=_keys(3, 5, 3), nk=3) == INVALID
    assert "selected twice" in _err(fn)
    assert call(n=-1) == INVALID
    assert "nrows < 0" in _err(fn)
    foo = schemas["foo"].handle
    for k, name in ((2, "f3"), (3, "f4"), (4, "f5")):                        # a LIST, a MAP, a STRUCT
        assert call(s=foo, keys=_keys(k), ro=aux) == UNSUPPORTED
        msg = _err(fn)
        assert f"field {k} ({name})" in msg and "LIST / STRUCT / MAP" in msg
    k = [f.name for f in SCHEMAS["narrow"]].index("k_ints")
    assert call(s=schemas["narrow"].handle, keys=_keys(k), ro=aux) == UNSUPPORTED
    assert "k_ints" in _err(fn)
    # the table
    assert call(table=None) == INVALID
    assert "table is null" in _err(fn)
    assert call(table=None, n=0, slots=2) == INVALID                         # even when empty
    assert call(table=table + 4) == INVALID
    assert "table / out_first must be 8-byte aligned" in _err(fn)
    assert call(first=aux + 4) == INVALID
    assert "table / out_first must be 8-byte aligned" in _err(fn)
    for n, slots in ((4, 4), (4, 16), (4, 0), (4, -8), (0, 0), (0, 4), (1, 4), (3, 4), (5, 8)):
        assert call(n=n, slots=slots) == INVALID, (n, slots)
        msg = _err(fn)
        assert f"table_slots {slots} is not fury_row_index_slots({n}) = {L.fury_row_index_slots(n)}" in msg
    # the hashes and the batch
    assert call(hashes=aux + 2) == INVALID
    assert "hashes must be 4-byte aligned" in _err(fn)
    assert call(hashes=aux + 4, rows=None) == INVALID                        # 4-byte alignment is enough
    assert "rows is null" in _err(fn)
    assert call(rows=rows + 4) == INVALID
    assert "rows must be 8-byte aligned" in _err(fn)
    b = [f.name for f in SCHEMAS["mixed"]].index("b")
    assert call(s=var, keys=_keys(b), ro=None) == INVALID
    assert "variable-length rows need row_offsets" in _err(fn)
    assert call(s=var, keys=_keys(b), ro=aux + 4) == INVALID
    assert "row_offsets must be 8-byte aligned" in _err(fn)
    # more rows than a table slot can name
    for n in (2 ** 31, 2 ** 40):
        assert call(n=n, slots=2 ** 32) == INVALID
        assert "batch too large" in _err(fn)


def test_lookup_argument_errors(L, schemas):
    fixed, var = schemas["struct100"].handle, schemas["mixed"].handle
    r1, rows = _buf()
    r2, out = _buf()
    r3, aux = _buf()
    r4, table = _buf()
    fn = "fury_row_lookup"

    def call(probe=None, build=None, nk=1, table=table, slots=8, hashes=None, flags=0, orows=out, om=aux, **kw):
        probe = _side(fixed, _keys(0), rows, **kw) if probe is None else probe
        build = _side(fixed, _keys(2), rows) if build is None else build
        return L.fury_row_lookup(probe if probe != "null" else None, build if build != "null" else None, nk,
                                 table, slots, hashes, flags, orows, om, None)

    def both(make):
        """The same mistake on the probe side and on the build side: (status, message) of each."""
        res = []
        for name in ("probe", "build"):
            st = call(**{name: make()})
            res.append((st, _err(fn)))
            assert name in res[-1][1], res[-1]
        return res

    # the sides and their schemas
    assert call(probe="null") == INVALID
    assert "probe is null" in _err(fn)
    assert call(build="null") == INVALID
    assert "build is null" in _err(fn)
    for st, msg in both(lambda: _side(None, _keys(0), rows)):
        assert st == INVALID and "schema is null" in msg
    for st, msg in both(lambda: _side(schemas["array"].handle, _keys(0), rows)):
        assert st == UNSUPPORTED and "collection schema" in msg
    # the key count and the key fields: as fury_row_keys_equal
    assert call(nk=0) == INVALID
    assert "num_selected <= 0" in _err(fn)
    many = _keys(*range(65))
    assert call(probe=_side(fixed, many, rows), build=_side(fixed, many, rows), nk=65) == UNSUPPORTED
    assert "at most 64 fields" in _err(fn)
    for st, msg in both(lambda: _side(fixed, None, rows)):
        assert st == INVALID and "fields is null" in msg
    for st, msg in both(lambda: _side(fixed, _keys(100), rows)):
        assert st == INVALID and "fields[0] = 100 is not a field" in msg
    assert call(probe=_side(fixed, _keys(1, 2, 3), rows), build=_side(fixed, _keys(3, 5, 3), rows), nk=3) == INVALID
    assert "build" in _err(fn) and "selected twice" in _err(fn)
    for st, msg in both(lambda: _side(fixed, _keys(0), rows, n=-1)):
        assert st == INVALID and "nrows < 0" in msg
    # a LIST, a MAP, a STRUCT key: not canonical bytes (hash rule 5)
    foo = schemas["foo"].handle
    for k, name in ((2, "f3"), (3, "f4"), (4, "f5")):
        for st, msg in both(lambda: _side(foo, _keys(k), rows, aux)):
            assert st == UNSUPPORTED and f"field {k} ({name})" in msg and "LIST / STRUCT / MAP" in msg
    k = [f.name for f in SCHEMAS["narrow"]].index("k_ints")
    for st, msg in both(lambda: _side(schemas["narrow"].handle, _keys(k), rows, aux)):
        assert st == UNSUPPORTED and "k_ints" in msg
    # rule 8: the type ids of a key position agree, the message names k and both fields
    names = [f.name for f in SCHEMAS["mixed"]]
    a, b, s1 = names.index("a"), names.index("b"), names.index("s1")
    assert call(probe=_side(var, _keys(b, a), rows, aux), build=_side(var, _keys(b, s1), rows, aux),
                nk=2) == INVALID
    msg = _err(fn)
    assert "key 1" in msg and f"probe field {a} (a)" in msg and f"build field {s1} (s1)" in msg
    assert call(probe=_side(var, _keys(a), rows, aux), build=_side(var, _keys(b), rows, aux)) == INVALID
    assert "key 0" in _err(fn)
    # whole batches only
    for st, msg in both(lambda: _side(fixed, _keys(0), rows, idx=aux)):
        assert st == INVALID and "indices must be null" in msg
    # the table
    assert call(table=None) == INVALID
    assert "table is null" in _err(fn)
    assert call(table=table + 4) == INVALID
    assert "table / out_rows must be 8-byte aligned" in _err(fn)
    for slots in (4, 16, 0, -8, 7):
        assert call(slots=slots) == INVALID
        assert f"table_slots {slots} is not fury_row_index_slots(4) = 8" in _err(fn)
    assert call(build=_side(fixed, _keys(2), None, n=0), slots=8) == INVALID
    assert "fury_row_index_slots(0) = 2" in _err(fn)
    for n in (2 ** 31, 2 ** 40):
        assert call(build=_side(fixed, _keys(2), rows, n=n), slots=2 ** 32) == INVALID
        assert "build" in _err(fn) and "batch too large" in _err(fn)
    # the flags, the outputs and the hashes
    for flags in (2, 3, -1, 1 << 30):
        assert call(flags=flags) == INVALID
        assert "unknown flags" in _err(fn)
    assert call(orows=None, om=None) == INVALID
    assert "out_rows and out_mask are both null" in _err(fn)
    assert call(orows=None, om=None, n=0) == INVALID                         # even when empty
    assert call(orows=out + 4) == INVALID
    assert "table / out_rows must be 8-byte aligned" in _err(fn)
    assert call(om=aux + 2) == INVALID
    assert "probe_hashes / out_mask must be 4-byte aligned" in _err(fn)
    assert call(hashes=aux + 2) == INVALID
    assert "probe_hashes / out_mask must be 4-byte aligned" in _err(fn)
    assert call(hashes=aux + 4, probe=_side(fixed, _keys(0), None)) == INVALID   # 4-byte alignment is enough
    assert "rows is null" in _err(fn)
    # the batches
    for st, msg in both(lambda: _side(fixed, _keys(0), None)):
        assert st == INVALID and "rows is null" in msg
    for st, msg in both(lambda: _side(fixed, _keys(0), rows + 4)):
        assert st == INVALID and "rows must be 8-byte aligned" in msg
    for st, msg in both(lambda: _side(var, _keys(b), rows, None)):
        assert st == INVALID and "variable-length rows need row_offsets" in msg
    for st, msg in both(lambda: _side(var, _keys(b), rows, aux + 4)):
        assert st == INVALID and "8-byte aligned" in msg and "row_offsets" in msg
    # a probe batch the grid cannot index
    assert call(probe=_side(fixed, _keys(0), rows, n=2 ** 31 * 256)) == INVALID
    assert "probe" in _err(fn) and "batch too large" in _err(fn)


def test_no_probe_rows_is_a_no_op(L, schemas):
    """probe->nrows == 0 returns FURY_OK without touching a buffer: rows and row_offsets may be NULL
    on the probe side, and the outputs keep their contents."""
    fixed, var = schemas["struct100"].handle, schemas["mixed"].handle
    raw, out = _buf(64)
    r2, table = _buf(64)
    ctypes.memset(out, 0xAB, 64)
    s1 = [f.name for f in SCHEMAS["mixed"]].index("s1")
    for flags in (0, NULL_EQUAL):
        assert L.fury_row_lookup(_side(fixed, _keys(0, 99), None, n=0), _side(fixed, _keys(2, 97), None, n=0), 2,
                                 table, 2, None, flags, out, out + 32, None) == OK
        assert L.fury_row_lookup(_side(var, _keys(s1), None, n=0), _side(var, _keys(s1), None, n=7), 1,
                                 table, 16, None, flags, out, None, None) == OK
        assert L.fury_row_lookup(_side(var, _keys(s1), None, n=0), _side(fixed, _keys(s1), None, n=3), 1,
                                 table, 8, out + 4, flags, None, out, None) == INVALID      # key types still checked
    assert ctypes.string_at(out, 64) == b"\xab" * 64


def test_python_surface_checks_before_any_device_work():
    import torch
    from fury_amd import (KeyIndex, KeySide, bind_lookup, build_index_into, index_slots, lookup, lookup_into,
                          lookup_join_pairs, semi_join)
    from fury_amd import types as T
    from fury_amd.encoder import ClassNotCompatibleException, Encoders, IllegalArgumentException, RowBatch
    import fury_amd
    # fury_amd.lookup is the module, and calling it calls its function lookup
    assert lookup is fury_amd.lookup and callable(lookup) and callable(lookup.lookup)
    enc = Encoders.bean(SCHEMAS["mixed"], device="cpu")
    other = Encoders.bean([T.field("x", T.INT32), T.field("y", T.STRING)], device="cpu")

    def batch(e, n):
        return RowBatch(torch.zeros(64, dtype=torch.uint8), torch.zeros(n + 1, dtype=torch.int64), n,
                        e.schema_hash)
    build = KeySide(enc, batch(enc, 4), ["a", "s1"])
    probe = KeySide(other, batch(other, 3), ["x", "y"])
    table = torch.zeros(index_slots(4), dtype=torch.int64)
    out = torch.zeros(8, dtype=torch.int64)
    mask = torch.zeros(1, dtype=torch.int32)
    # build_index_into
    with pytest.raises(IllegalArgumentException, match="table must be an int64 tensor"):
        build_index_into(build, table.to(torch.int32))
    with pytest.raises(IllegalArgumentException, match=r"table has 4 words, index_slots\(4\) = 8 needed"):
        build_index_into(build, table[:4])
    with pytest.raises(IllegalArgumentException, match="out_first must be an int64 tensor"):
        build_index_into(build, table, out.to(torch.int32))
    with pytest.raises(IllegalArgumentException, match="out_first has 3 entries, 4 needed"):
        build_index_into(build, table, out[:3])
    with pytest.raises(IllegalArgumentException, match="hashes must be an int32 or uint32"):
        build_index_into(build, table, hashes=out)
    with pytest.raises(IllegalArgumentException, match="hashes has 3 entries for 4 rows"):
        build_index_into(build, table, hashes=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(IllegalArgumentException, match="no field named"):
        build_index_into(build._replace(keys=["nope"]), table)
    with pytest.raises(IllegalArgumentException, match="indices must be None"):
        build_index_into(build._replace(indices=out), table)
    with pytest.raises(ClassNotCompatibleException):
        build_index_into(KeySide(other, build.batch, ["x"]), table)
    # lookup_into
    index = KeyIndex(build, table, None, False)
    hashed = KeyIndex(build, table, None, True)
    h3 = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(IllegalArgumentException, match="out_rows and out_mask are both None"):
        lookup_into(index, probe)
    with pytest.raises(IllegalArgumentException, match="out_rows must be an int64 tensor"):
        lookup_into(index, probe, out.to(torch.int32))
    with pytest.raises(IllegalArgumentException, match="out_rows has 2 entries for 3 rows"):
        lookup_into(index, probe, out[:2])
    with pytest.raises(IllegalArgumentException, match="out_mask must be an int32 or uint32"):
        lookup_into(index, probe, None, out)
    with pytest.raises(IllegalArgumentException, match=r"out_mask has 0 words for 3 rows \(1 needed\)"):
        lookup_into(index, probe, None, mask[:0])
    with pytest.raises(IllegalArgumentException, match="2 probe keys against 1 build keys"):
        lookup_into(KeyIndex(build._replace(keys=["a"]), table, None, False), probe, out)
    with pytest.raises(IllegalArgumentException, match=r"table has 4 words, index_slots\(4\) = 8"):
        lookup_into(KeyIndex(build, table[:4], None, False), probe, out)
    with pytest.raises(IllegalArgumentException, match="built from the call's own hashes"):
        lookup_into(index, probe, out, hashes=h3)                  # hashes on one side only
    with pytest.raises(IllegalArgumentException, match="built from the caller's hashes"):
        lookup_into(hashed, probe, out)
    with pytest.raises(IllegalArgumentException, match="hashes has 2 entries for 3 rows"):
        lookup_into(hashed, probe, out, hashes=h3[:2])
    with pytest.raises(IllegalArgumentException, match="hashes must be an int32 or uint32"):
        lookup_into(hashed, probe, out, hashes=out)
    with pytest.raises(IllegalArgumentException, match="indices must be None"):
        lookup_into(index, probe._replace(indices=out), out)
    with pytest.raises(ClassNotCompatibleException):
        lookup_into(index, KeySide(enc, probe.batch, ["a", "s1"]), out)
    with pytest.raises(ClassNotCompatibleException):
        bind_lookup(index, KeySide(enc, probe.batch, ["a", "s1"]), out)
    with pytest.raises(IllegalArgumentException, match="want_first=True"):
        lookup_join_pairs(index, probe)
    with pytest.raises(IllegalArgumentException, match="without caller hashes"):
        lookup_join_pairs(KeyIndex(build, table, out, True), probe)
    with pytest.raises(IllegalArgumentException, match="built from the caller's hashes"):
        semi_join(hashed, probe)
    # an empty probe batch finds nothing and launches nothing (there is no GPU here)
    empty = probe._replace(batch=batch(other, 0))
    lookup_into(index, empty, out)
    bind_lookup(index, empty, out, mask)()
    got = lookup(index, empty)
    assert got.dtype == torch.int64 and got.numel() == 0
    pj, bi = lookup_join_pairs(KeyIndex(build, table, out[:4], False), empty)
    assert pj.numel() == 0 and bi.numel() == 0 and pj.dtype == torch.int64
    with pytest.raises(IllegalArgumentException, match="no field named"):
        lookup(index, empty._replace(keys=["x", "nope"]))
