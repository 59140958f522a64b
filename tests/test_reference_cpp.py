"""The C restatement (oracle/row_oracle.c) against the reference's own C++ row code.

Every bit-exact test of the suite compares a kernel with ``oracle/row_oracle.c``, a restatement of
the Java writer / reader written by the same hands as the kernels.  Here that restatement meets an
implementation of the row format this project did not write: cpp/fury/row/{row,writer,type}.cc of
the reference, compiled as it lies by ``oracle/ref_cpp/Makefile`` and driven through
``oracle/ref_oracle.py``:

* sanity     the RowTest.Write row written through the driver reads back, with the reference's
             Row::ToString, as the string its own test expects (row_test.cc:96-98);
* encode     ``oracle.encode == ref_oracle.encode``, rows and offsets byte for byte;
* decode     ``ref_oracle.decode(oracle.encode(x)) == x`` and ``oracle.decode(ref_oracle.encode(x))
             == x``;
* fixtures   tests/golden/ref_cpp/*.npz, written by the reference: regenerating them gives the same
             arrays, and ``oracle.encode`` of their columns gives their rows.  The last one needs no
             library and runs everywhere; tests/test_reference_cpp_gpu.py holds the device to the
             same files.

over tests/ref_cases.py: the workload schemas, 60 random schemas and the edge batteries.  DECIMAL is
excluded by type (DESIGN.md section 5 has the table of real differences between the two
implementations).  CPU only.
"""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

from tests import ref_cases as RC
from tests import ref_fixtures as RF
from tests.helpers import assert_columns_equal

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ref():
    """The reference library: missing with the reference tree at hand means build() was not run --
    a failure; only a machine without the reference tree skips."""
    from oracle import ref_oracle as R
    if not R.available():
        if R.reference_present():
            pytest.fail("oracle/_ref/libfury_ref_row.so is missing: run build() "
                        "(python -c 'import __graft_entry__ as g; g.build()')")
        pytest.skip("no reference tree on this machine")
    R.lib()
    return R


_encoded: dict = {}


def _both(oracle, ref, cid):
    """(case, oracle rows, oracle offsets, reference rows, reference offsets), encoded once."""
    if cid not in _encoded:
        case = RC.get_case(cid)
        _encoded[cid] = (case,) + oracle.encode(case.fields, case.cols, case.n) \
            + ref.encode(case.fields, case.cols, case.n)
    return _encoded[cid]


def test_case_list_is_the_issue_s():
    """The cases are the ones asked for: every DECIMAL-free workload schema at 1 / 65 / 257 rows,
    60 random schemas, and the batteries in full."""
    from fury_amd.workloads import SCHEMAS
    ids = set(RC.CASE_IDS)
    for name, fields in SCHEMAS.items():
        if name not in ("narrow", "beana"):
            assert not RC.has_decimal(fields)
            assert {f"{name}-{n}" for n in (1, 65, 257)} <= ids
    assert RC.has_decimal(SCHEMAS["narrow"]) and RC.has_decimal(SCHEMAS["beana"])
    assert sum(c.startswith("fuzz") for c in ids) == 60
    assert RC.STRING_LENGTHS == tuple(range(18)) + (255, 256, 257)
    assert RC.LIST_LENGTHS == (0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129)
    assert len(RC.LIST_ELEMENTS) == 10
    assert sum(c.startswith("list_") and c.endswith(("_nullable", "_notnull")) for c in ids) == 20
    assert {f"flat{nf}" for nf in (63, 64, 65, 128, 129)} <= ids
    assert set(RC.NESTING_IDS) | {"strings", "float_bits", "int_extremes"} <= ids


def test_list_battery_has_a_null_at_every_position():
    """list<int16>, nullable items: for every length a row of values, an all-null row, and one
    row per position whose only null is there."""
    from fury_amd.beans import columns_to_beans
    case = RC.get_case("list_int16_nullable")
    seen = {}
    for b in columns_to_beans(case.fields, case.cols, case.n):
        v = b["l"]
        if v is not None:
            seen.setdefault(len(v), set()).add(tuple(i for i, x in enumerate(v) if x is None))
    assert set(seen) == set(RC.LIST_LENGTHS)
    for k, nulls in seen.items():
        assert () in nulls or k == 0
        assert tuple(range(k)) in nulls
        assert {(p,) for p in range(k)} <= nulls


def test_flat_battery_nulls_the_last_field_of_each_bitmap_word():
    from fury_amd.beans import columns_to_beans
    for nf in RC.FLAT_WIDTHS:
        case = RC.get_case(f"flat{nf}")
        assert len(case.fields) == nf
        beans = columns_to_beans(case.fields, case.cols, case.n)
        for w in range((nf + 63) // 64):
            last = case.fields[min(64 * w + 63, nf - 1)].name
            assert any(b[last] is None and sum(v is None for v in b.values()) == 1 for b in beans)


def test_driver_writes_the_row_test_row_as_the_reference_does(ref):
    """RowTest.Write's row (row_test.cc:31-99) through the driver: Row::ToString is the string the
    reference's own test expects -- the driver uses the writer the way the reference does."""
    from fury_amd.beans import beans_to_columns
    from fury_amd.workloads import SCHEMAS
    fields = SCHEMAS["row_test"]
    bean = {"f1": "str", "f2": 1, "f3": [2, 2], "f4": [("key1", 1.0), ("key2", 1.0)],
            "f5": {"n1": "str", "n2": 1}}
    rows, offs = ref.encode(fields, beans_to_columns(fields, [bean]), 1)
    want = json.load(open(os.path.join(GOLDEN, "known_answers.json")))["cpp_row_to_string"]["value"]
    assert ref.row_to_string(fields, rows, 0, int(offs[1])) == want


def test_decimal_is_refused_not_miswritten(ref):
    """DECIMAL is excluded by type: the driver refuses it (the C++ would size it as a 16-byte
    fixed field, type.cc:37-43)."""
    from fury_amd.workloads import SCHEMAS, gen_columns
    fields = SCHEMAS["narrow"]
    with pytest.raises(RuntimeError):
        ref.encode(fields, gen_columns("narrow", fields, 3), 3)


@pytest.mark.parametrize("cid", RC.CASE_IDS)
def test_encode_parity(oracle, ref, cid):
    case, rows, offs, ref_rows, ref_offs = _both(oracle, ref, cid)
    assert np.array_equal(offs, ref_offs), f"{cid}: row offsets differ"
    if not np.array_equal(rows, ref_rows):
        at = int(np.nonzero(rows != ref_rows)[0][0])
        r = int(np.searchsorted(offs, at, side="right")) - 1
        raise AssertionError(f"{cid}: first differing byte {at} = row {r} + {at - int(offs[r])}: "
                             f"oracle {rows[at]:#04x}, reference {ref_rows[at]:#04x}")


@pytest.mark.parametrize("cid", RC.CASE_IDS)
def test_decode_parity(oracle, ref, cid):
    case, rows, offs, ref_rows, ref_offs = _both(oracle, ref, cid)
    assert_columns_equal(case.fields, oracle.decode(case.fields, ref_rows, ref_offs, case.n),
                         case.cols, case.n)
    # the reference's getters check no bounds: rows that already differ from its own (a failure of
    # test_encode_parity) fail here too instead of being walked through unchecked pointers
    assert np.array_equal(offs, ref_offs) and np.array_equal(rows, ref_rows), \
        f"{cid}: the oracle's rows are not the reference's; its reader is not run on them"
    assert_columns_equal(case.fields, ref.decode(case.fields, rows, offs, case.n), case.cols, case.n)


# ---- fixtures written by the reference ----------------------------------------------------------
def _fixture_names():
    from tests.golden.make_ref_golden import FIXTURES
    return list(FIXTURES)


def test_fixture_directory_is_the_generator_s_list():
    assert RF.names() == sorted(_fixture_names())
    sizes = {n: os.path.getsize(os.path.join(RF.DIR, n + ".npz")) for n in RF.names()}
    biggest = os.path.getsize(os.path.join(GOLDEN, "struct100.npz"))
    assert max(sizes.values()) <= biggest, sizes
    assert sum(sizes.values()) <= 400 * 1024, sum(sizes.values())


@pytest.mark.parametrize("name", _fixture_names())
def test_fixture_regenerates_identically(ref, name):
    from tests.golden.make_ref_golden import build_arrays
    want = build_arrays(name)
    with np.load(os.path.join(RF.DIR, name + ".npz"), allow_pickle=False) as z:
        assert sorted(z.files) == sorted(want)
        for k in z.files:
            same = z[k].dtype == want[k].dtype and z[k].shape == want[k].shape
            assert same and z[k].tobytes() == want[k].tobytes(), f"{name}: {k}"   # NaNs: bytes


@pytest.mark.parametrize("name", _fixture_names())
def test_oracle_encodes_fixture_columns_to_the_reference_s_rows(oracle, name):
    """Needs no reference library: the rows in the file are the reference's."""
    fx = RF.load(name)
    assert fx.n <= 257
    rows, offs = oracle.encode(fx.fields, fx.columns, fx.n)
    assert np.array_equal(offs, fx.row_offsets)
    assert np.array_equal(rows, fx.rows)
    assert_columns_equal(fx.fields, oracle.decode(fx.fields, fx.rows, fx.row_offsets, fx.n),
                         fx.columns, fx.n)
