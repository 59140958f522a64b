"""Generates tests/golden/ref_cpp/*.npz: input columns with the rows the REFERENCE's own C++ writer
produced for them (oracle/ref_oracle.py over cpp/fury/row/writer.cc of the reference tree), the one
set of fixtures that does not pass through this project's reading of the row format.  Run on the
build machine only, after build() has made oracle/_ref/libfury_ref_row.so:

    python tests/golden/make_ref_golden.py

A compact selection of tests/ref_cases.py (at most 257 rows a file): string lengths around the
padding word; lists of 1-, 2-, 4- and 8-byte and variable-length elements at lengths around the
null-bitmap words, a null at the edge positions; the 65- and 129-field flat schemas; the nesting
and null set; float bit patterns and integer extremes; and the workload schemas foo, beana, nested,
mixed and narrow -- beana and narrow with their DECIMAL field as INT64 (the C++ sibling sizes
decimal128 differently from the Java writer).  File layout:
tests/ref_fixtures.py.  tests/test_reference_cpp.py checks that regenerating changes nothing and
that the oracle encodes the columns to the same rows; tests/test_reference_cpp_gpu.py holds the
device path to them.
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from fury_amd import types as T  # noqa: E402
from tests import ref_cases as RC  # noqa: E402
from tests import ref_fixtures as RF  # noqa: E402

_LENGTHS = (0, 1, 7, 8, 9, 63, 64, 65, 129)


def _list(elem: int, nullable: bool):
    return functools.partial(RC.list_case, elem, nullable, _LENGTHS, RC.edge_positions)


def _nesting(k: int):
    return lambda: RC.nesting_cases(12)[k]


FIXTURES = {
    "strings": functools.partial(RC.string_case, (0, 1, 7, 8, 9, 15, 16, 17, 255, 256, 257)),
    "list_bool_nullable": _list(T.BOOL, True),
    "list_int8_nullable": _list(T.INT8, True),
    "list_int8_notnull": _list(T.INT8, False),
    "list_int16_nullable": _list(T.INT16, True),
    "list_int16_notnull": _list(T.INT16, False),
    "list_int32_nullable": _list(T.INT32, True),
    "list_int64_nullable": _list(T.INT64, True),
    "list_utf8_nullable": _list(T.STRING, True),
    "flat65": functools.partial(RC.flat_case, 65, 2),
    "flat129": functools.partial(RC.flat_case, 129, 2),
    **{cid: _nesting(k) for k, cid in enumerate(RC.NESTING_IDS)},
    "float_bits": RC.float_case,
    "int_extremes": RC.int_case,
    "foo": functools.partial(RC.workload_case, "foo", 33),
    "beana": functools.partial(RC.beana_int64_case, 20),
    "nested": functools.partial(RC.workload_case, "nested", 257),
    "mixed": functools.partial(RC.workload_case, "mixed", 257),
    "narrow": functools.partial(RC.narrow_int64_case, 48),
}


def build_arrays(name: str) -> dict:
    from oracle import ref_oracle as R
    case = FIXTURES[name]()
    assert case.n <= 257, (name, case.n)
    rows, offs = R.encode(case.fields, case.cols, case.n)
    return RF.to_arrays(case.fields, case.cols, case.n, rows, offs)


def main() -> None:
    os.makedirs(RF.DIR, exist_ok=True)
    total = 0
    for name in FIXTURES:
        path = os.path.join(RF.DIR, name + ".npz")
        np.savez_compressed(path, **build_arrays(name))
        total += os.path.getsize(path)
        print(f"{name:24s} {os.path.getsize(path):8d} bytes")
    print(f"{len(FIXTURES)} fixtures, {total} bytes, in {RF.DIR}")


if __name__ == "__main__":
    main()
