"""TEST INFRASTRUCTURE ONLY -- ctypes front end of the reference's own C++ row writer / reader,
built by ``oracle/ref_cpp/Makefile`` into ``oracle/_ref/libfury_ref_row.so`` (never committed).

``encode`` / ``decode`` take and return what ``oracle.encode`` / ``oracle.decode`` do, so a test can
put the two side by side: ``oracle.py`` is this project's restatement of the Java writer, this
module an implementation the project did not write (cpp/fury/row/{row,writer,type}.cc driven by
``oracle/ref_cpp/ref_driver.cc``).  DECIMAL fields are refused (exclusions).

The library exists only where the reference tree and pyarrow's Arrow C++ headers do -- the build
machine.  Nothing that runs on the GPU machine may import this module's library; the fixtures under
``tests/golden/ref_cpp/`` carry its output there.
"""
from __future__ import annotations

import ctypes
import json
import os
import subprocess
import sys
from typing import List, Optional, Sequence

import numpy as np

from . import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "_ref", "libfury_ref_row.so")
RECIPE_DIR = os.path.join(HERE, "ref_cpp")

_lib = None


def reference_root() -> str:
    """Root of the reference tree: $FURY_REFERENCE_ROOT, else BASELINE.json's reference_path."""
    env = os.environ.get("FURY_REFERENCE_ROOT")
    if env:
        return env
    with open(os.path.join(os.path.dirname(HERE), "BASELINE.json")) as fh:
        return json.load(fh)["reference_path"]


def reference_present() -> bool:
    return os.path.isfile(os.path.join(reference_root(), "cpp", "fury", "row", "writer.cc"))


def arrow_headers_present() -> bool:
    try:
        import pyarrow
    except ImportError:
        return False
    return os.path.isfile(os.path.join(pyarrow.get_include(), "arrow", "api.h"))


def build(jobs: int = 1) -> bool:
    """Runs the recipe when the reference tree and pyarrow's headers are both present; returns
    whether it ran.  Where either is missing there is nothing to build, and that is no error."""
    if not (reference_present() and arrow_headers_present()):
        return False
    subprocess.run(["make", "-s", "-j", str(jobs), "-C", RECIPE_DIR, f"REF={reference_root()}",
                    f"PYTHON={sys.executable}"], check=True)
    return True


def available() -> bool:
    return os.path.isfile(LIB_PATH)


def lib():
    global _lib
    if _lib is None:
        import pyarrow  # noqa: F401  (loads the libarrow the library was linked against)
        L = ctypes.CDLL(LIB_PATH)
        fp, cp = ctypes.POINTER(O._CField), ctypes.POINTER(O._CColumn)
        L.ref_encode.restype = ctypes.c_int64
        L.ref_encode.argtypes = [fp, ctypes.c_int32, cp, ctypes.c_int64, ctypes.c_void_p,
                                 ctypes.c_int64, ctypes.c_void_p]
        L.ref_decode.restype = ctypes.c_int
        L.ref_decode.argtypes = [fp, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                 ctypes.c_int64, cp]
        L.ref_row_to_string.restype = ctypes.c_int64
        L.ref_row_to_string.argtypes = [fp, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64,
                                        ctypes.c_int64, ctypes.c_char_p, ctypes.c_int64]
        _lib = L
    return _lib


def encode(fields: Sequence[O.F], cols: Sequence[O.Col], nrows: int):
    """Returns (rows uint8[total], row_offsets int64[nrows+1]), written by RowWriter / ArrayWriter."""
    keep: list = []
    cf = O._c_fields(fields, keep)
    cc = O._c_columns(cols, keep)
    offs = np.zeros(nrows + 1, np.int64)
    total = lib().ref_encode(cf, len(fields), cc, nrows, None, 0, offs.ctypes.data)
    if total < 0:
        raise RuntimeError(f"reference encode failed with status {-total}")
    out = np.zeros(max(total, 1), np.uint8)
    total2 = lib().ref_encode(cf, len(fields), cc, nrows, out.ctypes.data, out.nbytes,
                              offs.ctypes.data)
    assert total2 == total
    return out[:total], offs


def decode(fields: Sequence[O.F], rows: np.ndarray, row_offsets: Optional[np.ndarray],
           nrows: int) -> List[O.Col]:
    """Columns read back with Row::PointTo and the reference's getters; null entries are zero."""
    if row_offsets is None:
        row_offsets = np.arange(nrows + 1, dtype=np.int64) * O.fixed_size(fields)
    rows = np.ascontiguousarray(rows, np.uint8)
    offs = np.ascontiguousarray(row_offsets, np.int64)
    keep: list = []
    outs = [O._alloc_out(f, nrows, int(rows.nbytes), True) for f in fields]
    st = lib().ref_decode(O._c_fields(fields, keep), len(fields), O._ptr(rows), O._ptr(offs),
                          nrows, O._c_columns(outs, keep))
    if st != 0:
        raise RuntimeError(f"reference decode failed with status {st}")
    return [O._trim(f, c, nrows) for f, c in zip(fields, outs)]


def row_to_string(fields: Sequence[O.F], rows: np.ndarray, offset: int, size: int) -> str:
    """Row::ToString of one row of a batch."""
    rows = np.ascontiguousarray(rows, np.uint8)
    keep: list = []
    cf = O._c_fields(fields, keep)
    need = lib().ref_row_to_string(cf, len(fields), O._ptr(rows), offset, size, None, 0)
    if need < 0:
        raise RuntimeError(f"reference ToString failed with status {-need}")
    buf = ctypes.create_string_buffer(int(need) + 1)
    lib().ref_row_to_string(cf, len(fields), O._ptr(rows), offset, size, buf, len(buf))
    return buf.value.decode("utf-8")
