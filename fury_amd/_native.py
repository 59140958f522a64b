"""ctypes binding of libfury_row.so (include/fury_row.h).

The library is built in-tree (``fury_amd/libfury_row.so``, see fury_amd/csrc/Makefile and
``__graft_entry__.build()``).  There is no fallback: if the library is missing or fails to load,
importing this module raises, so no code path silently runs on the CPU.
"""
from __future__ import annotations

import ctypes
import os

# torch first: its bundled libamdhip64.so.7 must be the HIP runtime our library binds to, so
# that torch streams/allocations and our launches share one runtime.
import torch  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
# FURY_ROW_LIB: alternative in-tree build of the same library (kernel-variant A/B experiments)
LIB_PATH = os.environ.get("FURY_ROW_LIB") or os.path.join(HERE, "libfury_row.so")


class FuryField(ctypes.Structure):
    pass


FuryField._fields_ = [("name", ctypes.c_char_p), ("type_id", ctypes.c_int32),
                      ("nullable", ctypes.c_int32), ("num_children", ctypes.c_int32),
                      ("children", ctypes.POINTER(FuryField))]


class FuryColumn(ctypes.Structure):
    pass


FuryColumn._fields_ = [("values", ctypes.c_void_p), ("validity", ctypes.c_void_p),
                       ("offsets", ctypes.c_void_p), ("capacity", ctypes.c_int64),
                       ("child", ctypes.POINTER(FuryColumn))]


class FurySchemaInfo(ctypes.Structure):
    _fields_ = [("num_fields", ctypes.c_int32), ("bitmap_bytes", ctypes.c_int32),
                ("fixed_size", ctypes.c_int32), ("is_fixed", ctypes.c_int32),
                ("schema_hash", ctypes.c_int64)]


class FuryZipSource(ctypes.Structure):
    _fields_ = [("schema", ctypes.c_void_p), ("rows", ctypes.c_void_p),
                ("row_offsets", ctypes.c_void_p)]


ZIP_MAX_SOURCES = 4


class FuryConcatSource(ctypes.Structure):
    _fields_ = [("rows", ctypes.c_void_p), ("row_offsets", ctypes.c_void_p),
                ("nrows", ctypes.c_int64)]


class FuryKeySide(ctypes.Structure):
    _fields_ = [("schema", ctypes.c_void_p), ("fields", ctypes.POINTER(ctypes.c_int32)),
                ("rows", ctypes.c_void_p), ("row_offsets", ctypes.c_void_p),
                ("nrows", ctypes.c_int64), ("indices", ctypes.c_void_p)]


class FuryAgg(ctypes.Structure):
    _fields_ = [("field", ctypes.c_int32), ("op", ctypes.c_int32), ("out", ctypes.c_void_p),
                ("out_count", ctypes.c_void_p)]


class FuryPredTerm(ctypes.Structure):
    _fields_ = [("field", ctypes.c_int32), ("op", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("literal", ctypes.c_void_p), ("literal_len", ctypes.c_int64)]


AGG_OPS = {"count": 1, "sum": 2, "min": 3, "max": 4, "argmin": 5, "argmax": 6}
AGG_MAX_AGGS = 16
PRED_OPS = {"is_null": 1, "eq": 2, "lt": 3, "le": 4, "gt": 5, "ge": 6, "starts_with": 7, "ends_with": 8,
            "contains": 9}
PRED_NOT = 1
PRED_OR = 2
PRED_MAX_TERMS = 32
PRED_MAX_LITERAL_BYTES = 2048
KEYS_NULL_EQUAL = 1
ORDER_DESC = 1
ORDER_NULLS_LAST = 2
PARTITION_MAX_PARTS = 65535
CONCAT_MAX_SOURCES = 32

# Exported symbols with their signatures (kept in sync with include/fury_row.h; the CPU test
# suite checks the header and this table agree).
_P = ctypes.c_void_p
_I32 = ctypes.c_int32
_I64 = ctypes.c_int64
_U32 = ctypes.c_uint32
SIGNATURES = {
    "fury_abi_version": (_I32, []),
    "fury_last_error": (ctypes.c_size_t, [ctypes.c_char_p, ctypes.c_size_t]),
    "fury_type_width": (_I32, [_I32]),
    "fury_sort_bean_fields": (ctypes.c_int, [ctypes.POINTER(ctypes.c_char_p), _I32,
                                             ctypes.POINTER(_I32)]),
    "fury_lower_camel_to_lower_underscore": (_I32, [ctypes.c_char_p, ctypes.c_char_p,
                                                    ctypes.c_size_t]),
    "fury_schema_create": (ctypes.c_int, [ctypes.POINTER(FuryField), _I32, ctypes.POINTER(_P)]),
    "fury_collection_schema_create": (ctypes.c_int, [ctypes.POINTER(FuryField), ctypes.POINTER(_P)]),
    "fury_schema_destroy": (None, [_P]),
    "fury_schema_get_info": (ctypes.c_int, [_P, ctypes.POINTER(FurySchemaInfo)]),
    "fury_row_measure": (ctypes.c_int, [_P, ctypes.POINTER(FuryColumn), _I64, _P, _P]),
    "fury_row_encode": (ctypes.c_int, [_P, ctypes.POINTER(FuryColumn), _I64, _P, _P, _P]),
    "fury_row_encode_measured": (ctypes.c_int, [_P, ctypes.POINTER(FuryColumn), _I64, _P, _P, _I64,
                                                _P]),
    "fury_row_decode_measure": (ctypes.c_int, [_P, _P, _P, _I64, ctypes.POINTER(FuryColumn),
                                               _P]),
    "fury_row_decode": (ctypes.c_int, [_P, _P, _P, _I64, ctypes.POINTER(FuryColumn), _P]),
    "fury_rows_to_arrow": (ctypes.c_int, [_P, _P, _P, _I64, ctypes.POINTER(FuryColumn), _P]),
    "fury_row_project": (ctypes.c_int, [_P, ctypes.POINTER(_I32), _I32, _P, _P, _I64,
                                        ctypes.POINTER(FuryColumn), _I32, _P]),
    "fury_row_project_measure": (ctypes.c_int, [_P, ctypes.POINTER(_I32), _I32, _P, _P, _I64,
                                                ctypes.POINTER(FuryColumn), _P]),
    "fury_row_update": (ctypes.c_int, [_P, ctypes.POINTER(_I32), _I32, _P, _P, _I64,
                                       ctypes.POINTER(FuryColumn), _P, _P]),
    "fury_row_take": (ctypes.c_int, [_P, _P, _P, _I64, _P, _I64, _P, _I64, _P, _P]),
    "fury_row_filter": (ctypes.c_int, [_P, _P, _P, _I64, _P, _P, _I64, _P, _P, _P, _P]),
    "fury_row_partition": (ctypes.c_int, [_P, _P, _P, _I64, _P, _I32, _P, _I64, _P, _P, _P, _P, _P]),
    "fury_row_concat": (ctypes.c_int, [_P, ctypes.POINTER(FuryConcatSource), _I32, _P, _I64, _P,
                                       _P]),
    "fury_row_hash": (ctypes.c_int, [_P, ctypes.POINTER(_I32), _I32, _P, _P, _I64, _U32, _I32, _P, _P,
                                     _P]),
    "fury_hash_bytes": (_U32, [_P, _I64, _U32]),
    "fury_hash_null": (_U32, [_U32]),
    "fury_row_keys_equal": (ctypes.c_int, [ctypes.POINTER(FuryKeySide), ctypes.POINTER(FuryKeySide),
                                           _I32, _I64, _I32, _P, _P, _P]),
    "fury_row_group": (ctypes.c_int, [_P, ctypes.POINTER(_I32), _I32, _P, _P, _I64, _P, _P, _P, _P, _P,
                                      _P]),
    "fury_row_index_slots": (_I64, [_I64]),
    "fury_row_index_build": (ctypes.c_int, [_P, ctypes.POINTER(_I32), _I32, _P, _P, _I64, _P, _P, _I64, _P,
                                            _P]),
    "fury_row_lookup": (ctypes.c_int, [ctypes.POINTER(FuryKeySide), ctypes.POINTER(FuryKeySide), _I32, _P,
                                       _I64, _P, _I32, _P, _P, _P]),
    "fury_row_compare": (ctypes.c_int, [ctypes.POINTER(FuryKeySide), ctypes.POINTER(FuryKeySide), _I32,
                                        ctypes.POINTER(_I32), _I64, _P, _P]),
    "fury_row_order_words": (ctypes.c_int, [_P, _I32, _I32, _I32, _P, _P, _I64, _P, _I64, _P, _P, _P]),
    "fury_row_aggregate": (ctypes.c_int, [_P, _P, _P, _I64, _P, _I64, ctypes.POINTER(FuryAgg), _I32, _P]),
    "fury_row_aggregate_lds_cells": (_I64, []),
    "fury_row_predicate": (ctypes.c_int, [_P, _P, _P, _I64, ctypes.POINTER(FuryPredTerm), _I32, _P, _P, _P, _P]),
    "fury_schema_child": (ctypes.c_int, [_P, ctypes.POINTER(_I32), _I32, ctypes.POINTER(_P)]),
    "fury_row_extract": (ctypes.c_int, [_P, ctypes.POINTER(_I32), _I32, _P, _P, _I64, _P, _I64, _P,
                                        _P, _P, _P, _P]),
    "fury_schema_element": (ctypes.c_int, [_P, ctypes.POINTER(_I32), _I32, _I32,
                                           ctypes.POINTER(_P)]),
    "fury_row_explode": (ctypes.c_int, [_P, ctypes.POINTER(_I32), _I32, _I32, _P, _P, _I64, _P, _P,
                                        _I64, _P, _I64, _P, _P, _P, _P, _P, _P]),
    "fury_schema_select": (ctypes.c_int, [_P, ctypes.POINTER(_I32), _I32, ctypes.POINTER(_P)]),
    "fury_row_select": (ctypes.c_int, [_P, ctypes.POINTER(_I32), _I32, _P, _P, _I64, _P, _I64, _P,
                                       _P]),
    "fury_schema_zip": (ctypes.c_int, [ctypes.POINTER(_P), _I32, ctypes.POINTER(_I32), _I32,
                                       ctypes.POINTER(_P)]),
    "fury_row_zip": (ctypes.c_int, [ctypes.POINTER(FuryZipSource), _I32, ctypes.POINTER(_I32), _I32,
                                    _I64, _P, _I64, _P, _P]),
    "fury_row_implode": (ctypes.c_int, [_P, _P, _P, _I64, _P, _I64, _P, _P, _I64, _P, _I64, _P, _P]),
    "fury_row_wrap": (ctypes.c_int, [_P, _P, _P, _I64, _P, _I64, _P, _I64, _P, _P]),
    "fury_schema_map_side": (ctypes.c_int, [_P, ctypes.POINTER(_I32), _I32, _I32,
                                            ctypes.POINTER(_P)]),
    "fury_row_map_split": (ctypes.c_int, [_P, ctypes.POINTER(_I32), _I32, _P, _P, _I64, _P, _I64, _P,
                                          _P, _I64, _P, _P, _P, _P, _P]),
    "fury_row_map_join": (ctypes.c_int, [_P, _P, _P, _P, _P, _I64, _P, _I64, _P, _I64, _P, _P]),
    "fury_schema_num_nodes": (_I32, [_P]),
    "fury_decode_prepare": (ctypes.c_int, [_P, _P, _P, _I64, ctypes.POINTER(_I64),
                                           ctypes.POINTER(_I64), ctypes.POINTER(_P), _P]),
    "fury_decode_execute": (ctypes.c_int, [_P, ctypes.POINTER(FuryColumn), _I32, _P]),
    "fury_decode_plan_destroy": (None, [_P]),
    "fury_device_status": (ctypes.c_int, [_P]),
    "fury_stream_release": (ctypes.c_int, [_P]),
    "fury_trim_workspace": (ctypes.c_int, [_I32]),
    "fury_set_tuning": (ctypes.c_int, [ctypes.c_char_p, _I32]),
    "fury_get_tuning": (_I32, [ctypes.c_char_p]),
    "fury_arrow_append": (ctypes.c_int, [_P, ctypes.POINTER(FuryColumn), _I64,
                                         ctypes.POINTER(FuryColumn), _I64, _P]),
    "fury_frame_rows": (ctypes.c_int, [_P, _P, _P, _I64, _P, _P, _P]),
    "fury_unframe_rows": (ctypes.c_int, [_P, _P, _I64, _I64, _P, _P, _P]),
    "fury_host_alloc": (ctypes.c_int, [_I64, ctypes.POINTER(ctypes.c_void_p)]),
    "fury_host_free": (ctypes.c_int, [_P]),
    "fury_host_register": (ctypes.c_int, [_P, _I64]),
    "fury_host_unregister": (ctypes.c_int, [_P]),
    "fury_row_encode_host": (ctypes.c_int, [_P, ctypes.POINTER(FuryColumn), _I64, _P, _I64, _P,
                                            ctypes.POINTER(_I64), _I32]),
    "fury_row_decode_host": (ctypes.c_int, [_P, _P, _P, _I64, ctypes.POINTER(FuryColumn), _I32]),
    "fury_decode_host_prepare": (ctypes.c_int, [_P, _P, _P, _I64, ctypes.POINTER(_I64),
                                                ctypes.POINTER(_I64), ctypes.POINTER(_P), _I32]),
    "fury_decode_host_execute": (ctypes.c_int, [_P, ctypes.POINTER(FuryColumn)]),
    "fury_jni_exception_class": (ctypes.c_char_p, [ctypes.c_int]),
    "fury_jni_schema_create": (ctypes.c_int, [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(_I32),
                                              _I32, _I32, ctypes.POINTER(_P)]),
    "fury_jni_encode_host": (ctypes.c_int, [_P, ctypes.POINTER(_I64), _I64, _I64, _P, _I64, _P,
                                            ctypes.POINTER(_I64), _I32]),
    "fury_jni_decode_host": (ctypes.c_int, [_P, _P, _P, _I64, ctypes.POINTER(_I64), _I64, _I32]),
    "fury_jni_decode_host_prepare": (ctypes.c_int, [_P, _P, _P, _I64, ctypes.POINTER(_I64), _I64,
                                                    ctypes.POINTER(_P), _I32]),
    "fury_jni_decode_host_execute": (ctypes.c_int, [_P, _P, ctypes.POINTER(_I64), _I64]),
    "fury_hbm_copy": (ctypes.c_int, [_P, _P, _I64, _P]),
    "fury_arrow_ipc_schema": (ctypes.c_int, [_P, _P, _I64, ctypes.POINTER(_I64)]),
    "fury_arrow_ipc_record_batch": (ctypes.c_int, [_P, ctypes.POINTER(FuryColumn), _I64, _P, _I64,
                                                   ctypes.POINTER(_I64), _P]),
}

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with "
                              "`python -c 'import __graft_entry__ as g; g.build()'`")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            if os.environ.get("FURY_ROW_LIB") and not hasattr(L, name):
                continue          # an older build for A/B: entry points it predates stay unbound
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def last_error() -> str:
    buf = ctypes.create_string_buffer(4096)
    lib().fury_last_error(buf, len(buf))
    return buf.value.decode("utf-8", "replace")
