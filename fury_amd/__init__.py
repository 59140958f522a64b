"""fury_amd — MI355X-native Fury row-format codec (java/fury-format's hot path on gfx950).

Public surface mirrors the reference's Java API (org.apache.fury.format.encoder.Encoders /
RowEncoder, org.apache.fury.format.vectorized.ArrowWriter); the compute runs in hand-written
HIP kernels behind the C ABI in include/fury_row.h (libfury_row.so, built in-tree).
"""
from . import types  # noqa: F401

_KEYS = ("KeySide", "keys_equal_into", "bind_keys_equal", "keys_equal", "candidate_pairs",
         "join_pairs")
_GROUP = ("Groups", "group_rows_into", "bind_group", "group_rows", "group_sizes", "distinct")
_LOOKUP = ("KeyIndex", "index_slots", "build_index_into", "build_index", "lookup_into", "bind_lookup",
           "lookup", "semi_join", "lookup_join_pairs")
_ORDER = ("order_flags", "compare_into", "bind_compare", "compare_rows", "order_words_into", "order_words",
          "word_continues", "refine_order", "argsort_rows", "sort_rows", "is_sorted", "search_bounds",
          "search_sorted")
_AGGREGATE = ("Agg", "AggResult", "aggregate_into", "bind_aggregate", "aggregate", "group_by", "group_by_rows")
_PREDICATE = ("Term", "eq", "ne", "lt", "le", "gt", "ge", "is_null", "not_null", "starts_with", "ends_with",
              "contains", "between", "predicate_into", "bind_predicate", "predicate_mask", "where", "count_where")
__all__ = ["types", "hash_bytes", "hash_null", *_KEYS, *_GROUP, *_LOOKUP, *_ORDER, *_AGGREGATE, *_PREDICATE]


def __getattr__(name):
    """The key-equality and join functions of ``fury_amd.keys``, the group functions of
    ``fury_amd.group`` and the index functions of ``fury_amd.lookup``, imported on first use (they need torch and the library; ``import fury_amd``
    alone does not)."""
    if name in _KEYS:
        from . import keys
        return getattr(keys, name)
    if name in _GROUP:
        from . import group
        return getattr(group, name)
    if name in _LOOKUP:
        import importlib                          # `from . import lookup` would ask for "lookup" here again
        module = importlib.import_module(".lookup", __name__)
        return module if name == "lookup" else getattr(module, name)      # the module is callable
    if name in _ORDER:                            # fury_amd.order: the order of rows by key fields
        import importlib
        return getattr(importlib.import_module(".order", __name__), name)
    if name in _AGGREGATE:                        # fury_amd.aggregate: per-group aggregates of value fields
        import importlib                          # `from . import aggregate` would ask for "aggregate" here again
        module = importlib.import_module(".aggregate", __name__)
        return module if name == "aggregate" else getattr(module, name)      # the module is callable
    if name in _PREDICATE:                        # fury_amd.predicate: WHERE masks from conditions on the rows
        import importlib
        return getattr(importlib.import_module(".predicate", __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def hash_bytes(b, seed: int = 0) -> int:
    """MurmurHash3_x86_32 of the bytes ``b`` (rule 1 of fury_row_hash in include/fury_row.h): the
    hash ``RowEncoder.hash_rows`` gives a non-null key with these value bytes, on the host.  Chain
    the keys of a row as the device does: ``h = seed``, then ``h = hash_bytes(value, h)`` or
    ``h = hash_null(h)`` per key, and ``h % num_parts`` is the row's partition."""
    from . import _native as N
    b = bytes(b)
    if not 0 <= int(seed) <= 0xFFFFFFFF:
        raise ValueError(f"seed {seed} is not an unsigned 32-bit value")
    return int(N.lib().fury_hash_bytes(b, len(b), int(seed)))


def hash_null(seed: int = 0) -> int:
    """The hash of a null key after ``seed`` (rule 2 of fury_row_hash)."""
    from . import _native as N
    if not 0 <= int(seed) <= 0xFFFFFFFF:
        raise ValueError(f"seed {seed} is not an unsigned 32-bit value")
    return int(N.lib().fury_hash_null(int(seed)))
