"""WHERE masks from conditions on the rows (fury_row_predicate, predicate.hip).

``predicate_mask`` answers "which rows pass this condition on their fields?" from the row bytes, as
the bit mask ``filter``, ``update_fields`` and ``semi_join`` speak: nothing is decoded, up to 32 tests
share one pass over the row headers, and STRING / BINARY / DECIMAL fields are tested where they lie.
A predicate is a conjunction of clauses; a clause is one ``Term`` or a sequence of ``Term``s that are
OR-ed::

    where(enc, batch, [between("a", 10, 20), (eq("s1", "abc"), starts_with("s2", "x")), not_null("c")])

is ``WHERE a BETWEEN 10 AND 20 AND (s1 = 'abc' OR s2 LIKE 'x%') AND c IS NOT NULL``.  Nulls follow
SQL: only ``is_null`` / ``not_null`` are ever true on a null value, with or without negation.  Values
compare in ``compare_into``'s order (floats by totalOrder of their bits: ``eq(f, 0.0)`` does not match
-0.0), so a range predicate selects exactly what ``search_sorted`` delimits in the sorted batch.  The
numbered rules are in ``include/fury_row.h``.  Like ``order.py`` these are module-level functions, not
``RowEncoder`` methods.
"""
from __future__ import annotations

import ctypes
import decimal
import struct
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import _native as N
from . import types as T
from .encoder import (IllegalArgumentException, RowBatch, RowEncoder, UnsupportedOperationException, _check,
                      _on, _ptr, _stream_handle)

__all__ = ["Term", "eq", "ne", "lt", "le", "gt", "ge", "is_null", "not_null", "starts_with", "ends_with",
           "contains", "between", "literal_bytes", "predicate_into", "bind_predicate", "predicate_mask",
           "where", "count_where"]

_INTS = {T.INT8: 1, T.INT16: 2, T.INT32: 4, T.INT64: 8, T.DATE32: 4, T.TIMESTAMP: 8}
_FLOATS = {T.FLOAT32: "<f", T.FLOAT64: "<d"}
_BYTES = (T.STRING, T.BINARY)
_PATTERNS = ("starts_with", "ends_with", "contains")


class Term(NamedTuple):
    """One test of one field: ``op`` is a key of ``_native.PRED_OPS``, ``value`` the Python literal
    (``None`` for ``"is_null"``), ``negate`` makes the term true where the test is false and the value
    is not null."""
    field: object                                # a field name or slot index
    op: str
    value: object = None
    negate: bool = False


class _Clauses(tuple):
    """Several clauses that stand where one does: ``between`` is two."""


def eq(field, value) -> Term:
    return Term(field, "eq", value)


def ne(field, value) -> Term:
    """``field <> value``: false on a null, as in SQL."""
    return Term(field, "eq", value, True)


def lt(field, value) -> Term:
    return Term(field, "lt", value)


def le(field, value) -> Term:
    return Term(field, "le", value)


def gt(field, value) -> Term:
    return Term(field, "gt", value)


def ge(field, value) -> Term:
    return Term(field, "ge", value)


def is_null(field) -> Term:
    return Term(field, "is_null")


def not_null(field) -> Term:
    return Term(field, "is_null", None, True)


def starts_with(field, value) -> Term:
    """``LIKE 'value%'`` with no wildcard inside ``value``: byte-wise on the payload."""
    return Term(field, "starts_with", value)


def ends_with(field, value) -> Term:
    return Term(field, "ends_with", value)


def contains(field, value) -> Term:
    return Term(field, "contains", value)


def between(field, lo, hi):
    """``lo <= field <= hi``: two clauses, used where one clause stands."""
    return _Clauses((ge(field, lo), le(field, hi)))


def literal_bytes(field: T.Field, op: str, value) -> bytes:
    """The literal of a term on ``field`` as rule 2 of fury_row_predicate wants it: the value's bytes as
    the projected decode would produce them.  Integers are range-checked at the field's width, floats
    are packed at it, a STRING / BINARY takes ``str`` (UTF-8) or ``bytes``.  A DECIMAL takes an ``int``,
    the unscaled value, or a ``decimal.Decimal``, whose own digits are the unscaled value: the schema
    carries no scale, so the Decimal must be written at the column's scale (``Decimal("1.50")`` for a
    scale of 2 is 150, ``Decimal("1.5")`` is 15; ``value.quantize(Decimal("0.01"))`` brings it there).  A
    Decimal with a positive exponent (``Decimal("1E+2")``) is at no column's scale and is rejected."""
    tid = field.type_id
    what = f"{op} on field {field.name!r} ({T.TYPE_NAMES.get(tid, tid)})"
    if op not in N.PRED_OPS:
        raise IllegalArgumentException(f"unknown predicate op {op!r}: one of {sorted(N.PRED_OPS)}")
    if tid in (T.LIST, T.STRUCT, T.MAP):
        raise UnsupportedOperationException(
            f"{what}: a LIST / STRUCT / MAP cannot be tested from the row bytes; project or extract it")
    if op == "is_null":
        if value is not None:
            raise IllegalArgumentException(f"{what}: is_null takes no value")
        return b""
    if op in _PATTERNS and tid not in _BYTES:
        raise UnsupportedOperationException(f"{what}: {op} takes STRING / BINARY fields")
    if value is None:
        raise IllegalArgumentException(f"{what}: the value is None; test nulls with is_null / not_null")
    isint = isinstance(value, int) and not isinstance(value, bool)
    if tid == T.BOOL:
        if not isinstance(value, bool):
            raise IllegalArgumentException(f"{what}: {value!r} is not a bool")
        return b"\x01" if value else b"\x00"
    if tid in _INTS:
        w = _INTS[tid]
        if not isint:
            raise IllegalArgumentException(f"{what}: {value!r} is not an int")
        if not -(1 << (8 * w - 1)) <= value < 1 << (8 * w - 1):
            raise IllegalArgumentException(f"{what}: {value} does not fit {8 * w} bits")
        return value.to_bytes(w, "little", signed=True)
    if tid in _FLOATS:
        if not (isinstance(value, float) or isint):
            raise IllegalArgumentException(f"{what}: {value!r} is not a float")
        try:
            return struct.pack(_FLOATS[tid], value)
        except (OverflowError, struct.error) as e:
            raise IllegalArgumentException(f"{what}: {value!r} does not fit the field's width: {e}") from None
    if tid == T.DECIMAL:
        if isinstance(value, decimal.Decimal):
            sign, digits, exp = value.as_tuple()
            if not isinstance(exp, int):
                raise IllegalArgumentException(f"{what}: {value!r} is not finite")
            if exp > 0:
                raise IllegalArgumentException(
                    f"{what}: {value!r} has a positive exponent; quantize it to the column's scale")
            value = int("".join(map(str, digits)) or "0") * (-1 if sign else 1)
        elif not isint:
            raise IllegalArgumentException(f"{what}: {value!r} is not an int or a decimal.Decimal")
        if not -(1 << 127) <= value < 1 << 127:
            raise IllegalArgumentException(f"{what}: {value} does not fit 128 bits")
        return value.to_bytes(16, "little", signed=True)
    if tid in _BYTES:
        if isinstance(value, str):
            return value.encode("utf-8")
        if isinstance(value, (bytes, bytearray, memoryview)):
            return bytes(value)
        raise IllegalArgumentException(f"{what}: {value!r} is not a str or bytes")
    raise UnsupportedOperationException(f"{what}: no predicate on this type")


def _flatten(predicate) -> list:
    """``[(Term, joins the clause before it)]`` of a predicate: a Term, or a sequence of clauses, each
    a Term, a sequence of Terms that are OR-ed, or ``between``'s pair of clauses."""
    if isinstance(predicate, Term):
        predicate = [predicate]
    elif isinstance(predicate, _Clauses):
        predicate = list(predicate)
    out = []
    for clause in predicate:
        for c in (clause if isinstance(clause, _Clauses) else [clause]):
            terms = [c] if isinstance(c, Term) else list(c)
            if not terms:
                raise IllegalArgumentException("a clause without terms is never true: drop it")
            for j, t in enumerate(terms):
                if not isinstance(t, Term):
                    raise IllegalArgumentException(f"{t!r} is not a Term (between() stands where a clause does)")
                out.append((t, j > 0))
    if not 1 <= len(out) <= N.PRED_MAX_TERMS:
        raise IllegalArgumentException(f"{len(out)} terms: 1 to {N.PRED_MAX_TERMS} per call")
    return out


def _c_terms(encoder: RowEncoder, predicate, keep: list):
    flat = _flatten(predicate)
    recs = (N.FuryPredTerm * len(flat))()
    fields = encoder._schema.fields
    pool = 0
    for j, (t, joins) in enumerate(flat):
        (k,) = encoder._select([t.field])
        if not 0 <= k < len(fields):
            raise IllegalArgumentException(f"field index {k} is not a field of {encoder._schema}")
        lit = literal_bytes(fields[k], t.op, t.value)
        pool += (len(lit) + 7) & ~7
        if pool > N.PRED_MAX_LITERAL_BYTES:
            raise IllegalArgumentException(
                f"the literals take more than {N.PRED_MAX_LITERAL_BYTES} bytes (each rounded up to 8)")
        recs[j].field, recs[j].op = k, N.PRED_OPS[t.op]
        recs[j].flags = (N.PRED_NOT if t.negate else 0) | (N.PRED_OR if joins else 0)
        recs[j].literal_len = len(lit)
        if lit:
            buf = ctypes.create_string_buffer(lit, len(lit))
            keep.append(buf)
            recs[j].literal = ctypes.addressof(buf)
    keep.append(recs)
    return recs, len(flat)


def _mask(t, name: str, n: int):
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.int32, torch.uint32):
        raise IllegalArgumentException(f"{name} must be an int32 or uint32 tensor")
    if t.numel() < (n + 31) // 32:
        raise IllegalArgumentException(f"{name} has {t.numel()} words for {n} rows ({(n + 31) // 32} needed)")


def _args(encoder: RowEncoder, batch: RowBatch, predicate, out_mask, out_count, row_mask, stream, keep: list):
    """Every check the host can make without the library, then the call's arguments (``None`` without
    rows: an empty tensor has no address to pass)."""
    encoder._check_hash(batch)
    recs, nt = _c_terms(encoder, predicate, keep)
    n = batch.nrows
    _mask(out_mask, "out_mask", n)
    if row_mask is not None:
        _mask(row_mask, "row_mask", n)
    if out_count is not None and (not isinstance(out_count, torch.Tensor) or out_count.dtype != torch.int64 or
                                  out_count.numel() < 1):
        raise IllegalArgumentException("out_count must be an int64 tensor of one entry")
    if n == 0:
        return None
    return (encoder._schema.handle, _ptr(batch.rows), _ptr(batch.row_offsets), n, recs, nt, _ptr(row_mask),
            _ptr(out_mask), _ptr(out_count), _stream_handle(stream))


def _no_rows(out_count, stream) -> None:
    if out_count is not None:                    # rule 6: no rows write the count and nothing else
        with _on(stream):
            out_count[:1].zero_()


def predicate_into(encoder: RowEncoder, batch: RowBatch, predicate, out_mask: torch.Tensor,
                   out_count: Optional[torch.Tensor] = None, row_mask: Optional[torch.Tensor] = None,
                   stream=None) -> None:
    """Bit i of ``out_mask`` (int32 or uint32, ``(nrows + 31) // 32`` words, LSB-first: what ``filter``
    reads through ``.view(torch.uint8)``) = row i of ``batch`` passes ``predicate``; whole words are
    written, the bits past ``nrows`` zero.  ``out_count`` (int64, one entry, optional) receives the
    number of rows that pass.  ``row_mask`` (same format, optional) names the rows to examine: a row
    whose bit is 0 is not read and fails; ``row_mask is out_mask`` refines a mask in place.  One call,
    no host synchronisation, no workspace.  A row or value outside the batch counts as null and is
    reported by ``device_status(stream)`` with the row number."""
    keep: list = []
    args = _args(encoder, batch, predicate, out_mask, out_count, row_mask, stream, keep)
    if args is None:
        _no_rows(out_count, stream)
    else:
        _check(N.lib().fury_row_predicate(*args))


def bind_predicate(encoder: RowEncoder, batch: RowBatch, predicate, out_mask: torch.Tensor,
                   out_count: Optional[torch.Tensor] = None, row_mask: Optional[torch.Tensor] = None,
                   stream=None):
    """``predicate_into`` bound like ``bind_compare``: fields, literals and pointers resolved once; the
    returned callable re-issues the same call."""
    keep: list = []
    args = _args(encoder, batch, predicate, out_mask, out_count, row_mask, stream, keep)
    if args is None:
        def call():
            _no_rows(out_count, stream)
        call.keep = (out_count,)
        return call
    return encoder._bound(N.lib().fury_row_predicate, args, keep, batch, out_mask, out_count, row_mask)


def predicate_mask(encoder: RowEncoder, batch: RowBatch, predicate, row_mask: Optional[torch.Tensor] = None,
                   stream=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(mask, count)``: ``predicate_into`` into new device tensors, int32 mask words and a one-entry
    int64 count, then ``device_status``."""
    n = batch.nrows
    with _on(stream):
        mask = torch.empty((n + 31) // 32, dtype=torch.int32, device=encoder.device)
        count = torch.empty(1, dtype=torch.int64, device=encoder.device)
    predicate_into(encoder, batch, predicate, mask, count, row_mask, stream)
    if n > 0:
        encoder.device_status(stream)
    return mask, count


def where(encoder: RowEncoder, batch: RowBatch, predicate, return_indices: bool = False,
          row_mask: Optional[torch.Tensor] = None, stream=None):
    """The rows of ``batch`` that pass ``predicate`` as a new batch (with ``return_indices``: and their
    row numbers): ``predicate_mask``, then ``filter``, on one stream."""
    mask, _ = predicate_mask(encoder, batch, predicate, row_mask, stream)
    if mask.numel() == 0:                        # no rows: filter still wants a mask with an address
        with _on(stream):
            mask = torch.zeros(1, dtype=torch.int32, device=encoder.device)
    return encoder.filter(batch, mask.view(torch.uint8), stream, return_indices)


def count_where(encoder: RowEncoder, batch: RowBatch, predicate, row_mask: Optional[torch.Tensor] = None,
                stream=None) -> int:
    """The number of rows of ``batch`` that pass ``predicate``: ``predicate_mask`` and one host read."""
    _, count = predicate_mask(encoder, batch, predicate, row_mask, stream)
    with _on(stream):
        return int(count.item())
