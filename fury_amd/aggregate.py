"""Per-group aggregates of a row batch (fury_row_aggregate, aggregate.hip).

``aggregate`` finishes a GROUP BY: COUNT / SUM / MIN / MAX of value fields, and the row that holds the
smallest or largest value (ARGMIN / ARGMAX), for every group of a batch whose rows carry a group id --
``group_rows(...).group_ids`` -- straight from the row bytes, in one pass over the row headers, with no
column decoded.  The values, the nulls and the order are those of the key operators; the numbered rules
are in ``include/fury_row.h``.  ``group_by`` is ``group_rows`` + ``aggregate``; ``group_by_rows`` gives
the result as a row batch again.  Like ``fury_amd.group`` this is a set of module-level functions that
take the batch's encoder first.

MIN / MAX of a STRING, BINARY or DECIMAL field is not a word: ask for ``"argmin"`` / ``"argmax"`` and
``take`` the rows whose count is not zero.

``fury_amd.aggregate`` names both this module and its function ``aggregate``: the module is callable
and calls the function, as ``fury_amd.lookup`` does.
"""
from __future__ import annotations

import sys
import types as _pytypes
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _native as N
from . import types as T
from .encoder import (IllegalArgumentException, RowBatch, RowEncoder, _check, _on, _ptr,
                      _stream_handle)
from .group import Groups, group_rows
from .workloads import Column, _t_packbits

__all__ = ["Agg", "AggResult", "aggregate_into", "bind_aggregate", "aggregate", "group_by",
           "group_by_rows", "lds_cells"]


class Agg(NamedTuple):
    """One aggregate: ``op`` is ``"count"``, ``"sum"``, ``"min"``, ``"max"``, ``"argmin"`` or
    ``"argmax"``; ``field`` a field name, a slot index, or ``None`` for ``count(*)``."""
    op: str
    field: object = None


class AggResult(NamedTuple):
    """What ``aggregate`` returns per aggregate (rules 2-5 of fury_row_aggregate)."""
    values: torch.Tensor        # num_groups entries: int64, float64, or float32 for a FLOAT32 min / max
    count: torch.Tensor         # int64[num_groups]: the values that took part; 0: the result is null


def lds_cells() -> int:
    """The dispatch threshold of fury_row_aggregate: ``num_groups * len(aggs)`` up to this many cells
    are combined per workgroup on chip, more with global atomics (``fury_row_aggregate_lds_cells``)."""
    return int(N.lib().fury_row_aggregate_lds_cells())


def _resolve(encoder: RowEncoder, aggs: Sequence) -> List[Tuple[int, int]]:
    """(op code, slot) of every aggregate; -1 is ``count(*)``."""
    if not 1 <= len(aggs) <= N.AGG_MAX_AGGS:
        raise IllegalArgumentException(f"{len(aggs)} aggregates: 1 to {N.AGG_MAX_AGGS} per call")
    out = []
    for a in aggs:
        op, field = a
        if op not in N.AGG_OPS:
            raise IllegalArgumentException(f"unknown aggregate op {op!r}: one of {sorted(N.AGG_OPS)}")
        if field is None:
            if op != "count":
                raise IllegalArgumentException(f"{op} needs a field; only count takes None (count(*))")
            out.append((N.AGG_OPS[op], -1))
        else:
            out.append((N.AGG_OPS[op], encoder._select([field])[0]))
    return out


def _kind(encoder: RowEncoder, op: int, slot: int) -> str:
    """The natural dtype of an aggregate's values: "i8", "f8", or "f4" (a FLOAT32 min / max)."""
    if slot < 0 or op in (N.AGG_OPS["count"], N.AGG_OPS["argmin"], N.AGG_OPS["argmax"]):
        return "i8"
    t = encoder._schema.fields[slot].type_id
    if t == T.FLOAT64 or (t == T.FLOAT32 and op == N.AGG_OPS["sum"]):
        return "f8"
    return "f4" if t == T.FLOAT32 else "i8"


def _args(encoder: RowEncoder, batch: RowBatch, group_ids, num_groups, aggs, outs, counts, stream,
          keep: list):
    """Every check the host can make without the library, then the call's arguments (``None`` when
    rule 6 has nothing to write: empty tensors have no address to pass)."""
    encoder._check_hash(batch)
    spec = _resolve(encoder, aggs)
    n, G = batch.nrows, int(num_groups)
    if G < 0:
        raise IllegalArgumentException("num_groups < 0")
    if group_ids is None:
        if G != 1:
            raise IllegalArgumentException(f"group_ids is None: num_groups must be 1, not {G}")
    else:
        if not isinstance(group_ids, torch.Tensor) or group_ids.dtype != torch.int64:
            raise IllegalArgumentException("group_ids must be an int64 tensor")
        if group_ids.numel() < n:
            raise IllegalArgumentException(f"group_ids has {group_ids.numel()} entries for {n} rows")
    if len(outs) != len(spec):
        raise IllegalArgumentException(f"{len(outs)} outputs for {len(spec)} aggregates")
    if counts is not None and len(counts) != len(spec):
        raise IllegalArgumentException(f"{len(counts)} counts for {len(spec)} aggregates")
    recs = (N.FuryAgg * len(spec))()
    for j, (op, slot) in enumerate(spec):
        t = outs[j]
        if not isinstance(t, torch.Tensor):
            raise IllegalArgumentException(f"outs[{j}] must be a tensor")
        need, allowed = G, (torch.int64, torch.float64)
        if _kind(encoder, op, slot) == "f4" and t.dtype == torch.float32:
            need, allowed = 2 * G, (torch.float32,)
        if t.dtype not in allowed:
            raise IllegalArgumentException(
                f"outs[{j}] must be an int64 or float64 tensor (float32 of twice the entries for a "
                "FLOAT32 min / max)")
        if t.numel() < need:
            raise IllegalArgumentException(f"outs[{j}] has {t.numel()} entries, {need} needed")
        c = None if counts is None else counts[j]
        if c is not None:
            if not isinstance(c, torch.Tensor) or c.dtype != torch.int64:
                raise IllegalArgumentException(f"counts[{j}] must be an int64 tensor")
            if c.numel() < G:
                raise IllegalArgumentException(f"counts[{j}] has {c.numel()} entries, {G} needed")
    if G == 0:
        return None
    for j, (op, slot) in enumerate(spec):
        recs[j].field, recs[j].op = slot, op
        recs[j].out = _ptr(outs[j])
        recs[j].out_count = None if counts is None else _ptr(counts[j])
    keep.append(recs)
    # no rows: group_ids is never read, but NULL would mean "one group"; any valid pointer stands in
    ids = None if group_ids is None else _ptr(group_ids) if n else recs[0].out
    return (encoder._schema.handle, _ptr(batch.rows) if n else None,
            _ptr(batch.row_offsets) if n else None, n, ids, G, recs, len(spec), _stream_handle(stream))


def aggregate_into(encoder: RowEncoder, batch: RowBatch, group_ids: Optional[torch.Tensor],
                   num_groups: int, aggs: Sequence, outs: Sequence[torch.Tensor],
                   counts: Optional[Sequence[Optional[torch.Tensor]]] = None, stream=None) -> None:
    """One fury_row_aggregate call into the caller's tensors.  ``group_ids`` (int64, ``nrows`` entries,
    or ``None``: every row in group 0, ``num_groups`` 1) names each row's group; a row whose id is
    outside ``[0, num_groups)`` takes part in nothing, which is how a WHERE mask is applied.  ``aggs``:
    1 to 16 ``Agg(op, field)``.  ``outs[i]`` (int64 or float64, ``num_groups`` entries; for a FLOAT32
    min / max also float32 of ``2 * num_groups`` entries, the value in every even entry) receives
    aggregate i as rules 2-5 store it, ``counts[i]`` (optional, int64) the number of values that took
    part: 0 is the result's null flag.  Every entry is written whatever the ids hold.  One call, no
    host synchronisation; workspace 24 bytes per group and aggregate.  A row or value outside the batch
    takes no part and is reported by ``device_status(stream)``.  ``num_groups == 0`` launches nothing.
    MIN / MAX of STRING, BINARY and DECIMAL: ``take`` at the ``"argmin"`` / ``"argmax"`` rows whose
    count is not zero."""
    keep: list = []
    args = _args(encoder, batch, group_ids, num_groups, aggs, outs, counts, stream, keep)
    if args is not None:
        _check(N.lib().fury_row_aggregate(*args))


def bind_aggregate(encoder: RowEncoder, batch: RowBatch, group_ids: Optional[torch.Tensor],
                   num_groups: int, aggs: Sequence, outs: Sequence[torch.Tensor],
                   counts: Optional[Sequence[Optional[torch.Tensor]]] = None, stream=None):
    """``aggregate_into`` bound like ``bind_group``: fields and pointers resolved once; the returned
    callable re-issues the same call."""
    keep: list = []
    args = _args(encoder, batch, group_ids, num_groups, aggs, outs, counts, stream, keep)
    if args is None:
        return lambda: None
    return encoder._bound(N.lib().fury_row_aggregate, args, keep, batch, group_ids, list(outs),
                          None if counts is None else list(counts))


def aggregate(encoder: RowEncoder, batch: RowBatch, group_ids: Optional[torch.Tensor], num_groups: int,
              aggs: Sequence, stream=None) -> List[AggResult]:
    """``[AggResult(values, count)]`` per aggregate, ``num_groups`` entries each, after
    ``device_status``.  ``values`` has the natural dtype: int64 for integer results, BOOL / DATE32 /
    TIMESTAMP min / max, counts and the row numbers of argmin / argmax (-1: no value); float64 for
    float sums and FLOAT64 min / max; float32 for a FLOAT32 min / max.  MIN / MAX of STRING, BINARY
    and DECIMAL: ``take`` at the argmin / argmax rows whose count is not zero."""
    spec = _resolve(encoder, aggs)
    G = int(num_groups)
    with _on(stream):
        outs = [torch.empty(max(G, 0), dtype=torch.int64, device=encoder.device) for _ in spec]
        counts = [torch.empty(max(G, 0), dtype=torch.int64, device=encoder.device) for _ in spec]
    aggregate_into(encoder, batch, group_ids, G, aggs, outs, counts, stream)
    if G > 0:
        encoder.device_status(stream)
    res = []
    for (op, slot), o, c in zip(spec, outs, counts):
        kind = _kind(encoder, op, slot)
        with _on(stream):
            v = o if kind == "i8" else o.view(torch.float64) if kind == "f8" else \
                o.view(torch.float32)[0::2].contiguous()
        res.append(AggResult(v, c))
    return res


def group_by(encoder: RowEncoder, batch: RowBatch, keys: Sequence, aggs: Sequence,
             stream=None) -> Tuple[Groups, List[AggResult]]:
    """``(Groups, [AggResult])``: ``group_rows`` by ``keys``, then ``aggregate`` under its ids.  Group g
    of every result is the group whose first row is ``groups.group_rows[g]``."""
    _resolve(encoder, aggs)
    g = group_rows(encoder, batch, keys, stream)
    return g, aggregate(encoder, batch, g.group_ids, g.num_groups, aggs, stream)


def group_by_rows(encoder: RowEncoder, batch: RowBatch, keys: Sequence, aggs: Sequence,
                  names: Sequence[str], stream=None) -> Tuple[RowBatch, RowEncoder]:
    """The GROUP BY result as rows: one row per group, in order of first occurrence, holding the key
    fields followed by one nullable field per aggregate named by ``names`` -- INT64 (integer results,
    counts, argmin / argmax row numbers) or FLOAT64 (float results), null where no value took part.
    Returns ``(RowBatch, RowEncoder)``.  The key fields are ``select_fields`` of ``take`` at the first
    rows, the aggregate fields are encoded from the result tensors, ``zip_fields`` joins the two."""
    if len(names) != len(aggs):
        raise IllegalArgumentException(f"{len(names)} names for {len(aggs)} aggregates")
    groups, res = group_by(encoder, batch, keys, aggs, stream)
    G = groups.num_groups
    key_enc = encoder.selected_encoder(keys)
    key_rows = encoder.select_fields(encoder.take(batch, groups.group_rows, stream), keys, stream)
    fields, cols = [], []
    with _on(stream):
        for name, r in zip(names, res):
            isfloat = r.values.dtype.is_floating_point
            fields.append(T.field(name, T.FLOAT64 if isfloat else T.INT64))
            valid = r.count > 0
            v = r.values.to(torch.float64 if isfloat else torch.int64)
            cols.append(Column(values=torch.where(valid, v, torch.zeros_like(v)).contiguous(),
                               validity=_t_packbits(valid)))
    agg_enc = RowEncoder(fields, encoder.device)
    agg_rows = agg_enc.encode_batch(cols, G, stream)
    nk = len(key_enc._schema.fields)
    picks = [(0, k) for k in range(nk)] + [(1, j) for j in range(len(fields))]
    out_enc = key_enc.zipped_encoder([agg_enc], picks)
    return key_enc.zip_fields(key_rows, [(agg_enc, agg_rows)], picks, stream), out_enc


class _CallableModule(_pytypes.ModuleType):
    """``fury_amd.aggregate(encoder, batch, ...)``: the package attribute ``aggregate`` is this module
    once it is imported, so calling the module calls its function ``aggregate``."""

    def __call__(self, *args, **kwargs):
        return aggregate(*args, **kwargs)


sys.modules[__name__].__class__ = _CallableModule
