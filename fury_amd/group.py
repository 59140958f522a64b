"""Group ids and distinct rows of a row batch by key fields (fury_row_group, group.hip).

``group_rows`` answers "which rows of this batch have the same key?" in time linear in the rows,
however many rows share a key; ``distinct`` keeps the first row of every key.  Two rows are in one
group when ``fury_amd.keys_equal`` would call them equal with ``null_equal=True``; the numbered
rules are in ``include/fury_row.h``.  Like ``fury_amd.keys`` this is a set of module-level functions
that take the batch's encoder first: ``group_rows(encoder, batch, keys)``.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Sequence

import torch

from . import _native as N
from .encoder import (IllegalArgumentException, RowBatch, RowEncoder, _check, _on, _ptr,
                      _stream_handle)

__all__ = ["Groups", "group_rows_into", "bind_group", "group_rows", "group_sizes", "distinct"]


class Groups(NamedTuple):
    """What ``group_rows`` returns (rules 2 and 3 of fury_row_group)."""
    first: torch.Tensor         # int64[nrows]: the smallest row number of each row's group
    group_ids: torch.Tensor     # int64[nrows]: the group's number, in order of first rows
    group_rows: torch.Tensor    # int64[num_groups]: the first row of every group
    num_groups: int


def _args(encoder: RowEncoder, batch: RowBatch, keys: Sequence, out_first, out_group_ids,
          out_group_rows, out_num_groups, hashes, stream, keep: list):
    """Every check the host can make without the library, then the call's arguments (``None`` for an
    empty batch: empty tensors have no address to pass)."""
    encoder._check_hash(batch)
    idx = encoder._select(keys)
    n = batch.nrows
    if out_first is None:
        raise IllegalArgumentException("out_first is required")
    for what, t, need in (("out_first", out_first, n), ("out_group_ids", out_group_ids, n),
                          ("out_group_rows", out_group_rows, n),
                          ("out_num_groups", out_num_groups, 1)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64:
            raise IllegalArgumentException(f"{what} must be an int64 tensor")
        if t.numel() < need:
            raise IllegalArgumentException(f"{what} has {t.numel()} entries, {need} needed")
    if hashes is not None:
        if not isinstance(hashes, torch.Tensor) or hashes.dtype not in (torch.int32, torch.uint32):
            raise IllegalArgumentException("hashes must be an int32 or uint32 tensor")
        if hashes.numel() < n:
            raise IllegalArgumentException(f"hashes has {hashes.numel()} entries for {n} rows")
    sel = (ctypes.c_int32 * max(len(idx), 1))(*idx)
    keep.append(sel)
    if n == 0:
        return None
    return (encoder._schema.handle, sel, len(idx), _ptr(batch.rows), _ptr(batch.row_offsets), n,
            _ptr(hashes), _ptr(out_first), _ptr(out_group_ids), _ptr(out_group_rows),
            _ptr(out_num_groups), _stream_handle(stream))


def group_rows_into(encoder: RowEncoder, batch: RowBatch, keys: Sequence, out_first: torch.Tensor,
                    out_group_ids: Optional[torch.Tensor] = None,
                    out_group_rows: Optional[torch.Tensor] = None,
                    out_num_groups: Optional[torch.Tensor] = None,
                    hashes: Optional[torch.Tensor] = None, stream=None) -> None:
    """Groups the rows of ``batch`` (of ``encoder``'s schema) by the key fields ``keys`` (names or
    slot indices, in key order; the fields ``hash_rows_into`` takes): two rows are in one group when
    every key is equal as ``keys_equal_into`` decides it with ``null_equal=True``.  ``out_first``
    (int64, ``nrows`` entries) receives the smallest row number of each row's group;
    ``out_group_ids`` (optional, int64, ``nrows``) the group's number, groups numbered in order of
    their first rows; ``out_group_rows`` (optional, int64, ``nrows``) the first row of every group,
    -1 past the group count; ``out_num_groups`` (optional, int64[1]) the count.  ``hashes``
    (optional, uint32 or int32, ``nrows``): a hash of the same keys that the caller already has,
    e.g. from ``hash_rows`` with any seed; without it the call hashes the keys itself.  One call, no
    host synchronisation; linear in ``nrows`` whatever the group sizes; workspace at most 48 bytes
    per row.  A row or key value outside the batch is a group of its own, reported by
    ``device_status(stream)``.  An empty batch only zeroes ``out_num_groups``."""
    keep: list = []
    args = _args(encoder, batch, keys, out_first, out_group_ids, out_group_rows, out_num_groups,
                 hashes, stream, keep)
    if args is not None:
        _check(N.lib().fury_row_group(*args))
    elif out_num_groups is not None:
        with _on(stream):
            out_num_groups[:1].zero_()


def bind_group(encoder: RowEncoder, batch: RowBatch, keys: Sequence, out_first: torch.Tensor,
               out_group_ids: Optional[torch.Tensor] = None,
               out_group_rows: Optional[torch.Tensor] = None,
               out_num_groups: Optional[torch.Tensor] = None,
               hashes: Optional[torch.Tensor] = None, stream=None):
    """``group_rows_into`` bound like ``RowEncoder.bind_hash``: keys and pointers resolved once; the
    returned callable re-issues the same call."""
    keep: list = []
    args = _args(encoder, batch, keys, out_first, out_group_ids, out_group_rows, out_num_groups,
                 hashes, stream, keep)
    if args is None:                             # an empty batch: the call of group_rows_into
        return lambda: group_rows_into(encoder, batch, keys, out_first, out_group_ids,
                                       out_group_rows, out_num_groups, hashes, stream)
    return encoder._bound(N.lib().fury_row_group, args, keep, batch, out_first, out_group_ids,
                          out_group_rows, out_num_groups, hashes)


def group_rows(encoder: RowEncoder, batch: RowBatch, keys: Sequence, stream=None) -> Groups:
    """``Groups(first, group_ids, group_rows, num_groups)`` of ``batch`` by ``keys``: int64 device
    tensors as ``group_rows_into`` writes them, ``group_rows`` trimmed to the ``num_groups`` (an
    int) first rows.  One host read, after ``device_status``.  An empty batch launches nothing."""
    n = batch.nrows
    with _on(stream):
        first, ids, rows = (torch.empty(n, dtype=torch.int64, device=encoder.device)
                            for _ in range(3))
        count = torch.zeros(1, dtype=torch.int64, device=encoder.device)
    if n == 0:
        encoder._check_hash(batch)
        encoder._select(keys)
        return Groups(first, ids, rows, 0)
    group_rows_into(encoder, batch, keys, first, ids, rows, count, None, stream)
    encoder.device_status(stream)
    g = int(count.item())
    return Groups(first, ids, rows[:g], g)


def group_sizes(groups: Groups) -> torch.Tensor:
    """The number of rows of every group of ``group_rows``' result: int64, ``num_groups`` entries
    (``torch.bincount`` of the ids)."""
    return torch.bincount(groups.group_ids, minlength=groups.num_groups)


def distinct(encoder: RowEncoder, batch: RowBatch, keys: Sequence, stream=None):
    """``(RowBatch, row numbers)``: the first row of every distinct key of ``batch``, in source
    order -- ``take`` at ``group_rows(encoder, batch, keys).group_rows``."""
    kept = group_rows(encoder, batch, keys, stream).group_rows
    return encoder.take(batch, kept, stream), kept
