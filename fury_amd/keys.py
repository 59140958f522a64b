"""Key equality and equi-join of row batches (fury_row_keys_equal, keys_equal.hip).

The operation is symmetric in two encoders, so it is a set of module-level functions over two
``KeySide``s, not a method of one encoder.  ``keys_equal`` answers "do the key fields of row i of one
batch equal the key fields of row j of another?" from the row bytes (the numbered rules are in
``include/fury_row.h``); ``candidate_pairs`` turns two hash arrays into the pairs whose hashes agree,
in plain torch; ``join_pairs`` composes them with ``RowEncoder.hash_rows`` into the matching row
pairs of an equi-join.  Group-by and de-duplication are ``fury_amd.group_rows`` / ``distinct``
(fury_row_group), linear in the rows; a batch joined with itself is a join, quadratic in a group.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Sequence

import torch

from . import _native as N
from .encoder import (IllegalArgumentException, RowBatch, RowEncoder, _check, _on, _ptr,
                      _stream_handle)

__all__ = ["KeySide", "keys_equal_into", "bind_keys_equal", "keys_equal", "candidate_pairs",
           "join_pairs"]


class KeySide(NamedTuple):
    """One side of a key comparison: the ``encoder`` of ``batch``, the key fields ``keys`` (names or
    slot indices, in key order) and the rows to compare, ``indices`` (an int64 device tensor, one
    entry per pair; ``None``: pair j uses row j)."""
    encoder: RowEncoder
    batch: RowBatch
    keys: Sequence
    indices: Optional[torch.Tensor] = None


def _num_pairs(left: KeySide, right: KeySide) -> int:
    counts = []
    for name, side in (("left", left), ("right", right)):
        idx = side.indices
        if idx is None:
            continue
        if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int64 or not idx.is_contiguous():
            raise IllegalArgumentException(f"{name}.indices must be a contiguous int64 tensor")
        if idx.device != side.batch.rows.device:
            raise IllegalArgumentException(f"{name}.indices must be on the batch's device")
        counts.append(idx.numel())
    if len(counts) == 2 and counts[0] != counts[1]:
        raise IllegalArgumentException(
            f"left.indices has {counts[0]} entries, right.indices has {counts[1]}")
    if counts:
        return counts[0]
    if left.batch.nrows != right.batch.nrows:
        raise IllegalArgumentException(
            f"without indices the batches pair row by row: {left.batch.nrows} rows against "
            f"{right.batch.nrows}")
    return left.batch.nrows


def _selected(side: KeySide):
    side.encoder._check_hash(side.batch)
    return side.encoder._select(side.keys)


def _c_side(side: KeySide, idx, keep: list):
    batch = side.batch
    sel = (ctypes.c_int32 * max(len(idx), 1))(*idx)
    c = N.FuryKeySide()
    c.schema = side.encoder._schema.handle
    c.fields = sel
    c.rows = _ptr(batch.rows) if batch.nrows else None
    c.row_offsets = _ptr(batch.row_offsets)
    c.nrows = batch.nrows
    c.indices = _ptr(side.indices) if side.indices is not None and side.indices.numel() else None
    keep += [sel, c]
    return c


def _args(left: KeySide, right: KeySide, out_equal, out_mask, null_equal, stream, keep: list):
    """Every check the host can make without the library, then the call's arguments."""
    n = _num_pairs(left, right)
    il, ir = _selected(left), _selected(right)
    if len(il) != len(ir):
        raise IllegalArgumentException(f"{len(il)} left keys against {len(ir)} right keys")
    if out_equal is not None:
        if not isinstance(out_equal, torch.Tensor) or out_equal.dtype not in (torch.uint8, torch.bool):
            raise IllegalArgumentException("out_equal must be a uint8 or bool tensor")
        if out_equal.numel() < n:
            raise IllegalArgumentException(f"out_equal has {out_equal.numel()} entries for {n} pairs")
    if out_mask is not None:
        if not isinstance(out_mask, torch.Tensor) or out_mask.dtype not in (torch.int32, torch.uint32):
            raise IllegalArgumentException("out_mask must be an int32 or uint32 tensor")
        if out_mask.numel() < (n + 31) // 32:
            raise IllegalArgumentException(
                f"out_mask has {out_mask.numel()} words for {n} pairs ({(n + 31) // 32} needed)")
    cl, cr = _c_side(left, il, keep), _c_side(right, ir, keep)
    return (ctypes.byref(cl), ctypes.byref(cr), len(il), n, N.KEYS_NULL_EQUAL if null_equal else 0,
            _ptr(out_equal), _ptr(out_mask), _stream_handle(stream))


def keys_equal_into(left: KeySide, right: KeySide, out_equal: Optional[torch.Tensor] = None,
                    out_mask: Optional[torch.Tensor] = None, null_equal: bool = False,
                    stream=None) -> None:
    """Pair j compares the key fields of row ``left.indices[j]`` of the left batch with those of row
    ``right.indices[j]`` of the right one (``indices=None``: row j), key position by key position:
    equal when both values are non-null with the same bytes -- the bytes ``project_batch`` would
    decode, floats as raw bits -- or both are null and ``null_equal`` is set.  ``out_equal`` (uint8
    or bool, one entry per pair) receives 0 / 1, ``out_mask`` (int32 or uint32, ``(pairs + 31) //
    32`` words, LSB first: the bitmap ``filter_into`` takes) the same bits; either may be ``None``,
    not both.  The number of pairs is the length of whichever ``indices`` is given (both lengths
    must agree); with neither, both batches have the same number of rows.  The two schemas need
    only agree on the key fields' types.  One call, no host synchronisation, no workspace.  An
    index or a key value outside its batch makes the pair unequal, reported by
    ``device_status(stream)`` with the pair number."""
    keep: list = []
    args = _args(left, right, out_equal, out_mask, null_equal, stream, keep)
    if args[3] > 0:                              # no pairs: nothing to do, and an empty tensor has no address
        _check(N.lib().fury_row_keys_equal(*args))


def bind_keys_equal(left: KeySide, right: KeySide, out_equal: Optional[torch.Tensor] = None,
                    out_mask: Optional[torch.Tensor] = None, null_equal: bool = False, stream=None):
    """``keys_equal_into`` bound like ``RowEncoder.bind_hash``: keys and pointers resolved once; the
    returned callable re-issues the same call."""
    keep: list = []
    args = _args(left, right, out_equal, out_mask, null_equal, stream, keep)
    fn = N.lib().fury_row_keys_equal

    def call():
        if args[3] > 0:
            _check(fn(*args))
    call.keep = (keep, left, right, out_equal, out_mask, left.encoder._schema, right.encoder._schema)
    return call


def keys_equal(left: KeySide, right: KeySide, null_equal: bool = False, stream=None) -> torch.Tensor:
    """``keys_equal_into`` into a new bool tensor, one entry per pair, then ``device_status``."""
    n = _num_pairs(left, right)
    with _on(stream):
        out = torch.empty(n, dtype=torch.bool, device=left.encoder.device)
    if n > 0:                                    # an empty tensor has no address to pass
        keys_equal_into(left, right, out, None, null_equal, stream)
        left.encoder.device_status(stream)
    return out


def candidate_pairs(left_hashes: torch.Tensor, right_hashes: torch.Tensor,
                    max_pairs: Optional[int] = None):
    """All ``(i, j)`` with ``left_hashes[i] == right_hashes[j]``, sorted by ``(i, j)``, as two int64
    tensors on the hashes' device: plain torch, any device.  The right hashes are sorted (stable),
    each left hash finds its run with two ``searchsorted`` calls, and the runs are expanded; the
    total is read by the host once.  One hot hash on both sides is quadratic: when the total
    exceeds ``max_pairs`` an ``IllegalArgumentException`` states it before the pairs are
    allocated."""
    def as_i32(h):                               # any order will do, as long as both sides use it
        h = h.reshape(-1)
        return h.view(torch.int32) if h.dtype == torch.uint32 else h
    lh, rh = as_i32(left_hashes), as_i32(right_hashes)
    if lh.dtype != rh.dtype or lh.device != rh.device:
        raise IllegalArgumentException("the two hash tensors differ in dtype or device")
    dev = lh.device
    if lh.numel() == 0 or rh.numel() == 0:
        return (torch.empty(0, dtype=torch.int64, device=dev),
                torch.empty(0, dtype=torch.int64, device=dev))
    sorted_rh, order = torch.sort(rh, stable=True)
    lo = torch.searchsorted(sorted_rh, lh, right=False)
    hi = torch.searchsorted(sorted_rh, lh, right=True)
    counts = hi - lo
    ends = torch.cumsum(counts, 0)
    total = int(ends[-1].item())
    if max_pairs is not None and total > max_pairs:
        raise IllegalArgumentException(
            f"{total} candidate pairs exceed max_pairs {max_pairs}: a hot key on both sides is "
            f"quadratic")
    li = torch.repeat_interleave(torch.arange(lh.numel(), dtype=torch.int64, device=dev), counts,
                                 output_size=total)
    # position of each pair inside its run, then the run's start in the sorted right side
    within = torch.arange(total, dtype=torch.int64, device=dev) - (ends - counts)[li]
    ri = order[lo[li] + within]
    return li, ri


def join_pairs(left: KeySide, right: KeySide, null_equal: bool = False, seed: int = 0,
               max_pairs: Optional[int] = None, stream=None):
    """The inner equi-join of two batches by key fields: every ``(i, j)`` such that the keys of
    left row i equal the keys of right row j (``keys_equal_into``'s rule), sorted by ``(i, j)``, as
    two int64 device tensors ``(left_rows, right_rows)``.  ``take`` on both sides and
    ``zip_fields`` turn them into joined rows.  Both sides are hashed with ``hash_rows`` under the
    same ``seed``, ``candidate_pairs`` pairs equal hashes (``max_pairs`` bounds them), and
    ``keys_equal`` keeps the candidates whose keys really are equal, so a hash collision never
    joins.  Sides must have ``indices=None``.  An empty side gives two empty tensors and launches
    nothing.  Synchronises with the host twice: once for the candidate count, once for the match
    count."""
    if left.indices is not None or right.indices is not None:
        raise IllegalArgumentException("join_pairs joins whole batches: indices must be None")
    dev = left.encoder.device
    if left.batch.nrows == 0 or right.batch.nrows == 0:
        left.encoder._check_hash(left.batch)
        right.encoder._check_hash(right.batch)
        return (torch.empty(0, dtype=torch.int64, device=dev),
                torch.empty(0, dtype=torch.int64, device=dev))
    lh = left.encoder.hash_rows(left.batch, left.keys, seed=seed, stream=stream)
    rh = right.encoder.hash_rows(right.batch, right.keys, seed=seed, stream=stream)
    with _on(stream):
        li, ri = candidate_pairs(lh, rh, max_pairs)
    if li.numel() == 0:
        return li, ri
    eq = keys_equal(left._replace(indices=li), right._replace(indices=ri), null_equal, stream)
    with _on(stream):
        return li[eq], ri[eq]
