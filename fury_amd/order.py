"""The order of rows by key fields (fury_row_compare, compare.hip; fury_row_order_words, order.hip).

``compare_rows`` answers "which of two rows' key fields is smaller?" from the row bytes, for pairs of
two ``KeySide``s; ``order_words`` turns one chunk of one key field into int64 words whose integer
order is the rows' order, so that ``torch.sort`` can order rows by STRING, BINARY, DECIMAL and
multi-field keys.  On top of them: ``argsort_rows`` / ``sort_rows`` (ORDER BY, top-k as
``argsort_rows(...)[:k]``), ``is_sorted``, and ``search_sorted`` (lower / upper bounds by binary search:
range partitioning and merge joins).  The numbered rules are in ``include/fury_row.h``.  Like
``keys.py`` these are module-level functions, not ``RowEncoder`` methods.
"""
from __future__ import annotations

import ctypes
from typing import Callable, Optional, Sequence

import torch

from . import _native as N
from .encoder import IllegalArgumentException, RowBatch, RowEncoder, _check, _on, _ptr, _stream_handle
from .keys import KeySide, _c_side, _num_pairs, _selected

__all__ = ["order_flags", "compare_into", "bind_compare", "compare_rows", "order_words_into",
           "order_words", "word_continues", "refine_order", "argsort_rows", "sort_rows", "is_sorted",
           "search_bounds", "search_sorted"]

_MORE = 9                                        # low byte of a word whose value continues past the chunk


def order_flags(num_keys: int, descending=False, nulls_last=False) -> list:
    """The FURY_ORDER_* flags of ``num_keys`` key positions: ``descending`` and ``nulls_last`` are a
    bool for every key or one bool per key."""
    def per_key(x, name):
        if isinstance(x, (bool, int)):
            return [bool(x)] * num_keys
        x = [bool(v) for v in x]
        if len(x) != num_keys:
            raise IllegalArgumentException(f"{name} has {len(x)} entries for {num_keys} keys")
        return x
    d, nl = per_key(descending, "descending"), per_key(nulls_last, "nulls_last")
    return [(N.ORDER_DESC if a else 0) | (N.ORDER_NULLS_LAST if b else 0) for a, b in zip(d, nl)]


# ---- fury_row_compare ---------------------------------------------------------------------------------------
def _compare_args(left: KeySide, right: KeySide, out, descending, nulls_last, stream, keep: list):
    n = _num_pairs(left, right)
    il, ir = _selected(left), _selected(right)
    if len(il) != len(ir):
        raise IllegalArgumentException(f"{len(il)} left keys against {len(ir)} right keys")
    if not isinstance(out, torch.Tensor) or out.dtype != torch.int8:
        raise IllegalArgumentException("out must be an int8 tensor")
    if out.numel() < n:
        raise IllegalArgumentException(f"out has {out.numel()} entries for {n} pairs")
    flags = order_flags(len(il), descending, nulls_last)
    cf = (ctypes.c_int32 * max(len(flags), 1))(*flags)
    keep.append(cf)
    cl, cr = _c_side(left, il, keep), _c_side(right, ir, keep)
    return (ctypes.byref(cl), ctypes.byref(cr), len(il), cf, n, _ptr(out) if n else None,
            _stream_handle(stream))


def compare_into(left: KeySide, right: KeySide, out: torch.Tensor, descending=False, nulls_last=False,
                 stream=None) -> None:
    """``out[j]`` (int8) = -1 / 0 / +1: the key fields of row ``left.indices[j]`` of the left batch sort
    before / with / after those of row ``right.indices[j]`` of the right one (``indices=None``: row j).
    Keys decide in key order; a null sorts before every value (``nulls_last``: after), whatever the
    direction; values order as signed integers, floats by IEEE totalOrder of their bits, decimals as
    128-bit integers, strings by unsigned bytes with a prefix first; ``descending`` reverses the value
    order.  Both options take a bool or one bool per key.  The result is 0 exactly where
    ``keys_equal(..., null_equal=True)`` is true.  One call, no host synchronisation, no workspace.  An
    index or a key value outside its batch ranks as null and is reported by ``device_status(stream)``
    with the pair number."""
    keep: list = []
    args = _compare_args(left, right, out, descending, nulls_last, stream, keep)
    if args[4] > 0:                              # no pairs: nothing to do, and an empty tensor has no address
        _check(N.lib().fury_row_compare(*args))


def bind_compare(left: KeySide, right: KeySide, out: torch.Tensor, descending=False, nulls_last=False,
                 stream=None):
    """``compare_into`` bound like ``bind_keys_equal``: keys, flags and pointers resolved once; the
    returned callable re-issues the same call."""
    keep: list = []
    args = _compare_args(left, right, out, descending, nulls_last, stream, keep)
    fn = N.lib().fury_row_compare

    def call():
        if args[4] > 0:
            _check(fn(*args))
    call.keep = (keep, left, right, out, left.encoder._schema, right.encoder._schema)
    return call


def compare_rows(left: KeySide, right: KeySide, descending=False, nulls_last=False,
                 stream=None) -> torch.Tensor:
    """``compare_into`` into a new int8 tensor, one entry per pair, then ``device_status``."""
    n = _num_pairs(left, right)
    with _on(stream):
        out = torch.empty(n, dtype=torch.int8, device=left.encoder.device)
    if n > 0:
        compare_into(left, right, out, descending, nulls_last, stream)
        left.encoder.device_status(stream)
    return out


# ---- fury_row_order_words -----------------------------------------------------------------------------------
def order_words_into(encoder: RowEncoder, batch: RowBatch, key, chunk: int, out_words: torch.Tensor,
                     out_more: Optional[torch.Tensor] = None, indices: Optional[torch.Tensor] = None,
                     descending: bool = False, nulls_last: bool = False, stream=None) -> None:
    """``out_words[j]`` (int64) = the order word of chunk ``chunk`` of key field ``key`` of row
    ``indices[j]`` (``None``: row j): 7 bytes of the value's normalised key bytes and a length byte,
    encoded so that, among rows equal on the earlier chunks, signed comparison of the words is the
    order of ``compare_into`` on this key; see ``word_continues`` for the rows whose next chunk
    decides.  ``out_more`` (one int32 / uint32 entry, optional) becomes 1 when any row continues, else
    0.  One call, no host synchronisation, no workspace."""
    encoder._check_hash(batch)
    (k,) = encoder._select([key])
    if indices is not None:
        if not isinstance(indices, torch.Tensor) or indices.dtype != torch.int64 or not indices.is_contiguous():
            raise IllegalArgumentException("indices must be a contiguous int64 tensor")
        n = indices.numel()
    else:
        n = batch.nrows
    if not isinstance(out_words, torch.Tensor) or out_words.dtype != torch.int64:
        raise IllegalArgumentException("out_words must be an int64 tensor")
    if out_words.numel() < n:
        raise IllegalArgumentException(f"out_words has {out_words.numel()} entries for {n} rows")
    if out_more is not None and (not isinstance(out_more, torch.Tensor) or out_more.numel() < 1 or
                                 out_more.dtype not in (torch.int32, torch.uint32)):
        raise IllegalArgumentException("out_more must be an int32 or uint32 tensor of one entry")
    (flags,) = order_flags(1, descending, nulls_last)
    if n == 0:
        if out_more is not None:
            with _on(stream):
                out_more.zero_()
        return
    _check(N.lib().fury_row_order_words(
        encoder._schema.handle, k, flags, int(chunk), _ptr(batch.rows) if batch.nrows else None,
        _ptr(batch.row_offsets), batch.nrows, _ptr(indices), n, _ptr(out_words), _ptr(out_more),
        _stream_handle(stream)))


def order_words(encoder: RowEncoder, batch: RowBatch, key, chunk: int,
                indices: Optional[torch.Tensor] = None, descending: bool = False,
                nulls_last: bool = False, stream=None):
    """``order_words_into`` into new tensors: ``(words, more)``, ``more`` an int32 device tensor of one
    entry.  No host synchronisation."""
    n = batch.nrows if indices is None else indices.numel()
    with _on(stream):
        words = torch.empty(n, dtype=torch.int64, device=encoder.device)
        more = torch.empty(1, dtype=torch.int32, device=encoder.device)
    order_words_into(encoder, batch, key, chunk, words, more, indices, descending, nulls_last, stream)
    return words, more


def word_continues(words: torch.Tensor, descending: bool = False) -> torch.Tensor:
    """Which order words say "more follows": the value has bytes past the chunk, so among rows with
    this same word the next chunk decides.  A null's word never continues."""
    low = (~words if descending else words) & 0xFF
    return low == _MORE


# ---- ORDER BY -------------------------------------------------------------------------------------------------
def refine_order(n: int, num_keys: int, descending: Sequence[bool],
                 word_source: Callable[[int, int, torch.Tensor], torch.Tensor], device) -> torch.Tensor:
    """The stable permutation that sorts ``n`` rows by ``num_keys`` keys, given only
    ``word_source(key, chunk, rows) -> int64 words`` (the order words of chunk ``chunk`` of key position
    ``key`` for the int64 row tensor ``rows``).  Plain torch on ``device``; ``argsort_rows`` drives it
    with ``order_words``, the CPU tests with a Python model of the words.

    Refinement: ``perm`` and a tie-group id per position (the group's first position).  For every key,
    for chunk 0, 1, ...: the words of the rows still tied, a stable sort of those positions by (group,
    word), groups split where the word changes, and the rows that are alone in their group, or whose
    value has ended, leave the round.  A key ends when nothing continues, everything ends when no ties
    remain.  The tied positions of a group are contiguous and a round only permutes rows inside their
    group, so ties keep source order.  Host synchronisations: one per round (the compaction of the
    rows that continue) and one per key after the first (the compaction of the rows still tied)."""
    perm = torch.arange(n, dtype=torch.int64, device=device)
    if n < 2:
        return perm
    group = torch.zeros(n, dtype=torch.int64, device=device)
    tied = torch.ones(n, dtype=torch.bool, device=device)
    for key in range(num_keys):
        # ascending positions, whole groups; the first key: every row
        cont = perm.clone() if key == 0 else torch.nonzero(tied).reshape(-1)
        chunk = 0
        while cont.numel() > 0:
            rows = perm[cont]
            words = word_source(key, chunk, rows)
            g = group[cont]                                # non-decreasing: ids are first positions
            order = torch.sort(words, stable=True).indices
            if key or chunk:                               # the very first round has one group
                order = order[torch.sort(g[order], stable=True).indices]
            rows, words = rows[order], words[order]
            perm[cont] = rows
            first = torch.ones_like(g, dtype=torch.bool)
            first[1:] = (g[1:] != g[:-1]) | (words[1:] != words[:-1])
            gi = torch.cumsum(first, 0) - 1                # the new group of every entry, 0-based
            group[cont] = cont[first][gi]
            many = torch.bincount(gi)[gi] > 1
            tied[cont] = many
            cont = cont[many & word_continues(words, descending[key])]
            chunk += 1
    return perm


def argsort_rows(encoder: RowEncoder, batch: RowBatch, keys: Sequence, descending=False,
                 nulls_last=False, stream=None) -> torch.Tensor:
    """The int64 permutation that sorts ``batch`` by the key fields ``keys`` under ``compare_into``'s
    order: row ``perm[i]`` is the i-th smallest.  Stable: rows that compare equal keep their source
    order.  ``descending`` / ``nulls_last``: a bool or one per key.  ``refine_order`` over
    ``order_words`` and ``torch.sort``: one round per 7 key bytes that still tie (8-byte keys take two
    rounds, DECIMAL three, a STRING key its longest tied prefix / 7), each round two stable sorts of
    the rows still tied; the host synchronises once per round and once per key.  ``argsort_rows(...)
    [:k]`` is top-k.  Ends with ``device_status``."""
    encoder._check_hash(batch)
    idx = encoder._select(keys)
    if not idx:
        raise IllegalArgumentException("no keys to sort by")
    flags = order_flags(len(idx), descending, nulls_last)
    desc = [bool(f & N.ORDER_DESC) for f in flags]
    last = [bool(f & N.ORDER_NULLS_LAST) for f in flags]

    def source(key, chunk, rows):
        words = torch.empty(rows.numel(), dtype=torch.int64, device=encoder.device)
        order_words_into(encoder, batch, idx[key], chunk, words, None, rows.contiguous(), desc[key],
                         last[key], stream)
        return words
    with _on(stream):
        perm = refine_order(batch.nrows, len(idx), desc, source, encoder.device)
    if batch.nrows > 1:                          # fewer rows: nothing was launched
        encoder.device_status(stream)
    return perm


def sort_rows(encoder: RowEncoder, batch: RowBatch, keys: Sequence, descending=False, nulls_last=False,
              stream=None) -> RowBatch:
    """``batch`` sorted by ``keys``: ``take`` of ``argsort_rows``."""
    perm = argsort_rows(encoder, batch, keys, descending, nulls_last, stream)
    return encoder.take(batch, perm, stream=stream)


def is_sorted(encoder: RowEncoder, batch: RowBatch, keys: Sequence, descending=False, nulls_last=False,
              stream=None) -> bool:
    """Whether every row of ``batch`` sorts before or with its successor: one ``compare_into`` of the
    rows (i, i + 1) and one host read."""
    n = batch.nrows
    if n < 2:
        encoder._check_hash(batch)
        return True
    with _on(stream):
        at = torch.arange(n, dtype=torch.int64, device=encoder.device)
        cmp = compare_rows(KeySide(encoder, batch, keys, at[:-1]), KeySide(encoder, batch, keys, at[1:]),
                           descending, nulls_last, stream)
        return bool((cmp <= 0).all())


def search_bounds(n: int, m: int, compare: Callable[[torch.Tensor], torch.Tensor], right: bool,
                  device) -> torch.Tensor:
    """``m`` binary searches over ``n`` sorted rows at once: ``compare(mid)`` gives, for every probe j,
    the order (-1 / 0 / +1) of sorted row ``mid[j]`` against probe j.  Returns the int64 lower bounds
    (``right``: upper bounds).  ceil(log2(n + 1)) calls, no host synchronisation."""
    lo = torch.zeros(m, dtype=torch.int64, device=device)
    hi = torch.full((m,), n, dtype=torch.int64, device=device)
    for _ in range(int(n).bit_length()):
        open_ = lo < hi
        mid = torch.clamp((lo + hi) >> 1, max=max(n - 1, 0))
        c = compare(mid)
        go_up = (c <= 0) if right else (c < 0)
        lo = torch.where(open_ & go_up, mid + 1, lo)
        hi = torch.where(open_ & ~go_up, mid, hi)
    return lo


def search_sorted(sorted_side: KeySide, probe_side: KeySide, right: bool = False, descending=False,
                  nulls_last=False, stream=None) -> torch.Tensor:
    """For every probe row (``probe_side.indices``, or every row of its batch) the first position in
    the sorted batch whose row does not sort before it (``right``: the first that sorts after it), as
    int64 in [0, n]: ``torch.searchsorted`` for rows.  ``sorted_side`` (``indices`` must be ``None``)
    is sorted under the same ``descending`` / ``nulls_last``.  A binary search in ceil(log2(n + 1))
    ``compare_into`` calls with no host synchronisation; the caller checks ``device_status``.  The
    bounds of a batch's splitter rows are the ids ``partition`` takes (range partitioning); lower and
    upper bounds of one side in the other are a merge join's runs."""
    if sorted_side.indices is not None:
        raise IllegalArgumentException("search_sorted searches a whole sorted batch: indices must be None")
    n = sorted_side.batch.nrows
    m = probe_side.batch.nrows if probe_side.indices is None else probe_side.indices.numel()
    dev = sorted_side.encoder.device
    with _on(stream):
        if n == 0 or m == 0:
            _selected(sorted_side), _selected(probe_side)
            return torch.zeros(m, dtype=torch.int64, device=dev)
        out = torch.empty(m, dtype=torch.int8, device=dev)
        probe = probe_side
        if probe.indices is None:
            probe = probe._replace(indices=torch.arange(m, dtype=torch.int64, device=dev))

        def compare(mid):
            compare_into(sorted_side._replace(indices=mid.contiguous()), probe, out, descending,
                         nulls_last, stream)
            return out
        return search_bounds(n, m, compare, right, dev)
