"""Key index and lookup: the probe side of a hash join (fury_row_index_build / fury_row_lookup,
group.hip / lookup.hip).

``build_index`` enters the rows of one batch (the build side) into a table on the device, once;
``lookup`` then answers, for every row of any number of probe batches, "is this row's key present in
the build batch, and at which row?": the smallest build row with equal key fields, or -1.  The
numbered rules are in ``include/fury_row.h``.  ``semi_join`` keeps the probe rows that have (or do
not have) a match; ``lookup_join_pairs`` expands build-side duplicates into the full inner join, the
pairs ``join_pairs`` gives.  Like ``fury_amd.keys`` this is a set of module-level functions over
``KeySide``s (whose ``indices`` must be ``None``: whole batches).

``fury_amd.lookup`` names both this module and its function ``lookup``: the module is callable and
calls the function.
"""
from __future__ import annotations

import ctypes
import sys
import types
from typing import NamedTuple, Optional

import torch

from . import _native as N
from .encoder import IllegalArgumentException, _check, _on, _ptr, _stream_handle
from .keys import KeySide, _c_side, _selected

__all__ = ["KeyIndex", "index_slots", "build_index_into", "build_index", "lookup_into", "bind_lookup",
           "lookup", "semi_join", "lookup_join_pairs", "expand_first"]

MAX_ROWS = 2 ** 31 - 1


class KeyIndex(NamedTuple):
    """What ``build_index`` returns: the build ``side``, its ``table`` (int64 device tensor of
    ``index_slots(nrows)`` opaque words), ``first`` (int64[nrows]: the smallest row of each row's
    key, what ``group_rows`` calls first; ``None`` unless asked for) and whether the table was built
    from the caller's hashes (``caller_hashes``: lookups must then bring theirs).  Valid while the
    build batch is unchanged."""
    side: KeySide
    table: torch.Tensor
    first: Optional[torch.Tensor]
    caller_hashes: bool


def index_slots(nrows: int) -> int:
    """The number of 8-byte words of the table of a build batch of ``nrows`` rows: the smallest power
    of two that is at least ``max(2, 2 * nrows)`` (fury_row_index_slots)."""
    nrows = int(nrows)
    if not 0 <= nrows <= MAX_ROWS:
        raise IllegalArgumentException(f"nrows {nrows} is not in [0, {MAX_ROWS}]")
    slots = 2
    while slots < 2 * nrows:
        slots *= 2
    return slots


def _whole(name: str, side: KeySide) -> None:
    if side.indices is not None:
        raise IllegalArgumentException(f"{name}.indices must be None: an index takes whole batches")


def _check_hashes(what: str, hashes, n: int) -> None:
    if hashes is None:
        return
    if not isinstance(hashes, torch.Tensor) or hashes.dtype not in (torch.int32, torch.uint32):
        raise IllegalArgumentException(f"{what} must be an int32 or uint32 tensor")
    if hashes.numel() < n:
        raise IllegalArgumentException(f"{what} has {hashes.numel()} entries for {n} rows")


def _check_table(table, n: int) -> None:
    if not isinstance(table, torch.Tensor) or table.dtype != torch.int64:
        raise IllegalArgumentException("table must be an int64 tensor")
    if table.numel() != index_slots(n):
        raise IllegalArgumentException(
            f"table has {table.numel()} words, index_slots({n}) = {index_slots(n)} needed")


def _build_args(side: KeySide, table, out_first, hashes, stream, keep: list):
    """Every check the host can make without the library, then the call's arguments."""
    _whole("side", side)
    idx = _selected(side)
    n = side.batch.nrows
    _check_table(table, n)
    if out_first is not None:
        if not isinstance(out_first, torch.Tensor) or out_first.dtype != torch.int64:
            raise IllegalArgumentException("out_first must be an int64 tensor")
        if out_first.numel() < n:
            raise IllegalArgumentException(f"out_first has {out_first.numel()} entries, {n} needed")
    _check_hashes("hashes", hashes, n)
    sel = (ctypes.c_int32 * max(len(idx), 1))(*idx)
    keep.append(sel)
    batch = side.batch
    return (side.encoder._schema.handle, sel, len(idx), _ptr(batch.rows) if n else None,
            _ptr(batch.row_offsets) if n else None, n, _ptr(hashes) if n else None, _ptr(table),
            table.numel(), _ptr(out_first) if n else None, _stream_handle(stream))


def build_index_into(side: KeySide, table: torch.Tensor, out_first: Optional[torch.Tensor] = None,
                     hashes: Optional[torch.Tensor] = None, stream=None) -> None:
    """Enters the rows of ``side.batch`` into ``table`` (int64, exactly ``index_slots(nrows)``
    entries, the caller's memory) by the key fields ``side.keys``, as ``group_rows_into`` builds its
    own table: null equals null, one slot per distinct key, holding the key's smallest row once the
    call has completed on ``stream``.  ``out_first`` (optional, int64, ``nrows``) receives
    ``group_rows_into``'s ``out_first``.  ``hashes`` (optional, uint32 or int32, ``nrows``): a hash
    of the same keys that the caller already has; lookups must then be given the same function of
    their keys.  One call, no host synchronisation; workspace 4 bytes per row without ``hashes``
    plus 4 with ``out_first``.  A row or key value outside the batch is not entered, reported by
    ``device_status(stream)``.  An empty batch marks the two slots empty."""
    keep: list = []
    _check(N.lib().fury_row_index_build(*_build_args(side, table, out_first, hashes, stream, keep)))


def build_index(side: KeySide, hashes: Optional[torch.Tensor] = None, want_first: bool = False,
                stream=None) -> KeyIndex:
    """``build_index_into`` into a new table (and ``first`` with ``want_first``, which
    ``lookup_join_pairs`` needs): a ``KeyIndex``.  No host synchronisation."""
    n = side.batch.nrows
    with _on(stream):
        table = torch.empty(index_slots(n), dtype=torch.int64, device=side.encoder.device)
        first = torch.empty(n, dtype=torch.int64, device=side.encoder.device) if want_first else None
    build_index_into(side, table, first, hashes, stream)
    return KeyIndex(side, table, first, hashes is not None)


def _lookup_args(index: KeyIndex, probe: KeySide, out_rows, out_mask, null_equal, hashes, stream,
                 keep: list):
    """Every check the host can make without the library, then the call's arguments."""
    build = index.side
    _whole("probe", probe)
    _whole("index.side", build)
    ip, ib = _selected(probe), _selected(build)
    if len(ip) != len(ib):
        raise IllegalArgumentException(f"{len(ip)} probe keys against {len(ib)} build keys")
    n = probe.batch.nrows
    _check_table(index.table, build.batch.nrows)
    if (hashes is not None) != bool(index.caller_hashes):
        raise IllegalArgumentException(
            "the index was built from the caller's hashes: the lookup needs the same function of its "
            "keys in `hashes`" if index.caller_hashes else
            "the index was built from the call's own hashes: the lookup takes no `hashes`")
    _check_hashes("hashes", hashes, n)
    if out_rows is None and out_mask is None:
        raise IllegalArgumentException("out_rows and out_mask are both None")
    if out_rows is not None:
        if not isinstance(out_rows, torch.Tensor) or out_rows.dtype != torch.int64:
            raise IllegalArgumentException("out_rows must be an int64 tensor")
        if out_rows.numel() < n:
            raise IllegalArgumentException(f"out_rows has {out_rows.numel()} entries for {n} rows")
    if out_mask is not None:
        if not isinstance(out_mask, torch.Tensor) or out_mask.dtype not in (torch.int32, torch.uint32):
            raise IllegalArgumentException("out_mask must be an int32 or uint32 tensor")
        if out_mask.numel() < (n + 31) // 32:
            raise IllegalArgumentException(
                f"out_mask has {out_mask.numel()} words for {n} rows ({(n + 31) // 32} needed)")
    if n == 0:                                   # nothing to do, and an empty tensor has no address
        return None
    cp, cb = _c_side(probe, ip, keep), _c_side(build, ib, keep)
    if build.batch.nrows == 0:
        cb.row_offsets = None
    return (ctypes.byref(cp), ctypes.byref(cb), len(ip), _ptr(index.table), index.table.numel(),
            _ptr(hashes), N.KEYS_NULL_EQUAL if null_equal else 0, _ptr(out_rows), _ptr(out_mask),
            _stream_handle(stream))


def lookup_into(index: KeyIndex, probe: KeySide, out_rows: Optional[torch.Tensor] = None,
                out_mask: Optional[torch.Tensor] = None, null_equal: bool = False,
                hashes: Optional[torch.Tensor] = None, stream=None) -> None:
    """For every row j of ``probe.batch``: ``out_rows[j]`` (int64, one entry per probe row) = the
    smallest row of the index's build batch whose key fields equal those of row j as
    ``keys_equal_into`` decides it (``null_equal``: a null key equals a null key; without it a probe
    row with a null key matches nothing), or -1; bit j of ``out_mask`` (int32 or uint32,
    ``(nrows + 31) // 32`` words, LSB first: the bitmap ``filter_into`` takes) = found.  Either may
    be ``None``, not both.  ``hashes``: required exactly when the index was built with the caller's
    hashes -- the same function of the probe keys.  The two schemas need only agree on the key
    fields' types.  One call, no host synchronisation; workspace 4 bytes per probe row without
    ``hashes``.  A probe row or key value outside its batch finds nothing, reported by
    ``device_status(stream)`` with the row.  An empty probe batch launches nothing."""
    keep: list = []
    args = _lookup_args(index, probe, out_rows, out_mask, null_equal, hashes, stream, keep)
    if args is not None:
        _check(N.lib().fury_row_lookup(*args))


def bind_lookup(index: KeyIndex, probe: KeySide, out_rows: Optional[torch.Tensor] = None,
                out_mask: Optional[torch.Tensor] = None, null_equal: bool = False,
                hashes: Optional[torch.Tensor] = None, stream=None):
    """``lookup_into`` bound like ``bind_group``: keys and pointers resolved once; the returned
    callable re-issues the same call."""
    keep: list = []
    args = _lookup_args(index, probe, out_rows, out_mask, null_equal, hashes, stream, keep)
    if args is None:                             # an empty probe batch: nothing to issue
        return lambda: None
    return probe.encoder._bound(N.lib().fury_row_lookup, args, keep, index, probe, out_rows, out_mask,
                                hashes, index.side.encoder._schema)


def lookup(index: KeyIndex, probe: KeySide, null_equal: bool = False,
           hashes: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
    """``lookup_into`` into a new int64 tensor, one entry per probe row, then ``device_status``."""
    n = probe.batch.nrows
    with _on(stream):
        out = torch.empty(n, dtype=torch.int64, device=probe.encoder.device)
    lookup_into(index, probe, out, None, null_equal, hashes, stream)
    if n > 0:
        probe.encoder.device_status(stream)
    return out


def semi_join(index: KeyIndex, probe: KeySide, anti: bool = False, null_equal: bool = False,
              hashes: Optional[torch.Tensor] = None, stream=None):
    """``(RowBatch, mask)``: the rows of ``probe.batch`` whose key is present in the index's build
    batch (``anti``: absent from it -- including, without ``null_equal``, every row with a null
    key), whole and in row order, and the int32 mask words that chose them: ``lookup_into`` into a
    mask, then the probe encoder's ``filter``."""
    n = probe.batch.nrows
    words = (n + 31) // 32
    with _on(stream):
        mask = torch.zeros(words, dtype=torch.int32, device=probe.encoder.device)
    lookup_into(index, probe, None, mask, null_equal, hashes, stream)
    if anti and n > 0:
        with _on(stream):
            mask = ~mask
            if n % 32:                           # the tail bits stay zero
                mask[-1] &= (1 << (n % 32)) - 1
    return probe.encoder.filter(probe.batch, mask.view(torch.uint8), stream), mask


def expand_first(found: torch.Tensor, first: torch.Tensor, max_pairs: Optional[int] = None):
    """The torch half of ``lookup_join_pairs``, on any device: ``found[j]`` = the smallest build row
    of probe row j's key or -1, ``first[i]`` = the smallest build row of build row i's key.  Every
    ``(j, i)`` with ``found[j] >= 0`` and ``first[i] == found[j]``, sorted by ``(j, i)``: a stable
    sort of the build rows by ``first``, the start and length of every first row's run, and the runs
    expanded as ``candidate_pairs`` expands its own.  One host read (the pair count)."""
    dev = found.device
    nb = first.numel()
    empty = (torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int64, device=dev))
    if found.numel() == 0 or nb == 0:
        return empty
    sorted_first, order = torch.sort(first, stable=True)          # a run per key, rows ascending
    counts_of = torch.bincount(first, minlength=nb)               # at a first row: its run's length
    starts_of = torch.cumsum(counts_of, 0) - counts_of            # ... and where the run starts
    hit = found >= 0
    at = torch.where(hit, found, torch.zeros_like(found))
    counts = torch.where(hit, counts_of[at], torch.zeros_like(found))
    ends = torch.cumsum(counts, 0)
    total = int(ends[-1].item())
    if max_pairs is not None and total > max_pairs:
        raise IllegalArgumentException(
            f"{total} pairs exceed max_pairs {max_pairs}: a hot key on both sides is quadratic")
    if total == 0:
        return empty
    pj = torch.repeat_interleave(torch.arange(found.numel(), dtype=torch.int64, device=dev), counts,
                                 output_size=total)
    within = torch.arange(total, dtype=torch.int64, device=dev) - (ends - counts)[pj]
    return pj, order[starts_of[at[pj]] + within]


def lookup_join_pairs(index: KeyIndex, probe: KeySide, null_equal: bool = False,
                      max_pairs: Optional[int] = None, stream=None):
    """The inner equi-join of ``probe.batch`` with the index's build batch, build-side duplicates
    included: every ``(j, i)`` such that the keys of probe row j equal the keys of build row i,
    sorted by ``(j, i)``, as two int64 device tensors ``(probe_rows, build_rows)`` -- exactly
    ``join_pairs(probe, index.side, null_equal)``.  Needs an index built with ``want_first=True``
    from the call's own hashes.  ``lookup`` finds every probe row's first build row; the duplicates
    of that row come from ``index.first`` in plain torch (``expand_first``).  Synchronises with the
    host twice: ``device_status``, and the pair count."""
    if index.first is None:
        raise IllegalArgumentException("lookup_join_pairs needs an index built with want_first=True")
    if index.caller_hashes:
        raise IllegalArgumentException("lookup_join_pairs needs an index built without caller hashes")
    found = lookup(index, probe, null_equal, None, stream)
    with _on(stream):
        return expand_first(found, index.first, max_pairs)


class _CallableModule(types.ModuleType):
    """``fury_amd.lookup(index, probe)``: the package attribute ``lookup`` is this module once it is
    imported, so calling the module calls its function ``lookup``."""

    def __call__(self, *args, **kwargs):
        return lookup(*args, **kwargs)


sys.modules[__name__].__class__ = _CallableModule
