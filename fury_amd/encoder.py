"""Host-side mirror of ``org.apache.fury.format.encoder.Encoders`` / ``RowEncoder`` over the
device C ABI.

Reference surface (FMT = java/fury-format/src/main/java/org/apache/fury/format):
  Encoders.bean(beanClass) -> RowEncoder<T>     FMT/encoder/Encoders.java:60-219
  RowEncoder.schema / toRow / fromRow / encode / decode   FMT/encoder/RowEncoder.java:26-32,
                                                          FMT/encoder/Encoder.java:31-40
  ArrowWriter.write(row) / finishAsRecordBatch  FMT/vectorized/ArrowWriter.java:74-99

A Java bean cannot cross onto the GPU, so the batch methods take/return Arrow-style columns
(``workloads.Column`` of torch tensors on the device) and ``RowBatch`` objects holding packed
rows in HBM.  The single-object methods (to_row / from_row / encode / decode) accept a bean as
a ``dict`` and run through the same device kernels as a batch of one.

Errors raise the Python counterparts of the reference's exceptions (see ``errors``).
"""
from __future__ import annotations

import contextlib
import ctypes
import struct
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native as N
from .types import (BINARY, BOOL, DECIMAL, FLOAT32, FLOAT64, LIST, MAP, STRING, STRUCT, Field,
                    type_width)
from .workloads import Column

# ---------------------------------------------------------------------------------------------
# Errors (status codes of include/fury_row.h fury_status)
# ---------------------------------------------------------------------------------------------


class FuryError(Exception):
    status = -1


class IllegalArgumentException(FuryError, ValueError):
    status = 1


class UnsupportedOperationException(FuryError, NotImplementedError):
    status = 2


class ClassNotCompatibleException(FuryError):
    """Schema hash mismatch on decode (Encoders.java:170-178)."""
    status = 3


class IndexOutOfBoundsException(FuryError, IndexError):
    status = 4


class EncoderException(FuryError):
    status = 5


class FuryDeviceError(FuryError, RuntimeError):
    status = 6


class CapacityError(FuryError):
    status = 7


_ERRORS = {c.status: c for c in (IllegalArgumentException, UnsupportedOperationException,
                                 ClassNotCompatibleException, IndexOutOfBoundsException,
                                 EncoderException, FuryDeviceError, CapacityError)}


def _check(status: int):
    if status != 0:
        raise _ERRORS.get(status, FuryError)(N.last_error())


# ---------------------------------------------------------------------------------------------
# Schema
# ---------------------------------------------------------------------------------------------
def _c_fields(fields: Sequence[Field], keep: list):
    arr = (N.FuryField * max(len(fields), 1))()
    for i, f in enumerate(fields):
        nm = f.name.encode("utf-8")
        keep.append(nm)
        arr[i].name = nm
        arr[i].type_id = f.type_id
        arr[i].nullable = int(bool(f.nullable))
        arr[i].num_children = len(f.children)
        arr[i].children = _c_fields(f.children, keep) if f.children else None
    keep.append(arr)
    return arr


class Schema:
    """A schema handle (``fury_schema``): layout + ``DataTypes.computeSchemaHash``.
    ``collection=True``: the schema of an ArrayEncoder / MapEncoder (one LIST or MAP field whose
    batch entries are top-level BinaryArrays / BinaryMaps, ``fury_collection_schema_create``)."""

    def __init__(self, fields: Sequence[Field], collection: bool = False):
        self.fields: List[Field] = list(fields)
        self.collection = collection
        keep: list = []
        h = ctypes.c_void_p()
        if collection:
            if len(self.fields) != 1:
                raise IllegalArgumentException("a collection schema has exactly one field")
            _check(N.lib().fury_collection_schema_create(_c_fields(self.fields, keep),
                                                         ctypes.byref(h)))
        else:
            _check(N.lib().fury_schema_create(_c_fields(self.fields, keep), len(self.fields),
                                              ctypes.byref(h)))
        self._h = h
        info = N.FurySchemaInfo()
        _check(N.lib().fury_schema_get_info(h, ctypes.byref(info)))
        self.num_fields = info.num_fields
        self.bitmap_bytes = info.bitmap_bytes
        self.fixed_size = info.fixed_size
        self.is_fixed = bool(info.is_fixed)
        self.schema_hash = int(info.schema_hash)

    @property
    def handle(self):
        return self._h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                N.lib().fury_schema_destroy(h)
            except Exception:
                pass
            self._h = None

    def __repr__(self):
        return f"Schema({self.fields}, hash={self.schema_hash})"


# ---------------------------------------------------------------------------------------------
# Device columns <-> C structs
# ---------------------------------------------------------------------------------------------
def _ptr(t) -> Optional[int]:
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        raise IllegalArgumentException("device columns must be torch tensors")
    if t.device.type != "cuda":
        raise IllegalArgumentException(f"tensor on {t.device}, expected a GPU tensor")
    if not t.is_contiguous():
        raise IllegalArgumentException("tensor must be contiguous")
    return t.data_ptr()


def _c_columns(cols: Sequence[Column], keep: list):
    arr = (N.FuryColumn * max(len(cols), 1))()
    for i, c in enumerate(cols):
        arr[i].values = _ptr(c.values)
        arr[i].validity = _ptr(c.validity)
        arr[i].offsets = _ptr(c.offsets)
        arr[i].capacity = 0 if c.values is None else c.values.numel() * c.values.element_size()
        arr[i].child = _c_columns(c.child, keep) if c.child else None
    keep.append(arr)
    return arr


def _hptr(a) -> Optional[int]:
    """Address of a HOST buffer: a contiguous numpy array or CPU tensor (e.g. pinned)."""
    if a is None:
        return None
    if isinstance(a, torch.Tensor):
        if a.device.type != "cpu" or not a.is_contiguous():
            raise IllegalArgumentException("host buffers must be contiguous CPU tensors")
        return a.data_ptr()
    a = np.asarray(a)
    if not a.flags["C_CONTIGUOUS"]:
        raise IllegalArgumentException("host buffers must be contiguous")
    return a.ctypes.data


def _nbytes(a) -> int:
    if a is None:
        return 0
    if isinstance(a, torch.Tensor):
        return a.numel() * a.element_size()
    return np.asarray(a).nbytes


def _c_host_columns(cols: Sequence[Column], keep: list):
    arr = (N.FuryColumn * max(len(cols), 1))()
    for i, c in enumerate(cols):
        for a in (c.values, c.validity, c.offsets):
            if a is not None:
                keep.append(a)
        arr[i].values = _hptr(c.values)
        arr[i].validity = _hptr(c.validity)
        arr[i].offsets = _hptr(c.offsets)
        arr[i].capacity = _nbytes(c.values)
        arr[i].child = _c_host_columns(c.child, keep) if c.child else None
    keep.append(arr)
    return arr


class _PinnedBlock:
    """hipHostMalloc'd host memory (fury_host_alloc), freed when the last array over it goes."""

    def __init__(self, nbytes: int):
        self._ptr = ctypes.c_void_p()
        _check(N.lib().fury_host_alloc(max(nbytes, 1), ctypes.byref(self._ptr)))
        self.__array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "version": 3,
                                    "data": (self._ptr.value, False)}

    def __del__(self):
        if self._ptr.value:
            try:
                N.lib().fury_host_free(self._ptr)
            except TypeError:           # interpreter shutdown: the module is already torn down
                pass
            self._ptr = ctypes.c_void_p()


def host_empty(nbytes: int, dtype=np.uint8) -> np.ndarray:
    """A pinned host buffer for the host-memory batch path (include/fury_row.h fury_host_alloc):
    the GPU reaches it directly, so fixed-width encode_host / decode_host run without staging
    (GpuRowEncoder.allocatePinned is the JVM's equivalent)."""
    return np.asarray(_PinnedBlock(nbytes)).view(dtype)


def _tree_bytes(cols: Sequence[Column]) -> int:
    return sum(_nbytes(c.values) + _nbytes(c.validity) + _nbytes(c.offsets) +
               (_tree_bytes(c.child) if c.child else 0) for c in cols)


def _stream_handle(stream: Optional[torch.cuda.Stream]) -> int:
    s = stream if stream is not None else torch.cuda.current_stream()
    return s.cuda_stream


def _on(stream: Optional[torch.cuda.Stream]):
    """Makes ``stream`` torch's current stream for the body: output allocations belong to it (the
    caching allocator does not hand them to other streams while the kernels run) and host reads
    (``.item()``, ``.cpu()``) wait for the kernels launched on it."""
    return torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()


def column_to_device(c: Column, device) -> Column:
    def t(a):
        if a is None:
            return None
        if isinstance(a, torch.Tensor):
            return a.to(device)
        return torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return Column(values=t(c.values), validity=t(c.validity), offsets=t(c.offsets),
                  child=[column_to_device(x, device) for x in c.child] if c.child else None)


def column_to_host(c: Column) -> Column:
    def h(a):
        if a is None:
            return None
        return a.detach().cpu().numpy()
    return Column(values=h(c.values), validity=h(c.validity), offsets=h(c.offsets),
                  child=[column_to_host(x) for x in c.child] if c.child else None)


@dataclass
class RowBatch:
    """Packed rows in device memory: row i = rows[row_offsets[i]:row_offsets[i+1]] (or
    i * fixed_size for fixed-width schemas, where row_offsets is None)."""
    rows: torch.Tensor
    row_offsets: Optional[torch.Tensor]
    nrows: int
    schema_hash: int

    def row_bytes(self, i: int, fixed_size: int) -> bytes:
        if self.row_offsets is None:
            b, e = i * fixed_size, (i + 1) * fixed_size
        else:
            b, e = int(self.row_offsets[i]), int(self.row_offsets[i + 1])
        return bytes(self.rows[b:e].cpu().numpy())


# ---------------------------------------------------------------------------------------------
# RowEncoder
# ---------------------------------------------------------------------------------------------
class RowEncoder:
    """``RowEncoder<T>`` with batch methods; not thread-safe per instance (like the reference,
    Encoders.java:74,146)."""

    def __init__(self, fields: Sequence[Field], device=None):
        self._schema = Schema(fields)
        self.device = torch.device(device if device is not None else "cuda")

    # -- RowEncoder API ------------------------------------------------------------------
    def schema(self) -> Schema:
        return self._schema

    @property
    def schema_hash(self) -> int:
        return self._schema.schema_hash

    # -- batch API -----------------------------------------------------------------------
    def measure(self, columns: Sequence[Column], nrows: int, stream=None) -> Optional[torch.Tensor]:
        """Row offsets (int64[nrows+1], device) for variable-length schemas; None if fixed."""
        if self._schema.is_fixed:
            return None
        with _on(stream):
            offs = torch.empty(nrows + 1, dtype=torch.int64, device=self.device)
        keep: list = []
        _check(N.lib().fury_row_measure(self._schema.handle, _c_columns(columns, keep), nrows,
                                        offs.data_ptr(), _stream_handle(stream)))
        return offs

    def measure_into(self, columns: Sequence[Column], nrows: int, offs: torch.Tensor,
                     stream=None) -> None:
        keep: list = []
        _check(N.lib().fury_row_measure(self._schema.handle, _c_columns(columns, keep), nrows,
                                        _ptr(offs), _stream_handle(stream)))

    def encode_into(self, columns: Sequence[Column], nrows: int, rows: torch.Tensor,
                    row_offsets: Optional[torch.Tensor], stream=None) -> None:
        keep: list = []
        _check(N.lib().fury_row_encode(self._schema.handle, _c_columns(columns, keep), nrows,
                                       _ptr(row_offsets), _ptr(rows), _stream_handle(stream)))

    def encode_measured_into(self, columns: Sequence[Column], nrows: int, rows: torch.Tensor,
                             row_offsets: Optional[torch.Tensor], stream=None) -> None:
        """Measure + encode in one call (no host sync) into a reused buffer (``rows`` capacity =
        its size): writes ``row_offsets``; when ``row_offsets[nrows]`` exceeds the capacity the
        rows did not fit (nothing past the capacity is written) — grow and call again."""
        keep: list = []
        _check(N.lib().fury_row_encode_measured(
            self._schema.handle, _c_columns(columns, keep), nrows, _ptr(row_offsets), _ptr(rows),
            rows.numel() * rows.element_size(), _stream_handle(stream)))

    # -- bound calls: the argument block built once, for hot loops --------------------------
    def _bound(self, fn, args, keep: list, *alive):
        """The callable every ``bind_*`` returns: it re-issues ``fn(*args)`` and raises on a
        failure status, nothing else per call.  Its ``keep`` holds what ``args`` points into --
        the ctypes objects in ``keep`` and the caller's buffers ``alive`` -- and this encoder with
        its Schema: the schema handle in ``args`` lives as long as the Schema object, so a dropped
        encoder would otherwise free it under the call."""
        def call():
            _check(fn(*args))
        call.keep = (keep, *alive, self, self._schema)
        return call

    def bind_encode(self, columns: Sequence[Column], nrows: int, rows: torch.Tensor,
                    row_offsets: Optional[torch.Tensor] = None, stream=None,
                    measured: bool = False):
        """``encode_into`` (``measured``: ``encode_measured_into``) with the column descriptors
        and pointers resolved once; the returned callable re-issues the same call.  Building the
        descriptors of 100 columns costs ~0.3 ms of Python per call -- more than the Struct-100
        kernel -- so a loop that re-encodes the same buffers should bind.  The buffers must stay
        alive and unmoved while the callable is used."""
        keep: list = []
        cc = _c_columns(columns, keep)
        L = N.lib()
        if measured:
            args = (self._schema.handle, cc, nrows, _ptr(row_offsets), _ptr(rows),
                    rows.numel() * rows.element_size(), _stream_handle(stream))
            fn = L.fury_row_encode_measured
        else:
            args = (self._schema.handle, cc, nrows, _ptr(row_offsets), _ptr(rows),
                    _stream_handle(stream))
            fn = L.fury_row_encode
        return self._bound(fn, args, keep, columns, rows, row_offsets)

    def bind_decode(self, batch: RowBatch, cols: List[Column], stream=None, arrow: bool = False):
        """``decode_into`` bound like ``bind_encode``."""
        keep: list = []
        cc = _c_columns(cols, keep)
        fn = N.lib().fury_rows_to_arrow if arrow else N.lib().fury_row_decode
        args = (self._schema.handle, _ptr(batch.rows), _ptr(batch.row_offsets), batch.nrows, cc,
                _stream_handle(stream))
        return self._bound(fn, args, keep, batch, cols)

    def encode_batch(self, columns: Sequence[Column], nrows: int, stream=None) -> RowBatch:
        offs = self.measure(columns, nrows, stream)
        with _on(stream):
            if offs is None:
                total = nrows * self._schema.fixed_size
            else:
                total = int(offs[nrows].item())
            rows = self._row_buffer(total)
        self.encode_into(columns, nrows, rows, offs, stream)
        return RowBatch(rows[:total] if total else rows[:0], offs, nrows, self.schema_hash)

    def alloc_columns(self, nrows: int, validity: bool = True) -> List[Column]:
        """Output columns for fixed-width fields (variable ones are sized by decode_measure).
        Validity and BOOL bitmaps are whole 32-bit words (the kernels store / OR them as words,
        include/fury_row.h: 4-byte aligned, padded to a multiple of 4 bytes)."""
        return self._alloc_fields(self._schema.fields, nrows, validity)

    def _alloc_fields(self, fields: Sequence[Field], nrows: int, validity: bool) -> List[Column]:
        out = []
        words = ((nrows + 31) // 32) * 4
        for f in fields:
            vb = (torch.empty(words, dtype=torch.uint8, device=self.device)
                  if validity else None)
            if f.type_id == BOOL:
                out.append(Column(values=torch.empty(words, dtype=torch.uint8,
                                                     device=self.device), validity=vb))
            elif type_width(f.type_id) > 0:
                out.append(Column(values=torch.empty(nrows * type_width(f.type_id),
                                                     dtype=torch.uint8, device=self.device),
                                  validity=vb))
            elif f.type_id == DECIMAL:
                out.append(Column(values=torch.empty(nrows * 16, dtype=torch.uint8,
                                                     device=self.device), validity=vb))
            elif f.type_id in (STRING, BINARY):
                out.append(Column(offsets=torch.empty(nrows + 1, dtype=torch.int32,
                                                      device=self.device), validity=vb))
            elif f.type_id == LIST:
                out.append(Column(offsets=torch.empty(nrows + 1, dtype=torch.int32,
                                                      device=self.device), validity=vb,
                                  child=[Column()]))
            else:
                raise UnsupportedOperationException(f"no device decode for {f}")
        return out

    @property
    def nested(self) -> bool:
        """True when the schema has STRUCT / MAP / LIST-of-variable-length fields, or more than
        256 fields of which some are variable-length (decoded by the two-step plan API: the generic
        engine); always for collection schemas."""
        if getattr(self._schema, "collection", False):
            return True
        if len(self._schema.fields) > 256 and not self._schema.is_fixed:
            return True
        def deep(f: Field) -> bool:
            if f.type_id in (STRUCT, MAP):
                return True
            if f.type_id == LIST:
                e = f.children[0]
                return type_width(e.type_id) < 0 or deep(e)
            return False
        return any(deep(f) for f in self._schema.fields)

    def _decode_nested(self, batch: RowBatch, validity: bool, arrow: bool,
                       stream=None) -> List[Column]:
        L = N.lib()
        h = self._schema.handle
        nn = L.fury_schema_num_nodes(h)
        entries = (ctypes.c_int64 * max(nn, 1))()
        nbytes = (ctypes.c_int64 * max(nn, 1))()
        plan = ctypes.c_void_p()
        sh = _stream_handle(stream)
        _check(L.fury_decode_prepare(h, _ptr(batch.rows), _ptr(batch.row_offsets), batch.nrows,
                                     entries, nbytes, ctypes.byref(plan), sh))
        try:
            order = _bfs(self._schema.fields)
            cols: List[Column] = []
            with _on(stream):
                cols = _alloc_nodes(order, entries, nbytes, validity or arrow, self.device)
            for i, (f, first) in enumerate(order):
                if f.children:
                    cols[i].child = [cols[first + j] for j in range(len(f.children))]
            top = cols[:len(self._schema.fields)]
            keep: list = []
            _check(L.fury_decode_execute(plan, _c_columns(top, keep), int(arrow), sh))
        finally:
            L.fury_decode_plan_destroy(plan)
        return top

    def _decode_bound(self, batch: RowBatch, validity: bool, arrow: bool,
                      stream=None) -> List[Column]:
        """Variable-length outputs sized from a bound the rows give (a column's payload bytes and
        list elements <= the batch's row bytes: every byte of them is inside some row), decoded
        in one pass, then trimmed to the real sizes after ONE host read of every column's
        offsets[n] -- no fury_row_decode_measure pass over the rows.  Rows that break the bound
        (a slot pointing outside its row) fall back to the exact-size ("measure") decode."""
        n = batch.nrows
        bound = int(batch.rows.numel() * batch.rows.element_size())
        with _on(stream):
            cols = self.alloc_columns(n, validity)
            for f, c in zip(self._schema.fields, cols):
                if f.type_id in (STRING, BINARY):
                    c.values = torch.empty(max(bound, 1), dtype=torch.uint8, device=self.device)
                elif f.type_id == LIST:
                    e = f.children[0]
                    nbytes = (bound + 7) // 8 if e.type_id == BOOL else bound
                    c.child = [Column(
                        values=torch.empty(nbytes + 8, dtype=torch.uint8, device=self.device),
                        validity=(torch.zeros((bound + 7) // 8 + 4, dtype=torch.uint8,
                                              device=self.device) if validity else None))]
        self.decode_into(batch, cols, stream, arrow)
        var = [(f, c) for f, c in zip(self._schema.fields, cols)
               if f.type_id in (STRING, BINARY, LIST)]
        if not var or n == 0:
            return cols
        with _on(stream):
            totals = torch.stack([c.offsets[n] for _, c in var]).cpu().tolist()
        for (f, c), total in zip(var, totals):
            if f.type_id == LIST:
                e = f.children[0]
                ch = c.child[0]
                nbytes = (total + 7) // 8 if e.type_id == BOOL else total * type_width(e.type_id)
                have = ch.values.numel() - 8
                if total < 0 or nbytes > have:
                    return self._decode(batch, validity, arrow, stream, None, "measure")
                ch.values = ch.values[:nbytes + 8]
                if ch.validity is not None:
                    ch.validity = ch.validity[:(total + 7) // 8 + 4]
            else:
                if total < 0 or total > c.values.numel():
                    return self._decode(batch, validity, arrow, stream, None, "measure")
                c.values = c.values[:max(total, 1)]
        return cols

    def _decode(self, batch: RowBatch, validity: bool, arrow: bool, stream=None,
                out: Optional[List[Column]] = None, sizing: str = "measure") -> List[Column]:
        if self.nested:
            return self._decode_nested(batch, validity, arrow, stream)
        if sizing not in ("measure", "bound"):
            raise ValueError(f"sizing must be 'measure' or 'bound', not {sizing!r}")
        if sizing == "measure" and out is None and self._wide_plan():
            # 17-256 fields: the plan API keeps the count pass's tile bases for the write pass
            # (fury_decode_prepare sizes, fury_decode_execute writes; the rows are counted once)
            return self._decode_nested(batch, validity, arrow, stream)
        if sizing == "bound" and out is None and not self._schema.is_fixed:
            return self._decode_bound(batch, validity, arrow, stream)
        n = batch.nrows
        if out is not None:
            cols = out
        else:
            with _on(stream):
                cols = self.alloc_columns(n, validity)
        keep: list = []
        sh = _stream_handle(stream)
        if not self._schema.is_fixed:
            _check(N.lib().fury_row_decode_measure(self._schema.handle, _ptr(batch.rows),
                                                   _ptr(batch.row_offsets), n,
                                                   _c_columns(cols, keep), sh))
            self._size_var_outputs(cols, n, validity, stream)
            keep = []
        fn = N.lib().fury_rows_to_arrow if arrow else N.lib().fury_row_decode
        _check(fn(self._schema.handle, _ptr(batch.rows), _ptr(batch.row_offsets), n,
                  _c_columns(cols, keep), sh))
        return cols

    def _wide_plan(self) -> bool:
        """Flat variable-length schemas the wide kernels decode (17-256 fields, tuning var_wide)."""
        nf = len(self._schema.fields)
        return (not self._schema.is_fixed and 16 < nf <= 256
                and N.lib().fury_get_tuning(b"var_wide") == 1)

    def _size_var_outputs(self, cols: List[Column], n: int, validity: bool, stream,
                          fields: Optional[Sequence[Field]] = None) -> None:
        """Allocates the payload / element buffers of the variable-length outputs from the
        offsets fury_row_decode_measure wrote (host read on ``stream``)."""
        with _on(stream):
            for f, c in zip(self._schema.fields if fields is None else fields, cols):
                if f.type_id in (STRING, BINARY):
                    total = int(c.offsets[n].item()) if n else 0
                    c.values = torch.empty(max(total, 1), dtype=torch.uint8, device=self.device)
                elif f.type_id == LIST:
                    total = int(c.offsets[n].item()) if n else 0
                    e = f.children[0]
                    nbytes = (total + 7) // 8 if e.type_id == BOOL else total * type_width(e.type_id)
                    c.child = [Column(
                        values=torch.empty(nbytes + 8, dtype=torch.uint8, device=self.device),
                        validity=(torch.zeros((total + 7) // 8 + 4, dtype=torch.uint8,
                                              device=self.device) if validity else None))]

    def decode_into(self, batch: RowBatch, cols: List[Column], stream=None,
                    arrow: bool = False) -> None:
        """Decode into preallocated columns in one device pass (the kernel computes the Arrow
        offsets itself): no host synchronisation, so the call can be captured/timed back to
        back.  Payloads past a buffer's capacity are not written; ``offsets[nrows]`` always holds
        the size the column needs (see ``check_capacity``)."""
        keep: list = []
        sh = _stream_handle(stream)
        fn = N.lib().fury_rows_to_arrow if arrow else N.lib().fury_row_decode
        _check(fn(self._schema.handle, _ptr(batch.rows), _ptr(batch.row_offsets), batch.nrows,
                  _c_columns(cols, keep), sh))

    def check_capacity(self, cols: List[Column], nrows: int,
                       select: Optional[Sequence] = None) -> None:
        """Raises CapacityError when a decode into preallocated ``cols`` needed more payload
        (STRING/BINARY bytes, LIST child elements) than the buffers hold (synchronises).
        ``select``: ``cols`` are the outputs of a projected decode of these fields."""
        self.device_status()
        if nrows == 0 or (select is None and (self._schema.is_fixed or self.nested)):
            return
        fields = (self._schema.fields if select is None
                  else [self._schema.fields[k] for k in self._select(select)])
        for f, c in zip(fields, cols):
            if f.type_id not in (STRING, BINARY, LIST) or c.offsets is None:
                continue
            need = int(c.offsets[nrows].item())
            if f.type_id == LIST:
                e = f.children[0]
                v = c.child[0].values if c.child else None
                have = 0 if v is None else v.numel() * v.element_size()
                have = have * 8 if e.type_id == BOOL else have // type_width(e.type_id)
            else:
                have = 0 if c.values is None else c.values.numel() * c.values.element_size()
            if need > have:
                raise CapacityError(f"column {f.name}: decode needs {need}, buffer holds {have}")

    def decode_batch(self, batch: RowBatch, validity: bool = True, stream=None,
                     out: Optional[List[Column]] = None, sizing: str = "measure") -> List[Column]:
        """Rows -> columns (generated fromRow semantics).  Variable-length outputs are sized by
        ``sizing``: "measure" (default) runs fury_row_decode_measure first and allocates exactly;
        "bound" allocates each from the batch's row bytes (HBM for speed: no sizing pass over the
        rows) and trims after one host read.  Memory cost of "bound": the returned columns are
        views of those row-sized buffers, so while they live every STRING / BINARY / LIST output
        holds about the batch's row bytes of HBM (K variable-length columns: ~K x row bytes).
        ``stream``: every kernel, output allocation and host read of the call runs on it."""
        if batch.schema_hash != self.schema_hash:
            raise ClassNotCompatibleException(
                f"Schema is not consistent, encoder schema is {self._schema}. self/peer schema "
                f"hash are {self.schema_hash}/{batch.schema_hash}. Please check writer schema.")
        cols = self._decode(batch, validity, False, stream, out, sizing)
        self.device_status(stream)
        return cols

    # -- projected decode: selected fields only (BinaryRow getters over a batch) ---------------
    def _select(self, select: Sequence) -> List[int]:
        """Slot indices of ``select`` (field names or slot indices, in selection order)."""
        names = {f.name: k for k, f in enumerate(self._schema.fields)}
        out = []
        for x in select:
            if isinstance(x, str):
                if x not in names:
                    raise IllegalArgumentException(f"no field named {x!r} in {self._schema}")
                out.append(names[x])
            else:
                out.append(int(x))
        return out

    def alloc_projected(self, select: Sequence, nrows: int, validity: bool = True) -> List[Column]:
        """Output columns for the selected fields, like ``alloc_columns`` (variable-length ones
        are sized by ``project_batch``)."""
        idx = self._select(select)
        for k in idx:
            if not 0 <= k < len(self._schema.fields):
                raise IllegalArgumentException(f"field index {k} is not a field of {self._schema}")
        return self._alloc_fields([self._schema.fields[k] for k in idx], nrows, validity)

    def project_into(self, batch: RowBatch, select: Sequence, cols: List[Column], stream=None,
                     arrow: bool = False) -> None:
        """Decode only the fields ``select`` (names or slot indices, any order) of every row into
        the preallocated ``cols`` (selection order): one call, no host synchronisation.  Only the
        bitmap words and slots of the selected fields are read, so the rest of the schema may be
        anything, nested fields included; payload capacity as in ``decode_into``."""
        idx = self._select(select)
        keep: list = []
        sel = (ctypes.c_int32 * max(len(idx), 1))(*idx)
        _check(N.lib().fury_row_project(self._schema.handle, sel, len(idx), _ptr(batch.rows),
                                        _ptr(batch.row_offsets), batch.nrows,
                                        _c_columns(cols, keep), int(arrow), _stream_handle(stream)))

    def bind_project(self, batch: RowBatch, select: Sequence, cols: List[Column], stream=None,
                     arrow: bool = False):
        """``project_into`` bound like ``bind_decode``: descriptors and pointers resolved once."""
        idx = self._select(select)
        keep: list = []
        sel = (ctypes.c_int32 * max(len(idx), 1))(*idx)
        fn = N.lib().fury_row_project
        args = (self._schema.handle, sel, len(idx), _ptr(batch.rows), _ptr(batch.row_offsets),
                batch.nrows, _c_columns(cols, keep), int(arrow), _stream_handle(stream))
        return self._bound(fn, args, keep, sel, batch, cols)

    def project_batch(self, batch: RowBatch, select: Sequence, validity: bool = True, stream=None,
                      arrow: bool = False) -> List[Column]:
        """Rows -> the selected columns.  Variable-length outputs are sized exactly
        (fury_row_project_measure, one host read of the offsets' last entries)."""
        if batch.schema_hash != self.schema_hash:
            raise ClassNotCompatibleException(
                f"Schema is not consistent, encoder schema is {self._schema}. self/peer schema "
                f"hash are {self.schema_hash}/{batch.schema_hash}. Please check writer schema.")
        idx = self._select(select)
        n = batch.nrows
        validity = validity or arrow
        with _on(stream):
            cols = self.alloc_projected(idx, n, validity)
        fields = [self._schema.fields[k] for k in idx]
        if any(f.type_id in (STRING, BINARY, LIST) for f in fields):
            keep: list = []
            sel = (ctypes.c_int32 * max(len(idx), 1))(*idx)
            _check(N.lib().fury_row_project_measure(
                self._schema.handle, sel, len(idx), _ptr(batch.rows), _ptr(batch.row_offsets), n,
                _c_columns(cols, keep), _stream_handle(stream)))
            self._size_var_outputs(cols, n, validity, stream, fields)
        self.project_into(batch, idx, cols, stream, arrow)
        self.device_status(stream)
        return cols

    # -- in-place update: selected fixed-width fields (BinaryRow setters over a batch) ----------
    def _update_args(self, batch: RowBatch, select: Sequence, cols: Sequence[Column], row_mask,
                     stream, keep: list):
        if batch.schema_hash != self.schema_hash:
            raise ClassNotCompatibleException(
                f"Schema is not consistent, encoder schema is {self._schema}. self/peer schema "
                f"hash are {self.schema_hash}/{batch.schema_hash}. Please check writer schema.")
        idx = self._select(select)
        if len(cols) != len(idx):
            raise IllegalArgumentException(f"{len(idx)} fields selected, {len(cols)} columns given")
        sel = (ctypes.c_int32 * max(len(idx), 1))(*idx)
        keep.append(sel)
        return (self._schema.handle, sel, len(idx), _ptr(batch.rows), _ptr(batch.row_offsets),
                batch.nrows, _c_columns(cols, keep), _ptr(row_mask), _stream_handle(stream))

    def update_fields(self, batch: RowBatch, select: Sequence, cols: Sequence[Column],
                      row_mask: Optional[torch.Tensor] = None, stream=None) -> None:
        """Overwrite the fixed-width fields ``select`` (names or slot indices, any order) of every
        row of ``batch.rows`` in place with the columns ``cols`` (selection order, the layout
        ``encode_batch`` takes for the same fields): a valid value clears the field's null bit and
        writes the value's own bytes, a null one sets the bit and zeroes the slot; nothing else of
        the rows changes.  ``row_mask``: optional device bitmap (LSB-first, whole 32-bit words),
        bit = 1 updates the row.  One call, no host synchronisation: a row outside the batch is
        left unwritten and reported by ``device_status(stream)``.  Two updates of one batch must
        be ordered by the caller (same stream)."""
        keep: list = []
        _check(N.lib().fury_row_update(*self._update_args(batch, select, cols, row_mask, stream,
                                                          keep)))

    def bind_update(self, batch: RowBatch, select: Sequence, cols: Sequence[Column],
                    row_mask: Optional[torch.Tensor] = None, stream=None):
        """``update_fields`` bound like ``bind_project``: descriptors and pointers resolved once."""
        keep: list = []
        args = self._update_args(batch, select, cols, row_mask, stream, keep)
        return self._bound(N.lib().fury_row_update, args, keep, batch, cols, row_mask)

    # -- row selection: whole rows gathered into a new batch (BinaryRow.copy() over a batch) -----
    def _check_hash(self, batch: RowBatch) -> None:
        if batch.schema_hash != self.schema_hash:
            raise ClassNotCompatibleException(
                f"Schema is not consistent, encoder schema is {self._schema}. self/peer schema "
                f"hash are {self.schema_hash}/{batch.schema_hash}. Please check writer schema.")

    def _fixed_size(self) -> Optional[int]:
        """The row size of a fixed-width schema (row i at ``i * fixed_size``), else None."""
        return self._schema.fixed_size if self._schema.is_fixed else None

    def _row_buffer(self, total: int) -> torch.Tensor:
        """A device buffer for ``total`` row bytes: never empty, so it always has an address."""
        return torch.empty(max(total, 16), dtype=torch.uint8, device=self.device)

    def _measured(self, n: int, fixed_size: Optional[int], schema_hash: int, into,
                  stream) -> RowBatch:
        """The eager form of an ``*_into`` call, issued by ``into(out_rows, out_offsets)``, as a new
        batch of ``n`` rows.  Output rows of ``fixed_size`` bytes know the size up front (no
        offsets); ``None``: measure first with ``out_rows=None`` (one host read of the byte
        total).  Then allocate, write, and ``device_status``."""
        with _on(stream):
            if fixed_size is not None:
                offs = None
                total = n * fixed_size
            else:
                offs = torch.empty(n + 1, dtype=torch.int64, device=self.device)
                into(None, offs)
                total = int(offs[n].item())
            rows = self._row_buffer(total)
        into(rows, offs)
        self.device_status(stream)
        return RowBatch(rows[:total], offs, n, schema_hash)

    @staticmethod
    def _counted(head: torch.Tensor, *ends: torch.Tensor):
        """The count-and-total variant's one host read: ``head[0]`` is the entry count a measure
        call wrote, ``ends`` are the one-entry tails of its offsets (the byte totals), gathered
        behind it on the device.  Returns the ints ``(count, *totals)``."""
        for k, end in enumerate(ends, 1):
            head[k:k + 1] = end
        return (int(x) for x in head.cpu())

    def _take_kept(self, batch: RowBatch, idx: torch.Tensor, offs: Optional[torch.Tensor],
                   count: int, total: int, stream):
        """The second half of ``filter`` and ``partition``: the ``count`` rows ``idx[:count]`` a
        measure call kept (``offs``: their offsets, None for a fixed-width schema; ``total``
        bytes) copied into a new batch.  Returns ``(batch, idx[:count])``."""
        with _on(stream):
            rows = self._row_buffer(total)
            kept = idx[:count]
            offs = None if offs is None else offs[:count + 1]
        self.take_into(batch, kept, rows, offs, stream)
        self.device_status(stream)
        return RowBatch(rows[:total], offs, count, self.schema_hash), kept

    def _indices(self, indices, stream) -> torch.Tensor:
        if not isinstance(indices, torch.Tensor):
            indices = torch.as_tensor(np.asarray(indices, dtype=np.int64))
        if indices.dtype in (torch.bool, torch.float16, torch.float32, torch.float64,
                             torch.bfloat16):
            raise IllegalArgumentException(f"indices must be an integer tensor, not {indices.dtype}")
        with _on(stream):
            return indices.to(device=self.device, dtype=torch.int64).contiguous().reshape(-1)

    def _take_args(self, batch: RowBatch, indices, out_rows, out_offsets, stream, keep: list):
        self._check_hash(batch)
        idx = self._indices(indices, stream)
        keep.append(idx)
        return (self._schema.handle, _ptr(batch.rows), _ptr(batch.row_offsets), batch.nrows,
                _ptr(idx), idx.numel(), _ptr(out_rows), _nbytes(out_rows), _ptr(out_offsets),
                _stream_handle(stream))

    def take_into(self, batch: RowBatch, indices, out_rows: Optional[torch.Tensor],
                  out_offsets: Optional[torch.Tensor] = None, stream=None) -> None:
        """Output row j = the bytes of row ``indices[j]`` of ``batch`` (any integer tensor, any
        order, repeats allowed), written to the preallocated ``out_rows`` (capacity = its size)
        with their offsets in ``out_offsets`` (int64, ``len(indices) + 1`` entries; optional for
        fixed-width schemas): one call, no host synchronisation.  Bytes at or past the capacity
        are not written while ``out_offsets`` is always complete; ``out_rows=None`` only measures.
        An index outside the batch gives a 0-byte row, reported by ``device_status(stream)``.
        ``out_rows`` must not overlap ``batch.rows``."""
        keep: list = []
        _check(N.lib().fury_row_take(*self._take_args(batch, indices, out_rows, out_offsets, stream,
                                                      keep)))

    def bind_take(self, batch: RowBatch, indices, out_rows: Optional[torch.Tensor],
                  out_offsets: Optional[torch.Tensor] = None, stream=None):
        """``take_into`` bound like ``bind_update``: pointers resolved once."""
        keep: list = []
        args = self._take_args(batch, indices, out_rows, out_offsets, stream, keep)
        return self._bound(N.lib().fury_row_take, args, keep, batch, out_rows, out_offsets)

    def take(self, batch: RowBatch, indices, stream=None) -> RowBatch:
        """The rows ``indices`` of ``batch`` as a new batch.  Fixed-width schemas know the size up
        front; the others measure first (one host read of the byte total), then copy."""
        self._check_hash(batch)
        idx = self._indices(indices, stream)
        return self._measured(idx.numel(), self._fixed_size(), self.schema_hash,
                              lambda rows, offs: self.take_into(batch, idx, rows, offs, stream),
                              stream)

    def _mask_words(self, row_mask: torch.Tensor, nrows: int, stream) -> torch.Tensor:
        """``row_mask`` as the device bitmap the kernels read (LSB-first, whole 32-bit words): a
        uint8 bitmap is taken as it is, a bool tensor of ``nrows`` entries is packed."""
        if row_mask is None or row_mask.dtype != torch.bool:
            return row_mask
        if row_mask.numel() != nrows:
            raise IllegalArgumentException(f"row_mask has {row_mask.numel()} entries for {nrows} rows")
        with _on(stream):
            m = torch.zeros(((nrows + 31) // 32) * 32, dtype=torch.uint8, device=self.device)
            m[:nrows] = row_mask.to(self.device).reshape(-1)
            w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=self.device)
            return (m.reshape(-1, 8) * w).sum(dim=1, dtype=torch.int32).to(torch.uint8)

    def filter_into(self, batch: RowBatch, row_mask: torch.Tensor,
                    out_rows: Optional[torch.Tensor], out_offsets: Optional[torch.Tensor],
                    out_count: torch.Tensor, out_indices: Optional[torch.Tensor] = None,
                    stream=None) -> None:
        """Keeps the rows of ``batch`` whose ``row_mask`` bit is 1 (device bitmap, LSB-first, whole
        32-bit words; or a bool tensor), in row order: one call, no host synchronisation.
        ``out_count`` (int64[1]) receives the number kept, ``out_offsets`` (int64, nrows + 1
        entries; optional for fixed-width schemas) the offsets -- entries past the count repeat the
        total -- and ``out_indices`` (optional, int64, nrows entries) the row numbers kept, -1
        past the count.  Capacity and ``out_rows=None`` as in ``take_into``."""
        self._check_hash(batch)
        mask = self._mask_words(row_mask, batch.nrows, stream)
        _check(N.lib().fury_row_filter(
            self._schema.handle, _ptr(batch.rows), _ptr(batch.row_offsets), batch.nrows, _ptr(mask),
            _ptr(out_rows), _nbytes(out_rows), _ptr(out_offsets), _ptr(out_count),
            _ptr(out_indices), _stream_handle(stream)))

    def filter(self, batch: RowBatch, row_mask: torch.Tensor, stream=None,
               return_indices: bool = False):
        """The rows of ``batch`` whose ``row_mask`` bit is 1 as a new batch (with
        ``return_indices``: and their row numbers).  The mask is compacted and measured on the
        device, count and byte total come back in one host read, then the kept rows are copied."""
        self._check_hash(batch)
        n = batch.nrows
        fixed = self._schema.is_fixed
        with _on(stream):
            head = torch.empty(2, dtype=torch.int64, device=self.device)      # count, total
            idx = torch.empty(max(n, 1), dtype=torch.int64, device=self.device)
            offs = None if fixed else torch.empty(n + 1, dtype=torch.int64, device=self.device)
            self.filter_into(batch, row_mask, None, offs, head[:1], idx[:n] if n else None, stream)
            if fixed:
                count = int(head[0].item())
                total = count * self._schema.fixed_size
            else:
                count, total = self._counted(head, offs[n:])
        out, kept = self._take_kept(batch, idx, offs, count, total, stream)
        return (out, kept) if return_indices else out

    # -- rows by key, batches end to end (fury_row_partition / fury_row_concat) -------------------
    def _part_ids(self, part_ids, nrows: int, stream) -> torch.Tensor:
        """``part_ids`` as the device int32 tensor the kernels read: a value outside int32 becomes
        -1 before narrowing, so it drops its row instead of wrapping into a partition."""
        if not isinstance(part_ids, torch.Tensor):
            a = np.asarray(part_ids)
            if a.size == 0:                    # an empty list has no dtype of its own
                a = a.astype(np.int32)
            if a.dtype.kind not in "iu":
                raise IllegalArgumentException(f"part_ids must be integers, not {a.dtype}")
            if a.dtype.kind == "u" and a.dtype.itemsize >= 4:      # torch has no wide unsigned
                a = np.where(a > np.iinfo(np.int32).max, -1, a.astype(np.int64))
            part_ids = torch.as_tensor(np.ascontiguousarray(a))
        if part_ids.dtype.is_floating_point or part_ids.dtype.is_complex or \
                part_ids.dtype == torch.bool:
            raise IllegalArgumentException(
                f"part_ids must be an integer tensor, not {part_ids.dtype}")
        if part_ids.numel() != nrows:
            raise IllegalArgumentException(f"part_ids has {part_ids.numel()} entries for {nrows} rows")
        with _on(stream):
            ids = part_ids.to(self.device).reshape(-1)
            if ids.dtype == torch.int64:
                lim = torch.iinfo(torch.int32)
                ids = torch.where((ids < lim.min) | (ids > lim.max), -1, ids)
            return ids.to(torch.int32).contiguous()

    def _partition_args(self, batch: RowBatch, part_ids, num_parts, out_rows, out_offsets,
                        out_part_rows, out_indices, out_positions, stream, keep: list):
        self._check_hash(batch)
        ids = self._part_ids(part_ids, batch.nrows, stream)
        keep.append(ids)
        return (self._schema.handle, _ptr(batch.rows), _ptr(batch.row_offsets), batch.nrows,
                _ptr(ids), int(num_parts), _ptr(out_rows), _nbytes(out_rows), _ptr(out_offsets),
                _ptr(out_part_rows), _ptr(out_indices), _ptr(out_positions),
                _stream_handle(stream))

    def partition_into(self, batch: RowBatch, part_ids, num_parts: int,
                       out_rows: Optional[torch.Tensor], out_offsets: Optional[torch.Tensor],
                       out_part_rows: torch.Tensor, out_indices: Optional[torch.Tensor] = None,
                       out_positions: Optional[torch.Tensor] = None, stream=None) -> None:
        """Splits the rows of ``batch`` by ``part_ids`` (any integer tensor or array, ``nrows``
        entries): row i is kept when ``0 <= part_ids[i] < num_parts`` and dropped otherwise, and
        the kept rows come out sorted by (id, row number) -- each partition contiguous and in
        source order.  One call, no host synchronisation.  ``out_part_rows`` (int64,
        ``num_parts + 1`` entries) receives the first output row of every partition and the count
        of kept rows last; ``out_offsets`` (int64, nrows + 1 entries; optional for fixed-width
        schemas) the offsets, entries past the count repeating the total; ``out_indices`` /
        ``out_positions`` (optional, int64, nrows entries) the source row of every output position
        and the output position of every source row, -1 past the count / for a dropped row.
        Capacity and ``out_rows=None`` as in ``take_into``."""
        keep: list = []
        _check(N.lib().fury_row_partition(*self._partition_args(
            batch, part_ids, num_parts, out_rows, out_offsets, out_part_rows, out_indices,
            out_positions, stream, keep)))

    def bind_partition(self, batch: RowBatch, part_ids, num_parts: int,
                       out_rows: Optional[torch.Tensor], out_offsets: Optional[torch.Tensor],
                       out_part_rows: torch.Tensor, out_indices: Optional[torch.Tensor] = None,
                       out_positions: Optional[torch.Tensor] = None, stream=None):
        """``partition_into`` bound like ``bind_take``: pointers resolved once (``part_ids`` is
        converted now; an int32 device tensor is read in place by every call)."""
        keep: list = []
        args = self._partition_args(batch, part_ids, num_parts, out_rows, out_offsets,
                                    out_part_rows, out_indices, out_positions, stream, keep)
        return self._bound(N.lib().fury_row_partition, args, keep, batch, out_rows, out_offsets,
                           out_part_rows, out_indices, out_positions)

    def partition(self, batch: RowBatch, part_ids, num_parts: int, stream=None,
                  return_indices: bool = False):
        """``(RowBatch of the kept rows in partition order, part_rows[num_parts + 1])`` (with
        ``return_indices``: and their source row numbers).  The ids are ranked and measured on the
        device, count and byte total come back in one host read, then the kept rows are copied.
        Partition p is ``slice_rows(out, part_rows[p], part_rows[p + 1])``."""
        self._check_hash(batch)
        n = batch.nrows
        fixed = self._schema.is_fixed
        ids = self._part_ids(part_ids, n, stream)
        with _on(stream):
            part_rows = torch.empty(num_parts + 1 if num_parts > 0 else 1, dtype=torch.int64,
                                    device=self.device)
            idx = torch.empty(max(n, 1), dtype=torch.int64, device=self.device)
            offs = None if fixed else torch.empty(n + 1, dtype=torch.int64, device=self.device)
            self.partition_into(batch, ids, num_parts, None, offs, part_rows,
                                idx[:n] if n else None, None, stream)
            if fixed:
                count = int(part_rows[num_parts].item())
                total = count * self._schema.fixed_size
            else:
                count, total = (int(x) for x in torch.stack((part_rows[num_parts], offs[n])).cpu())
        out, kept = self._take_kept(batch, idx, offs, count, total, stream)
        return (out, part_rows, kept) if return_indices else (out, part_rows)

    def slice_rows(self, batch: RowBatch, start: int, stop: int) -> RowBatch:
        """Rows ``[start, stop)`` of ``batch`` as a batch: ``rows`` is a view (no copy), the
        offsets are rebased to start at 0 (``None`` for fixed-width schemas).  One host read of the
        two byte positions for a variable-length schema."""
        self._check_hash(batch)
        start, stop = int(start), int(stop)
        if not 0 <= start <= stop <= batch.nrows:
            raise IndexOutOfBoundsException(
                f"rows [{start}, {stop}) are not inside a batch of {batch.nrows} rows")
        if self._schema.is_fixed or batch.row_offsets is None:
            fs = self._schema.fixed_size
            return RowBatch(batch.rows[start * fs:stop * fs], None, stop - start, self.schema_hash)
        offs = batch.row_offsets[start:stop + 1]
        b, e = (int(x) for x in offs[[0, -1]].cpu())
        return RowBatch(batch.rows[b:e], offs - b, stop - start, self.schema_hash)

    def _concat_args(self, batches: Sequence[RowBatch], out_rows, out_offsets, stream, keep: list):
        for b in batches:
            self._check_hash(b)
        tab = (N.FuryConcatSource * max(len(batches), 1))()
        for k, b in enumerate(batches):
            tab[k].rows = _ptr(b.rows) if b.nrows else None
            tab[k].row_offsets = _ptr(b.row_offsets)
            tab[k].nrows = b.nrows
        keep.append(tab)
        return (self._schema.handle, tab, len(batches), _ptr(out_rows), _nbytes(out_rows),
                _ptr(out_offsets), _stream_handle(stream))

    def concat_into(self, batches: Sequence[RowBatch], out_rows: Optional[torch.Tensor],
                    out_offsets: Optional[torch.Tensor] = None, stream=None) -> None:
        """The rows of ``batches`` (1 to 32 batches of this encoder's schema) end to end, written
        to the preallocated ``out_rows`` with their offsets in ``out_offsets`` (int64, total rows
        + 1 entries; optional for fixed-width schemas): one call, no host synchronisation.  A
        batch's offsets need not start at 0.  Capacity and ``out_rows=None`` as in ``take_into``;
        a row outside its own batch gives a 0-byte row, reported by ``device_status(stream)``.
        ``out_rows`` must not overlap any of the batches."""
        keep: list = []
        _check(N.lib().fury_row_concat(*self._concat_args(batches, out_rows, out_offsets, stream,
                                                          keep)))

    def concat(self, batches: Sequence[RowBatch], stream=None) -> RowBatch:
        """``batches`` end to end as a new batch.  Fixed-width schemas know the size up front; the
        others measure first (one host read of the byte total), then copy."""
        batches = list(batches)
        return self._measured(sum(b.nrows for b in batches), self._fixed_size(), self.schema_hash,
                              lambda rows, offs: self.concat_into(batches, rows, offs, stream),
                              stream)

    # -- key hash: key fields of every row -> hash and partition id (fury_row_hash) ----------------
    def _hash_args(self, batch: RowBatch, keys: Sequence, out_hashes, out_part_ids, seed, num_parts,
                   stream, keep: list):
        self._check_hash(batch)
        idx = self._select(keys)
        for what, t in (("out_hashes", out_hashes), ("out_part_ids", out_part_ids)):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or t.dtype not in (torch.int32, torch.uint32):
                raise IllegalArgumentException(f"{what} must be an int32 or uint32 tensor")
            if t.numel() < batch.nrows:
                raise IllegalArgumentException(
                    f"{what} has {t.numel()} entries for {batch.nrows} rows")
        seed = int(seed)
        if not 0 <= seed <= 0xFFFFFFFF:
            raise IllegalArgumentException(f"seed {seed} is not an unsigned 32-bit value")
        if out_part_ids is None:
            num_parts = 0                       # unused by the call
        elif num_parts is None or not 1 <= int(num_parts) <= 0x7FFFFFFF:
            raise IllegalArgumentException(f"num_parts {num_parts} is not in [1, 2**31 - 1]")
        sel = (ctypes.c_int32 * max(len(idx), 1))(*idx)
        keep.append(sel)
        return (self._schema.handle, sel, len(idx), _ptr(batch.rows), _ptr(batch.row_offsets),
                batch.nrows, seed, int(num_parts), _ptr(out_hashes), _ptr(out_part_ids),
                _stream_handle(stream))

    def hash_rows_into(self, batch: RowBatch, keys: Sequence, out_hashes: Optional[torch.Tensor],
                       out_part_ids: Optional[torch.Tensor] = None, seed: int = 0,
                       num_parts: Optional[int] = None, stream=None) -> None:
        """Hashes the key fields ``keys`` (names or slot indices, in key order; 1 to 64 fixed-width,
        BOOL, DECIMAL, STRING or BINARY fields) of every row: MurmurHash3_x86_32 over the bytes
        ``project_batch`` would decode for each key, each value's hash seeding the next, a null key
        hashed as ``hash_null`` (the numbered rules are in ``include/fury_row.h``).
        ``out_hashes`` (uint32 or int32, ``nrows`` entries) receives the hash, ``out_part_ids``
        (int32, ``nrows`` entries) ``hash % num_parts``, the ids ``partition_into`` takes; either
        may be ``None``, not both.  One call, no host synchronisation, no workspace.  A row or key
        value outside the batch is a null key, reported by ``device_status(stream)``."""
        keep: list = []
        _check(N.lib().fury_row_hash(*self._hash_args(batch, keys, out_hashes, out_part_ids, seed,
                                                      num_parts, stream, keep)))

    def bind_hash(self, batch: RowBatch, keys: Sequence, out_hashes: Optional[torch.Tensor],
                  out_part_ids: Optional[torch.Tensor] = None, seed: int = 0,
                  num_parts: Optional[int] = None, stream=None):
        """``hash_rows_into`` bound like ``bind_project``: keys and pointers resolved once."""
        keep: list = []
        args = self._hash_args(batch, keys, out_hashes, out_part_ids, seed, num_parts, stream, keep)
        return self._bound(N.lib().fury_row_hash, args, keep, batch, out_hashes, out_part_ids)

    def hash_rows(self, batch: RowBatch, keys: Sequence, seed: int = 0,
                  num_parts: Optional[int] = None, stream=None):
        """The uint32 hash of every row's key fields; with ``num_parts``: ``(hashes, part_ids)``,
        ``part_ids`` int32 = ``hashes % num_parts``.  See ``hash_rows_into``."""
        n = batch.nrows
        with _on(stream):
            hashes = torch.empty(n, dtype=torch.uint32, device=self.device)
            ids = None if num_parts is None else torch.empty(n, dtype=torch.int32,
                                                             device=self.device)
        if n > 0:                                # an empty tensor has no address to pass
            self.hash_rows_into(batch, keys, hashes, ids, seed, num_parts, stream)
            self.device_status(stream)
        return hashes if num_parts is None else (hashes, ids)

    def partition_by(self, batch: RowBatch, keys: Sequence, num_parts: int, seed: int = 0,
                     stream=None):
        """``partition`` by the hash of the key fields: ``(out, part_rows)`` with every row in
        partition ``hash_rows(batch, keys, seed) % num_parts``.  The ids are hashed and the rows
        ranked on ``stream`` with no host synchronisation in between; ``num_parts`` is
        ``partition``'s (at most 65535)."""
        with _on(stream):
            ids = torch.empty(batch.nrows, dtype=torch.int32, device=self.device)
        if batch.nrows > 0:
            self.hash_rows_into(batch, keys, None, ids, seed, num_parts, stream)
        return self.partition(batch, ids, num_parts, stream)

    # -- field selection: a subset of the fields, as rows (getters feeding a BinaryRowWriter) -----
    def selected_encoder(self, select: Sequence) -> "RowEncoder":
        """The ``RowEncoder`` of the fields ``select`` (names or slot indices, in selection order,
        no duplicates), on this encoder's device and cached per selection: the codec of what
        ``select_fields`` returns."""
        idx = self._select(select)
        cache = self.__dict__.setdefault("_selected", {})
        enc = cache.get(tuple(idx))
        if enc is None:
            sel = (ctypes.c_int32 * max(len(idx), 1))(*idx)
            h = ctypes.c_void_p()              # the library checks the selection: its rules, its messages
            _check(N.lib().fury_schema_select(self._schema.handle, sel, len(idx), ctypes.byref(h)))
            N.lib().fury_schema_destroy(h)
            enc = RowEncoder([self._schema.fields[k] for k in idx], self.device)
            cache[tuple(idx)] = enc
        return enc

    def _select_args(self, batch: RowBatch, select: Sequence, out_rows, out_offsets, stream,
                     keep: list):
        self._check_hash(batch)
        idx = self._select(select)
        sel = (ctypes.c_int32 * max(len(idx), 1))(*idx)
        keep.append(sel)
        return (self._schema.handle, sel, len(idx), _ptr(batch.rows), _ptr(batch.row_offsets),
                batch.nrows, _ptr(out_rows), _nbytes(out_rows), _ptr(out_offsets),
                _stream_handle(stream))

    def select_fields_into(self, batch: RowBatch, select: Sequence,
                           out_rows: Optional[torch.Tensor],
                           out_offsets: Optional[torch.Tensor] = None, stream=None) -> None:
        """Row r of the output = the fields ``select`` (names or slot indices, any order, no
        duplicates) of row r of ``batch``, as a row of ``selected_encoder(select)``: written to the
        preallocated ``out_rows`` (capacity = its size) with the offsets in ``out_offsets`` (int64,
        nrows + 1 entries; optional when every selected field is fixed-width).  One call, no host
        synchronisation; every field type may be selected, nested ones included.  Capacity and
        ``out_rows=None`` as in ``take_into``; a malformed value comes out null, a malformed row all
        null, both reported by ``device_status(stream)``.  ``out_rows`` must not overlap
        ``batch.rows``."""
        keep: list = []
        _check(N.lib().fury_row_select(*self._select_args(batch, select, out_rows, out_offsets,
                                                          stream, keep)))

    def bind_select_fields(self, batch: RowBatch, select: Sequence,
                           out_rows: Optional[torch.Tensor],
                           out_offsets: Optional[torch.Tensor] = None, stream=None):
        """``select_fields_into`` bound like ``bind_take``: selection and pointers resolved once."""
        keep: list = []
        args = self._select_args(batch, select, out_rows, out_offsets, stream, keep)
        return self._bound(N.lib().fury_row_select, args, keep, batch, out_rows, out_offsets)

    def select_fields(self, batch: RowBatch, select: Sequence, stream=None) -> RowBatch:
        """The fields ``select`` of every row of ``batch`` as a new batch of
        ``selected_encoder(select)`` (its ``schema_hash``).  A fixed-width selection knows its size
        up front; the others measure first (one host read of the byte total), then write."""
        self._check_hash(batch)
        idx = self._select(select)
        child = self.selected_encoder(idx)
        return self._measured(
            batch.nrows, child._fixed_size(), child.schema_hash,
            lambda rows, offs: self.select_fields_into(batch, idx, rows, offs, stream), stream)

    # -- zip: the fields of several batches joined row by row (several BinaryRows' getters feeding
    # one BinaryRowWriter).  ``self`` is source 0, ``others`` the (encoder, batch) pairs of sources
    # 1 ...; ``picks`` is a sequence of (source index, field name or slot).
    @staticmethod
    def _picks(encoders: Sequence["RowEncoder"], picks: Sequence) -> List[Tuple[int, int]]:
        out = []
        for p in picks:
            s, x = p
            s = int(s)
            if isinstance(x, str):
                if not 0 <= s < len(encoders):
                    raise IllegalArgumentException(
                        f"pick {p!r} names source {s} of {len(encoders)} sources")
                x = encoders[s]._select([x])[0]
            out.append((s, int(x)))
        return out

    @staticmethod
    def _c_picks(picks: Sequence[Tuple[int, int]]):
        flat = [w for p in picks for w in p]
        return (ctypes.c_int32 * max(len(flat), 2))(*flat)

    def zipped_encoder(self, others_encoders: Sequence["RowEncoder"], picks: Sequence,
                       names: Optional[Sequence[str]] = None) -> "RowEncoder":
        """The ``RowEncoder`` of the fields ``picks`` of the sources ``[self, *others_encoders]``, in
        pick order, on this encoder's device and cached per picks: the codec of what ``zip_fields``
        returns.  ``names`` renames the output fields (names do not enter row bytes or the schema's
        layout; the rename only lets callers avoid clashing names)."""
        encoders = [self, *others_encoders]
        idx = self._picks(encoders, picks)
        key = (tuple(id(e) for e in others_encoders), tuple(idx), None if names is None else tuple(names))
        cache = self.__dict__.setdefault("_zipped", {})
        hit = cache.get(key)
        if hit is None:
            hs = (ctypes.c_void_p * len(encoders))(*[e._schema.handle for e in encoders])
            h = ctypes.c_void_p()              # the library checks the picks: its rules, its messages
            _check(N.lib().fury_schema_zip(hs, len(encoders), self._c_picks(idx), len(idx),
                                           ctypes.byref(h)))
            N.lib().fury_schema_destroy(h)
            fields = [encoders[s]._schema.fields[k] for s, k in idx]
            if names is not None:
                if len(names) != len(fields):
                    raise IllegalArgumentException(f"{len(names)} names for {len(fields)} picks")
                fields = [Field(n, f.type_id, f.nullable, f.children) for n, f in zip(names, fields)]
            hit = (RowEncoder(fields, self.device), tuple(others_encoders))   # the ids stay taken
            cache[key] = hit
        return hit[0]

    def _zip_sources(self, batch: RowBatch, others: Sequence):
        """The encoders and batches of all sources, schema hashes and row counts checked."""
        encoders = [self] + [e for e, _ in others]
        batches = [batch] + [b for _, b in others]
        for e, b in zip(encoders, batches):
            e._check_hash(b)
        for s, b in enumerate(batches):
            if b.nrows != batch.nrows:
                raise IllegalArgumentException(
                    f"source {s} has {b.nrows} rows, source 0 has {batch.nrows}: zip joins rows one "
                    "to one")
        return encoders, batches

    def _zip_args(self, batch: RowBatch, others: Sequence, picks: Sequence, out_rows, out_offsets,
                  stream, keep: list):
        encoders, batches = self._zip_sources(batch, others)
        n = batch.nrows
        idx = self._picks(encoders, picks)
        srcs = (N.FuryZipSource * max(len(encoders), 1))()
        for s, (e, b) in enumerate(zip(encoders, batches)):
            srcs[s].schema = e._schema.handle
            srcs[s].rows = _ptr(b.rows)
            srcs[s].row_offsets = _ptr(b.row_offsets)
        cp = self._c_picks(idx)
        keep.extend((srcs, cp, encoders, batches))
        return (srcs, len(encoders), cp, len(idx), n, _ptr(out_rows), _nbytes(out_rows),
                _ptr(out_offsets), _stream_handle(stream))

    def zip_fields_into(self, batch: RowBatch, others: Sequence, picks: Sequence,
                        out_rows: Optional[torch.Tensor],
                        out_offsets: Optional[torch.Tensor] = None, stream=None) -> None:
        """Row r of the output holds, in slot j, field ``picks[j]`` = (source, name or slot) of row r of
        that source -- source 0 is ``batch`` (of this encoder), sources 1 ... are the ``(encoder,
        batch)`` pairs ``others`` -- as a row of ``zipped_encoder``: written to the preallocated
        ``out_rows`` with the offsets in ``out_offsets`` (int64, nrows + 1 entries; optional when
        every picked field is fixed-width).  One call, no host synchronisation; every field type may
        be picked.  Capacity, ``out_rows=None`` and malformed input as in ``select_fields_into``,
        except that a malformed row nulls only the fields picked from its own source.  ``out_rows``
        must not overlap any source; sources may alias each other."""
        keep: list = []
        _check(N.lib().fury_row_zip(*self._zip_args(batch, others, picks, out_rows, out_offsets,
                                                    stream, keep)))

    def bind_zip_fields(self, batch: RowBatch, others: Sequence, picks: Sequence,
                        out_rows: Optional[torch.Tensor],
                        out_offsets: Optional[torch.Tensor] = None, stream=None):
        """``zip_fields_into`` bound like ``bind_take``: picks and pointers resolved once."""
        keep: list = []
        args = self._zip_args(batch, others, picks, out_rows, out_offsets, stream, keep)
        return self._bound(N.lib().fury_row_zip, args, keep, batch, out_rows, out_offsets)

    def zip_fields(self, batch: RowBatch, others: Sequence, picks: Sequence,
                   stream=None) -> RowBatch:
        """The fields ``picks`` of ``batch`` and of the batches in ``others``, joined row by row, as
        a new batch of ``zipped_encoder`` (its ``schema_hash``).  Fixed-width picks know their size
        up front; the others measure first (one host read of the byte total), then write."""
        encoders, _ = self._zip_sources(batch, others)
        idx = self._picks(encoders, picks)
        child = self.zipped_encoder(encoders[1:], idx)
        return self._measured(
            batch.nrows, child._fixed_size(), child.schema_hash,
            lambda rows, offs: self.zip_fields_into(batch, others, idx, rows, offs, stream), stream)

    def _with_fields_picks(self, other_encoder: "RowEncoder") -> List[Tuple[int, int]]:
        """The picks of ``with_fields``: every field of this encoder in order, a field of
        ``other_encoder`` of the same name in its place, then the rest of ``other_encoder``."""
        theirs = {f.name: k for k, f in enumerate(other_encoder._schema.fields)}
        picks = [(1, theirs[f.name]) if f.name in theirs else (0, k)
                 for k, f in enumerate(self._schema.fields)]
        mine = {f.name for f in self._schema.fields}
        picks += [(1, k) for k, f in enumerate(other_encoder._schema.fields) if f.name not in mine]
        return picks

    def with_fields(self, batch: RowBatch, other_encoder: "RowEncoder", other_batch: RowBatch,
                    stream=None):
        """Replace or append: ``batch`` with the fields of ``other_batch`` (row r to row r) -- a
        field of ``other_encoder`` whose name this encoder has takes that field's position, whatever
        its type, the others are appended.  Returns ``(encoder, batch)`` of the result."""
        picks = self._with_fields_picks(other_encoder)
        enc = self.zipped_encoder([other_encoder], picks)
        return enc, self.zip_fields(batch, [(other_encoder, other_batch)], picks, stream)

    # -- nested values as batches (BinaryRow.getStruct / getArray / getMap over a batch) ----------
    def _path(self, path) -> List[int]:
        """Slot indices of ``path``: field names or slot indices from the top level down through
        STRUCT fields; a single name or index is a path of one."""
        if isinstance(path, (str, int)):
            path = [path]
        fields, out = self._schema.fields, []
        for x in path:
            if isinstance(x, str):
                names = {f.name: k for k, f in enumerate(fields)}
                if x not in names:
                    raise IllegalArgumentException(
                        f"no field named {x!r} at path position {len(out)} in {self._schema}")
                x = names[x]
            k = int(x)
            out.append(k)
            node = fields[k] if 0 <= k < len(fields) else None
            fields = node.children if node is not None and node.type_id == STRUCT else ()
        return out

    def child_encoder(self, path):
        """The encoder of the nested field ``path`` reaches (see ``_path``), on this encoder's
        device and cached per path: a ``RowEncoder`` of a STRUCT's fields, the ``ArrayEncoder`` of
        a LIST field, the ``MapEncoder`` of a MAP field -- the codec of what ``extract`` returns."""
        idx = self._path(path)
        cache = self.__dict__.setdefault("_children", {})
        enc = cache.get(tuple(idx))
        if enc is None:
            sel = (ctypes.c_int32 * max(len(idx), 1))(*idx)
            h = ctypes.c_void_p()              # the library checks the path: its rules, its messages
            _check(N.lib().fury_schema_child(self._schema.handle, sel, len(idx), ctypes.byref(h)))
            N.lib().fury_schema_destroy(h)
            fields = self._schema.fields
            for k in idx:
                node, fields = fields[k], fields[k].children
            enc = (RowEncoder(node.children, self.device) if node.type_id == STRUCT else
                   ArrayEncoder(node, self.device) if node.type_id == LIST else
                   MapEncoder(node, self.device))
            cache[tuple(idx)] = enc
        return enc

    def _extract_args(self, batch: RowBatch, path, out_rows, out_offsets, out_count, out_indices,
                      out_validity, stream, keep: list):
        self._check_hash(batch)
        idx = self._path(path)
        sel = (ctypes.c_int32 * max(len(idx), 1))(*idx)
        keep.append(sel)
        return (self._schema.handle, sel, len(idx), _ptr(batch.rows), _ptr(batch.row_offsets),
                batch.nrows, _ptr(out_rows), _nbytes(out_rows), _ptr(out_offsets), _ptr(out_count),
                _ptr(out_indices), _ptr(out_validity), _stream_handle(stream))

    def extract_into(self, batch: RowBatch, path, out_rows: Optional[torch.Tensor],
                     out_offsets: torch.Tensor, out_count: torch.Tensor,
                     out_indices: Optional[torch.Tensor] = None,
                     out_validity: Optional[torch.Tensor] = None, stream=None) -> None:
        """The value of the nested field ``path`` (see ``_path``; a STRUCT, LIST or MAP) of every
        row of ``batch``, packed in row order into the preallocated ``out_rows`` as a batch of
        ``child_encoder(path)``: one call, no host synchronisation.  Rows where the field (or a
        struct on the way to it) is null produce no entry: ``out_count`` (int64[1]) receives the
        number of entries, ``out_offsets`` (int64, nrows + 1 entries) their offsets -- entries past
        the count repeat the total --, ``out_indices`` (optional, int64, nrows entries) their source
        rows, -1 past the count, and ``out_validity`` (optional, uint8, whole 32-bit words) the Arrow
        bitmap of the rows that produced one.  Capacity and ``out_rows=None`` as in ``take_into``; a
        malformed value counts as null and is reported by ``device_status(stream)``."""
        keep: list = []
        _check(N.lib().fury_row_extract(*self._extract_args(
            batch, path, out_rows, out_offsets, out_count, out_indices, out_validity, stream, keep)))

    def bind_extract(self, batch: RowBatch, path, out_rows: Optional[torch.Tensor],
                     out_offsets: torch.Tensor, out_count: torch.Tensor,
                     out_indices: Optional[torch.Tensor] = None,
                     out_validity: Optional[torch.Tensor] = None, stream=None):
        """``extract_into`` bound like ``bind_take``: path and pointers resolved once."""
        keep: list = []
        args = self._extract_args(batch, path, out_rows, out_offsets, out_count, out_indices,
                                  out_validity, stream, keep)
        return self._bound(N.lib().fury_row_extract, args, keep, batch, out_rows, out_offsets,
                           out_count, out_indices, out_validity)

    def extract(self, batch: RowBatch, path, stream=None, return_indices: bool = False):
        """``(values, validity)`` of the nested field ``path``: the non-null values as a new batch
        of ``child_encoder(path)`` (its ``schema_hash``; 0 for a LIST or MAP) and the Arrow bitmap
        (uint8, LSB-first) of the rows that have one; with ``return_indices`` also their row
        numbers.  The values are located and measured on the device, count and byte total come back
        in one host read, then they are copied."""
        self._check_hash(batch)
        idx = self._path(path)
        child = self.child_encoder(idx)
        n = batch.nrows
        with _on(stream):
            head = torch.empty(2, dtype=torch.int64, device=self.device)      # count, total
            offs = torch.empty(n + 1, dtype=torch.int64, device=self.device)
            src = (torch.empty(max(n, 1), dtype=torch.int64, device=self.device)[:n]
                   if return_indices else None)
            valid = torch.zeros(((n + 31) // 32) * 4, dtype=torch.uint8, device=self.device)
            self.extract_into(batch, idx, None, offs, head[:1], None, None, stream)
            count, total = self._counted(head, offs[n:])
            rows = self._row_buffer(total)
        self.extract_into(batch, idx, rows, offs, head[:1], src if n else None,
                          valid if n else None, stream)
        self.device_status(stream)
        out = RowBatch(rows[:total], offs[:count + 1], count, child.schema_hash)
        valid = valid[:(n + 7) // 8]
        return (out, valid, src[:count]) if return_indices else (out, valid)

    # -- list and map elements as batches (BinaryArray.getStruct / getArray / getMap over a batch) -
    def _explode_sel(self, path, side):
        """(slot indices of ``path``, the C ``side``): "elements" (a LIST) and "keys" (a MAP) are
        side 0, "values" (a MAP) is side 1.  A collection encoder's own path is empty."""
        sides = {"elements": 0, "keys": 0, "values": 1}
        if side not in sides:
            raise IllegalArgumentException(f"side {side!r} is not one of {sorted(sides)}")
        return self._path(() if path is None else path), sides[side]

    def element_encoder(self, path, side: str = "elements"):
        """The encoder of the elements (``side`` "elements" of a LIST, "keys" / "values" of a MAP)
        of the LIST or MAP field ``path`` reaches (see ``_path``), cached like ``child_encoder``: a
        ``RowEncoder`` of a STRUCT element's fields, the ``ArrayEncoder`` / ``MapEncoder`` of a
        LIST / MAP element -- the codec of what ``explode`` returns."""
        idx, sd = self._explode_sel(path, side)
        cache = self.__dict__.setdefault("_elements", {})
        enc = cache.get((tuple(idx), sd))
        if enc is None:
            sel = (ctypes.c_int32 * max(len(idx), 1))(*idx)
            h = ctypes.c_void_p()              # the library checks path and side: its rules, its messages
            _check(N.lib().fury_schema_element(self._schema.handle, sel, len(idx), sd,
                                               ctypes.byref(h)))
            N.lib().fury_schema_destroy(h)
            fields = self._schema.fields
            node = fields[0]                   # a collection schema: its one field
            for k in idx:
                node, fields = fields[k], fields[k].children
            e = node.children[sd]
            enc = (RowEncoder(e.children, self.device) if e.type_id == STRUCT else
                   ArrayEncoder(e, self.device) if e.type_id == LIST else MapEncoder(e, self.device))
            cache[(tuple(idx), sd)] = enc
        return enc

    def _explode_args(self, batch: RowBatch, path, side, out_list_offsets, out_entry_validity,
                      out_rows, out_offsets, out_count, out_parents, out_ordinals, out_validity,
                      elem_capacity, stream, keep: list):
        self._check_hash(batch)
        idx, sd = self._explode_sel(path, side)
        sel = (ctypes.c_int32 * max(len(idx), 1))(*idx)
        keep.append(sel)
        if elem_capacity is None:
            elem_capacity = 0 if out_offsets is None else out_offsets.numel() - 1
        return (self._schema.handle, sel, len(idx), sd, _ptr(batch.rows), _ptr(batch.row_offsets),
                batch.nrows, _ptr(out_list_offsets), _ptr(out_entry_validity), int(elem_capacity),
                _ptr(out_rows), _nbytes(out_rows), _ptr(out_offsets), _ptr(out_count),
                _ptr(out_parents), _ptr(out_ordinals), _ptr(out_validity), _stream_handle(stream))

    def explode_into(self, batch: RowBatch, path, out_list_offsets: torch.Tensor,
                     out_entry_validity: Optional[torch.Tensor] = None,
                     out_rows: Optional[torch.Tensor] = None,
                     out_offsets: Optional[torch.Tensor] = None,
                     out_count: Optional[torch.Tensor] = None,
                     out_parents: Optional[torch.Tensor] = None,
                     out_ordinals: Optional[torch.Tensor] = None,
                     out_validity: Optional[torch.Tensor] = None, side: str = "elements",
                     elem_capacity: Optional[int] = None, stream=None) -> None:
        """The non-null elements of the LIST or MAP field ``path`` (``side``: see
        ``element_encoder``) of every row of ``batch``, packed in (row, ordinal) order into the
        preallocated ``out_rows`` as a batch of ``element_encoder(path, side)``: one call, no host
        synchronisation.  ``out_list_offsets`` (int64, nrows + 1 entries) receives the Arrow list
        offsets of the column -- its last entry is the element count E, nulls included --,
        ``out_entry_validity`` (optional, uint8, whole 32-bit words) the bitmap of the rows that
        have an array.  Per element, for at most ``elem_capacity`` elements (default: the entries
        of ``out_offsets`` - 1): ``out_count`` (int64[1]) the number of entries, ``out_offsets``
        (int64, elem_capacity + 1 entries) their offsets -- entries past the count repeat the total
        --, ``out_parents`` (optional, int64) / ``out_ordinals`` (optional, int32) the source row
        and the ordinal of each entry, -1 past the count, and ``out_validity`` (optional, uint8,
        whole 32-bit words) the Arrow validity of the LIST's child.  ``out_offsets=None`` is the
        count form: only the first two outputs.  Capacity and ``out_rows=None`` as in
        ``take_into``; a malformed array or element counts as null and is reported by
        ``device_status(stream)``."""
        keep: list = []
        _check(N.lib().fury_row_explode(*self._explode_args(
            batch, path, side, out_list_offsets, out_entry_validity, out_rows, out_offsets,
            out_count, out_parents, out_ordinals, out_validity, elem_capacity, stream, keep)))

    def bind_explode(self, batch: RowBatch, path, out_list_offsets: torch.Tensor,
                     out_entry_validity: Optional[torch.Tensor] = None,
                     out_rows: Optional[torch.Tensor] = None,
                     out_offsets: Optional[torch.Tensor] = None,
                     out_count: Optional[torch.Tensor] = None,
                     out_parents: Optional[torch.Tensor] = None,
                     out_ordinals: Optional[torch.Tensor] = None,
                     out_validity: Optional[torch.Tensor] = None, side: str = "elements",
                     elem_capacity: Optional[int] = None, stream=None):
        """``explode_into`` bound like ``bind_extract``: path and pointers resolved once."""
        keep: list = []
        args = self._explode_args(batch, path, side, out_list_offsets, out_entry_validity, out_rows,
                                  out_offsets, out_count, out_parents, out_ordinals, out_validity,
                                  elem_capacity, stream, keep)
        return self._bound(N.lib().fury_row_explode, args, keep, batch, out_list_offsets,
                           out_entry_validity, out_rows, out_offsets, out_count, out_parents,
                           out_ordinals, out_validity)

    def explode(self, batch: RowBatch, path, side: str = "elements", stream=None):
        """``(elements, list_offsets, entry_validity, elem_validity, parents, ordinals)`` of the
        LIST or MAP field ``path``: the non-null elements as a new batch of
        ``element_encoder(path, side)``, the Arrow list offsets (int64, nrows + 1) and validity
        (uint8, LSB-first) of the column, the Arrow validity of its child (one bit per element,
        nulls included), and the source row (int64) and ordinal (int32) of every entry of
        ``elements``.  The arrays are counted on the device (one host read of the element count),
        the elements located and measured (one host read of entry count and byte total), then
        copied."""
        self._check_hash(batch)
        idx, _ = self._explode_sel(path, side)
        # RowEncoder.*: a collection encoder overrides these methods without the path
        child = RowEncoder.element_encoder(self, idx, side)
        n = batch.nrows
        with _on(stream):
            lo = torch.empty(n + 1, dtype=torch.int64, device=self.device)
            ev = torch.zeros(((n + 31) // 32) * 4, dtype=torch.uint8, device=self.device)
            into = lambda *a: RowEncoder.explode_into(self, batch, idx, lo, ev if n else None, *a,  # noqa: E731
                                                      side=side, stream=stream)
            into()
            E = int(lo[n].item())
            head = torch.empty(2, dtype=torch.int64, device=self.device)      # count, total
            offs = torch.empty(E + 1, dtype=torch.int64, device=self.device)
            par = torch.empty(max(E, 1), dtype=torch.int64, device=self.device)[:E]
            ords = torch.empty(max(E, 1), dtype=torch.int32, device=self.device)[:E]
            valid = torch.zeros(((E + 31) // 32) * 4, dtype=torch.uint8, device=self.device)
            outs = (par if E else None, ords if E else None, valid if E else None)
            into(None, offs, head[:1], *outs)
            count, total = self._counted(head, offs[E:])
            rows = self._row_buffer(total)
        into(rows, offs, head[:1], *outs)
        self.device_status(stream)
        out = RowBatch(rows[:total], offs[:count + 1], count, child.schema_hash)
        return (out, lo, ev[:(n + 7) // 8], valid[:(E + 7) // 8], par[:count], ords[:count])

    # -- elements and nested values back into rows (BinaryArrayWriter / BinaryRowWriter.write of a
    #    nested value over a batch): the inverses of explode and extract ---------------------------
    def field_encoder(self, name) -> "RowEncoder":
        """The one-field ``RowEncoder`` of the field ``name`` (a name or slot index), cached: the
        target of ``implode`` / ``wrap`` for that field, and what ``with_fields`` takes back."""
        return self.selected_encoder([name])

    def _value_encoder(self, wrap: bool):
        """The encoder of the values ``wrap`` (the field) / ``implode`` (the LIST's elements) take,
        or None when this encoder is no target: the library then says why."""
        key = "_wrap_values" if wrap else "_implode_values"
        if key not in self.__dict__:
            f = self._schema.fields
            node = f[0] if len(f) == 1 and (not wrap or not self._schema.collection) else None
            if node is not None and not wrap:
                node = node.children[0] if node.type_id == LIST else None
            self.__dict__[key] = (
                None if node is None or node.type_id not in (STRUCT, LIST, MAP) else
                RowEncoder(node.children, self.device) if node.type_id == STRUCT else
                ArrayEncoder(node, self.device) if node.type_id == LIST else
                MapEncoder(node, self.device))
        return self.__dict__[key]

    def _value_args(self, values: RowBatch, wrap: bool, stream, keep: list):
        """(values, value_offsets, num_values) of a compact batch of values."""
        child = self._value_encoder(wrap)
        if child is not None:
            child._check_hash(values)
        vo = values.row_offsets
        if vo is None:                         # fixed-width rows: row i at i * fixed_size
            size = child._schema.fixed_size if child is not None else 0
            with _on(stream):
                vo = torch.arange(values.nrows + 1, dtype=torch.int64, device=self.device) * size
            keep.append(vo)
        rows = values.rows
        if rows.numel() == 0:                  # every value empty: still a pointer, never read
            with _on(stream):
                rows = torch.empty(16, dtype=torch.uint8, device=self.device)
            keep.append(rows)
        return _ptr(rows), _ptr(vo), vo.numel() - 1

    def _bitmap_words(self, bits, count: Optional[int], stream, keep: list):
        """``bits`` as the device bitmap the kernels read (see ``_mask_words``; a uint8 bitmap that
        is no whole number of 32-bit words is copied into one that is) and the number of bits a
        ``count`` of None stands for: a bool tensor's entries, a bitmap's 8 per byte."""
        if bits is None:
            return None, count
        if bits.dtype == torch.bool:
            n = bits.numel()
            words = self._mask_words(bits, n, stream)
        else:
            n = 8 * bits.numel()
            words = bits
            if bits.numel() % 4:
                with _on(stream):
                    words = torch.zeros((bits.numel() + 3) // 4 * 4, dtype=torch.uint8,
                                        device=self.device)
                    words[:bits.numel()] = bits
        keep.append(words)
        return words, n if count is None else count

    def _implode_args(self, elements: RowBatch, list_offsets, entry_validity, elem_validity,
                      num_elements, out_rows, out_offsets, stream, keep: list):
        vals = self._value_args(elements, False, stream, keep)
        nrows = list_offsets.numel() - 1
        ev, _ = self._bitmap_words(entry_validity, nrows, stream, keep)
        lv, num_elements = self._bitmap_words(elem_validity, num_elements, stream, keep)
        if num_elements is None:               # every element present: as many as there are values
            num_elements = elements.nrows
        return (self._schema.handle, *vals, _ptr(list_offsets), nrows, _ptr(ev), _ptr(lv),
                int(num_elements), _ptr(out_rows), _nbytes(out_rows), _ptr(out_offsets),
                _stream_handle(stream))

    def implode_into(self, elements: RowBatch, list_offsets: torch.Tensor,
                     out_rows: Optional[torch.Tensor], out_offsets: torch.Tensor,
                     entry_validity: Optional[torch.Tensor] = None,
                     elem_validity: Optional[torch.Tensor] = None,
                     num_elements: Optional[int] = None, stream=None) -> None:
        """The inverse of ``explode``, on the TARGET encoder -- a one-field encoder whose field is a
        LIST of STRUCT / LIST / MAP (``field_encoder(name)``: output row r is a row holding the list)
        or the ``ArrayEncoder`` of such a list (output entry r is the array; no ``entry_validity``).
        ``elements`` is the compact batch of element values ``explode`` returned (processed or not),
        ``list_offsets`` (int64, nrows + 1 entries) the Arrow list offsets, ``entry_validity`` /
        ``elem_validity`` (optional; device bitmaps, LSB-first, or bool tensors) the rows that have
        a list and the elements that are not null: a present element takes the next value in
        order.  ``num_elements`` defaults to the bits of ``elem_validity`` (a bool tensor's entries,
        8 per byte of a bitmap) or, without one, to ``elements.nrows``.  One call, no host
        synchronisation; ``out_offsets`` (int64, nrows + 1 entries), capacity and ``out_rows=None``
        as in ``take_into``; a malformed value or range comes out null and is reported by
        ``device_status(stream)``.  ``out_rows`` must not overlap ``elements.rows``."""
        keep: list = []
        _check(N.lib().fury_row_implode(*self._implode_args(
            elements, list_offsets, entry_validity, elem_validity, num_elements, out_rows,
            out_offsets, stream, keep)))

    def bind_implode(self, elements: RowBatch, list_offsets: torch.Tensor,
                     out_rows: Optional[torch.Tensor], out_offsets: torch.Tensor,
                     entry_validity: Optional[torch.Tensor] = None,
                     elem_validity: Optional[torch.Tensor] = None,
                     num_elements: Optional[int] = None, stream=None):
        """``implode_into`` bound like ``bind_explode``: pointers resolved once."""
        keep: list = []
        args = self._implode_args(elements, list_offsets, entry_validity, elem_validity,
                                  num_elements, out_rows, out_offsets, stream, keep)
        return self._bound(N.lib().fury_row_implode, args, keep, elements, list_offsets, out_rows,
                           out_offsets)

    def implode(self, elements: RowBatch, list_offsets: torch.Tensor,
                entry_validity: Optional[torch.Tensor] = None,
                elem_validity: Optional[torch.Tensor] = None,
                num_elements: Optional[int] = None, stream=None) -> RowBatch:
        """``implode_into`` into a new batch of this encoder: measured on the device (one host read
        of the byte total), then written."""
        child = self._value_encoder(False)
        if child is not None:
            child._check_hash(elements)
        return self._measured(
            list_offsets.numel() - 1, None, self.schema_hash,
            lambda rows, offs: self.implode_into(elements, list_offsets, rows, offs, entry_validity,
                                                 elem_validity, num_elements, stream), stream)

    def _wrap_args(self, values: RowBatch, validity, nrows, out_rows, out_offsets, stream,
                   keep: list):
        vals = self._value_args(values, True, stream, keep)
        bits, nrows = self._bitmap_words(validity, nrows, stream, keep)
        if nrows is None:                      # every row present: as many as there are values
            nrows = values.nrows
        return (self._schema.handle, *vals, _ptr(bits), int(nrows), _ptr(out_rows),
                _nbytes(out_rows), _ptr(out_offsets), _stream_handle(stream))

    def wrap_into(self, values: RowBatch, out_rows: Optional[torch.Tensor],
                  out_offsets: torch.Tensor, validity: Optional[torch.Tensor] = None,
                  nrows: Optional[int] = None, stream=None) -> None:
        """The inverse of ``extract``, on the TARGET encoder -- a one-field encoder whose field is a
        STRUCT, LIST or MAP (``field_encoder(name)``): output row r holds the next value of the
        compact batch ``values`` when its ``validity`` bit (optional; device bitmap, LSB-first, or
        bool tensor) is 1, else a null field.  ``nrows`` defaults like ``implode_into``'s
        ``num_elements``.  One call, no host synchronisation; outputs as in ``implode_into``."""
        keep: list = []
        _check(N.lib().fury_row_wrap(*self._wrap_args(values, validity, nrows, out_rows, out_offsets,
                                                      stream, keep)))

    def bind_wrap(self, values: RowBatch, out_rows: Optional[torch.Tensor],
                  out_offsets: torch.Tensor, validity: Optional[torch.Tensor] = None,
                  nrows: Optional[int] = None, stream=None):
        """``wrap_into`` bound like ``bind_extract``: pointers resolved once."""
        keep: list = []
        args = self._wrap_args(values, validity, nrows, out_rows, out_offsets, stream, keep)
        return self._bound(N.lib().fury_row_wrap, args, keep, values, out_rows, out_offsets)

    def wrap(self, values: RowBatch, validity: Optional[torch.Tensor] = None,
             nrows: Optional[int] = None, stream=None) -> RowBatch:
        """``wrap_into`` into a new batch of this encoder: measured on the device (one host read of
        the byte total), then written."""
        keep: list = []
        n = self._wrap_args(values, validity, nrows, None, None, stream, keep)[5]
        return self._measured(
            n, None, self.schema_hash,
            lambda rows, offs: self.wrap_into(values, rows, offs, validity, n, stream), stream)

    def with_elements(self, batch: RowBatch, name, elements: RowBatch, list_offsets: torch.Tensor,
                      entry_validity: Optional[torch.Tensor] = None,
                      elem_validity: Optional[torch.Tensor] = None, stream=None):
        """``batch`` with its LIST field ``name`` rebuilt from ``elements`` (``implode`` on
        ``field_encoder(name)``, then ``with_fields``): explode, process the elements, put them
        back.  Returns ``(encoder, batch)`` of the result."""
        enc = self.field_encoder(name)
        lists = enc.implode(elements, list_offsets, entry_validity, elem_validity, stream=stream)
        return self.with_fields(batch, enc, lists, stream)

    def with_nested(self, batch: RowBatch, name, values: RowBatch,
                    validity: Optional[torch.Tensor] = None, stream=None):
        """``batch`` with its STRUCT / LIST / MAP field ``name`` replaced by ``values`` (``wrap`` on
        ``field_encoder(name)``, then ``with_fields``).  Returns ``(encoder, batch)``."""
        enc = self.field_encoder(name)
        rows = enc.wrap(values, validity, batch.nrows, stream)
        return self.with_fields(batch, enc, rows, stream)

    # -- maps as key / value arrays and back (BinaryMap.keyArray / valueArray and the constructor
    #    BinaryMap(keys, values, field) over a batch) ------------------------------------------------
    def _map_side_encoder(self, path, side: int) -> "ArrayEncoder":
        idx = self._path(() if path is None else path)
        cache = self.__dict__.setdefault("_map_sides", {})
        enc = cache.get((tuple(idx), side))
        if enc is None:
            sel = (ctypes.c_int32 * max(len(idx), 1))(*idx)
            h = ctypes.c_void_p()              # the library checks the path: its rules, its messages
            _check(N.lib().fury_schema_map_side(self._schema.handle, sel, len(idx), side,
                                                ctypes.byref(h)))
            N.lib().fury_schema_destroy(h)
            fields = self._schema.fields
            node = fields[0]                   # a collection schema: its one field
            for k in idx:
                node, fields = fields[k], fields[k].children
            enc = ArrayEncoder(Field(node.name, LIST, node.nullable, (node.children[side],)),
                               self.device)
            cache[(tuple(idx), side)] = enc
        return enc

    def key_array_encoder(self, path) -> "ArrayEncoder":
        """The ``ArrayEncoder`` of the key arrays of the MAP field ``path`` reaches (see ``_path``),
        cached: the codec of the first batch ``split_map`` returns."""
        return self._map_side_encoder(path, 0)

    def value_array_encoder(self, path) -> "ArrayEncoder":
        """The ``ArrayEncoder`` of the value arrays of the MAP field ``path``: the codec of the
        second batch ``split_map`` returns."""
        return self._map_side_encoder(path, 1)

    def _split_map_args(self, batch: RowBatch, path, out_keys, out_key_offsets, out_values,
                        out_value_offsets, out_count, out_indices, out_validity, stream, keep: list):
        self._check_hash(batch)
        idx = self._path(() if path is None else path)
        sel = (ctypes.c_int32 * max(len(idx), 1))(*idx)
        keep.append(sel)
        return (self._schema.handle, sel, len(idx), _ptr(batch.rows), _ptr(batch.row_offsets),
                batch.nrows, _ptr(out_keys), _nbytes(out_keys), _ptr(out_key_offsets),
                _ptr(out_values), _nbytes(out_values), _ptr(out_value_offsets), _ptr(out_count),
                _ptr(out_indices), _ptr(out_validity), _stream_handle(stream))

    def split_map_into(self, batch: RowBatch, path, out_keys: Optional[torch.Tensor],
                       out_key_offsets: Optional[torch.Tensor],
                       out_values: Optional[torch.Tensor],
                       out_value_offsets: Optional[torch.Tensor], out_count: torch.Tensor,
                       out_indices: Optional[torch.Tensor] = None,
                       out_validity: Optional[torch.Tensor] = None, stream=None) -> None:
        """The key array and the value array of the MAP field ``path`` (see ``_path``) of every row
        of ``batch``, packed in row order into ``out_keys`` / ``out_values`` as batches of
        ``key_array_encoder(path)`` / ``value_array_encoder(path)``: one call, no host
        synchronisation.  Both batches have the same entries: ``out_count``, ``out_indices`` and
        ``out_validity`` are shared and each side has its own offsets (int64, nrows + 1 entries),
        capacity and measure form (buffer None), all as in ``extract_into``.  A side whose offsets
        are None is skipped.  A malformed map counts as null and is reported by
        ``device_status(stream)``."""
        keep: list = []
        _check(N.lib().fury_row_map_split(*self._split_map_args(
            batch, path, out_keys, out_key_offsets, out_values, out_value_offsets, out_count,
            out_indices, out_validity, stream, keep)))

    def bind_split_map(self, batch: RowBatch, path, out_keys: Optional[torch.Tensor],
                       out_key_offsets: Optional[torch.Tensor],
                       out_values: Optional[torch.Tensor],
                       out_value_offsets: Optional[torch.Tensor], out_count: torch.Tensor,
                       out_indices: Optional[torch.Tensor] = None,
                       out_validity: Optional[torch.Tensor] = None, stream=None):
        """``split_map_into`` bound like ``bind_extract``: path and pointers resolved once."""
        keep: list = []
        args = self._split_map_args(batch, path, out_keys, out_key_offsets, out_values,
                                    out_value_offsets, out_count, out_indices, out_validity, stream,
                                    keep)
        return self._bound(N.lib().fury_row_map_split, args, keep, batch, out_keys, out_key_offsets,
                           out_values, out_value_offsets, out_count, out_indices, out_validity)

    def split_map(self, batch: RowBatch, path, stream=None):
        """``(keys, values, indices, validity)`` of the MAP field ``path``: the key arrays and the
        value arrays of the non-null maps as two batches of ``key_array_encoder(path)`` /
        ``value_array_encoder(path)`` (schema_hash 0), their row numbers (int64) and the Arrow
        bitmap (uint8, LSB-first) of the rows that have a map.  Located and measured on the device,
        count and byte totals come back in one host read, then both sides are copied in one call."""
        self._check_hash(batch)
        idx = self._path(() if path is None else path)
        n = batch.nrows
        with _on(stream):
            head = torch.empty(3, dtype=torch.int64, device=self.device)      # count, key / value bytes
            ko = torch.empty(n + 1, dtype=torch.int64, device=self.device)
            vo = torch.empty(n + 1, dtype=torch.int64, device=self.device)
            src = torch.empty(max(n, 1), dtype=torch.int64, device=self.device)[:n]
            valid = torch.zeros(((n + 31) // 32) * 4, dtype=torch.uint8, device=self.device)
            into = lambda k, v, *opt: RowEncoder.split_map_into(                 # noqa: E731
                self, batch, idx, k, ko, v, vo, head[:1], *opt, stream=stream)
            into(None, None)
            count, kt, vt = self._counted(head, ko[n:], vo[n:])
            keys = self._row_buffer(kt)
            vals = self._row_buffer(vt)
        into(keys, vals, src if n else None, valid if n else None)
        self.device_status(stream)
        return (RowBatch(keys[:kt], ko[:count + 1], count, 0),
                RowBatch(vals[:vt], vo[:count + 1], count, 0), src[:count], valid[:(n + 7) // 8])

    def _join_map_args(self, keys: RowBatch, values: RowBatch, validity, nrows, out_rows,
                       out_offsets, stream, keep: list):
        for b in (keys, values):
            if b.schema_hash != 0:
                raise ClassNotCompatibleException(
                    f"join_map takes two array batches (schema hash 0), not one of hash "
                    f"{b.schema_hash}")
        if keys.nrows != values.nrows:
            raise IllegalArgumentException(
                f"join_map: {keys.nrows} key arrays and {values.nrows} value arrays")
        ptrs = []
        for b in (keys, values):
            rows = b.rows
            if rows.numel() == 0:              # no entries: still a pointer, never read
                with _on(stream):
                    rows = torch.empty(16, dtype=torch.uint8, device=self.device)
                keep.append(rows)
            ptrs += [_ptr(rows), _ptr(b.row_offsets)]
        bits, nrows = self._bitmap_words(validity, nrows, stream, keep)
        if nrows is None:                      # every row present: as many as there are entries
            nrows = keys.nrows
        return (self._schema.handle, *ptrs, keys.row_offsets.numel() - 1, _ptr(bits), int(nrows),
                _ptr(out_rows), _nbytes(out_rows), _ptr(out_offsets), _stream_handle(stream))

    def join_map_into(self, keys: RowBatch, values: RowBatch, out_rows: Optional[torch.Tensor],
                      out_offsets: torch.Tensor, validity: Optional[torch.Tensor] = None,
                      nrows: Optional[int] = None, stream=None) -> None:
        """The inverse of ``split_map``, on the TARGET encoder -- a one-field encoder whose field is
        a MAP (``field_encoder(name)``: output row r is a row holding the map) or the ``MapEncoder``
        of such a map (output entry r is the map; no ``validity``).  ``keys`` / ``values`` are the
        two compact array batches ``split_map`` returned (processed or not, with the same number of
        entries); output row r takes the next entry of both when its ``validity`` bit (optional;
        device bitmap, LSB-first, or bool tensor) is 1, else it holds a null field.  ``nrows``
        defaults like ``wrap_into``'s.  One call, no host synchronisation; outputs as in
        ``implode_into``; a malformed entry or two arrays of different element counts come out null
        and are reported by ``device_status(stream)``.  ``out_rows`` must overlap neither input."""
        keep: list = []
        _check(N.lib().fury_row_map_join(*self._join_map_args(keys, values, validity, nrows, out_rows,
                                                              out_offsets, stream, keep)))

    def bind_join_map(self, keys: RowBatch, values: RowBatch, out_rows: Optional[torch.Tensor],
                      out_offsets: torch.Tensor, validity: Optional[torch.Tensor] = None,
                      nrows: Optional[int] = None, stream=None):
        """``join_map_into`` bound like ``bind_wrap``: pointers resolved once."""
        keep: list = []
        args = self._join_map_args(keys, values, validity, nrows, out_rows, out_offsets, stream, keep)
        return self._bound(N.lib().fury_row_map_join, args, keep, keys, values, out_rows, out_offsets)

    def join_map(self, keys: RowBatch, values: RowBatch, validity: Optional[torch.Tensor] = None,
                 nrows: Optional[int] = None, stream=None) -> RowBatch:
        """``join_map_into`` into a new batch of this encoder: measured on the device (one host read
        of the byte total), then written."""
        keep: list = []
        n = self._join_map_args(keys, values, validity, nrows, None, None, stream, keep)[7]
        return self._measured(
            n, None, self.schema_hash,
            lambda rows, offs: self.join_map_into(keys, values, rows, offs, validity, n, stream),
            stream)

    def with_map(self, batch: RowBatch, name, keys: RowBatch, values: RowBatch,
                 validity: Optional[torch.Tensor] = None, stream=None):
        """``batch`` with its MAP field ``name`` rebuilt from the array batches ``keys`` and
        ``values`` (``join_map`` on ``field_encoder(name)``, then ``with_fields``): split, process
        either side, put them back.  Returns ``(encoder, batch)`` of the result."""
        enc = self.field_encoder(name)
        maps = enc.join_map(keys, values, validity, batch.nrows, stream)
        return self.with_fields(batch, enc, maps, stream)

    def device_status(self, stream=None) -> None:
        """Synchronises ``stream`` and raises FuryDeviceError if an earlier asynchronous call's
        kernel could not produce a valid result (``fury_device_status``)."""
        _check(N.lib().fury_device_status(_stream_handle(stream)))

    # -- host-memory batch path: the JNI boundary (off-heap buffers in, off-heap buffers out) --
    def encode_host(self, columns: Sequence[Column], nrows: int, rows=None, row_offsets=None,
                    device_index: int = 0):
        """Host columns (numpy arrays or CPU/pinned tensors, fury_row.h layout) -> host rows,
        through HBM inside the call (``fury_row_encode_host``).  Returns (rows, row_offsets);
        row_offsets is None for fixed-width schemas unless a buffer was passed."""
        keep: list = []
        cc = _c_host_columns(columns, keep)
        fixed = self._schema.is_fixed
        if rows is None:
            bound = nrows * self._schema.fixed_size
            if not fixed:
                bound += 2 * _tree_bytes(columns) + 64 * nrows * (len(self._schema.fields) + 1)
            rows = np.empty(max(bound, 16), dtype=np.uint8)
        if row_offsets is None and not fixed:
            row_offsets = np.empty(nrows + 1, dtype=np.int64)
        nb = ctypes.c_int64(0)
        st = N.lib().fury_row_encode_host(self._schema.handle, cc, nrows, _hptr(rows),
                                          _nbytes(rows), _hptr(row_offsets), ctypes.byref(nb),
                                          device_index)
        if st == 7:                               # FURY_ERR_CAPACITY: retry at the exact size
            rows = np.empty(max(nb.value, 16), dtype=np.uint8)
            st = N.lib().fury_row_encode_host(self._schema.handle, cc, nrows, _hptr(rows),
                                              _nbytes(rows), _hptr(row_offsets),
                                              ctypes.byref(nb), device_index)
        _check(st)
        return rows[:nb.value], row_offsets

    def decode_host(self, rows, row_offsets, nrows: int, out: Optional[List[Column]] = None,
                    device_index: int = 0, pinned: bool = False) -> List[Column]:
        """Host rows -> host columns (``fury_row_decode_host``; nested schemas through the
        two-step host decode).  Without ``out``, numpy columns are allocated (pinned ones with
        ``pinned``, nested schemas): validity for nullable fields, and payload / element buffers
        bounded by the row bytes (a row holds every byte it decodes to)."""
        from .workloads import Column as C
        if self.nested and out is None:
            return self._decode_host_nested(rows, row_offsets, nrows, device_index, pinned)
        if out is None:
            out = []
            rb = max(_nbytes(rows), 16)
            for f in self._schema.fields:
                vb = np.zeros((nrows + 7) // 8 + 8, dtype=np.uint8) if f.nullable else None
                if f.type_id in (STRING, BINARY):
                    out.append(C(values=np.empty(rb, dtype=np.uint8), validity=vb,
                                 offsets=np.empty(nrows + 1, dtype=np.int32)))
                elif f.type_id == LIST:
                    e = f.children[0]
                    ev = np.zeros(rb // 8 + 8, dtype=np.uint8) if e.nullable else None
                    out.append(C(validity=vb, offsets=np.empty(nrows + 1, dtype=np.int32),
                                 child=[C(values=np.empty(rb, dtype=np.uint8), validity=ev)]))
                elif f.type_id == BOOL:
                    out.append(C(values=np.empty((nrows + 7) // 8 + 8, dtype=np.uint8),
                                 validity=vb))
                elif f.type_id == DECIMAL:
                    out.append(C(values=np.empty(nrows * 16, dtype=np.uint8), validity=vb))
                else:
                    out.append(C(values=np.empty(max(nrows * type_width(f.type_id), 8),
                                                 dtype=np.uint8), validity=vb))
        keep: list = []
        _check(N.lib().fury_row_decode_host(self._schema.handle, _hptr(rows), _hptr(row_offsets),
                                            nrows, _c_host_columns(out, keep), device_index))
        return out

    def _decode_host_nested(self, rows, row_offsets, nrows: int, device_index: int = 0,
                            pinned: bool = False):
        """Nested schemas through fury_decode_host_prepare / fury_decode_host_execute: node
        sizes first, then host buffers of exactly those sizes (pinned: written in place by the
        kernels), filled in one call."""
        L = N.lib()
        h = self._schema.handle
        nn = L.fury_schema_num_nodes(h)
        entries = (ctypes.c_int64 * max(nn, 1))()
        nbytes = (ctypes.c_int64 * max(nn, 1))()
        plan = ctypes.c_void_p()
        _check(L.fury_decode_host_prepare(h, _hptr(rows), _hptr(row_offsets), nrows, entries,
                                          nbytes, ctypes.byref(plan), device_index))
        try:
            order = _bfs(self._schema.fields)
            zeros = _pinned_zeros if pinned else np.zeros
            cols = [_alloc_host_node(f, int(entries[i]), int(nbytes[i]), zeros)
                    for i, (f, _) in enumerate(order)]
            for i, (f, first) in enumerate(order):
                if f.children:
                    cols[i].child = [cols[first + j] for j in range(len(f.children))]
            top = cols[:len(self._schema.fields)]
            keep: list = []
            _check(L.fury_decode_host_execute(plan, _c_host_columns(top, keep)))
        finally:
            L.fury_decode_plan_destroy(plan)
        return top

    # -- framing (Encoders.java:165-182, 201-213) ------------------------------------------
    def frame(self, batch: RowBatch, stream=None):
        """Java ``encode(MemoryBuffer, T)`` stream for every row: returns (bytes, frame_offsets)."""
        n = batch.nrows
        total = batch.rows.numel() + 12 * n
        with _on(stream):
            out = self._row_buffer(total)
            fo = torch.empty(n + 1, dtype=torch.int64, device=self.device)
        _check(N.lib().fury_frame_rows(self._schema.handle, _ptr(batch.rows),
                                       _ptr(batch.row_offsets), n, _ptr(out), _ptr(fo),
                                       _stream_handle(stream)))
        return out[:total], fo

    def unframe(self, stream_bytes: torch.Tensor, nrows: int, stream=None) -> RowBatch:
        """Parses a ``decode(MemoryBuffer)`` stream; raises ClassNotCompatibleException on a
        schema-hash mismatch."""
        with _on(stream):
            rows = self._row_buffer(stream_bytes.numel())
            offs = torch.empty(nrows + 1, dtype=torch.int64, device=self.device)
        _check(N.lib().fury_unframe_rows(self._schema.handle, _ptr(stream_bytes),
                                         stream_bytes.numel(), nrows, _ptr(rows), _ptr(offs),
                                         _stream_handle(stream)))
        with _on(stream):
            total = int(offs[nrows].item()) if nrows else 0
        return RowBatch(rows[:total], None if self._schema.is_fixed else offs, nrows,
                        self.schema_hash)

    def encode_stream(self, columns: Sequence[Column], nrows: int, stream=None) -> torch.Tensor:
        """Batch ``encode(MemoryBuffer, T)`` over every row: the byte stream a Java writer loop
        produces (``[int32 len][int64 hash][row]`` per row), in device memory."""
        out, _ = self.frame(self.encode_batch(columns, nrows, stream=stream), stream=stream)
        return out

    def decode_stream(self, stream_bytes: torch.Tensor, nrows: int, validity: bool = True,
                      stream=None) -> List[Column]:
        """Batch ``decode(MemoryBuffer)`` of nrows frames: parallel stream parse, then the
        columns (ClassNotCompatibleException on a schema-hash mismatch, like the reference)."""
        return self.decode_batch(self.unframe(stream_bytes, nrows, stream=stream),
                                 validity=validity, stream=stream)

    # -- single-object API (a bean is a dict name -> value) --------------------------------
    def to_row(self, bean: dict) -> bytes:
        """``toRow(obj).toBytes()``: canonical row bytes of one bean."""
        from .beans import beans_to_columns
        cols = [column_to_device(c, self.device)
                for c in beans_to_columns(self._schema.fields, [bean])]
        b = self.encode_batch(cols, 1)
        return b.row_bytes(0, self._schema.fixed_size)

    def from_row(self, row: bytes) -> dict:
        from .beans import columns_to_beans
        t = torch.frombuffer(bytearray(row), dtype=torch.uint8).to(self.device)
        offs = None if self._schema.is_fixed else torch.tensor([0, len(row)], dtype=torch.int64,
                                                              device=self.device)
        cols = self.decode_batch(RowBatch(t, offs, 1, self.schema_hash))
        return columns_to_beans(self._schema.fields, [column_to_host(c) for c in cols], 1)[0]

    def encode(self, bean: dict) -> bytes:
        """``encode(T)``: [int64 schemaHash][row] (Encoders.java:191-198)."""
        return struct.pack("<q", self.schema_hash) + self.to_row(bean)

    def decode(self, data: bytes) -> dict:
        """``decode(byte[])``: checks the 8-byte schema hash first (Encoders.java:169-188)."""
        if len(data) < 8:
            raise IndexOutOfBoundsException("buffer shorter than the schema hash")
        peer = struct.unpack_from("<q", data, 0)[0]
        if peer != self.schema_hash:
            raise ClassNotCompatibleException(
                f"Schema is not consistent, encoder schema is {self._schema}. self/peer schema "
                f"hash are {self.schema_hash}/{peer}. Please check writer schema.")
        return self.from_row(data[8:])


def _bfs(fields: Sequence[Field]):
    """Schema nodes in the C ABI's breadth-first order: [(field, first_child_index)]."""
    q = list(fields)
    out = []
    i = 0
    while i < len(q):
        f = q[i]
        out.append((f, len(q)))
        q.extend(f.children)
        i += 1
    return out


def _node_sizes(order, cols: List[Column], n: int, stream=None):
    """Arrow entries and STRING / BINARY payload bytes of every schema node (breadth-first
    ``order``) of decoded columns ``cols`` with n top-level entries (device offsets read back)."""
    nodes: List[Optional[Column]] = [None] * len(order)
    m = [0] * len(order)
    b = [0] * len(order)
    ntop = len(cols)
    for k in range(ntop):
        nodes[k] = cols[k]
        m[k] = n
    with _on(stream):
        for i, (f, first) in enumerate(order):
            c = nodes[i]
            t = f.type_id
            end = int(c.offsets[m[i]].item()) if (t in (STRING, BINARY, LIST, MAP) and m[i]) else 0
            if t in (STRING, BINARY):
                b[i] = end
            for j in range(len(f.children)):
                nodes[first + j] = c.child[j]
                m[first + j] = m[i] if t == STRUCT else end
    return m, b


def _pinned_zeros(n: int, dtype=np.uint8) -> np.ndarray:
    a = host_empty(max(int(n), 1) * np.dtype(dtype).itemsize, dtype)
    a[:] = 0
    return a[:n]


def _alloc_host_node(f: Field, m: int, nbytes: int, zeros=np.zeros) -> Column:
    """Host buffers for one schema node with m Arrow entries (fury_decode_host_execute contract:
    exact sizes); ``zeros=_pinned_zeros`` gives pinned ones (the execute writes them in place)."""
    vb = zeros((m + 7) // 8 + 8, np.uint8)
    t = f.type_id
    if t == BOOL:
        return Column(values=zeros((m + 7) // 8 + 8, np.uint8), validity=vb)
    if type_width(t) > 0:
        return Column(values=zeros(m * type_width(t) + 8, np.uint8), validity=vb)
    if t in (STRING, BINARY):
        return Column(values=zeros(max(nbytes, 1), np.uint8), validity=vb,
                      offsets=zeros(m + 1, np.int32))
    if t == DECIMAL:
        return Column(values=zeros(16 * m + 16, np.uint8), validity=vb)
    if t in (LIST, MAP):
        return Column(validity=vb, offsets=zeros(m + 1, np.int32))
    if t == STRUCT:
        return Column(validity=vb)
    raise UnsupportedOperationException(f"no device decode for {f}")


def _alloc_nodes(order, entries, nbytes, validity: bool, device) -> List[Column]:
    """The output buffers of every schema node (breadth-first ``order``) carved from ONE device
    allocation: bitmaps (validity, BOOL values; zeroed -- the decode only sets bits of shared
    words) first, so a single memset clears them, then the int32 Arrow offsets, then values /
    payloads, each 256-B aligned.  One allocation and one memset instead of a few per node (~17
    nodes: the per-tensor cost was a third of a 400k-row decode's wall time), and the views of
    each region cut by ONE split_with_sizes call (round 6: per-view slicing in Python cost ~1 ms
    for a 128-field bean)."""
    def al(x):
        return (x + 255) & ~255
    regions = {"z": [], "o": [], "e": []}       # per region: (node, name, nbytes)
    for i, (f, _first) in enumerate(order):
        m, nb, t = int(entries[i]), int(nbytes[i]), f.type_id
        if validity:
            regions["z"].append((i, "validity", (m + 7) // 8 + 4))
        if t == BOOL:
            regions["z"].append((i, "values", (m + 7) // 8 + 4))
        elif type_width(t) > 0:
            regions["e"].append((i, "values", m * type_width(t) + 8))
        elif t in (STRING, BINARY):
            regions["e"].append((i, "values", max(nb, 1)))
            regions["o"].append((i, "offsets", 4 * (m + 1)))
        elif t == DECIMAL:
            regions["e"].append((i, "values", 16 * m + 16))
        elif t in (LIST, MAP):
            regions["o"].append((i, "offsets", 4 * (m + 1)))
        elif t != STRUCT:
            raise UnsupportedOperationException(f"no device decode for {f}")
    size = {k: sum(al(n) for _, _, n in v) for k, v in regions.items()}
    arena = torch.empty(max(size["z"] + size["o"] + size["e"], 256), dtype=torch.uint8, device=device)
    if size["z"]:
        arena[:size["z"]].zero_()
    views = [dict() for _ in order]
    base = 0
    for k in ("z", "o", "e"):
        segs = regions[k]
        if segs:
            region = arena[base:base + size[k]]
            unit = 4 if k == "o" else 1
            if unit == 4:
                region = region.view(torch.int32)
            sizes = []
            for _, _, n in segs:                 # each view, then its padding to 256 B
                sizes += [n // unit, (al(n) - n) // unit]
            parts = region.split_with_sizes(sizes)
            for j, (i, name, _) in enumerate(segs):
                views[i][name] = parts[2 * j]
        base += size[k]
    return [Column(values=v.get("values"), validity=v.get("validity"), offsets=v.get("offsets"))
            for v in views]


class _CollectionEncoder(RowEncoder):
    """Batch codec of top-level collections over the device engine: batch entry i is one
    BinaryArray (ArrayEncoder) / BinaryMap (MapEncoder).  The batch methods of RowEncoder apply
    unchanged with ONE column, the collection column (no validity: toArray / toMap of a null
    collection is not defined)."""

    def __init__(self, field: Field, device=None):
        self._schema = Schema([field], collection=True)
        self.device = torch.device(device if device is not None else "cuda")
        self._field = field

    def _column(self, values: list) -> Column:
        from .beans import values_to_column
        c = values_to_column(self._field, list(values))
        c.validity = None
        return column_to_device(c, self.device)

    def _values(self, data: bytes) -> list:
        from .beans import value_at
        t = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(self.device)
        offs = torch.tensor([0, len(data)], dtype=torch.int64, device=self.device)
        cols = self.decode_batch(RowBatch(t, offs, 1, 0))
        return value_at(self._field, column_to_host(cols[0]), 0)

    def _bytes(self, values: list) -> bytes:
        b = self.encode_batch([self._column([values])], 1)
        return bytes(b.rows.cpu().numpy())

    # -- the elements of every entry as a batch: RowEncoder's methods with the empty path ------------
    def element_encoder(self, side: str = "elements"):
        """The encoder of this collection's elements ("elements" of a list, "keys" / "values" of a
        map): see ``RowEncoder.element_encoder``."""
        return RowEncoder.element_encoder(self, (), side)

    def explode_into(self, batch: RowBatch, out_list_offsets: torch.Tensor, *outs, **kw) -> None:
        """``RowEncoder.explode_into`` without the path: every batch entry is the array / map."""
        RowEncoder.explode_into(self, batch, (), out_list_offsets, *outs, **kw)

    def bind_explode(self, batch: RowBatch, out_list_offsets: torch.Tensor, *outs, **kw):
        return RowEncoder.bind_explode(self, batch, (), out_list_offsets, *outs, **kw)

    def explode(self, batch: RowBatch, side: str = "elements", stream=None):
        """``RowEncoder.explode`` without the path: the elements of every entry of ``batch``."""
        return RowEncoder.explode(self, batch, (), side, stream)

    def encode_stream(self, values: list) -> bytes:
        """``encode(MemoryBuffer, T)``: [int32 size][bytes] (Encoders.java:372-386 / 575-590)."""
        body = self._bytes(values)
        return struct.pack("<i", len(body)) + body

    def decode_stream(self, data: bytes, offset: int = 0):
        """``decode(MemoryBuffer)`` at ``offset``: returns (value, next offset)."""
        size = struct.unpack_from("<i", data, offset)[0]
        return self._values(data[offset + 4:offset + 4 + size]), offset + 4 + size


class ArrayEncoder(_CollectionEncoder):
    """``Encoders.arrayEncoder`` (Encoders.java:230-386): List -> BinaryArray.  ``field`` is the
    LIST field TypeInference infers for the collection type (its element: a bean STRUCT, a LIST,
    a MAP, or a scalar)."""

    def field(self) -> Field:
        return self._field

    def to_array(self, values: list) -> bytes:
        """``toArray(obj)`` bytes: [int64 n][null bitmap][n slots][variable section]."""
        return self._bytes(values)

    def from_array(self, data: bytes) -> list:
        return self._values(data)

    def encode(self, values: list) -> bytes:
        """``encode(T)`` of a fresh encoder: ``writer.getBuffer().getBytes(0, 8 + size)``
        (Encoders.java:365-369) = the array followed by 8 bytes of the zeroed buffer -- the length
        ArrayEncoderTest pins (224 / 1576 / 10824).  The reference never rewinds its writer, so a
        second encode() on the same Java encoder returns the FIRST array's bytes (SURVEY §7 trap 5);
        that bug is not reproduced: every call here returns this fresh-encoder result."""
        return self._bytes(values) + bytes(8)

    def decode(self, data: bytes) -> list:
        """``decode(byte[])``: the array at offset 0 (trailing bytes ignored, as pointTo does)."""
        return self._values(data)


class MapEncoder(_CollectionEncoder):
    """``Encoders.mapEncoder`` (Encoders.java:420-600, MapEncoderBuilder.java:152-208): Map ->
    BinaryMap [int64 keyArrayBytes][key BinaryArray][value BinaryArray].  A map value is a list
    of (key, value) pairs in iteration order."""

    def key_field(self) -> Field:
        return self._field.children[0]

    def value_field(self) -> Field:
        return self._field.children[1]

    # -- every entry as its key array and its value array, and back: RowEncoder's methods with the
    #    empty path / in collection form --------------------------------------------------------------
    def key_array_encoder(self) -> "ArrayEncoder":
        """The ``ArrayEncoder`` of this map's key arrays: see ``RowEncoder.key_array_encoder``."""
        return RowEncoder.key_array_encoder(self, ())

    def value_array_encoder(self) -> "ArrayEncoder":
        return RowEncoder.value_array_encoder(self, ())

    def split_into(self, batch: RowBatch, *outs, **kw) -> None:
        """``RowEncoder.split_map_into`` without the path: every batch entry is the map."""
        RowEncoder.split_map_into(self, batch, (), *outs, **kw)

    def bind_split(self, batch: RowBatch, *outs, **kw):
        return RowEncoder.bind_split_map(self, batch, (), *outs, **kw)

    def split(self, batch: RowBatch, stream=None):
        """``RowEncoder.split_map`` without the path: the key and value arrays of every entry."""
        return RowEncoder.split_map(self, batch, (), stream)

    def join_into(self, keys: RowBatch, values: RowBatch, out_rows: Optional[torch.Tensor],
                  out_offsets: torch.Tensor, stream=None) -> None:
        """``RowEncoder.join_map_into`` in collection form: output entry r is the map of entry r of
        ``keys`` and ``values`` (a map entry is never null: no validity)."""
        RowEncoder.join_map_into(self, keys, values, out_rows, out_offsets, stream=stream)

    def bind_join(self, keys: RowBatch, values: RowBatch, out_rows: Optional[torch.Tensor],
                  out_offsets: torch.Tensor, stream=None):
        return RowEncoder.bind_join_map(self, keys, values, out_rows, out_offsets, stream=stream)

    def join(self, keys: RowBatch, values: RowBatch, stream=None) -> RowBatch:
        """``RowEncoder.join_map`` in collection form, into a new batch of this encoder."""
        return RowEncoder.join_map(self, keys, values, stream=stream)

    def to_map(self, pairs: list) -> bytes:
        return self._bytes(pairs)

    def from_map(self, data: bytes) -> list:
        return self._values(data)

    def encode(self, pairs: list) -> bytes:
        """``encode(T)``: ``map.getBuf().getBytes(baseOffset, sizeInBytes)`` = the BinaryMap."""
        return self._bytes(pairs)

    def decode(self, data: bytes) -> list:
        return self._values(data)


class Encoders:
    """``Encoders`` factory (Encoders.java:60-73, 230-420)."""

    @staticmethod
    def bean(fields: Sequence[Field], device=None) -> RowEncoder:
        return RowEncoder(fields, device)

    @staticmethod
    def array_encoder(elem: Field, device=None, name: str = "value") -> ArrayEncoder:
        """``arrayEncoder(List<elem>)``: the LIST field of element field ``elem``."""
        return ArrayEncoder(Field(name, LIST, True, (elem,)), device)

    @staticmethod
    def map_encoder(key: Field, value: Field, device=None, name: str = "value") -> MapEncoder:
        """``mapEncoder(Map<key, value>)``: the MAP field of the key / value fields."""
        return MapEncoder(Field(name, MAP, True, (key, value)), device)


class ArrowWriter:
    """``ArrowWriter`` (ArrowWriter.java:55-99) over RowBatches: ``write(batch)`` converts a whole
    batch on the device and APPENDS it after everything written since ``reset()`` -- the
    reference's write(row) appends at the vectors' rowCount -- so two writes then
    ``finish_as_record_batch()`` give the concatenation.  ``finish()`` returns the accumulated
    device Arrow columns; ``finish_as_record_batch()`` a pyarrow.RecordBatch on the host.

    The accumulated buffers grow like Arrow's setSafe (capacity doubling, amortised O(1) per
    row): a batch that does not fit moves the accumulation into buffers of twice the size first.
    Appends run on the device (``fury_arrow_append``: copies, offset rebasing, bit shifting)."""

    def __init__(self, encoder: RowEncoder):
        self._enc = encoder
        self.reset()

    def write(self, batch: RowBatch, stream=None) -> None:
        """Synchronous like the reference's write(row): a row whose values lie outside the batch
        raises IndexOutOfBoundsException here (nothing of the batch is appended then)."""
        cols = self._enc._decode(batch, True, True, stream)
        self._enc.device_status(stream)
        n = batch.nrows
        order = _bfs(self._enc.schema().fields)
        m, b = _node_sizes(order, cols, n, stream)
        if self._acc is None or self._n == 0:
            self._acc, self._m, self._b = cols, m, b
            self._cap_m, self._cap_b = list(m), list(b)
        else:
            need_m = [x + y for x, y in zip(self._m, m)]
            need_b = [x + y for x, y in zip(self._b, b)]
            if any(x > c for x, c in zip(need_m, self._cap_m)) or \
                    any(x > c for x, c in zip(need_b, self._cap_b)):
                self._grow(order, need_m, need_b, stream)
            keep: list = []
            _check(N.lib().fury_arrow_append(self._enc.schema().handle,
                                             _c_columns(self._acc[:len(cols)], keep), self._n,
                                             _c_columns(cols, keep), n, _stream_handle(stream)))
            self._m, self._b = need_m, need_b
        self._n += n

    def _grow(self, order, need_m, need_b, stream) -> None:
        cap_m = [max(2 * c, x) for c, x in zip(self._cap_m, need_m)]
        cap_b = [max(2 * c, x) for c, x in zip(self._cap_b, need_b)]
        with _on(stream):
            nodes = _alloc_nodes(order, cap_m, cap_b, True, self._enc.device)
        for i, (f, first) in enumerate(order):
            if f.children:
                nodes[i].child = [nodes[first + j] for j in range(len(f.children))]
        top = nodes[:len(self._enc.schema().fields)]
        keep: list = []
        _check(N.lib().fury_arrow_append(self._enc.schema().handle, _c_columns(top, keep), 0,
                                         _c_columns(self._acc, keep), self._n,
                                         _stream_handle(stream)))
        self._acc, self._cap_m, self._cap_b = top, cap_m, cap_b

    def finish(self) -> List[Column]:
        """The device Arrow columns of every row written since reset() (views trimmed to the
        written entries)."""
        if self._acc is None:
            return []
        order = _bfs(self._enc.schema().fields)
        flat: List[Column] = []

        def walk(c: Column, i: int):
            f, first = order[i]
            m, nb = self._m[i], self._b[i]
            t = f.type_id
            out = Column(validity=None if c.validity is None else c.validity[:((m + 31) // 32) * 4])
            if t == BOOL:
                out.values = c.values[:((m + 31) // 32) * 4]
            elif type_width(t) > 0:
                out.values = c.values[:m * type_width(t)]
            elif t == DECIMAL:
                out.values = c.values[:16 * m]
            elif t in (STRING, BINARY):
                out.values = c.values[:max(nb, 1)]
                out.offsets = c.offsets[:m + 1]
            elif t in (LIST, MAP):
                out.offsets = c.offsets[:m + 1]
            if f.children:
                out.child = [walk(c.child[j], first + j) for j in range(len(f.children))]
            return out

        return [walk(c, i) for i, c in enumerate(self._acc)]

    def finish_as_record_batch(self):
        from .arrow import columns_to_record_batch
        return columns_to_record_batch(self._enc.schema().fields,
                                       [column_to_host(c) for c in self.finish()], self._n)

    # -- Arrow IPC (ArrowUtils.serializeRecordBatch / ArrowSerializers, ArrowUtils.java:63-72,
    #    ArrowSerializers.java:128-167) ---------------------------------------------------------
    def ipc_schema(self) -> bytes:
        """Encapsulated IPC Schema message (host bytes)."""
        return ipc_schema_message(self._enc)

    def finish_as_ipc_message(self, stream=None) -> torch.Tensor:
        """The written batch as ONE encapsulated IPC RecordBatch message in device memory
        (``serializeRecordBatch`` of ``finishAsRecordBatch()``)."""
        return ipc_record_batch_message(self._enc, self.finish(), self._n, stream)

    def finish_as_ipc_stream(self, stream=None) -> bytes:
        """Schema message + the batch + end-of-stream marker, on the host: the bytes
        ``ArrowStreamWriter`` writes for the batch (ArrowSerializers.java:128-134)."""
        body = self.finish_as_ipc_message(stream).cpu().numpy().tobytes()
        return self.ipc_schema() + body + IPC_EOS

    def reset(self) -> None:
        """ArrowWriter.reset(): the next write starts a new batch (ArrowWriter.java:95-99)."""
        self._acc: Optional[List[Column]] = None
        self._n = 0
        self._m: List[int] = []
        self._b: List[int] = []
        self._cap_m: List[int] = []
        self._cap_b: List[int] = []


IPC_EOS = b"\xff\xff\xff\xff\x00\x00\x00\x00"


def ipc_schema_message(enc: "RowEncoder") -> bytes:
    n = ctypes.c_int64(0)
    _check(N.lib().fury_arrow_ipc_schema(enc._schema.handle, None, 0, ctypes.byref(n)))
    buf = ctypes.create_string_buffer(n.value)
    _check(N.lib().fury_arrow_ipc_schema(enc._schema.handle, buf, n.value, ctypes.byref(n)))
    return buf.raw[:n.value]


def ipc_record_batch_message(enc: "RowEncoder", cols: List[Column], nrows: int,
                             stream=None) -> torch.Tensor:
    """Encapsulated IPC RecordBatch message of device columns, gathered on the device."""
    keep: list = []
    cc = _c_columns(cols, keep)
    n = ctypes.c_int64(0)
    sh = _stream_handle(stream)
    _check(N.lib().fury_arrow_ipc_record_batch(enc._schema.handle, cc, nrows, None, 0,
                                               ctypes.byref(n), sh))
    out = torch.empty(max(n.value, 16), dtype=torch.uint8, device=enc.device)
    _check(N.lib().fury_arrow_ipc_record_batch(enc._schema.handle, cc, nrows, _ptr(out), n.value,
                                               ctypes.byref(n), sh))
    return out[:n.value]
