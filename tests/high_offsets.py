"""Row batches placed across byte 2^31 and byte 2^32 of their buffer: the placements, the inputs and
one adapter per entry point that takes a row batch.

Plain data and helpers: no torch and no pytest at import (the adapters import torch when they run).
Every bounds rule of include/fury_row.h reads "inside [0, row_offsets[nrows])", and a batch's
position inside its buffer is free, so a 100 KB batch can sit across byte 2^32 of an otherwise
untouched allocation: tests/test_high_offsets_gpu.py runs every adapter of CONSUMERS on the same
bytes at base 0 (the control) and at the eight PLACEMENTS x BOUNDARIES and compares every output.
tests/test_high_offsets.py checks the placements from the oracle's offsets and that every public
method taking a RowBatch resolves to an adapter here or to a reason in EXEMPT."""
from __future__ import annotations

import re
import zlib

import numpy as np

INT32_MAX = (1 << 31) - 1
X31, X32 = 1 << 31, 1 << 32
BOUNDARIES = {"2g": X31, "4g": X32}
PLACEMENTS = ("ends_at", "starts_at", "row_starts_at", "inside_row")
STRADDLING = ("row_starts_at", "inside_row")
CASES = [f"{p}-{x}" for x in BOUNDARIES for p in PLACEMENTS]      # the 8 placements of the matrix

# ---- the arena ------------------------------------------------------------------------------------
# One allocation of SLACK + VIEW bytes of 0xAB.  `rows` is the view SLACK bytes in: a sign-extended
# 32-bit truncation of an offset in [2^31, 2^32) lands in the slack, an unsigned truncation of an
# offset >= 2^32 low in the view -- a wrong cast reads or writes 0xAB inside the allocation.
FILL = 0xAB
SLACK = X31
TAIL = 64 << 20
VIEW_BYTES = X32 + TAIL
ARENA_BYTES = SLACK + VIEW_BYTES

N = 1300                      # rows of every sparse batch: three or more tiles of every kernel


def base(placement: str, X: int, offs) -> int:
    """The base B of `placement` at boundary X for the 0-based offsets offs[0..n]; m = n // 2."""
    n = len(offs) - 1
    m = n // 2
    if placement == "ends_at":          # total == X exactly
        return X - int(offs[n])
    if placement == "starts_at":        # every row at or above X
        return X
    if placement == "row_starts_at":    # row m starts exactly at X
        return X - int(offs[m])
    if placement == "inside_row":       # X falls inside row m, 8-aligned
        return X - (((int(offs[m]) + int(offs[m + 1])) // 2) & ~7)
    raise KeyError(placement)


def case_base(case: str, offs) -> int:
    p, x = case.rsplit("-", 1)
    return base(p, BOUNDARIES[x], offs)


def other_cases(case: str):
    """The placements a multi-input adapter tries for its further inputs, in order: the other
    boundary first, then this one; the arena takes the first that overlaps nothing placed."""
    k = CASES.index(case)
    rot = CASES[k + 1:] + CASES[:k]
    x = case.rsplit("-", 1)[1]
    return [c for c in rot if not c.endswith(x)] + [c for c in rot if c.endswith(x)]


# ---- schemas and inputs ---------------------------------------------------------------------------
# name -> (seed, generator knobs or None for the bean generator of tests/test_tree.py).  The seeds
# are chosen so that MISALIGNED16 holds (tests/test_high_offsets.py checks it).
SCHEMAS = {
    "mixed": (1, dict(null_pct=10, str_max=32)),                 # register-staged, <= 16 fields
    "wide33": (33, dict(null_pct=10, str_max=40, list_max=8, list_null_pct=10, elem_null_pct=10)),
    "nested": (7, dict(null_pct=0, list_max=16, list_null_pct=5)),      # LIST of int64
    "nested7": (11, None),
    "maps": (13, None),
}
# schemas whose inside_row base is 8 (mod 16): the 16-byte load paths meet a misaligned source
MISALIGNED16 = ("mixed", "wide33", "nested", "nested7")

# (knob, value) legs: the decode engines of a schema, and the encode's
DECODE_KNOBS = {
    "mixed": [None], "nested": [None],
    "wide33": [("wide_engine", 1), ("wide_engine", 2)],
    "nested7": [("nested_decode", k) for k in (1, 2, 3, 4)],
    "maps": [("nested_decode", k) for k in (1, 2, 3, 4)],
}
ENCODE_KNOBS = {
    "mixed": [None], "nested": [None],
    "wide33": [("wide_enc_engine", 1), ("wide_enc_engine", 2)],
    "nested7": [None, ("rowenc_img", 1024)],       # the row encode's tiles / its HBM-direct path
    "maps": [None, ("rowenc_img", 1024)],
}

# per schema: what each adapter selects.  A missing key: the operator does not apply (maps has no
# top-level field a projected decode, an update or a key hash takes).
SPEC = {
    "mixed": dict(project=["s2", "a", "s3"], update=["c", "a"], hash=["b", "s1"],
                  select=["s3", "a", "s1"], zip=[(0, "a"), (1, "s2"), (0, "s1"), (1, "b")]),
    "wide33": dict(project=["f003", "f005", "f004", "f001"], update=["f001", "f005", "f000"],
                   hash=["f001", "f003"], select=["f010", "f004", "f000", "f006", "f012"],
                   zip=[(0, "f003"), (1, "f004"), (1, "f000"), (0, "f011")]),
    "nested": dict(project=["vals", "id"], update=["score"], hash=["id"], select=["vals", "id"],
                   zip=[(1, "vals"), (0, "id"), (1, "score")]),
    "nested7": dict(project=["z", "id"], update=["id", "z"], hash=["id"],
                    select=["pts", "id", "m", "tags"],
                    zip=[(0, "inner"), (1, "ll"), (1, "id"), (0, "m")],
                    extract=["inner", "m", "tags"], explode=[("pts", "elements"), ("ll", "elements")],
                    split_map=["m"], implode=["pts", "ll"], wrap=["inner", "m"], join_map=["m"]),
    "maps": dict(select=["m2", "lm"], zip=[(1, "m1"), (0, "m2"), (1, "lm")],
                 extract=["m1", "lm"], explode=[("m1", "values"), ("lm", "elements")],
                 explode_map_sides=["lm"], split_map=["m1", "m2"], implode=["lm"],
                 wrap=["m1", "lm"], join_map=["m1", "m2"]),
}


def fields_of(schema: str):
    from fury_amd.workloads import SCHEMAS as W
    if schema in ("mixed", "nested"):
        return W[schema]
    if schema == "wide33":
        from tests.test_device import _wide_fields
        return _wide_fields(33)
    from tests.test_tree import _schemas
    return _schemas()[schema]


def host_columns(schema: str, alt: bool = False):
    """The host columns of a schema's N-row batch (`alt`: other values of the same schema, what
    update_fields writes)."""
    from fury_amd.workloads import gen_columns
    seed, knobs = SCHEMAS[schema]
    seed += 1000 if alt else 0
    fields = fields_of(schema)
    if knobs is None:
        from fury_amd.beans import beans_to_columns
        from tests.test_tree import _beans
        return beans_to_columns(fields, _beans(fields, N, seed))
    return gen_columns("wide" if schema == "wide33" else schema, fields, N, seed=seed, **knobs)


class Ref:
    """A schema's batch as the oracle encodes and decodes it: computed once, shared, never
    modified."""

    def __init__(self, oracle, schema):
        self.schema, self.n = schema, N
        self.fields = list(fields_of(schema))
        self.host = host_columns(schema)
        rows, offs = oracle.encode(self.fields, self.host, N)
        self.rows, self.offs = rows, np.asarray(offs, np.int64)
        self.cols = oracle.decode(self.fields, self.rows, self.offs, N)
        self.rows.setflags(write=False)
        self.offs.setflags(write=False)


_REF: dict = {}


def ref(oracle, schema) -> Ref:
    if schema not in _REF:
        _REF[schema] = Ref(oracle, schema)
    return _REF[schema]


def rng_of(*key) -> np.random.Generator:
    """The same random operands for the control and every placement of one (consumer, schema)."""
    return np.random.default_rng(zlib.crc32(":".join(map(str, key)).encode()))


# ---- dense shapes: the produced bytes themselves pass 2^32 ----------------------------------------
GIB = 1 << 30
LIVE_LIMIT = 32 * GIB
D1_ROWS, D1_ROW_BYTES, D1_FIELDS = 5_300_000, 816, 100      # Struct-100, 4.32 GB
# the long-row schema id INT64, a / b / c BINARY: bitmap 8 + 4 slots of 8, payloads padded to 8
LONG_HEAD = 8 + 8 * 4
LONG_ROWS = 1440
LONG_VALUE = (1 << 20) + (1 << 16)                 # about 1 MiB per value
LONG_NULL_EVERY = 11                               # a null value where (row + field) % 11 == 3
LONG_DISTINCT = 8                                  # source rows of the take / select / zip legs
LONG_TAKE = 1500                                   # output rows of those legs
LIST_LEN = 4                                       # values per map of the join_map leg
LIST_LENGTHS = (3, 4, 5, 4)                        # elements per list of the implode leg, cycling
IMPLODE_ELEMENTS = 4224                            # elements of about 1 MiB, cycling through 8
JOIN_MAPS = 1056


def long_fields():
    from fury_amd import types as T
    return [T.not_null_field("id", T.INT64), T.field("a", T.BINARY), T.field("b", T.BINARY),
            T.field("c", T.BINARY)]


def long_lengths(rows: int = LONG_ROWS) -> np.ndarray:
    """Value bytes [rows, 3] of the long-row schema: about 1 MiB, jittered by multiples of 1 (field
    a), of 8 (field b) and of 9 (c); -1 marks a null."""
    r = np.arange(rows, dtype=np.int64)[:, None]
    f = np.arange(3, dtype=np.int64)[None, :]
    h = (r * 2654435761 + f * 40503 + 12345) % 4093
    out = LONG_VALUE + h * np.array([1, 8, 9], np.int64)[None, :]
    out[(r + f) % LONG_NULL_EVERY == 3] = -1
    return out


def long_row_bytes(lengths: np.ndarray) -> np.ndarray:
    """The row-layout formula: bitmap + slots + every non-null payload rounded up to 8 bytes."""
    v = np.where(lengths < 0, 0, (lengths + 7) & ~7)
    return LONG_HEAD + v.sum(axis=1)


def take_indices(rows: int = LONG_TAKE) -> np.ndarray:
    """Output row j of the take / select / zip legs is source row (5 j + 3) mod 8."""
    return (np.arange(rows, dtype=np.int64) * 5 + 3) % LONG_DISTINCT


def dense_shapes() -> dict:
    """leg -> dict(batch=bytes of the row batch (or stream) produced, columns=[payload bytes of
    every Arrow column a decode in the leg produces], rows=[the largest row or array], live=the
    device bytes the leg holds at once).  From the layout formula alone: no data."""
    ln = long_lengths()
    rb = long_row_bytes(ln)
    total = int(rb.sum())
    payload = [int(np.where(ln[:, k] < 0, 0, ln[:, k]).sum()) for k in range(3)]
    cols = sum(payload) + 8 * LONG_ROWS
    d1 = D1_ROWS * D1_ROW_BYTES
    d1_cols = 8 * D1_ROWS * D1_FIELDS
    taken = int(rb[take_indices()].sum())
    elem_lo, elem_hi = 16 + LONG_VALUE, 16 + LONG_VALUE + 9 * 4093 + 8     # a struct of one BINARY
    imploded_lo = IMPLODE_ELEMENTS * elem_lo
    imploded_hi = IMPLODE_ELEMENTS * (elem_hi + 8) + 64 * IMPLODE_ELEMENTS
    held = ARENA_BYTES                             # the sparse matrix's arena lives as long as the module
    return {
        "D1": dict(batch=d1, columns=[8 * D1_ROWS] * D1_FIELDS, rows=[D1_ROW_BYTES],
                   live=held + SLACK + d1 + 3 * d1_cols),
        "D2": dict(batch=total, columns=payload + [8 * LONG_ROWS], rows=[int(rb.max())],
                   live=held + SLACK + total + 2 * cols),
        "D3": dict(batch=taken, columns=[], rows=[int(rb.max())],
                   live=held + 2 * (SLACK + taken * 9 // 8) + taken * 9 // 8),
        "D4": dict(batch=taken - 8 * LONG_TAKE, columns=[], rows=[int(rb.max())],
                   live=held + 2 * (SLACK + taken + 64 * LONG_TAKE) + taken),
        "D5": dict(batch=imploded_lo, columns=[], rows=[max(LIST_LENGTHS) * (elem_hi + 8) + 64],
                   live=held + 2 * (SLACK + imploded_hi) + imploded_hi),
        "D6": dict(batch=total + 12 * LONG_ROWS, columns=[], rows=[int(rb.max())],
                   live=held + 3 * (SLACK + total + 12 * LONG_ROWS) + cols),
    }


# ---- results --------------------------------------------------------------------------------------
def row_of(message: str):
    """The row number an error message names ("row 650 ..."), else None."""
    m = re.search(r"\brow (\d+)\b", message)
    return int(m.group(1)) if m else None


def _batch_items(name, b):
    """A produced batch: its rows, its offsets and its count."""
    return [(f"{name}.rows", b.rows), (f"{name}.row_offsets", b.row_offsets),
            (f"{name}.nrows", b.nrows), (f"{name}.schema_hash", b.schema_hash)]


# ---- the adapters ---------------------------------------------------------------------------------
# Each takes the context `c` of tests/test_high_offsets_gpu.py:
#   c.enc, c.ref, c.schema, c.spec   the encoder, the oracle's Ref, the schema's name and SPEC entry
#   c.primary()                      the schema's batch at this case's placement (the control: base 0
#                                    in a tight buffer)
#   c.put(batch, slot)               a 0-based batch (made at the control) placed likewise; slot > 0:
#                                    another placement of the same arena
#   c.out(offsets, slot)             (rows, base): where an output with these 0-based offsets goes
#   c.written(rows, base, total)     a copy of the bytes written there
#   c.written_batch(batch)           a copy of a placed batch's own bytes
#   c.control()                      the schema's batch at base 0, shared and never written
#   c.slice(batch, a, b)             rows [a, b) of a placed batch: the same rows, interior offsets
#   c.clear()                        forget what is placed (its bytes go back to 0xAB)
#   c.cols() / c.alt_cols(names)     the batch's device columns / other values of some of its fields
# and returns a list of (name, value): tensors, ints, or ("columns", fields, columns, n).  Outputs
# are complete: every buffer the call fills.  The caller adds the device_status outcome.
def _decode(c):
    return [("columns", ("columns", c.ref.fields, c.enc.decode_batch(c.primary()), c.ref.n))]


def _arrow(c):
    from fury_amd.encoder import ArrowWriter
    w = ArrowWriter(c.enc)
    w.write(c.primary())
    return [("columns", ("columns", c.ref.fields, w.finish(), c.ref.n))]


def _project(c):
    names = c.spec["project"]
    fields = [c.ref.fields[k] for k in c.enc._select(names)]
    out = []
    for arrow in (False, True):
        cols = c.enc.project_batch(c.primary(), names, arrow=arrow)
        out.append((f"arrow={arrow}", ("columns", fields, cols, c.ref.n)))
    return out


def _update(c):
    import torch
    names = c.spec["update"]
    b = c.primary()
    mask = torch.from_numpy(rng_of("update", c.schema).random(c.ref.n) < 0.7).to(c.dev)
    c.enc.update_fields(b, names, c.alt_cols(names), row_mask=mask)
    c.enc.device_status()
    return [("rows", c.written_batch(b))]


def _hash(c):
    import torch
    h, ids = c.enc.hash_rows(c.primary(), c.spec["hash"], seed=0x9E3779B9, num_parts=7)
    return [("hashes", h.view(torch.int32)), ("part_ids", ids)]


def _take(c):
    idx = rng_of("take", c.schema).integers(0, c.ref.n, c.ref.n + 37)
    return _batch_items("out", c.enc.take(c.primary(), idx))


def _filter(c):
    import torch
    mask = torch.from_numpy(rng_of("filter", c.schema).random(c.ref.n) < 0.6).to(c.dev)
    out, kept = c.enc.filter(c.primary(), mask, return_indices=True)
    return _batch_items("out", out) + [("indices", kept)]


def _partition(c):
    ids = rng_of("partition", c.schema).integers(-1, 5, c.ref.n)      # -1 and 4: dropped
    out, part_rows, kept = c.enc.partition(c.primary(), ids, 4, return_indices=True)
    return _batch_items("out", out) + [("part_rows", part_rows), ("indices", kept)]


def _concat(c):
    """Three interior slices of the batch, each from a copy at its own placement; the slice of the
    case's own placement holds row m."""
    n = c.ref.n
    p0 = c.primary()
    ctrl = c.control()
    srcs = [c.slice(c.put(ctrl, 1), n - n // 3, n), c.slice(p0, n // 3, n - n // 4),
            c.slice(c.put(ctrl, 2), 0, n // 3 + 17)]
    return _batch_items("out", c.enc.concat(srcs))


def _select(c):
    return _batch_items("out", c.enc.select_fields(c.primary(), c.spec["select"]))


def _zip(c):
    """Source 1: the batch's rows in reverse order (made at the control), at another placement."""
    import torch
    other = c.enc.take(c.control(), torch.arange(c.ref.n - 1, -1, -1))
    out = c.enc.zip_fields(c.primary(), [(c.enc, c.put(other, 1))], c.spec["zip"])
    return _batch_items("out", out)


def _extract(c):
    out = []
    for path in c.spec["extract"]:
        b, valid, src = c.enc.extract(c.primary(), path, return_indices=True)
        out += _batch_items(path, b) + [(f"{path}.validity", valid), (f"{path}.indices", src)]
    return out


def _explode_items(name, res):
    b, lo, ev, valid, par, ords = res
    return _batch_items(name, b) + [(f"{name}.list_offsets", lo), (f"{name}.entry_validity", ev),
                                    (f"{name}.elem_validity", valid), (f"{name}.parents", par),
                                    (f"{name}.ordinals", ords)]


def _explode(c):
    """The elements of LIST fields and the nested side of MAP fields; `explode_map_sides`: the
    elements of a LIST of MAP (made at the control) as a collection batch at this placement, and
    both of its sides that hold nested values."""
    out = []
    for path, side in c.spec["explode"]:
        out += _explode_items(f"{path}.{side}", c.enc.explode(c.primary(), path, side))
    for path in c.spec.get("explode_map_sides", ()):
        maps = c.enc.explode(c.control(), path)[0]
        menc = c.enc.element_encoder(path)
        c.clear()
        placed = c.put(maps, 0)
        for side in ("keys", "values"):
            e = menc._field.children[side == "values"]
            if e.children:                             # a scalar side has no batch form
                out += _explode_items(f"{path}[].{side}", menc.explode(placed, side))
    return out


def _split_map(c):
    out = []
    for path in c.spec["split_map"]:
        k, v, src, valid = c.enc.split_map(c.primary(), path)
        out += (_batch_items(f"{path}.keys", k) + _batch_items(f"{path}.values", v) +
                [(f"{path}.indices", src), (f"{path}.validity", valid)])
    return out


def _implode(c):
    """The inverse of explode: elements (made at the control) at this placement."""
    out = []
    for path in c.spec["implode"]:
        el, lo, ev, valid, _, _ = c.enc.explode(c.control(), path)
        E = int(lo[-1])
        c.clear()
        rows = c.enc.field_encoder(path).implode(c.put(el, 0), lo, ev, valid, num_elements=E)
        out += _batch_items(path, rows)
    return out


def _wrap(c):
    out = []
    for path in c.spec["wrap"]:
        vals, valid = c.enc.extract(c.control(), path)
        c.clear()
        rows = c.enc.field_encoder(path).wrap(c.put(vals, 0), valid, nrows=c.ref.n)
        out += _batch_items(path, rows)
    return out


def _join_map(c):
    """Keys and values (made at the control) each at a placement of its own."""
    out = []
    for path in c.spec["join_map"]:
        keys, vals, _, valid = c.enc.split_map(c.control(), path)
        c.clear()
        rows = c.enc.field_encoder(path).join_map(c.put(keys, 0), c.put(vals, 1), valid,
                                                  nrows=c.ref.n)
        out += _batch_items(path, rows)
    return out


def _encode(c):
    """encode_into with row_offsets = measured + B: an output at a base."""
    cols = c.cols()
    offs = c.enc.measure(cols, c.ref.n)
    rows, B = c.out(offs, 0)
    total = int(offs[-1])
    c.enc.encode_into(cols, c.ref.n, rows, offs + B)
    c.enc.device_status()
    return [("row_offsets", offs), ("rows", c.written(rows, B, total))]


class Consumer:
    def __init__(self, run, needs=None, writes=False, knobs=None):
        self.run, self.needs, self.writes, self.knobs = run, needs, writes, knobs

    def applies(self, schema) -> bool:
        return self.needs is None or self.needs in SPEC[schema]

    def legs(self, schema):
        return (self.knobs or {}).get(schema, [None])


# entry point -> adapter.  `writes`: it writes through the high offsets (the guard check follows).
CONSUMERS = {
    "decode_batch": Consumer(_decode, knobs=DECODE_KNOBS),
    "rows_to_arrow": Consumer(_arrow, knobs=DECODE_KNOBS),
    "project_batch": Consumer(_project, "project"),
    "update_fields": Consumer(_update, "update", writes=True),
    "hash_rows": Consumer(_hash, "hash"),
    "take": Consumer(_take),
    "filter": Consumer(_filter),
    "partition": Consumer(_partition),
    "concat": Consumer(_concat),
    "select_fields": Consumer(_select, "select"),
    "zip_fields": Consumer(_zip, "zip"),
    "extract": Consumer(_extract, "extract"),
    "explode": Consumer(_explode, "explode"),
    "split_map": Consumer(_split_map, "split_map"),
    "implode": Consumer(_implode, "implode"),
    "wrap": Consumer(_wrap, "wrap"),
    "join_map": Consumer(_join_map, "join_map"),
    "encode_into": Consumer(_encode, writes=True, knobs=ENCODE_KNOBS),
}

# public method -> the CONSUMERS entry that runs the same C entry point (the *_into and bind_* forms
# and the compositions go through the call their eager form makes)
RESOLVES = {
    "decode_batch": "decode_batch", "decode_into": "decode_batch", "bind_decode": "decode_batch",
    "write": "rows_to_arrow",
    "project_batch": "project_batch", "project_into": "project_batch",
    "bind_project": "project_batch",
    "update_fields": "update_fields", "bind_update": "update_fields",
    "hash_rows": "hash_rows", "hash_rows_into": "hash_rows", "bind_hash": "hash_rows",
    "take": "take", "take_into": "take", "bind_take": "take",
    "filter": "filter", "filter_into": "filter",
    "partition": "partition", "partition_into": "partition", "bind_partition": "partition",
    "partition_by": "partition",
    "concat": "concat", "concat_into": "concat",
    "select_fields": "select_fields", "select_fields_into": "select_fields",
    "bind_select_fields": "select_fields",
    "zip_fields": "zip_fields", "zip_fields_into": "zip_fields", "bind_zip_fields": "zip_fields",
    "with_fields": "zip_fields",
    "extract": "extract", "extract_into": "extract", "bind_extract": "extract",
    "explode": "explode", "explode_into": "explode", "bind_explode": "explode",
    "split_map": "split_map", "split_map_into": "split_map", "bind_split_map": "split_map",
    "split": "split_map", "split_into": "split_map", "bind_split": "split_map",
    "implode": "implode", "implode_into": "implode", "bind_implode": "implode",
    "with_elements": "implode",
    "wrap": "wrap", "wrap_into": "wrap", "bind_wrap": "wrap", "with_nested": "wrap",
    "join_map": "join_map", "join_map_into": "join_map", "bind_join_map": "join_map",
    "join": "join_map", "join_into": "join_map", "bind_join": "join_map", "with_map": "join_map",
}

# public method (or path) -> why it has no high-offset leg
EXEMPT = {
    "frame": "places frame i at row_offsets[i] + 12 * i: defined for 0-based batches only",
    "unframe": "takes a byte stream, not row offsets",
    "decode_host": "the host-memory path stages [0, total) of a host buffer",
    "encode_host": "the host-memory path stages [0, total) of a host buffer",
    "slice_rows": "host-side view, no kernel: rebases the offsets to 0 itself",
}

# ---- malformed rows whose outcome does not depend on the base ---------------------------------------
# tests/test_bounds.py's corruptions of a victim row above X.  "negative_offset" is left out: the
# contract's lower bound is 0, not row_offsets[0], so at a base the same slot points at bytes that
# are legitimately in bounds.
MALFORMED = ("offset_past_end", "size_past_end", "negative_size", "huge_list_count")
MALFORMED_SCHEMAS = ("mixed", "wide33", "nested")


def malformed_kinds(schema: str, how: str):
    """The type ids of the fields `how` can corrupt in `schema` (tests/test_bounds.py's rule)."""
    from fury_amd import types as T
    kinds = {"mixed": {T.STRING}, "wide33": {T.STRING, T.LIST}, "nested": {T.LIST}}[schema]
    if how == "huge_list_count":
        kinds = kinds & {T.LIST}
    elif how in ("size_past_end", "negative_size"):
        kinds = kinds - {T.LIST}          # a list's slot size is not read (BinaryArray.pointTo)
    return kinds


def malformed_cases():
    return [(s, h) for s in MALFORMED_SCHEMAS for h in MALFORMED if malformed_kinds(s, h)]


def victim(fields, rows, offs, n, kinds):
    """The first row after row m = n // 2 (above X at inside_row) with a non-null field of one of
    the type ids `kinds`, and that field."""
    for i in range(n // 2 + 1, n):
        for k, f in enumerate(fields):
            if f.type_id in kinds and not (rows[int(offs[i]) + (k >> 3)] >> (k & 7)) & 1:
                return i, k
    raise AssertionError("no victim")
