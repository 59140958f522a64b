"""The batches of the differential tests against the reference's C++ row code
(tests/test_reference_cpp.py) and of the fixtures it writes (tests/golden/make_ref_golden.py):
schemas with their input columns, built where a restatement of the row format goes wrong -- string
lengths around the 8-byte padding, list lengths around the 64-element null-bitmap words for every
element width, flat schemas around the 64-field bitmap words, nesting with a null at every level,
float bit patterns and integer extremes.

DECIMAL never appears: the reference's C++ sizes decimal128 as a 16-byte fixed field where the Java
writer puts it in the variable section (exclusions), so ``no_decimal`` replaces
a DECIMAL field by INT64 -- the field stays, the case count is unchanged."""
from __future__ import annotations

import functools
import random
from typing import Callable, List, NamedTuple, Optional, Sequence

import numpy as np

from fury_amd import types as T
from fury_amd.beans import beans_to_columns
from fury_amd.workloads import (BEANA_DECIMAL_UNSCALED, SCHEMAS, Column, JavaRandom, create_beana,
                                gen_columns)


class Case(NamedTuple):
    id: str
    fields: List[T.Field]
    cols: List[Column]
    n: int


# ---- DECIMAL ------------------------------------------------------------------------------------
def has_decimal(fields: Sequence[T.Field]) -> bool:
    return any(f.type_id == T.DECIMAL or has_decimal(f.children) for f in fields)


def no_decimal(fields: Sequence[T.Field]) -> List[T.Field]:
    return [T.Field(f.name, T.INT64 if f.type_id == T.DECIMAL else f.type_id, f.nullable,
                    tuple(no_decimal(f.children))) for f in fields]


def _from_beans(cid: str, fields, beans) -> Case:
    return Case(cid, list(fields), beans_to_columns(fields, beans), len(beans))


def _random_beans(fields, n: int, seed: int) -> list:
    from tests.test_reference_beans import random_bean
    jr = JavaRandom(seed)
    return [random_bean(fields, jr) for _ in range(n)]


# ---- the project's workload schemas -------------------------------------------------------------
def _gen_columns_can(fields) -> bool:
    """gen_columns covers scalars, STRING / BINARY and lists of fixed-width elements."""
    def ok(f):
        if f.type_id == T.LIST:
            return T.type_width(f.children[0].type_id) > 0
        return not f.children
    return all(ok(f) for f in fields)


def workload_case(name: str, n: int, fields: Optional[Sequence[T.Field]] = None,
                  seed: int = 1234) -> Case:
    """Schema ``name`` of fury_amd.workloads.SCHEMAS with gen_columns values; the schemas
    gen_columns has no generator for (struct / map fields) take random beans instead."""
    fields = list(SCHEMAS[name] if fields is None else fields)
    if _gen_columns_can(fields):
        return Case(f"{name}-{n}", fields, gen_columns(name, fields, n, seed=seed), n)
    return _from_beans(f"{name}-{n}", fields, _random_beans(fields, n, seed + n))


def beana_int64_beans(n: int, seed: int = 37) -> list:
    """createBeanA(0..6), then random beans, for BeanA with its BigDecimal f16 as an INT64."""
    fields = no_decimal(SCHEMAS["beana"])
    low = BEANA_DECIMAL_UNSCALED & 0xFFFFFFFFFFFFFFFF
    low = low - (1 << 64) if low >= 1 << 63 else low
    beans = []
    for k in range(min(n, 7)):
        b = create_beana(k)
        b["f16"] = low
        beans.append(b)
    return beans + _random_beans(fields, n - len(beans), seed)


def narrow_int64_case(n: int = 130) -> Case:
    return workload_case("narrow", n, no_decimal(SCHEMAS["narrow"]))._replace(id="narrow_int64")


def beana_int64_case(n: int = 40) -> Case:
    return _from_beans("beana_int64", no_decimal(SCHEMAS["beana"]), beana_int64_beans(n))


# ---- random schemas (tests/test_host_fuzz.random_schema, values as that file builds them) -------
FUZZ_SEEDS = 60


def fuzz_case(i: int) -> Case:
    from tests.test_host_fuzz import random_schema
    rnd = random.Random(20261019 + i)
    fields = no_decimal(random_schema(rnd))
    n = rnd.choice([0, 1, 7, 64, 65, 300])
    return _from_beans(f"fuzz{i:02d}", fields, _random_beans(fields, n, i))


# ---- strings and binaries: lengths around the padding word --------------------------------------
STRING_LENGTHS = tuple(range(18)) + (255, 256, 257)


def _text(rng, k: int) -> str:
    return "".join(chr(33 + int(x)) for x in rng.integers(0, 90, k))


def string_case(lengths: Sequence[int] = STRING_LENGTHS, cid: str = "strings") -> Case:
    fields = [T.field("s", T.STRING), T.field("b", T.BINARY), T.not_null_field("t", T.STRING),
              T.field("i", T.INT32)]
    rng = np.random.default_rng(17)
    beans = []
    for k in lengths:
        beans.append({"s": _text(rng, k), "b": bytes(rng.integers(0, 256, k, dtype=np.uint8)),
                      "t": _text(rng, (k * 7) % 19), "i": k})
        beans.append({"s": None, "b": bytes(rng.integers(0, 256, k, dtype=np.uint8)), "t": "",
                      "i": None})
        beans.append({"s": _text(rng, k), "b": None, "t": _text(rng, k), "i": -k})
    beans.append({"s": None, "b": None, "t": "", "i": None})
    return _from_beans(cid, fields, beans)


# ---- lists: every element width, lengths around the null-bitmap words ---------------------------
LIST_ELEMENTS = (T.BOOL, T.INT8, T.INT16, T.INT32, T.FLOAT32, T.INT64, T.FLOAT64, T.DATE32,
                 T.TIMESTAMP, T.STRING)
LIST_LENGTHS = (0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129)


def _scalar(t: int, rng):
    if t == T.BOOL:
        return bool(rng.integers(0, 2))
    if t == T.STRING:
        return _text(rng, int(rng.integers(0, 11)))
    if t == T.BINARY:
        return bytes(rng.integers(0, 256, int(rng.integers(0, 11)), dtype=np.uint8))
    if t == T.FLOAT32:
        return float(np.float32(rng.standard_normal()))
    if t == T.FLOAT64:
        return float(rng.standard_normal())
    bits = 8 * T.type_width(t)
    return int(rng.integers(-(1 << (bits - 1)), (1 << (bits - 1)) - 1, endpoint=True))


def all_positions(k: int) -> Sequence[int]:
    return range(k)


def edge_positions(k: int) -> Sequence[int]:
    """Every position of a short list; of a long one the first, the last and both sides of each
    64-element bitmap word boundary."""
    if k <= 9:
        return range(k)
    return sorted({p for p in (0, 63, 64, 127, 128, k - 1) if p < k})


def list_case(elem: int, nullable: bool, lengths: Sequence[int] = LIST_LENGTHS,
              null_at: Callable[[int], Sequence[int]] = all_positions) -> Case:
    """list<elem> of each length: one row of values; with nullable items also an all-null row and a
    row per position ``null_at(length)`` with that one element null; a null list; and an INT16
    field after the list, whose slot follows it."""
    fields = [T.Field("l", T.LIST, True, (T.Field("item", elem, nullable),)),
              T.field("after", T.INT16)]
    rng = np.random.default_rng(100 + elem)
    beans = []

    def row(values):
        beans.append({"l": values, "after": len(beans) - 100})
    for k in lengths:
        row([_scalar(elem, rng) for _ in range(k)])
        if nullable:
            row([None] * k)
            for p in null_at(k):
                v = [_scalar(elem, rng) for _ in range(k)]
                v[p] = None
                row(v)
    row(None)
    return _from_beans(list_case_id(elem, nullable), fields, beans)


def list_case_id(elem: int, nullable: bool) -> str:
    name = T.TYPE_NAMES[elem].split("[")[0]
    return f"list_{name}_{'nullable' if nullable else 'notnull'}"


# ---- flat schemas around the 64-field bitmap words ----------------------------------------------
FLAT_WIDTHS = (63, 64, 65, 128, 129)
_FLAT_TYPES = (T.INT32, T.STRING, T.BOOL, T.INT64, T.INT8, T.FLOAT64, T.BINARY, T.INT16,
               T.FLOAT32, T.DATE32, T.TIMESTAMP)


def flat_case(nf: int, random_rows: int = 6) -> Case:
    """nf nullable fields of every scalar type.  Rows: no null; for each bitmap word its last field
    null (the schema's last field in a partial word), then its first field, then both; all null;
    every field but the last of each word null; random rows."""
    fields = [T.field(f"f{k:03d}", _FLAT_TYPES[k % len(_FLAT_TYPES)]) for k in range(nf)]
    rng = np.random.default_rng(nf)
    words = (nf + 63) // 64
    last = [min(64 * w + 63, nf - 1) for w in range(words)]
    first = [64 * w for w in range(words)]

    def bean(nulls):
        return {f.name: None if k in nulls else _scalar(f.type_id, rng)
                for k, f in enumerate(fields)}
    beans = [bean(())]
    for w in range(words):
        beans += [bean({last[w]}), bean({first[w]}), bean({first[w], last[w]})]
    beans.append(bean(set(last)))
    beans.append(bean(set(range(nf))))
    beans.append(bean(set(range(nf)) - set(last)))
    for _ in range(random_rows):
        beans.append(bean({k for k in range(nf) if rng.random() < 0.3}))
    return _from_beans(f"flat{nf}", fields, beans)


# ---- nesting and nulls --------------------------------------------------------------------------
def _lst(name: str, item: T.Field) -> T.Field:
    return T.Field(name, T.LIST, True, (T.Field("item", item.type_id, item.nullable, item.children),))


NESTING_IDS = ("list_list_struct", "map_utf8_list_int32", "map_int32_struct", "struct_chain6",
               "empties")


@functools.lru_cache(maxsize=None)
def nesting_cases(random_rows: int = 24) -> List[Case]:
    out = []

    def case(cid, fields, beans, seed):
        out.append(_from_beans(cid, fields, beans + _random_beans(fields, random_rows, seed)))

    st = T.struct_field("item", [T.field("a", T.INT32), T.field("s", T.STRING)])
    fields = [_lst("ll", _lst("item", st))]
    full = {"a": 7, "s": "seven"}
    case("list_list_struct", fields, [{"ll": v} for v in (
        None, [], [None], [[]], [[None]], [[{"a": None, "s": None}]], [[full]],
        [[full, None, {"a": None, "s": "x"}], None, [], [{"a": -1, "s": None}]],
        [[full] * 9, [None] * 65, [{"a": k, "s": "k" * (k % 10)} for k in range(64)]])], 1)

    fields = [T.map_field("m", T.field("key", T.STRING), _lst("value", T.field("item", T.INT32)))]
    case("map_utf8_list_int32", fields, [{"m": v} for v in (
        None, [], [("k", None)], [("k", [])], [("", [None])], [("k", [1, None, 3]), ("kk", None)],
        [(f"key{j:02d}", list(range(j))) for j in range(12)],
        [("a" * 8, [0] * 64), ("b" * 9, [None] * 65)])], 2)

    fields = [T.map_field("m", T.field("key", T.INT32),
                          T.struct_field("value", [T.field("x", T.INT64), T.field("y", T.STRING)]))]
    case("map_int32_struct", fields, [{"m": v} for v in (
        None, [], [(1, None)], [(-1, {"x": None, "y": None})], [(0, {"x": 1 << 62, "y": ""})],
        [(j, {"x": j, "y": "y" * j} if j % 3 else None) for j in range(-5, 70)])], 3)

    # a chain of six structs, s0 outermost: a null at each depth in turn, then each leaf
    def chain(d: int) -> T.Field:
        kids = [T.field(f"v{d}", T.INT32 if d % 2 else T.STRING)]
        kids.append(chain(d + 1) if d < 5 else T.field("leaf", T.INT64))
        return T.struct_field(f"s{d}", kids)

    def chain_value(null_depth: int, null_leaf: bool = False, null_v: int = -1):
        v = None if null_leaf else 1234567890123
        for d in range(5, -1, -1):
            vd = None if d == null_v else (d if d % 2 else f"v{d}")
            v = None if d == null_depth else {f"v{d}": vd, ("leaf" if d == 5 else f"s{d + 1}"): v}
        return v
    fields = [T.not_null_field("id", T.INT64), chain(0)]
    beans = [{"id": 0, "s0": chain_value(-1)}]
    beans += [{"id": 1 + d, "s0": chain_value(d)} for d in range(6)]
    beans += [{"id": 10, "s0": chain_value(-1, null_leaf=True)}]
    beans += [{"id": 20 + d, "s0": chain_value(-1, null_v=d)} for d in range(6)]
    case("struct_chain6", fields, beans, 4)

    fields = [T.array_field("l", T.INT32),
              T.map_field("m", T.field("key", T.STRING), T.field("value", T.INT32)),
              T.struct_field("s", [T.field("a", T.INT32), T.field("b", T.STRING)]),
              T.array_field("ls", T.STRING), T.field("x", T.BOOL)]
    case("empties", fields, [
        {"l": [], "m": [], "s": {"a": None, "b": None}, "ls": [], "x": False},
        {"l": None, "m": None, "s": None, "ls": None, "x": None},
        {"l": [None], "m": [("", None)], "s": {"a": 0, "b": ""}, "ls": [""], "x": True},
        {"l": [], "m": None, "s": {"a": None, "b": ""}, "ls": [None, "", None], "x": None}], 5)
    return out


# ---- special values -----------------------------------------------------------------------------
F32_BITS = (0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7FC12345,
            0xFFFFFFFF, 0x7F800001, 0xFF923456, 0x7FBFFFFF, 0x00000001, 0x807FFFFF, 0x7F7FFFFF,
            0x3F800000)
F64_BITS = (0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000,
            0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000012345, 0xFFFFFFFFFFFFFFFF,
            0x7FF0000000000001, 0xFFF4000000ABCDEF, 0x7FF7FFFFFFFFFFFF, 0x0000000000000001,
            0x800FFFFFFFFFFFFF, 0x7FEFFFFFFFFFFFFF, 0x3FF0000000000000)


def float_case() -> Case:
    """Every pattern as a scalar (non-null and nullable) and as list elements, raw bits kept."""
    n = len(F32_BITS)
    f32 = np.array(F32_BITS, np.uint32).view(np.float32)
    f64 = np.array(F64_BITS, np.uint64).view(np.float64)
    fields = [T.not_null_field("a", T.FLOAT32), T.field("b", T.FLOAT32),
              T.not_null_field("c", T.FLOAT64), T.field("d", T.FLOAT64),
              T.array_field("la", T.FLOAT32), T.array_field("lc", T.FLOAT64, elem_nullable=False)]
    valid = np.arange(n) % 5 != 4
    bits = np.packbits(valid.astype(np.uint8), bitorder="little")
    offs = np.arange(0, (n + 1) * n, n, dtype=np.int32)
    la = np.concatenate([np.roll(f32, i) for i in range(n)])
    lc = np.concatenate([np.roll(f64, -i) for i in range(n)])
    la_valid = (np.arange(n * n) % 7) != 3
    la = np.where(la_valid, la.view(np.uint32), 0).astype(np.uint32).view(np.float32)
    cols = [Column(values=f32.copy()),
            Column(values=np.where(valid, f32.view(np.uint32), 0).astype(np.uint32).view(np.float32),
                   validity=bits),
            Column(values=f64.copy()),
            Column(values=np.where(valid, f64.view(np.uint64), 0).astype(np.uint64).view(np.float64),
                   validity=bits),
            Column(offsets=offs, child=[Column(values=la, validity=np.packbits(
                la_valid.astype(np.uint8), bitorder="little"))]),
            Column(offsets=offs, child=[Column(values=lc)])]
    return Case("float_bits", fields, cols, n)


def int_case() -> Case:
    """Minimum, maximum, -1, 0 and 1 of every integer type, as scalars and as list elements."""
    kinds = (T.INT8, T.INT16, T.INT32, T.INT64, T.DATE32, T.TIMESTAMP)
    fields, lists = [], []
    for t in kinds:
        nm = T.TYPE_NAMES[t].split("[")[0]
        fields += [T.not_null_field(f"{nm}_a", t), T.field(f"{nm}_b", t)]
        lists.append(T.array_field(f"{nm}_l", t))
    fields += lists

    def ext(t):
        bits = 8 * T.type_width(t)
        return [-(1 << (bits - 1)), (1 << (bits - 1)) - 1, -1, 0, 1]
    beans = []
    for i in range(5):
        b = {}
        for t in kinds:
            nm = T.TYPE_NAMES[t].split("[")[0]
            b[f"{nm}_a"] = ext(t)[i]
            b[f"{nm}_b"] = None if i == 3 else ext(t)[(i + 1) % 5]
            b[f"{nm}_l"] = ext(t)[i:] + [None] + ext(t)[:i]
        beans.append(b)
    return _from_beans("int_extremes", fields, beans)


# ---- the registry: every case by id, built on demand ---------------------------------------------
def _registry() -> dict:
    reg = {}
    for name, fields in SCHEMAS.items():
        if not has_decimal(fields):
            for n in (1, 65, 257):
                reg[f"{name}-{n}"] = functools.partial(workload_case, name, n)
    # the two workload schemas with a DECIMAL field, that field as INT64: extra cases
    reg["narrow_int64"] = narrow_int64_case
    reg["beana_int64"] = beana_int64_case
    for i in range(FUZZ_SEEDS):
        reg[f"fuzz{i:02d}"] = functools.partial(fuzz_case, i)
    reg["strings"] = string_case
    for e in LIST_ELEMENTS:
        for nl in (True, False):
            reg[list_case_id(e, nl)] = functools.partial(list_case, e, nl)
    for nf in FLAT_WIDTHS:
        reg[f"flat{nf}"] = functools.partial(flat_case, nf)
    for k, cid in enumerate(NESTING_IDS):
        reg[cid] = functools.partial(lambda k: nesting_cases()[k], k)
    reg["float_bits"] = float_case
    reg["int_extremes"] = int_case
    return reg


REGISTRY = _registry()
CASE_IDS = tuple(REGISTRY)


@functools.lru_cache(maxsize=None)
def get_case(cid: str) -> Case:
    case = REGISTRY[cid]()
    assert case.id == cid, (case.id, cid)
    return case
