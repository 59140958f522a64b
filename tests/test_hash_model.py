"""A numpy model of fury_row_hash, written from rules 1-4 of include/fury_row.h alone, and pinned
here without a GPU: on the known answers of MurmurHash3_x86_32, on the host entry points
fury_hash_bytes / fury_hash_null through the C ABI, on vectors recorded from scikit-learn's
murmurhash3_32 (tests/golden/murmur3_x86_32.json; where sklearn imports, on fresh ones too), and on
the properties the rules promise: key order matters, null differs from the empty string, -0.0 from
0.0.  The GPU tests (tests/test_hash.py) compare the kernels with this model applied to decoded
columns."""
from __future__ import annotations

import ctypes
import json
import os
import struct

import numpy as np
import pytest

from fury_amd import types as T
from fury_amd.workloads import Column
from tests.helpers import as_u8, bits

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "murmur3_x86_32.json")
M32 = np.uint64(0xFFFFFFFF)
C1, C2 = np.uint64(0xCC9E2D51), np.uint64(0x1B873593)


# ---- rule 1, vectorised over rows: uint64 arrays holding 32-bit values -------------------------------
def _rotl(x, r):
    return ((x << np.uint64(r)) | (x >> np.uint64(32 - r))) & M32


def _scramble(k):
    return (_rotl((k * C1) & M32, 15) * C2) & M32


def _fmix(h):
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & M32
    return h ^ (h >> np.uint64(16))


def hash_spans(data, starts, lens, seeds):
    """H(data[starts[i]:starts[i] + lens[i]], seeds[i]) for every i, as a uint64 array of 32-bit
    values."""
    data = np.concatenate([as_u8(data) if len(data) else np.zeros(0, np.uint8),
                           np.zeros(4, np.uint8)]).astype(np.uint64)
    starts = np.asarray(starts, np.int64)
    lens = np.asarray(lens, np.int64)
    h = np.asarray(seeds, np.uint64).copy()
    nb = lens // 4
    for j in range(int(nb.max()) if len(nb) else 0):
        act = nb > j
        at = starts[act] + 4 * j
        k = data[at] | data[at + 1] << np.uint64(8) | data[at + 2] << np.uint64(16) | \
            data[at + 3] << np.uint64(24)
        x = _rotl(h[act] ^ _scramble(k), 13)
        h[act] = (x * np.uint64(5) + np.uint64(0xE6546B64)) & M32
    rem = lens & 3
    at = starts + 4 * nb
    k = np.zeros(len(lens), np.uint64)
    for b in (2, 1, 0):                              # the 1-3 bytes left over, little-endian
        has = rem > b
        k[has] = (k[has] << np.uint64(8)) | data[at[has] + b]
    tail = rem > 0
    h[tail] ^= _scramble(k[tail])
    return _fmix(h ^ (lens.astype(np.uint64) & M32))


def mm3(b: bytes, seed: int = 0) -> int:
    return int(hash_spans(np.frombuffer(b, np.uint8), [0], [len(b)], [seed])[0])


def mm3_null(seed: int = 0) -> int:
    return int(_fmix(np.asarray([seed], np.uint64) ^ M32)[0])


# ---- rules 2-4 over decoded columns --------------------------------------------------------------------
def value_spans(f, c, n):
    """(bytes, starts, lens, valid) of the n values of host column c of field f: rule 3."""
    valid = np.ones(n, bool) if c.validity is None else bits(c.validity, n)
    t = f.type_id
    if t == T.BOOL:
        data, w = bits(c.values, n).astype(np.uint8), 1
    elif t == T.DECIMAL:
        data, w = as_u8(c.values)[:16 * n], 16
    elif T.type_width(t) > 0:
        w = T.type_width(t)
        data = as_u8(c.values)[:w * n]
    elif t in (T.STRING, T.BINARY):
        offs = as_u8(c.offsets).view(np.int32)[:n + 1].astype(np.int64)
        data = as_u8(c.values) if c.values is not None else np.zeros(0, np.uint8)
        return data, offs[:-1], np.diff(offs), valid
    else:
        raise ValueError(f"field {f.name}: a LIST / STRUCT / MAP cannot be a hash key")
    return data, np.arange(n, dtype=np.int64) * w, np.full(n, w, np.int64), valid


def hash_columns(fields, cols, n, seed=0, null_rows=()):
    """hash[r] of rule 2 over the key columns, in order, as uint32.  null_rows: rows whose keys are
    all null whatever the columns say (rows outside the batch)."""
    h = np.full(n, seed, np.uint64)
    dead = np.zeros(n, bool)
    dead[list(null_rows)] = True
    for f, c in zip(fields, cols):
        data, starts, lens, valid = value_spans(f, c, n)
        valid = valid & ~dead
        hv = hash_spans(data, np.where(valid, starts, 0), np.where(valid, lens, 0), h)
        h = np.where(valid, hv, _fmix(h ^ M32))
    return h.astype(np.uint32)


def part_ids(hashes, num_parts):
    return (np.asarray(hashes, np.uint32).astype(np.uint64) % np.uint64(num_parts)).astype(np.int32)


def fixed_column(dtype, values, nulls=()):
    a = np.asarray(values, dtype)
    v = np.ones(len(a), bool)
    v[list(nulls)] = False
    return Column(values=a, validity=np.packbits(v, bitorder="little"))


def string_column(values):
    data = b"".join(v or b"" for v in values)
    offs = np.zeros(len(values) + 1, np.int32)
    np.cumsum([len(v or b"") for v in values], out=offs[1:])
    valid = np.array([v is not None for v in values])
    return Column(values=np.frombuffer(data, np.uint8), offsets=offs,
                  validity=np.packbits(valid, bitorder="little"))


# ---- the pins ------------------------------------------------------------------------------------------
KNOWN = [(b"", 0, 0), (b"", 1, 0x514E28B7), (b"", 42, 0x087FCD5C), (b"hello", 0, 0x248BFA47),
         (b"test", 0, 0xBA6BD213), (b"Hello, world!", 0, 0xC0363E43),
         (b"The quick brown fox jumps over the lazy dog", 0, 0x2E4FF723)]


def test_known_answers_of_h():
    for b, seed, want in KNOWN:
        assert mm3(b, seed) == want, (b, seed)


def test_known_answers_of_key_chains():
    i64, i32 = T.field("k", T.INT64), T.field("i", T.INT32)
    s, b = T.field("s", T.STRING), T.field("b", T.BOOL)
    assert hash_columns([i64], [fixed_column(np.int64, [42])], 1)[0] == 0x6F8F913E
    bool_col = Column(values=np.array([1], np.uint8), validity=np.array([1], np.uint8))
    assert hash_columns([b], [bool_col], 1)[0] == 0xE45AD1AB
    null = fixed_column(np.int64, [5], nulls=[0])
    assert hash_columns([i64], [null], 1, seed=0)[0] == 0x81F16F39 == mm3_null(0)
    assert hash_columns([i64], [null], 1, seed=42)[0] == 0x20BEE985 == mm3_null(42)
    seven, abc = fixed_column(np.int32, [7]), string_column([b"abc"])
    assert hash_columns([i32, s], [seven, abc], 1, seed=42)[0] == 0x826E53AF
    assert hash_columns([i32, i64, s], [seven, null, abc], 1, seed=42)[0] == 0xB62575B1


def test_host_entry_points_agree_with_the_model():
    """fury_hash_bytes / fury_hash_null through the C ABI, and the module-level wrappers."""
    import fury_amd
    from fury_amd import _native as N
    L = N.lib()
    assert L.fury_hash_bytes.restype is ctypes.c_uint32
    for b, seed, want in KNOWN:
        assert L.fury_hash_bytes(b, len(b), seed) == want
        assert fury_amd.hash_bytes(b, seed) == want
    assert L.fury_hash_bytes(None, 0, 42) == 0x087FCD5C            # NULL is fine for no bytes
    rng = np.random.default_rng(1)
    for n in list(range(0, 41)) + [255, 256, 257, 4099]:
        b = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        seed = int(rng.integers(0, 2 ** 32))
        assert L.fury_hash_bytes(b, n, seed) == mm3(b, seed), n
    for seed in (0, 1, 42, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF):
        assert L.fury_hash_null(seed) == mm3_null(seed) == fury_amd.hash_null(seed)
    # a CPU worker chaining the keys (INT32 7, null, STRING "abc") as rule 2 does
    h = fury_amd.hash_bytes(struct.pack("<i", 7), 42)
    assert fury_amd.hash_bytes(b"abc", fury_amd.hash_null(h)) == 0xB62575B1
    assert L.fury_hash_bytes(b"x", -1, 0) == 0 and "fury_hash_bytes" in N.last_error()
    assert L.fury_hash_bytes(None, 3, 0) == 0 and "fury_hash_bytes" in N.last_error()
    with pytest.raises(ValueError):
        fury_amd.hash_bytes(b"", -1)
    with pytest.raises(ValueError):
        fury_amd.hash_null(2 ** 32)


def _vector_inputs():
    """The inputs of the recorded vectors: byte strings of length 0..40, three seeds each."""
    rng = np.random.default_rng(20240229)
    out = []
    for n in range(41):
        for seed in (0, 42, int(rng.integers(0, 2 ** 32))):
            out.append((rng.integers(0, 256, n, dtype=np.uint8).tobytes(), seed))
    return out


def test_recorded_sklearn_vectors():
    """The vectors scikit-learn's murmurhash3_32 gave for _vector_inputs(), read from the data file:
    the model and the library agree with every one."""
    from fury_amd import _native as N
    with open(GOLDEN) as f:
        vectors = json.load(f)["vectors"]
    assert [(bytes.fromhex(v["hex"]), v["seed"]) for v in vectors] == _vector_inputs()
    for v in vectors:
        b = bytes.fromhex(v["hex"])
        assert mm3(b, v["seed"]) == v["hash"], v
        assert N.lib().fury_hash_bytes(b, len(b), v["seed"]) == v["hash"], v


def test_sklearn_agrees_on_random_byte_strings():
    murmurhash = pytest.importorskip("sklearn.utils.murmurhash")
    with open(GOLDEN) as f:
        recorded = {(v["hex"], v["seed"]): v["hash"] for v in json.load(f)["vectors"]}
    for b, seed in _vector_inputs():
        want = int(murmurhash.murmurhash3_32(b, seed=seed, positive=True))
        assert recorded[(b.hex(), seed)] == want
    rng = np.random.default_rng(7)
    for _ in range(300):
        b = rng.integers(0, 256, int(rng.integers(0, 41)), dtype=np.uint8).tobytes()
        seed = int(rng.integers(0, 2 ** 32))
        assert mm3(b, seed) == int(murmurhash.murmurhash3_32(b, seed=seed, positive=True))


def test_key_order_null_and_float_bits():
    i32, i64, s = T.field("i", T.INT32), T.field("k", T.INT64), T.field("s", T.STRING)
    f32, f64 = T.field("f", T.FLOAT32), T.field("d", T.FLOAT64)
    a, b = fixed_column(np.int32, [7, 8]), fixed_column(np.int64, [8, 7])
    assert (hash_columns([i32, i64], [a, b], 2) != hash_columns([i64, i32], [b, a], 2)).all()
    # null, the empty string and a one-byte zero are three different keys
    strs = string_column([None, b"", b"\x00"])
    assert len(set(hash_columns([s], [strs], 3).tolist())) == 3
    assert hash_columns([s], [strs], 3)[0] == mm3_null(0) and hash_columns([s], [strs], 3)[1] == 0
    # the position of a null among the keys matters
    x, nul = fixed_column(np.int32, [1]), fixed_column(np.int32, [1], nulls=[0])
    assert hash_columns([i32, i32], [x, nul], 1)[0] != hash_columns([i32, i32], [nul, x], 1)[0]
    # floats are raw bits
    for f, dt in ((f32, np.float32), (f64, np.float64)):
        z = hash_columns([f], [fixed_column(dt, [0.0, -0.0])], 2)
        assert z[0] != z[1]
        assert z[0] == mm3(bytes(np.dtype(dt).itemsize))
    nans = np.array([0x7FC00000, 0x7FC00001], np.uint32).view(np.float32)
    z = hash_columns([f32], [fixed_column(np.float32, nans)], 2)
    assert z[0] != z[1]
    # rule 4: the hash is unsigned
    assert part_ids(np.array([0xFFFFFFFF], np.uint32), 7)[0] == 0xFFFFFFFF % 7
    assert part_ids(np.array([0xFFFFFFFF], np.uint32), 2 ** 31 - 1)[0] == 1


def test_null_rows_and_wide_values():
    """null_rows overrides the columns, and the model's vectorised H equals H row by row."""
    rng = np.random.default_rng(3)
    vals = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in
            (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 300, 8191)]
    col = string_column(vals)
    got = hash_columns([T.field("s", T.STRING)], [col], len(vals), seed=9, null_rows=[2])
    for r, v in enumerate(vals):
        assert got[r] == (mm3_null(9) if r == 2 else mm3(v, 9))
