"""Fixed-width encode, tail window of default-policy row stores (tuning fixed_enc_tail_kib): every
window writes the oracle's rows, and the decode reads the oracle's columns back from them, at each
tile height's edges.  The knob only changes the cache policy of a tile's row stores, so the bar is
the one of tests/test_device.py: bit exact."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from fury_amd import types as T  # noqa: E402
from fury_amd.workloads import SCHEMAS, gen_columns  # noqa: E402
from tests.helpers import assert_columns_equal  # noqa: E402

KEY = b"fixed_enc_tail_kib"
# KiB: no window; exactly one 64-row Struct-100 tile (64 * 816 B); a boundary inside a tile's byte
# range; a window larger than every batch here
TAILS = (0, 51, 120, 1 << 18)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _lib():
    from fury_amd import _native as N
    return N.lib()


def _int64_fields(k):
    return [T.not_null_field(f"f{i:03d}", T.INT64) for i in range(k)]


def _fields_of(schema):
    return {"int64x50": lambda: _int64_fields(50),       # 408-B rows: 128-row tiles
            "int64x20": lambda: _int64_fields(20),       # 168-B rows: 256-row tiles
            }.get(schema, lambda: SCHEMAS[schema])()


_REF = {}


def _reference(oracle, schema, n):
    """Host columns, oracle rows and oracle-decoded columns of one shape, computed once."""
    key = (schema, n)
    if key not in _REF:
        fields = _fields_of(schema)
        host = gen_columns(schema, fields, n, seed=n)
        want, offs = oracle.encode(fields, host, n)
        _REF[key] = (fields, host, want, oracle.decode(fields, want, offs, n))
    return _REF[key]


def _check(oracle, dev, schema, n, misalign=None):
    from fury_amd.encoder import Encoders, column_to_device, column_to_host
    fields, host, want, ref = _reference(oracle, schema, n)
    enc = Encoders.bean(fields, device=dev)
    dcols = [column_to_device(c, dev) for c in host]
    fast = all(T.type_width(f.type_id) == 8 and not f.nullable for f in fields)
    saved = _lib().fury_get_tuning(KEY)
    try:
        for tail in TAILS:
            assert _lib().fury_set_tuning(KEY, tail) == 0
            batch = enc.encode_batch(dcols, n)
            got = batch.rows.cpu().numpy()
            assert np.array_equal(got, want), (schema, n, tail, "rows")
            # with validity buffers: the general tile kernel
            dec = [column_to_host(c) for c in enc.decode_batch(batch)]
            assert_columns_equal(fields, dec, ref, n)
            if fast:     # without: the fast path (pair kernel; non-pair for a misaligned column)
                out = enc.alloc_columns(n, validity=False)
                for c in out:
                    c.values.fill_(0x5A)
                if misalign is not None:
                    pad = torch.full((n * 8 + 8,), 0x5A, dtype=torch.uint8, device=dev)
                    out[misalign].values = pad[8:]
                enc.decode_into(batch, out)
                assert_columns_equal(fields, [column_to_host(c) for c in out], ref, n)
    finally:
        assert _lib().fury_set_tuning(KEY, saved) == 0


@pytest.mark.parametrize("schema,n", [
    ("struct100", 1), ("struct100", 63), ("struct100", 64), ("struct100", 65),
    ("struct100", 129), ("struct100", 1001),
    ("int64x50", 127), ("int64x50", 128), ("int64x50", 129), ("int64x50", 257),
    ("int64x20", 255), ("int64x20", 256), ("int64x20", 257), ("int64x20", 513),
    ("narrow", 65), ("narrow", 1001)])
def test_every_window_bit_exact(oracle, dev, schema, n):
    _check(oracle, dev, schema, n)


def test_misaligned_column(oracle, dev):
    """A column at an 8- but not 16-byte-aligned address: the decode takes the non-pair kernel."""
    _check(oracle, dev, "struct100", 257, misalign=3)


def test_window_splits_the_batch_where_stated(oracle, dev):
    """The window's first tile is the first one that lies wholly inside the batch's last W bytes;
    rows in front of it and inside it are the oracle's for every boundary around one tile."""
    n = 64 * 5 + 7                       # five full Struct-100 tiles and a ragged one
    from fury_amd.encoder import Encoders, column_to_device
    fields, host, want, _ = _reference(oracle, "struct100", n)
    enc = Encoders.bean(fields, device=dev)
    dcols = [column_to_device(c, dev) for c in host]
    saved = _lib().fury_get_tuning(KEY)
    try:
        for tail in (5, 6, 56, 57, 107, 108, 260, 261):   # KiB around 7, 71, 135, 327 rows
            assert _lib().fury_set_tuning(KEY, tail) == 0
            got = enc.encode_batch(dcols, n).rows.cpu().numpy()
            assert np.array_equal(got, want), tail
    finally:
        assert _lib().fury_set_tuning(KEY, saved) == 0


@pytest.mark.parametrize("bad", [-1, (1 << 22) + 1, -(1 << 31)])
def test_out_of_range_window_is_refused(dev, bad):
    before = _lib().fury_get_tuning(KEY)
    assert _lib().fury_set_tuning(KEY, bad) != 0
    assert _lib().fury_get_tuning(KEY) == before
