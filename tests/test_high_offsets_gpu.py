"""Every row consumer on batches that cross byte 2^31 and byte 2^32 of their buffer (GPU).

Sparse matrix: a ~100 KB-1 MB batch is copied to the placements of tests/high_offsets.py inside one
6 GiB arena of 0xAB and every adapter of CONSUMERS runs on it; every output buffer and the
device_status outcome must equal what the same adapter gives for the same bytes at base 0 in a tight
buffer (the control), which is tied to the oracle once per schema.  A consumer that writes through
the high offsets (encode at a base, update in place) is followed by a check that every arena byte
outside the written range is still 0xAB.  The arena starts 2^31 bytes before the `rows` view, so an
offset truncated to 32 bits -- sign-extended or not -- still lands inside the allocation: a wrong
cast shows as wrong bytes, never as a fault.

Dense legs: the produced bytes themselves pass 2^32 (long rows keep the row counts small); inputs
and outputs sit 2^31 bytes into slack buffers of their own, and the expected bytes are built with
torch on the device, independently of the kernels.

No tolerance anywhere: every comparison is bit-exact.  Marked gpu."""
from __future__ import annotations

import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import high_offsets as H  # noqa: E402
from tests.helpers import assert_columns_equal  # noqa: E402

_WORD = int.from_bytes(bytes([H.FILL]) * 8, "little", signed=True)
_CHUNK = 1 << 26                                     # int64 words per compare: 512 MiB


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def report(dev):
    """Wall time and peak device memory of this file (shown with -s)."""
    import time
    torch.zeros(1, device=dev)                       # the allocator exists from the first use on
    torch.cuda.reset_peak_memory_stats(dev)
    t0 = time.perf_counter()
    yield
    print(f"\ntest_high_offsets_gpu: {time.perf_counter() - t0:.1f} s, peak "
          f"torch.cuda.max_memory_allocated {torch.cuda.max_memory_allocated(dev) / 2**30:.2f} GiB")


class Arena:
    """SLACK + VIEW bytes of 0xAB; `rows` is the view SLACK bytes in.  `placed`: the (base, bytes)
    ranges of the view that hold a batch or receive an output."""

    def __init__(self, dev, view_bytes=H.VIEW_BYTES, slack=H.SLACK):
        self.slack = slack
        self.buf = torch.full((slack + view_bytes,), H.FILL, dtype=torch.uint8, device=dev)
        self.rows = self.buf[slack:]
        self.placed: list = []

    def free(self, B, total) -> bool:
        return (B >= 0 and B + total <= self.rows.numel() and
                all(B + total <= b or b + t <= B for b, t in self.placed))

    def reserve(self, B, total):
        assert B % 8 == 0 and total % 8 == 0, (B, total)
        assert self.free(B, total), (B, total, self.placed)
        self.placed.append((B, total))

    def place(self, data, B):
        self.reserve(B, data.numel())
        self.rows[B:B + data.numel()] = data

    def clear(self):
        for B, total in self.placed:
            self.rows[B:B + total] = H.FILL
        self.placed = []

    def _dirty(self, a, b):
        """Device bool: a byte of buf[a:b] is not 0xAB (a, b multiples of 8)."""
        bad = torch.zeros((), dtype=torch.bool, device=self.buf.device)
        words = self.buf[a:b].view(torch.int64)
        for k in range(0, words.numel(), _CHUNK):
            bad |= words[k:k + _CHUNK].ne(_WORD).any()
        return bad

    def _gaps(self):
        pos = 0
        for a, b in sorted((self.slack + B, self.slack + B + t) for B, t in self.placed):
            yield pos, a
            pos = b
        yield pos, self.buf.numel()

    def assert_guard(self):
        """Everything outside the placed ranges is still 0xAB, compared in chunks."""
        bad = torch.zeros((), dtype=torch.bool, device=self.buf.device)
        for a, b in self._gaps():
            bad |= self._dirty(a, b)
        if not bool(bad):
            return
        where = []
        for a, b in self._gaps():                     # the slow path: name the first stray bytes
            for k in range(a, b, 8 * _CHUNK):
                e = min(b, k + 8 * _CHUNK)
                hit = torch.nonzero(self.buf[k:e] != H.FILL)[:4].flatten().tolist()
                where += [k + h - self.slack for h in hit]
                self.buf[k:e] = H.FILL                # the next test starts from a clean arena
        raise AssertionError(f"bytes written outside {self.placed}: view offsets {where[:8]}")


@pytest.fixture(scope="module")
def arena(dev):
    a = Arena(dev)
    yield a
    a.rows = a.buf = None
    del a
    torch.cuda.empty_cache()


@contextlib.contextmanager
def tuned(leg):
    """A (knob, value) leg of tests/high_offsets.py, restored afterwards."""
    from fury_amd import _native as N
    L = N.lib()
    if leg is None:
        yield
        return
    key = leg[0].encode()
    old = L.fury_get_tuning(key)
    try:
        assert L.fury_set_tuning(key, leg[1]) == 0, N.last_error()
        yield
    finally:
        assert L.fury_set_tuning(key, old) == 0


_ENC: dict = {}
_DEVICE: dict = {}


def encoder(dev, schema):
    from fury_amd.encoder import Encoders
    if schema not in _ENC:
        _ENC[schema] = Encoders.bean(H.fields_of(schema), device=dev)
    return _ENC[schema]


def device_batch(dev, enc, rows, offs, n):
    from fury_amd.encoder import RowBatch
    return RowBatch(torch.from_numpy(np.array(rows)).to(dev), torch.from_numpy(np.array(offs)).to(dev),
                    n, enc.schema_hash)


class Ctx:
    """What an adapter of tests/high_offsets.py sees (its comment lists the methods).  case None: the
    control -- every batch at base 0 in a tight buffer of its own."""

    def __init__(self, oracle, dev, schema, arena=None, case=None, control=None):
        self.dev, self.schema, self.arena, self.case = dev, schema, arena, case
        self.ref = H.ref(oracle, schema)
        self.enc = encoder(dev, schema)
        self.spec = H.SPEC[schema]
        if control is None:
            key = ("control", schema)
            if key not in _DEVICE:
                _DEVICE[key] = device_batch(dev, self.enc, self.ref.rows, self.ref.offs, self.ref.n)
            control = _DEVICE[key]
        self._control = control
        self._primary = None
        assert (arena is None) == (case is None)

    def control(self):
        return self._control

    def primary(self):
        if self._primary is None:
            self._primary = self.put(self._control, 0)
        return self._primary

    def _base(self, offs, total, slot):
        """The base of this case's placement for 0-based offsets (slot > 0: the first of the other
        placements that is free)."""
        if len(offs) < 3:                              # no row m to straddle
            offs = np.array([0, total // 2 & ~7, total], np.int64)
        cases = [self.case]
        if slot:
            others = H.other_cases(self.case)
            cases = others[slot - 1:] + others[:slot - 1]
        for case in cases:
            B = H.case_base(case, offs)
            if self.arena.free(B, total):
                return B
        raise AssertionError(f"no free placement for {total} bytes among {cases}")

    def put(self, batch, slot=0):
        from fury_amd.encoder import RowBatch
        offs = batch.row_offsets
        n = offs.numel() - 1
        host = offs.cpu().numpy()
        total = int(host[n])
        assert int(host[0]) == 0 and total <= batch.rows.numel()
        if self.arena is None:
            return RowBatch(batch.rows[:total].clone(), offs.clone(), batch.nrows, batch.schema_hash)
        B = self._base(host, total, slot)
        self.arena.place(batch.rows[:total], B)
        return RowBatch(self.arena.rows, offs + B, batch.nrows, batch.schema_hash)

    def out(self, offs, slot=0):
        host = offs.cpu().numpy()
        total = int(host[-1])
        if self.arena is None:
            return torch.full((max(total, 16),), H.FILL, dtype=torch.uint8, device=self.dev), 0
        B = self._base(host, total, slot)
        self.arena.reserve(B, total)
        return self.arena.rows, B

    @staticmethod
    def written(rows, B, total):
        return rows[B:B + total].clone()

    @staticmethod
    def written_batch(b):
        lo, hi = (int(x) for x in b.row_offsets[[0, -1]].cpu())
        return b.rows[lo:hi].clone()

    @staticmethod
    def slice(b, start, stop):
        from fury_amd.encoder import RowBatch
        return RowBatch(b.rows, b.row_offsets[start:stop + 1], stop - start, b.schema_hash)

    def clear(self):
        self._primary = None
        if self.arena is not None:
            self.arena.clear()

    def cols(self):
        from fury_amd.encoder import column_to_device
        key = ("cols", self.schema)
        if key not in _DEVICE:
            _DEVICE[key] = [column_to_device(c, self.dev) for c in self.ref.host]
        return _DEVICE[key]

    def alt_cols(self, names):
        from fury_amd.encoder import column_to_device
        key = ("alt", self.schema)
        if key not in _DEVICE:
            _DEVICE[key] = [column_to_device(c, self.dev) for c in H.host_columns(self.schema, True)]
        return [_DEVICE[key][k] for k in self.enc._select(names)]


def freeze(items):
    """Adapter outputs on the host."""
    from fury_amd.encoder import column_to_host
    out = []
    for name, v in items:
        if isinstance(v, tuple) and v and v[0] == "columns":
            v = ("columns", v[1], [column_to_host(c) for c in v[2]], v[3])
        elif isinstance(v, torch.Tensor):
            v = v.detach().cpu().clone()
        out.append((name, v))
    return out


def run(fn, ctx):
    """(outputs on the host, device_status outcome) of one adapter."""
    from fury_amd.encoder import FuryError
    try:
        items = fn(ctx)
        ctx.enc.device_status()
        return freeze(items), ("ok", None)
    except FuryError as e:
        return [], (type(e).__name__, H.row_of(str(e)))


def assert_same(got, want, where=""):
    assert [k for k, _ in got] == [k for k, _ in want], where
    for (name, g), (_, w) in zip(got, want):
        at = f"{where}{name}"
        if isinstance(w, tuple) and w and w[0] == "columns":
            assert_columns_equal(w[1], g[2], w[2], w[3], path=at + ": ")
        elif isinstance(w, torch.Tensor):
            assert g.dtype == w.dtype and g.shape == w.shape, f"{at}: {g.dtype}{tuple(g.shape)}"
            if not torch.equal(g, w):
                bad = torch.nonzero(g != w).flatten()
                raise AssertionError(f"{at}: {bad.numel()} of {g.numel()} entries differ, first at "
                                     f"{bad[:8].tolist()}")
        else:
            assert g == w, f"{at}: {g} != {w}"


_CONTROL: dict = {}


def control_result(oracle, dev, name, schema, leg):
    """The adapter's outputs for the batch at base 0 in a tight buffer: once per leg (the caller has
    set the leg's knob)."""
    key = (name, schema, leg)
    if key not in _CONTROL:
        _CONTROL[key] = run(H.CONSUMERS[name].run, Ctx(oracle, dev, schema))
    return _CONTROL[key]


def _matrix():
    out = []
    for name, cons in H.CONSUMERS.items():
        for schema in H.SCHEMAS:
            if cons.applies(schema):
                for leg in cons.legs(schema):
                    tag = schema if leg is None else f"{schema}:{leg[0]}={leg[1]}"
                    out.append(pytest.param(name, schema, leg, id=f"{name}-{tag}"))
    return out


@pytest.mark.parametrize("schema", list(H.SCHEMAS))
def test_control_equals_oracle(oracle, dev, schema):
    """The control of the matrix below is itself right: the decode and the encode of every schema's
    batch at base 0, under every engine leg, equal the oracle's."""
    ref = H.ref(oracle, schema)
    for leg in H.DECODE_KNOBS[schema]:
        with tuned(leg):
            got, status = control_result(oracle, dev, "decode_batch", schema, leg)
        assert status == ("ok", None), (leg, status)
        assert_columns_equal(ref.fields, got[0][1][2], ref.cols, ref.n)
    for leg in H.ENCODE_KNOBS[schema]:
        with tuned(leg):
            got, status = control_result(oracle, dev, "encode_into", schema, leg)
        assert status == ("ok", None), (leg, status)
        out = dict(got)
        assert np.array_equal(out["row_offsets"].numpy(), ref.offs), leg
        assert np.array_equal(out["rows"].numpy(), ref.rows), leg


@pytest.mark.parametrize("case", H.CASES)
@pytest.mark.parametrize("name,schema,leg", _matrix())
def test_placed_equals_control(oracle, dev, arena, name, schema, leg, case):
    """The same adapter on the same bytes at a placement across 2^31 / 2^32: every output buffer and
    the device_status outcome equal the control's; a writing consumer leaves every arena byte
    outside the written range 0xAB."""
    cons = H.CONSUMERS[name]
    ctx = Ctx(oracle, dev, schema, arena, case)
    try:
        with tuned(leg):
            want, want_status = control_result(oracle, dev, name, schema, leg)
            got, status = run(cons.run, ctx)
        assert want_status == ("ok", None), want_status
        assert status == want_status
        if cons.writes:
            arena.assert_guard()
    finally:
        ctx.clear()
    assert_same(got, want, f"{name} {schema} {case}: ")


# ---- malformed rows whose outcome does not depend on the base --------------------------------------
def _status(enc):
    from fury_amd.encoder import FuryError
    try:
        enc.device_status()
        return ("ok", None)
    except FuryError as e:
        return (type(e).__name__, H.row_of(str(e)))


def _raised(call):
    from fury_amd.encoder import FuryError
    try:
        call()
        return ("ok", None)
    except FuryError as e:
        return (type(e).__name__, H.row_of(str(e)))


def _malformed_outcomes(c, names):
    """decode, projected decode, take and select of a batch with one malformed row: what each raises
    or reports, and the rows take and select produce all the same."""
    b = c.primary()
    n, enc = b.nrows, c.enc
    out = [("decode", _raised(lambda: enc.decode_batch(b))),
           ("project", _raised(lambda: enc.project_batch(b, names)))]
    idx = torch.arange(n - 1, -1, -1, device=c.dev)
    for what, into in (("take", lambda rows, offs: enc.take_into(b, idx, rows, offs)),
                       ("select", lambda rows, offs: enc.select_fields_into(b, names, rows, offs))):
        offs = torch.empty(n + 1, dtype=torch.int64, device=c.dev)
        into(None, offs)
        total = int(offs[-1])
        _status(enc)
        rows = torch.full((max(total, 16),), H.FILL, dtype=torch.uint8, device=c.dev)
        into(rows, offs)
        out += [(f"{what}.status", _status(enc)), (f"{what}.rows", rows[:total]),
                (f"{what}.row_offsets", offs)]
    return freeze(out)


@pytest.mark.parametrize("x", list(H.BOUNDARIES))
@pytest.mark.parametrize("schema,how", H.malformed_cases())
def test_malformed_row_above_the_boundary(oracle, dev, arena, schema, how, x):
    """tests/test_bounds.py's offset_past_end, size_past_end, negative_size and huge_list_count on a
    victim row above X, at inside_row: the decode and the projected decode raise the control's
    exception for the control's row, take copies and select nulls-and-reports exactly as at the
    control.  These four are translation-invariant (they point past row_offsets[nrows], which moves
    with the base).  negative_offset is left out on purpose: the contract's lower bound is 0, not
    row_offsets[0], so at a base the same slot points at bytes that are legitimately in bounds."""
    from tests.test_bounds import _corrupt
    ref = H.ref(oracle, schema)
    enc = encoder(dev, schema)
    i, k = H.victim(ref.fields, ref.rows, ref.offs, ref.n, H.malformed_kinds(schema, how))
    bad = _corrupt(ref.fields, ref.rows, ref.offs, ref.n, i, k, how)
    control = device_batch(dev, enc, bad, ref.offs, ref.n)
    names = [ref.fields[k].name, ref.fields[0].name]
    want = _malformed_outcomes(Ctx(oracle, dev, schema, control=control), names)
    ctx = Ctx(oracle, dev, schema, arena, f"inside_row-{x}", control=control)
    try:
        got = _malformed_outcomes(ctx, names)
    finally:
        ctx.clear()
    outcome = dict(want)
    assert outcome["decode"] == ("IndexOutOfBoundsException", i), outcome["decode"]
    assert outcome["project"] == ("IndexOutOfBoundsException", i), outcome["project"]
    if how != "huge_list_count":       # select copies a list's bytes whole: it never reads the count
        assert outcome["select.status"][0] == "IndexOutOfBoundsException", outcome["select.status"]
    assert_same(got, want, f"{schema} {how} {x}: ")


# ---- dense legs: the produced bytes themselves pass 2^32 ---------------------------------------------
_TAIL = 1 << 20


@pytest.fixture
def dense(dev):
    """Everything a dense leg allocated is released after it."""
    import gc
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _slack(dev, nbytes):
    """A buffer for `nbytes` of rows that starts 2^31 bytes into an allocation of 0xAB."""
    a = Arena(dev, nbytes + _TAIL)
    a.reserve(0, nbytes)
    return a


def _cumsum0(sizes):
    out = np.zeros(len(sizes) + 1, np.int64)
    np.cumsum(sizes, out=out[1:])
    return out


def _cat_rows(rows, offs, order):
    """torch.cat of the rows `order` of a batch with host offsets `offs`."""
    return torch.cat([rows[int(offs[i]):int(offs[i + 1])] for i in order])


def _equal_rows(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    if not torch.equal(got, want):
        step = 1 << 28
        for k in range(0, got.numel(), step):
            bad = torch.nonzero(got[k:k + step] != want[k:k + step]).flatten()
            if bad.numel():
                raise AssertionError(f"rows differ from byte {k + int(bad[0])} on")


def _binary_column(dev, lengths, g):
    """A device BINARY column of random bytes for value bytes `lengths` (-1 = null)."""
    from fury_amd.workloads import Column
    n = len(lengths)
    valid = lengths >= 0
    offs = _cumsum0(np.where(valid, lengths, 0))
    assert offs[-1] <= H.INT32_MAX
    bits = np.zeros((n + 31) // 32 * 4, np.uint8)
    packed = np.packbits(valid.astype(np.uint8), bitorder="little")
    bits[:len(packed)] = packed
    values = torch.randint(0, 256, (max(int(offs[-1]), 1),), dtype=torch.uint8, device=dev,
                           generator=g)
    return Column(values=values, validity=torch.from_numpy(bits).to(dev),
                  offsets=torch.from_numpy(offs.astype(np.int32)).to(dev))


def long_columns(dev, lengths, seed):
    """Device columns of the long-row schema for value bytes `lengths` ([rows, 3], -1 = null)."""
    from fury_amd.workloads import Column
    n = len(lengths)
    g = torch.Generator(device=dev).manual_seed(seed)
    ids = torch.arange(n, dtype=torch.int64, device=dev) * 1000003 + seed
    return [Column(values=ids)] + [_binary_column(dev, lengths[:, k], g) for k in range(3)]


def _host_row(cols, r):
    """Row r of long_columns as one-row host columns (what the oracle encodes)."""
    from fury_amd.workloads import Column
    out = [Column(values=cols[0].values[r:r + 1].cpu().numpy())]
    for c in cols[1:]:
        b, e = (int(x) for x in c.offsets[r:r + 2].cpu())
        valid = (int(c.validity[r >> 3]) >> (r & 7)) & 1
        out.append(Column(values=c.values[b:e].cpu().numpy().copy() if e > b else np.zeros(1, np.uint8),
                          validity=np.array([valid], np.uint8),
                          offsets=np.array([0, e - b], np.int32)))
    return out


def _long_batch(dev):
    """The LONG_ROWS-row long-row batch encoded into a slack buffer: (enc, cols, offsets on the
    host, the buffer, the batch)."""
    from fury_amd.encoder import Encoders, RowBatch
    ln = H.long_lengths()
    want = _cumsum0(H.long_row_bytes(ln))
    total = int(want[-1])
    enc = Encoders.bean(H.long_fields(), device=dev)
    cols = long_columns(dev, ln, 17)
    offs = enc.measure(cols, H.LONG_ROWS)
    assert torch.equal(offs.cpu(), torch.cumsum(torch.from_numpy(np.concatenate(
        [[0], H.long_row_bytes(ln)])), 0)), "measured offsets != the layout formula"
    a = _slack(dev, total)
    enc.encode_into(cols, H.LONG_ROWS, a.rows, offs)
    enc.device_status()
    a.assert_guard()
    return enc, cols, want, a, RowBatch(a.rows, offs, H.LONG_ROWS, enc.schema_hash)


def test_dense_struct100_roundtrip(dev, dense):
    """D1: Struct-100 at 5.3M rows (4.32 GB) encoded into a view 2^31 bytes into a slack buffer and
    decoded back: the stacked-slots equality of test_struct100_full_size_roundtrip_property."""
    from fury_amd.encoder import Encoders, RowBatch
    from fury_amd.workloads import SCHEMAS, Column
    rows, size = H.D1_ROWS, H.D1_ROW_BYTES
    fields = SCHEMAS["struct100"]
    g = torch.Generator(device=dev).manual_seed(5)
    cols = [Column(values=torch.randint(-2**63, 2**63 - 1, (rows,), dtype=torch.int64, device=dev,
                                        generator=g)) for _ in fields]
    enc = Encoders.bean(fields, device=dev)
    assert enc.schema().fixed_size == size and rows * size > H.X32
    a = _slack(dev, rows * size)
    enc.encode_into(cols, rows, a.rows, None)
    enc.device_status()
    a.assert_guard()
    r = a.rows[:rows * size].view(rows, size)
    assert not bool(r[:, :16].any())
    slots = r[:, 16:].contiguous().view(torch.int64).view(rows, 100)
    stacked = torch.stack([c.values for c in cols], dim=1)
    assert torch.equal(slots, stacked)
    del slots, stacked
    dec = enc.decode_batch(RowBatch(a.rows[:rows * size], None, rows, enc.schema_hash),
                           validity=False)
    for c, d in zip(cols, dec):
        assert torch.equal(c.values.view(torch.uint8), d.values)


def test_dense_long_rows_encode_decode(oracle, dev, dense):
    """D2: the long-row schema, 1440 rows of about 3 MiB: the measured offsets equal a torch cumsum
    of the layout formula, the rows that straddle 2^31 and 2^32 equal the oracle's encode of those
    rows, and decode(encode(cols)) == cols for every buffer."""
    enc, cols, want, a, batch = _long_batch(dev)
    n = H.LONG_ROWS
    assert int(want[-1]) > H.X32
    for X in (H.X31, H.X32):
        r = int(np.searchsorted(want, X, side="right")) - 1
        assert want[r] < X < want[r + 1]
        ref_rows, _ = oracle.encode(H.long_fields(), _host_row(cols, r), 1)
        got = a.rows[int(want[r]):int(want[r + 1])].cpu().numpy()
        assert np.array_equal(got, ref_rows), f"row {r} across {X}"
    dec = enc.decode_batch(batch)
    assert torch.equal(dec[0].values.view(torch.int64)[:n], cols[0].values)
    for c, d in zip(cols[1:], dec[1:]):
        total = int(c.offsets[n])
        assert torch.equal(d.offsets[:n + 1], c.offsets)
        assert torch.equal(d.values[:total], c.values[:total])
        assert torch.equal(d.validity[:n // 8], c.validity[:n // 8])


def _taken(dev):
    """LONG_TAKE rows cycling through an 8-row source, taken into a slack buffer (more than 2^32
    bytes): (enc, the 8-row batch, its host offsets, the row order, the buffer, the big batch, its
    host offsets)."""
    from fury_amd.encoder import Encoders, RowBatch
    ln = H.long_lengths()[:H.LONG_DISTINCT]
    enc = Encoders.bean(H.long_fields(), device=dev)
    src = enc.encode_batch(long_columns(dev, ln, 23), H.LONG_DISTINCT)
    so = _cumsum0(H.long_row_bytes(ln))
    assert np.array_equal(src.row_offsets.cpu().numpy(), so)
    order = H.take_indices()
    want = _cumsum0(np.diff(so)[order])
    total = int(want[-1])
    assert total > H.X32
    a = _slack(dev, total)
    offs = torch.empty(len(order) + 1, dtype=torch.int64, device=dev)
    enc.take_into(src, order, a.rows[:total], offs)
    enc.device_status()
    a.assert_guard()
    assert np.array_equal(offs.cpu().numpy(), want)
    return enc, src, so, order, a, RowBatch(a.rows, offs, len(order), enc.schema_hash), want


def test_dense_take_concat_partition(dev, dense):
    """D3: take with repeated indices from an 8-row source to more than 2^32 output bytes, then a
    concat of three interior slices and a partition into 3 of that batch: each equals torch.cat of
    the source rows' slices in the expected order, with the cumsum's offsets."""
    enc, src, so, order, a, big, bo = _taken(dev)
    total = int(bo[-1])
    _equal_rows(a.rows[:total], _cat_rows(src.rows, so, order))
    n = big.nrows
    # concat: three interior slices, each starting above 0 or crossing a boundary
    cuts = [(n - n // 3, n), (0, n // 2 - 150), (n // 3, n - n // 3)]
    srcs = [Ctx.slice(big, s, e) for s, e in cuts]
    rows_of = [i for s, e in cuts for i in range(s, e)]
    want = _cumsum0(np.diff(bo)[rows_of])
    assert int(want[-1]) > H.X32
    out = _slack(dev, int(want[-1]))
    offs = torch.empty(len(rows_of) + 1, dtype=torch.int64, device=dev)
    enc.concat_into(srcs, out.rows[:int(want[-1])], offs)
    enc.device_status()
    out.assert_guard()
    assert np.array_equal(offs.cpu().numpy(), want)
    _equal_rows(out.rows[:int(want[-1])], torch.cat([a.rows[int(bo[s]):int(bo[e])] for s, e in cuts]))
    # partition into 3, every row kept
    out.clear()
    out.reserve(0, total)
    ids = (np.arange(n) * 7 + 1) % 3
    rows_of = np.argsort(ids, kind="stable")
    want = _cumsum0(np.diff(bo)[rows_of])
    offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
    part_rows = torch.empty(4, dtype=torch.int64, device=dev)
    indices = torch.empty(n, dtype=torch.int64, device=dev)
    positions = torch.empty(n, dtype=torch.int64, device=dev)
    enc.partition_into(big, ids, 3, out.rows[:total], offs, part_rows, indices, positions)
    enc.device_status()
    out.assert_guard()
    assert np.array_equal(offs.cpu().numpy(), want)
    assert part_rows.tolist() == _cumsum0(np.bincount(ids, minlength=3)).tolist()
    assert np.array_equal(indices.cpu().numpy(), rows_of)
    assert np.array_equal(positions.cpu().numpy()[rows_of], np.arange(n))
    _equal_rows(out.rows[:total], _cat_rows(a.rows, bo, rows_of))


def test_dense_select_zip(dev, dense):
    """D4: select_fields (drop id, reorder) and zip_fields (the long-row source plus a short-row
    source) of a batch above 2^32 bytes: each equals torch.cat of the outputs the same operator gives
    for the 8 distinct rows."""
    from fury_amd import types as T
    from fury_amd.encoder import Encoders, column_to_device
    from fury_amd.workloads import gen_columns
    enc, src, so, order, a, big, bo = _taken(dev)
    names = ["c", "a", "b"]
    small = enc.select_fields(src, names)
    sm = small.row_offsets.cpu().numpy()
    want = _cumsum0(np.diff(sm)[order])
    total = int(want[-1])
    assert total == int(bo[-1]) - 8 * len(order) and total > H.X32
    out = _slack(dev, int(bo[-1]) + 64 * len(order))
    offs = torch.empty(len(order) + 1, dtype=torch.int64, device=dev)
    enc.select_fields_into(big, names, out.rows[:total], offs)
    enc.device_status()
    out.placed = [(0, total)]
    out.assert_guard()
    assert np.array_equal(offs.cpu().numpy(), want)
    _equal_rows(out.rows[:total], _cat_rows(small.rows, sm, order))
    # zip: fields of the long rows and of short rows, alternating
    sfields = [T.not_null_field("x", T.INT64), T.field("s", T.STRING)]
    senc = Encoders.bean(sfields, device=dev)
    short = senc.encode_batch([column_to_device(c, dev) for c in gen_columns(
        "wide", sfields, H.LONG_DISTINCT, seed=3, null_pct=10, str_max=20)], H.LONG_DISTINCT)
    shorts = senc.take(short, order)
    picks = [(0, "a"), (1, "s"), (0, "b"), (1, "x"), (0, "c")]
    small = enc.zip_fields(src, [(senc, short)], picks)
    sm = small.row_offsets.cpu().numpy()
    want = _cumsum0(np.diff(sm)[order])
    total = int(want[-1])
    assert H.X32 < total <= int(bo[-1]) + 64 * len(order)
    out.clear()
    out.reserve(0, total)
    enc.zip_fields_into(big, [(senc, shorts)], picks, out.rows[:total], offs)
    enc.device_status()
    out.assert_guard()
    assert np.array_equal(offs.cpu().numpy(), want)
    _equal_rows(out.rows[:total], _cat_rows(small.rows, sm, order))


def test_dense_frame_unframe(dev, dense):
    """D6: frame then unframe of the D2 batch, both through buffers that start 2^31 bytes into slack:
    the stream is [int32 len = 8 + row size][int64 hash][row] per row, unframe gives the batch back, and the
    sequential walk (tuning counter unframe_walks) is not taken."""
    import ctypes
    from fury_amd import _native as N
    enc, cols, want, a, batch = _long_batch(dev)
    del cols
    n, total = H.LONG_ROWS, int(want[-1])
    L = N.lib()
    walks = L.fury_get_tuning(b"unframe_walks")
    framed = _slack(dev, total + 12 * n)
    fo = torch.empty(n + 1, dtype=torch.int64, device=dev)
    st = L.fury_frame_rows(enc.schema().handle, a.rows.data_ptr(), batch.row_offsets.data_ptr(), n,
                           framed.rows.data_ptr(), fo.data_ptr(), None)
    assert st == 0, N.last_error()
    enc.device_status()
    assert np.array_equal(fo.cpu().numpy(), want + 12 * np.arange(n + 1))
    framed.assert_guard()
    head = np.zeros(12, np.uint8)
    for r in (0, n // 2, n - 1):
        b = int(want[r]) + 12 * r
        head[:4] = np.frombuffer(np.int32(8 + want[r + 1] - want[r]).tobytes(), np.uint8)
        head[4:] = np.frombuffer(np.int64(enc.schema_hash).tobytes(), np.uint8)
        assert np.array_equal(framed.rows[b:b + 12].cpu().numpy(), head)
        _equal_rows(framed.rows[b + 12:b + 12 + int(want[r + 1] - want[r])],
                    a.rows[int(want[r]):int(want[r + 1])])
    back = _slack(dev, total)
    offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
    st = L.fury_unframe_rows(enc.schema().handle, framed.rows.data_ptr(),
                             ctypes.c_int64(total + 12 * n), n, back.rows.data_ptr(),
                             offs.data_ptr(), None)
    assert st == 0, N.last_error()
    enc.device_status()
    back.assert_guard()
    assert np.array_equal(offs.cpu().numpy(), want)
    _equal_rows(back.rows[:total], a.rows[:total])
    assert L.fury_get_tuning(b"unframe_walks") == walks


def _element_batches(dev):
    """8 one-field struct rows v BINARY of about 1 MiB, and IMPLODE_ELEMENTS of them, cycling, taken
    into a slack buffer (more than 2^32 bytes)."""
    from fury_amd import types as T
    from fury_amd.encoder import Encoders, RowBatch
    efields = [T.field("v", T.BINARY)]
    eenc = Encoders.bean(efields, device=dev)
    ln = H.long_lengths()[:H.LONG_DISTINCT, 0]
    ln = np.where(ln < 0, H.LONG_VALUE + 5, ln)
    g = torch.Generator(device=dev).manual_seed(29)
    el8 = eenc.encode_batch([_binary_column(dev, ln, g)], H.LONG_DISTINCT)
    eo = el8.row_offsets.cpu().numpy()
    assert np.array_equal(np.diff(eo), 16 + ((ln + 7) & ~7))
    order = H.take_indices(H.IMPLODE_ELEMENTS)
    want = _cumsum0(np.diff(eo)[order])
    total = int(want[-1])
    assert total > H.X32
    a = _slack(dev, total)
    offs = torch.empty(len(order) + 1, dtype=torch.int64, device=dev)
    eenc.take_into(el8, order, a.rows[:total], offs)
    eenc.device_status()
    a.assert_guard()
    assert np.array_equal(offs.cpu().numpy(), want)
    return efields, eenc, el8, order, a, RowBatch(a.rows, offs, len(order), eenc.schema_hash)


def test_dense_implode(dev, dense):
    """D5: implode of about 4 elements of 1 MiB per list into more than 2^32 bytes of rows: equals
    torch.cat of the rows the same operator gives for the 4 distinct lists."""
    from fury_amd import types as T
    from fury_amd.encoder import Encoders
    efields, eenc, el8, order, a, elements = _element_batches(dev)
    E = len(order)
    lens = np.tile(np.array(H.LIST_LENGTHS, np.int64), E // sum(H.LIST_LENGTHS))
    assert int(lens.sum()) == E and sum(H.LIST_LENGTHS) % H.LONG_DISTINCT == 0
    nlists, period = len(lens), len(H.LIST_LENGTHS)
    tgt = Encoders.bean([T.Field("l", T.LIST, True, (T.struct_field("item", efields),))],
                        device=dev)
    k = sum(H.LIST_LENGTHS)
    small = tgt.implode(eenc.take(el8, order[:k]),
                        torch.from_numpy(_cumsum0(lens[:period])).to(dev))
    sm = small.row_offsets.cpu().numpy()
    which = np.arange(nlists) % period
    want = _cumsum0(np.diff(sm)[which])
    total = int(want[-1])
    assert total > H.X32 and int(np.diff(sm).max()) <= H.INT32_MAX - 7
    out = _slack(dev, total)
    offs = torch.empty(nlists + 1, dtype=torch.int64, device=dev)
    tgt.implode_into(elements, torch.from_numpy(_cumsum0(lens)).to(dev), out.rows[:total], offs)
    tgt.device_status()
    out.assert_guard()
    assert np.array_equal(offs.cpu().numpy(), want)
    _equal_rows(out.rows[:total], _cat_rows(small.rows, sm, which))


def test_dense_join_map(dev, dense):
    """D5: join_map of key arrays and value arrays (4 values of about 1 MiB each) into more than
    2^32 bytes of rows: equals torch.cat of the rows the same operator gives for the 8 distinct
    maps."""
    from fury_amd import types as T
    from fury_amd.beans import beans_to_columns
    from fury_amd.encoder import Encoders, RowBatch, column_to_device
    fields = [T.map_field("m", T.field("key", T.INT64), T.field("value", T.BINARY))]
    menc = Encoders.bean(fields, device=dev)
    rng = np.random.default_rng(31)
    ln = H.long_lengths()[:H.LONG_DISTINCT]
    ln = np.where(ln < 0, H.LONG_VALUE + 5, ln)
    beans = [{"m": [(int(r * 100 + j), bytes(rng.integers(0, 256, int(ln[r, j % 3]), dtype=np.uint8)))
                    for j in range(H.LIST_LEN)]} for r in range(H.LONG_DISTINCT)]
    cols = [column_to_device(c, dev) for c in beans_to_columns(fields, beans)]
    maps8 = menc.encode_batch(cols, H.LONG_DISTINCT)
    keys8, vals8, _, _ = menc.split_map(maps8, "m")
    small = menc.join_map(keys8, vals8)
    _equal_rows(small.rows, maps8.rows)
    sm = small.row_offsets.cpu().numpy()
    order = H.take_indices(H.JOIN_MAPS)
    keys = menc.key_array_encoder("m").take(keys8, order)
    venc = menc.value_array_encoder("m")
    vo = vals8.row_offsets.cpu().numpy()
    vwant = _cumsum0(np.diff(vo)[order])
    vtotal = int(vwant[-1])
    a = _slack(dev, vtotal)
    voffs = torch.empty(len(order) + 1, dtype=torch.int64, device=dev)
    venc.take_into(vals8, order, a.rows[:vtotal], voffs)
    venc.device_status()
    a.assert_guard()
    assert np.array_equal(voffs.cpu().numpy(), vwant)
    want = _cumsum0(np.diff(sm)[order])
    total = int(want[-1])
    assert vtotal > H.X32 and total > H.X32
    out = _slack(dev, total)
    offs = torch.empty(len(order) + 1, dtype=torch.int64, device=dev)
    menc.join_map_into(keys, RowBatch(a.rows, voffs, len(order), 0), out.rows[:total], offs)
    menc.device_status()
    out.assert_guard()
    assert np.array_equal(offs.cpu().numpy(), want)
    _equal_rows(out.rows[:total], _cat_rows(small.rows, sm, order))


def across_2g(dev):
    """The narrowest batch whose rows pass 2^31 bytes: 40 rows of 64 and 48 MiB in turn (id INT64, a
    BINARY), two distinct ones, taken into a slack buffer; row 36 starts 32 MiB below 2^31.  For
    tests/test_select.py and tests/test_zip.py: (enc, the 2-row batch, the row order, the big batch,
    the slack buffer)."""
    from fury_amd import types as T
    from fury_amd.encoder import Encoders, RowBatch
    from fury_amd.workloads import Column
    enc = Encoders.bean([T.not_null_field("id", T.INT64), T.field("a", T.BINARY)], device=dev)
    g = torch.Generator(device=dev).manual_seed(41)
    ln = np.array([(64 << 20) + 3, (48 << 20) - 13], np.int64)
    cols = [Column(values=torch.tensor([7, -9], dtype=torch.int64, device=dev)),
            _binary_column(dev, ln, g)]
    src = enc.encode_batch(cols, 2)
    so = src.row_offsets.cpu().numpy()
    order = np.arange(40) % 2
    want = _cumsum0(np.diff(so)[order])
    total = int(want[-1])
    assert np.any((want[:-1] < H.X31 - (1 << 20)) & (want[1:] > H.X31 + (1 << 20)))
    a = _slack(dev, total)
    offs = torch.empty(len(order) + 1, dtype=torch.int64, device=dev)
    enc.take_into(src, order, a.rows[:total], offs)
    enc.device_status()
    assert np.array_equal(offs.cpu().numpy(), want)
    return enc, src, order, RowBatch(a.rows, offs, len(order), enc.schema_hash), a


def check_across_2g(dev, small, order, write):
    """`write(out_rows, out_offsets)` must produce torch.cat of the rows `order` of the batch `small`
    (the operator's output for the distinct rows) in a slack buffer, and nothing else."""
    sm = small.row_offsets.cpu().numpy()
    want = _cumsum0(np.diff(sm)[order])
    total = int(want[-1])
    assert np.any((want[:-1] < H.X31 - (1 << 20)) & (want[1:] > H.X31 + (1 << 20)))
    out = _slack(dev, total)
    offs = torch.empty(len(order) + 1, dtype=torch.int64, device=dev)
    write(out.rows[:total], offs)
    out.assert_guard()
    assert np.array_equal(offs.cpu().numpy(), want)
    _equal_rows(out.rows[:total], _cat_rows(small.rows, sm, order))
