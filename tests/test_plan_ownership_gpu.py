"""The two-step decode's plan owns what it allocates: every way out of fury_decode_prepare /
fury_decode_host_prepare gives back each block of the workspace cache (tuning counter
"workspace_live") and each device error slot ("err_slots"), a live plan holds blocks until
fury_decode_plan_destroy, the tile BFS's retries and its fallback leak nothing, and the wide
execute launches with the geometry its prepare fixed.  Corrupt rows here have a slot that points
out of the batch: the kernels bounds-check it and raise the device error flag.  Marked gpu."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from fury_amd import types as T  # noqa: E402
from fury_amd.workloads import SCHEMAS  # noqa: E402
from tests.helpers import assert_columns_equal  # noqa: E402

OUT_OF_BOUNDS = 4                     # FURY_ERR_OUT_OF_BOUNDS
N_NESTED = 200                        # two 128-row count tiles, the last one partial
N_WIDE = 130                          # three 64-row tiles, the last one partial


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _lib():
    from fury_amd import _native as N
    return N.lib()


@pytest.fixture
def knobs():
    """Sets tuning knobs for the test and restores every one it touched afterwards."""
    L = _lib()
    old = {}

    def tune(key, v):
        old.setdefault(key, L.fury_get_tuning(key.encode()))
        assert L.fury_set_tuning(key.encode(), v) == 0, key
    try:
        yield tune
    finally:
        for k, v in old.items():
            assert L.fury_set_tuning(k.encode(), v) == 0, k


def _held():
    L = _lib()
    return L.fury_get_tuning(b"workspace_live"), L.fury_get_tuning(b"err_slots")


class _Case:
    """A batch of intact rows, the oracle's decode of it, and the same rows with one slot of a row
    of the last tile pointing out of the batch."""

    def __init__(self, oracle, fields, enc, rows, offs, n, first_bad_row):
        from tests.test_bounds import _corrupt, _is_null
        self.fields, self.enc, self.rows, self.offs, self.n = fields, enc, rows, offs, n
        self.ref = oracle.decode(fields, rows, offs, n)
        i, k = next((i, k) for i in range(first_bad_row, n) for k, f in enumerate(fields)
                    if f.type_id == T.STRING and not _is_null(fields, rows, offs, i, k))
        self.bad = _corrupt(fields, rows, offs, n, i, k, "offset_past_end")

    def batch(self, dev, bad=False):
        from tests.test_bounds import _batch
        return _batch(self.enc, self.bad if bad else self.rows, self.offs, self.n, dev)


@pytest.fixture(scope="module")
def nested(oracle, dev):
    from tests.test_bounds import _nested_batch
    fields = SCHEMAS["foo"]
    enc, rows, offs = _nested_batch(oracle, fields, N_NESTED, 9, dev)
    return _Case(oracle, fields, enc, rows, offs, N_NESTED, 128)


@pytest.fixture(scope="module")
def wide(oracle, dev):
    from tests.test_bounds import _encode
    from tests.test_device import _wide_fields
    fields = _wide_fields(33)
    enc, _, rows, offs = _encode(oracle, fields, N_WIDE, 33, dev, null_pct=10, str_max=40,
                                 list_max=8, list_null_pct=10, elem_null_pct=10)
    return _Case(oracle, fields, enc, rows, offs, N_WIDE, 128)


class _Plan:
    """fury_decode_prepare / _execute / _plan_destroy (host=True: the host-memory flavour) as
    separate steps, the way the encoder's decode strings them together."""

    def __init__(self, enc, rows, offs, n, host=False):
        from fury_amd import encoder as E
        L = _lib()
        self.enc, self.host = enc, host
        self.batch = (rows, offs)          # the plan reads them again in the execute
        h = enc._schema.handle
        nn = max(L.fury_schema_num_nodes(h), 1)
        self.entries, self.nbytes = (ctypes.c_int64 * nn)(), (ctypes.c_int64 * nn)()
        self.plan = ctypes.c_void_p()
        if host:
            self.status = L.fury_decode_host_prepare(h, E._hptr(rows), E._hptr(offs), n, self.entries,
                                                     self.nbytes, ctypes.byref(self.plan), 0)
        else:
            self.status = L.fury_decode_prepare(h, E._ptr(rows), E._ptr(offs), n, self.entries,
                                                self.nbytes, ctypes.byref(self.plan), 0)

    def execute(self):
        from fury_amd import encoder as E
        L = _lib()
        enc = self.enc
        order = E._bfs(enc._schema.fields)
        if self.host:
            cols = [E._alloc_host_node(f, int(self.entries[i]), int(self.nbytes[i]), np.zeros)
                    for i, (f, _) in enumerate(order)]
        else:
            cols = E._alloc_nodes(order, self.entries, self.nbytes, True, enc.device)
        for i, (f, first) in enumerate(order):
            if f.children:
                cols[i].child = [cols[first + j] for j in range(len(f.children))]
        top = cols[:len(enc._schema.fields)]
        keep: list = []
        if self.host:
            E._check(L.fury_decode_host_execute(self.plan, E._c_host_columns(top, keep)))
            return top
        E._check(L.fury_decode_execute(self.plan, E._c_columns(top, keep), 0, 0))
        enc.device_status()
        return [E.column_to_host(c) for c in top]

    def destroy(self):
        _lib().fury_decode_plan_destroy(self.plan)
        self.plan = ctypes.c_void_p()


def _prepare_fails_clean(case, dev, host=False):
    """A good decode first (the stream takes its error slot on its first launch), then the corrupt
    batch: the prepare reports the row and holds nothing afterwards."""
    good = _Plan(case.enc, *_args(case, dev, False, host), host=host)
    try:
        assert good.status == 0
        assert_columns_equal(case.fields, good.execute(), case.ref, case.n)
    finally:
        good.destroy()
    before = _held()
    bad = _Plan(case.enc, *_args(case, dev, True, host), host=host)
    try:
        assert bad.status == OUT_OF_BOUNDS
        assert not bad.plan
    finally:
        bad.destroy()
    assert _held() == before


def _args(case, dev, bad, host):
    if host:
        return (case.bad if bad else case.rows), case.offs, case.n
    b = case.batch(dev, bad)
    return b.rows, b.row_offsets, case.n


# 1. every prepare error path gives everything back -----------------------------------------------
@pytest.mark.parametrize("engine", [1, 2, 4])
def test_nested_prepare_error_gives_everything_back(nested, dev, knobs, engine):
    knobs("nested_decode", engine)
    _prepare_fails_clean(nested, dev)


@pytest.mark.parametrize("engine", [1, 2])
def test_wide_prepare_error_gives_everything_back(wide, dev, knobs, engine):
    knobs("wide_engine", engine)
    _prepare_fails_clean(wide, dev)


def test_host_prepare_error_gives_everything_back(nested, dev, knobs):
    """The host flavour: the private stream's error slot is released and the staged rows go back."""
    knobs("nested_decode", 2)
    _prepare_fails_clean(nested, dev, host=True)


# 2. the success path: a live plan holds blocks, a destroyed one none -----------------------------
@pytest.mark.parametrize("which,host", [("nested", False), ("nested", True), ("wide", False)],
                         ids=["nested-device", "nested-host", "wide-device"])
def test_plan_holds_blocks_until_destroyed(nested, wide, dev, which, host):
    case = nested if which == "nested" else wide
    _Plan(case.enc, *_args(case, dev, False, host), host=host).destroy()      # (warm: as above)
    live0, slots0 = _held()
    p = _Plan(case.enc, *_args(case, dev, False, host), host=host)
    try:
        assert p.status == 0
        assert _held()[0] > live0
        assert_columns_equal(case.fields, p.execute(), case.ref, case.n)
        assert _held()[0] > live0
    finally:
        p.destroy()
    assert _held() == (live0, slots0)


# 3. the tile BFS's retries and its fallback ------------------------------------------------------
def test_bfs_fallback_leaks_nothing(oracle, dev, knobs):
    """The arena leg of tests/test_tree.py (nested7, 128-row tiles, a 1 KB arena): every attempt
    overflows, cnt / byt are given back and taken again per attempt, the row walk decodes."""
    from fury_amd.beans import beans_to_columns
    from fury_amd.encoder import Encoders
    from tests.test_device import _nested_fields
    from tests.test_tree import _beans
    L = _lib()
    fields = _nested_fields()
    n = 2999
    host = beans_to_columns(fields, _beans(fields, n, len("nested7") * 31))
    enc = Encoders.bean(fields, device=dev)
    rows, offs = oracle.encode(fields, host, n)
    offs = np.asarray(offs, np.int64)
    t_rows, t_offs = torch.from_numpy(rows).to(dev), torch.from_numpy(offs).to(dev)
    for k, v in (("nested_decode", 4), ("bfs_threads", 128), ("bfs_rows", 128), ("bfs_stage", 0),
                 ("bfs_arena", 1024)):
        knobs(k, v)
    _Plan(enc, t_rows, t_offs, n).destroy()
    before = _held()
    fallbacks = L.fury_get_tuning(b"bfs_fallbacks")
    p = _Plan(enc, t_rows, t_offs, n)
    try:
        assert p.status == 0
        assert L.fury_get_tuning(b"bfs_fallbacks") == fallbacks + 1
        assert_columns_equal(fields, p.execute(), oracle.decode(fields, rows, offs, n), n)
    finally:
        p.destroy()
    assert _held() == before


# 4. the wide execute launches with the prepare's geometry ----------------------------------------
@pytest.mark.parametrize("prepared,executed", [(256, 512), (512, 256)])
def test_wide_execute_uses_the_prepared_geometry(wide, dev, knobs, prepared, executed):
    """A plan prepared under one wide_threads setting and executed under another decodes to the
    oracle's columns.  This pins the outputs, not which thread count the execute launched with:
    the kept tile bases do not depend on the thread count, so an execute that read the knob again
    would pass too (as it did before the plan kept its geometry)."""
    knobs("wide_engine", 1)
    knobs("wide_threads", prepared)
    b = wide.batch(dev)
    p = _Plan(wide.enc, b.rows, b.row_offsets, wide.n)
    try:
        assert p.status == 0
        knobs("wide_threads", executed)
        assert_columns_equal(wide.fields, p.execute(), wide.ref, wide.n)
    finally:
        p.destroy()
