"""The high-offset matrix of tests/high_offsets.py is well-formed and complete.  Host only: every
placement, computed from the oracle's offsets, has the relation to 2^31 / 2^32 it is named for and
fits the arena; the dense shapes pass 2^32 bytes while every Arrow column stays inside int32; and
every public method that takes a RowBatch resolves to an adapter of CONSUMERS or to a reason in
EXEMPT, so an operator added without a high-offset leg fails the suite."""
from __future__ import annotations

import inspect

import numpy as np
import pytest

from tests import high_offsets as H


@pytest.mark.parametrize("schema", list(H.SCHEMAS))
def test_placements_hit_their_edges(oracle, schema):
    ref = H.ref(oracle, schema)
    offs, n = ref.offs, ref.n
    m = n // 2
    total = int(offs[n])
    assert n == H.N and len(offs) == n + 1 and int(offs[0]) == 0 and total == ref.rows.size
    assert not np.any(offs % 8), "row extents are 8-aligned"
    for x, X in H.BOUNDARIES.items():
        for p in H.PLACEMENTS:
            B = H.case_base(f"{p}-{x}", offs)
            pos = offs + B
            assert B % 8 == 0 and B >= 0, (p, x, B)
            assert B + total <= H.VIEW_BYTES, (p, x)
            if p == "ends_at":
                assert int(pos[n]) == X and (int(pos[n]) & 0xFFFFFFFF) in (0, H.X31)
            elif p == "starts_at":
                assert int(pos[0]) == X
            elif p == "row_starts_at":
                assert int(pos[m]) == X
            else:
                assert int(pos[m]) < X < int(pos[m + 1]) and (X - int(pos[m])) % 8 == 0
            if p in H.STRADDLING:      # at least 100 rows wholly on each side
                assert int(np.sum(pos[1:] <= X)) >= 100 and int(np.sum(pos[:-1] >= X)) >= 100
    mis = H.base("inside_row", H.X32, offs) % 16 == 8
    assert mis == (schema in H.MISALIGNED16), "tests/high_offsets.py MISALIGNED16 is out of date"


def test_a_16_byte_load_path_meets_a_misaligned_source():
    assert H.MISALIGNED16, "no schema's inside_row base is 8 (mod 16): pick another seed"
    assert set(H.MISALIGNED16) <= set(H.SCHEMAS)


def test_arena_and_case_tables():
    assert H.ARENA_BYTES == (1 << 31) + (1 << 32) + (64 << 20) and H.SLACK == 1 << 31
    assert len(H.CASES) == 8 == len(set(H.CASES))
    for case in H.CASES:
        others = H.other_cases(case)
        assert len(others) == 7 and case not in others
        assert not others[0].endswith(case.rsplit("-", 1)[1])     # the other boundary first
    for table in (H.DECODE_KNOBS, H.ENCODE_KNOBS, H.SPEC):
        assert set(table) == set(H.SCHEMAS)
    for name, cons in H.CONSUMERS.items():
        assert any(cons.applies(s) for s in H.SCHEMAS), name
    assert "negative_offset" not in H.MALFORMED
    assert len(H.malformed_cases()) >= 6


def test_knob_legs_are_legal():
    from fury_amd import _native as N
    from tests.test_tuning import KNOBS
    L = N.lib()
    for table in (H.DECODE_KNOBS, H.ENCODE_KNOBS):
        for legs in table.values():
            for leg in legs:
                if leg is None:
                    continue
                key = leg[0].encode()
                assert leg[0] in KNOBS
                old = L.fury_get_tuning(key)
                try:
                    assert L.fury_set_tuning(key, leg[1]) == 0, (leg, N.last_error())
                finally:
                    assert L.fury_set_tuning(key, old) == 0


# ---- the dense shapes, from the row-layout formula alone ---------------------------------------------
@pytest.mark.parametrize("leg", ["D1", "D2", "D3", "D4", "D5", "D6"])
def test_dense_shapes(leg):
    s = H.dense_shapes()[leg]
    assert s["batch"] > H.X32, "the produced bytes must pass 2^32"
    for nbytes in s["columns"]:           # Arrow offsets are int32
        assert nbytes <= H.INT32_MAX
    for nbytes in s["rows"]:
        assert nbytes <= H.INT32_MAX - 7
    assert s["live"] <= H.LIVE_LIMIT


def test_long_rows_layout():
    ln = H.long_lengths()
    assert ln.shape == (H.LONG_ROWS, 3) and 1400 <= H.LONG_ROWS <= 1500
    live = ln[ln >= 0]
    assert abs(int(live.mean()) - (1 << 20)) < (1 << 18)           # about 1 MiB each
    assert np.any(ln[:, 0] % 8) and not np.any(ln[:, 1][ln[:, 1] >= 0] % 8)
    assert 0 < np.sum(ln < 0) < ln.size // 5
    rb = H.long_row_bytes(ln)
    assert not np.any(rb % 8)
    ends = np.cumsum(rb)
    assert ends[-1] > H.X32
    for X in (H.X31, H.X32):              # one row straddles each boundary
        r = int(np.searchsorted(ends, X, side="right"))
        assert ends[r] - rb[r] < X < ends[r]
    assert len(set(rb[:H.LONG_DISTINCT])) == H.LONG_DISTINCT


# ---- the coverage gate ------------------------------------------------------------------------------
def _row_batch_methods():
    """name -> classes: every public method of the encoders (and ArrowWriter) whose signature takes
    a RowBatch or a sequence of them."""
    from fury_amd import encoder as E
    found: dict = {}
    for cls in (E.RowEncoder, E.ArrayEncoder, E.MapEncoder, E.ArrowWriter):
        for name, fn in inspect.getmembers(cls, inspect.isfunction):
            if name.startswith("_"):
                continue
            params = inspect.signature(fn).parameters.values()
            if any("RowBatch" in str(p.annotation) for p in params):
                found.setdefault(name, []).append(cls.__name__)
    return found


def check_coverage(consumers, resolves, exempt):
    found = _row_batch_methods()
    assert len(found) >= 50, sorted(found)          # the enumeration itself works
    for name in sorted(found):
        if name in exempt:
            assert name not in resolves, f"{name}: both exempt and resolved"
            continue
        assert name in resolves, (f"{name} ({', '.join(found[name])}) takes a RowBatch and has neither "
                                  "a high-offset adapter nor an EXEMPT reason in tests/high_offsets.py")
        assert resolves[name] in consumers, (f"{name} resolves to {resolves[name]!r}, which is not in "
                                             "CONSUMERS")
    from fury_amd import encoder as E
    for name in list(resolves) + list(exempt):
        assert any(callable(getattr(c, name, None))
                   for c in (E.RowEncoder, E.ArrayEncoder, E.MapEncoder, E.ArrowWriter)), name
    unused = set(consumers) - set(resolves.values()) - {"rows_to_arrow", "encode_into"}
    assert not unused, f"no public method resolves to {sorted(unused)}"
    assert all(isinstance(why, str) and len(why) > 10 for why in exempt.values())


def test_every_row_batch_method_has_a_high_offset_leg():
    check_coverage(H.CONSUMERS, H.RESOLVES, H.EXEMPT)
    for name in ("frame", "unframe", "decode_host"):
        assert name in H.EXEMPT


def test_the_gate_notices_a_missing_consumer():
    for name in ("take", "join_map", "update_fields"):
        fewer = {k: v for k, v in H.CONSUMERS.items() if k != name}
        with pytest.raises(AssertionError, match="not in CONSUMERS"):
            check_coverage(fewer, H.RESOLVES, H.EXEMPT)
    with pytest.raises(AssertionError, match="neither"):
        check_coverage(H.CONSUMERS, {k: v for k, v in H.RESOLVES.items() if k != "bind_take"},
                       H.EXEMPT)
