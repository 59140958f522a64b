"""Implode and wrap (fury_row_implode / fury_row_wrap) against the only route from element rows back
to list rows there was before -- decode_batch of the elements, then encode_batch under the one-field
list schema -- and against fury_hbm_copy of the same output bytes, the copy bound (not part of
bench.py).

The batch: `--rows` rows of the explode test schema (id INT64, items LIST<STRUCT{a INT32, s STRING}>,
m MAP<INT32, STRUCT{x INT64, y STRING}>, ll LIST<LIST<INT32>>, fx LIST<STRUCT{p INT64, q INT32}>), a
4096-row pattern of row values encoded once and repeated with take.  `items` is null in one row of 11,
holds 0 .. 12 elements, and has no null element: the compact element columns a decode returns are then
the list's child columns as they are, so the compose leg needs no scatter of its own.
Legs, timed in the same process:
  implode  bind_implode of explode's `items` elements into preallocated buffers, rows form: everything
           the call launches (rank, elems, rows, the scans, write), no host synchronisation
  wrap     bind_wrap of extract's `items` arrays into preallocated buffers
  compose  element_encoder.decode_batch of the elements + field_encoder.encode_batch of the list column
           as a caller runs them today: allocations, the measure passes and their host reads included
  copy     fury_hbm_copy of as many bytes as the output has (rounded down to its 16 KB unit)
Each timed call has its own pair of HIP events and follows a 512 MiB copy that empties the Infinity
Cache of the batches.  The legs are interleaved over `--rounds` rounds of `--iters` calls; the median
call of the median round is reported, with the fastest and slowest round beside it.  Before timing,
the outputs of implode, wrap and compose are checked byte for byte against select_fields of the
source batch.

One JSON line: element and output bytes, ms per leg, GBps = (output bytes read + written by an ideal
implode: twice) / time, and the ratios time of the yardstick / time of implode (compose_over_implode >
1: implode is faster; copy_over_implode: the fraction of the copy bound reached).

    python scripts/bench_implode.py [--rows 1000000] [--out profiles/implode_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PATTERN = 4096
LEGS = ("implode", "wrap", "compose", "copy")


def explode_fields():
    from fury_amd import types as T
    item = T.struct_field("item", [T.field("a", T.INT32), T.field("s", T.STRING)])
    val = T.struct_field("value", [T.field("x", T.INT64), T.field("y", T.STRING)])
    fxi = T.struct_field("item", [T.field("p", T.INT64), T.field("q", T.INT32)])
    return [T.field("id", T.INT64), T.Field("items", T.LIST, True, (item,)),
            T.map_field("m", T.field("key", T.INT32), val),
            T.Field("ll", T.LIST, True, (T.array_field("item", T.INT32),)),
            T.Field("fx", T.LIST, True, (fxi,))]


def beans(n):
    return [{"id": i,
             "items": None if i % 11 == 3 else [{"a": i * 131 + j, "s": None if j % 5 == 0 else "s" * (j % 7)}
                                                for j in range(i % 13)],
             "m": [(j, {"x": i + j, "y": "y" * (j % 9)}) for j in range(i % 3)],
             "ll": [[i + j + k for k in range(j % 4)] for j in range(i % 5)],
             "fx": [{"p": i - j, "q": j} for j in range(i % 4)]} for i in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--legs", default=",".join(LEGS), help="comma-separated subset of the legs")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    want_legs = [x for x in args.legs.split(",") if x]
    assert set(want_legs) <= set(LEGS), f"legs are {LEGS}"

    import torch
    assert torch.cuda.is_available(), "bench_implode.py measures on the GPU; there is no fallback"
    from fury_amd import _native as N
    from fury_amd.beans import beans_to_columns
    from fury_amd.encoder import Encoders, column_to_device
    from fury_amd.workloads import Column
    dev = torch.device("cuda:0")
    n = args.rows

    fsrc = torch.zeros(512 << 20, dtype=torch.uint8, device=dev)
    fdst = torch.empty_like(fsrc)

    def flush():
        assert N.lib().fury_hbm_copy(fdst.data_ptr(), fsrc.data_ptr(), fsrc.numel(), None) == 0

    def timed(legs):
        """Median call of every round per leg, the legs interleaved."""
        rounds = {name: [] for name in legs}
        for call in legs.values():
            call()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for name, call in legs.items():
                ev = []
                for _ in range(args.iters):
                    flush()
                    a = torch.cuda.Event(enable_timing=True)
                    b = torch.cuda.Event(enable_timing=True)
                    a.record()
                    call()
                    b.record()
                    ev.append((a, b))
                torch.cuda.synchronize()
                rounds[name].append(statistics.median(a.elapsed_time(b) for a, b in ev))
        return rounds

    fields = explode_fields()
    enc = Encoders.bean(fields, device=dev)
    cols = [column_to_device(c, dev) for c in beans_to_columns(fields, beans(PATTERN))]
    batch = enc.take(enc.encode_batch(cols, PATTERN), torch.arange(n, device=dev) % PATTERN)
    del cols
    target = enc.field_encoder("items")
    child = enc.element_encoder("items")
    want = enc.select_fields(batch, ["items"])
    elems, lo, ev, valid, _, _ = enc.explode(batch, "items")
    arrays, avalid = enc.extract(batch, "items")
    E = int(lo[n].item())
    assert elems.nrows == E, "the bench batch has no null elements"
    del batch
    torch.cuda.empty_cache()
    out_bytes = want.rows.numel()

    out = torch.empty(max(out_bytes, 16), dtype=torch.uint8, device=dev)
    offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
    implode = target.bind_implode(elems, lo, out, offs, ev, valid, E)
    implode()
    target.device_status()
    assert torch.equal(out[:out_bytes], want.rows) and torch.equal(offs, want.row_offsets), \
        "implode(explode) differs from select_fields"
    wout = torch.empty_like(out)
    woffs = torch.empty_like(offs)
    wrap = target.bind_wrap(arrays, wout, woffs, avalid, n)
    wrap()
    target.device_status()
    assert torch.equal(wout[:out_bytes], want.rows) and torch.equal(woffs, want.row_offsets), \
        "wrap(extract) differs from select_fields"

    def compose():
        kids = child.decode_batch(elems)
        col = Column(validity=ev, offsets=lo.to(torch.int32),
                     child=[Column(child=kids)])
        return target.encode_batch([col], n)

    got = compose()
    assert torch.equal(got.rows, want.rows) and torch.equal(got.row_offsets, want.row_offsets), \
        "decode + encode differs from select_fields"
    del got
    cdst = torch.empty_like(out)
    copy_bytes = out_bytes & ~0x3FFF           # fury_hbm_copy takes multiples of 16 KB
    assert copy_bytes > 0, "too few rows for the copy leg"

    def copy():
        assert N.lib().fury_hbm_copy(cdst.data_ptr(), out.data_ptr(), copy_bytes, None) == 0

    legs = {"implode": implode, "wrap": wrap, "compose": compose, "copy": copy}
    legs = {k: v for k, v in legs.items() if k in want_legs}
    rounds = timed(legs)
    target.device_status()
    med = {k: statistics.median(v) for k, v in rounds.items()}
    line = {"workload": "explode_fields", "rows": n, "field": "items", "elements": E,
            "element_bytes": elems.rows.numel(), "array_bytes": arrays.rows.numel(),
            "output_bytes": out_bytes,
            **{f"{k}_ms": round(med[k], 4) for k in med},
            **{f"{k}_min_ms": round(min(rounds[k]), 4) for k in med},
            **{f"{k}_max_ms": round(max(rounds[k]), 4) for k in med}}
    for k in ("implode", "wrap", "copy"):
        if k in med:
            line[f"{k}_GBps"] = round(2 * out_bytes / (med[k] * 1e-3) / 1e9, 1)
    if "implode" in med:
        for k in ("compose", "copy", "wrap"):
            if k in med:
                line[f"{k}_over_implode"] = round(med[k] / med["implode"], 3)
        if "compose" in med:
            line["implode_max_le_compose_min"] = max(rounds["implode"]) <= min(rounds["compose"])
    s = json.dumps(line)
    print(s, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
