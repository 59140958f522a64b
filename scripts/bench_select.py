"""Field selection (fury_row_select) against the only route from rows to narrower rows there was
before -- project_batch of the selected fields, then encode_batch with the selected encoder -- and
against fury_row_take of every row of the OUTPUT batch, the copy bound (not part of bench.py).

Cases, `--rows` rows each:
  struct100  10 of 100 fields, and 97 of 100 (fixed-width source: the no-scan kernel)
  mixed      a, s1, s3: one number and two of the three strings
  foo        f1, f5 of RowEncoderTest.Foo (a 4096-row pattern of row values, encoded once and repeated
             with take); project cannot read the struct f5, so this case has no compose leg
Per case these legs are timed in the same process:
  select   bind_select_fields into preallocated buffers: everything the call launches (measure, scan,
           write; one kernel for a fixed-width selection), no host synchronisation
  compose  project_batch (64 fields a call, its limit) + selected_encoder.encode_batch as a caller
           runs them today: allocations, the measure passes and their host reads included
  take     bind_take of rows 0 .. n-1 of the selected batch into preallocated buffers
Each timed call has its own pair of HIP events and follows a 512 MiB copy that empties the Infinity
Cache of the batch.  The legs are interleaved over `--rounds` rounds of `--iters` calls; the median
call of the median round is reported, with the fastest and slowest round beside it.  Before timing,
the bound call's output is checked byte for byte against the compose leg's batch (foo: against
select_fields of the pattern alone, repeated).

One JSON line per case: source and selected bytes, ms per leg, GBps = (bytes read + bytes written by
an ideal select: selected bytes twice) / time, and the ratios time of the yardstick / time of select
(compose_over_select > 1: select is faster; take_over_select: the fraction of the copy bound reached).

    python scripts/bench_select.py [--rows 1000000] [--legs select,take] [--out profiles/select_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PATTERN = 4096
LEGS = ("select", "compose", "take")


def foo_beans(n):
    return [{"f1": i, "f2": None if i % 3 == 0 else f"s{i}" * (i % 5),
             "f3": [f"x{j}" for j in range(i % 4)],
             "f4": [(f"k{j}", j) for j in range(i % 3)] if i % 5 else None,
             "f5": None if i % 7 == 0 else {"f1": i, "f2": "b" * (i % 11)}} for i in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--legs", default=",".join(LEGS), help="comma-separated subset of the legs")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    want_legs = [x for x in args.legs.split(",") if x]
    assert set(want_legs) <= set(LEGS), f"legs are {LEGS}"

    import torch
    assert torch.cuda.is_available(), "bench_select.py measures on the GPU; there is no fallback"
    from bench import make_device_columns
    from fury_amd import _native as N
    from fury_amd.beans import beans_to_columns
    from fury_amd.encoder import Encoders, column_to_device
    from fury_amd.workloads import SCHEMAS
    dev = torch.device("cuda:0")
    n = args.rows
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

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

    def foo_batch(enc):
        cols = [column_to_device(c, dev) for c in beans_to_columns(SCHEMAS["foo"], foo_beans(PATTERN))]
        pattern = enc.encode_batch(cols, PATTERN)
        return pattern, enc.take(pattern, torch.arange(n, device=dev) % PATTERN)

    s100 = [f.name for f in SCHEMAS["struct100"]]
    cases = [("struct100", "10_of_100", s100[3::10]),
             ("struct100", "97_of_100", [x for k, x in enumerate(s100) if k not in (10, 50, 90)]),
             ("mixed", "a_s1_s3", ["a", "s1", "s3"]),
             ("foo", "f1_f5", ["f1", "f5"])]
    batches = {}
    for name, case, sel in cases:
        fields = SCHEMAS[name]
        enc = Encoders.bean(fields, device=dev)
        if name not in batches:
            batches.clear()
            torch.cuda.empty_cache()
            batches[name] = (foo_batch(enc) if name == "foo" else
                             (None, enc.encode_batch(make_device_columns(name, fields, n, 0, dev), n)))
        pattern, batch = batches[name]
        child = enc.selected_encoder(sel)
        fixed = child.schema().is_fixed
        can_compose = name != "foo"

        def compose():                      # fury_row_project takes at most 64 fields per call
            cols = []
            for at in range(0, len(sel), 64):
                cols += enc.project_batch(batch, sel[at:at + 64])
            return child.encode_batch(cols, n)

        if can_compose:
            want = compose()
            want_rows, want_offs = want.rows, want.row_offsets
        else:                               # the pattern's selection, repeated like the rows
            p = enc.select_fields(pattern, sel)
            want = child.take(p, torch.arange(n, device=dev) % PATTERN)
            want_rows, want_offs = want.rows, want.row_offsets
        sel_bytes = want_rows.numel()
        out = torch.empty(max(sel_bytes, 16), dtype=torch.uint8, device=dev)
        offs = None if fixed else torch.empty(n + 1, dtype=torch.int64, device=dev)
        select = enc.bind_select_fields(batch, sel, out, offs)
        select()
        enc.device_status()
        assert torch.equal(out[:sel_bytes], want_rows), f"{name} {case}: selected rows differ"
        if not fixed:
            assert torch.equal(offs, want_offs), f"{name} {case}: offsets differ"
        tout = torch.empty_like(out)
        toffs = None if fixed else torch.empty(n + 1, dtype=torch.int64, device=dev)
        take = child.bind_take(want, torch.arange(n, device=dev), tout, toffs)
        legs = {"select": select, "compose": compose, "take": take}
        legs = {k: v for k, v in legs.items() if k in want_legs and (k != "compose" or can_compose)}
        rounds = timed(legs)
        enc.device_status()
        med = {k: statistics.median(v) for k, v in rounds.items()}
        line = {"workload": name, "rows": n, "case": case, "selected_fields": len(sel),
                "source_bytes": batch.rows.numel(), "selected_bytes": sel_bytes,
                **{f"{k}_ms": round(med[k], 4) for k in med},
                **{f"{k}_min_ms": round(min(rounds[k]), 4) for k in med},
                **{f"{k}_max_ms": round(max(rounds[k]), 4) for k in med}}
        if "select" in med:
            line["select_GBps"] = round(2 * sel_bytes / (med["select"] * 1e-3) / 1e9, 1)
            for k in ("compose", "take"):
                if k in med:
                    line[f"{k}_over_select"] = round(med[k] / med["select"], 3)
            if "compose" in med:
                line["no_slower_than_compose"] = med["select"] <= med["compose"]
        emit(line)
        del out, tout, want, want_rows, want_offs, select, take
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
