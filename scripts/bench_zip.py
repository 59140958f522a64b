"""Zip (fury_row_zip) against the only route from several row batches to one there was before --
project_batch of every source, then encode_batch with the zipped encoder -- and against fury_row_take
of every row of the OUTPUT batch, the copy bound (not part of bench.py).

Cases, `--rows` rows each:
  struct100  split into fields 0..49 and 50..99 and zipped back (no variable-length pick: the no-scan
             kernel); the output is the source batch
  mixed      with_fields: `mixed` zipped with a batch of one STRING field named s2 (mixed's own s1
             column encoded alone), which takes s2's place
  foo        every field of RowEncoderTest.Foo (a 4096-row pattern of row values, encoded once and
             repeated with take) followed by ten fields of struct100; project cannot read foo's
             nested fields, so this case has no compose leg
Per case these legs are timed in the same process:
  zip      bind_zip_fields into preallocated buffers: everything the call launches (measure, scan,
           write; one kernel for fixed-width picks), no host synchronisation
  compose  project_batch of every source (64 fields a call, its limit) + zipped_encoder.encode_batch as
           a caller runs them today: allocations, the measure passes and their host reads included
  take     bind_take of rows 0 .. n-1 of the zipped batch into preallocated buffers
Each timed call has its own pair of HIP events and follows a 512 MiB copy that empties the Infinity
Cache of the batches.  The legs are interleaved over `--rounds` rounds of `--iters` calls; the median
call of the median round is reported, with the fastest and slowest round beside it.  Before timing,
the bound call's output is checked byte for byte against the compose leg's batch (struct100: also
against the source batch; foo: select_fields of the output gives back the bytes of either source).

One JSON line per case: source and zipped bytes, ms per leg, GBps = (bytes read + bytes written by an
ideal zip: zipped bytes twice) / time, the ratios time of the yardstick / time of zip
(compose_over_zip > 1: zip is faster; take_over_zip: the fraction of the copy bound reached), and
zip_max_le_compose_min: the slowest zip round against the fastest compose round.

    python scripts/bench_zip.py [--rows 1000000] [--legs zip,take] [--out profiles/zip_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PATTERN = 4096
LEGS = ("zip", "compose", "take")


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
    ap.add_argument("--cases", default="struct100,mixed,foo", help="comma-separated subset of the cases")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    want_legs = [x for x in args.legs.split(",") if x]
    assert set(want_legs) <= set(LEGS), f"legs are {LEGS}"

    import torch
    assert torch.cuda.is_available(), "bench_zip.py measures on the GPU; there is no fallback"
    from bench import make_device_columns
    from fury_amd import _native as N
    from fury_amd import types as T
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

    def encoded(name):
        fields = SCHEMAS[name]
        enc = Encoders.bean(fields, device=dev)
        return enc, enc.encode_batch(make_device_columns(name, fields, n, 0, dev), n)

    def struct100_case():
        enc, batch = encoded("struct100")
        s1, s2 = list(range(50)), list(range(50, 100))
        srcs = [(enc.selected_encoder(s1), enc.select_fields(batch, s1)),
                (enc.selected_encoder(s2), enc.select_fields(batch, s2))]
        picks = [(0, k) for k in range(50)] + [(1, k) for k in range(50)]

        def check(out, offs):
            assert torch.equal(out, batch.rows), "struct100: the halves zipped back differ from the source"
        return "halves_rezipped", srcs, picks, True, check

    def mixed_case():
        enc, batch = encoded("mixed")
        other = Encoders.bean([T.field("s2", T.STRING)], device=dev)
        ob = other.encode_batch(enc.project_batch(batch, ["s1"]), n)
        return "with_fields_s2", [(enc, batch), (other, ob)], enc._with_fields_picks(other), True, None

    def foo_case():
        foo = Encoders.bean(SCHEMAS["foo"], device=dev)
        cols = [column_to_device(c, dev) for c in beans_to_columns(SCHEMAS["foo"], foo_beans(PATTERN))]
        fb = foo.take(foo.encode_batch(cols, PATTERN), torch.arange(n, device=dev) % PATTERN)
        enc, batch = encoded("struct100")
        ten = list(range(3, 100, 10))
        tb = enc.select_fields(batch, ten)
        del batch
        picks = [(0, k) for k in range(5)] + [(1, k) for k in range(10)]

        def check(out, offs):               # either source's fields, selected back out of the output
            z = foo.zipped_encoder([enc.selected_encoder(ten)], picks)
            from fury_amd.encoder import RowBatch
            zb = RowBatch(out, offs, n, z.schema_hash)
            back = z.select_fields(zb, list(range(5)))
            assert torch.equal(back.rows, fb.rows) and torch.equal(back.row_offsets, fb.row_offsets), \
                "foo: the foo fields of the zipped rows differ from the source"
            assert torch.equal(z.select_fields(zb, list(range(5, 15))).rows, tb.rows), \
                "foo: the struct100 fields of the zipped rows differ from the source"
        return "foo_plus_ten", [(foo, fb), (enc.selected_encoder(ten), tb)], picks, False, check

    builders = {"struct100": struct100_case, "mixed": mixed_case, "foo": foo_case}
    for name in [x for x in args.cases.split(",") if x]:
        torch.cuda.empty_cache()
        case, srcs, picks, can_compose, check = builders[name]()
        enc0, batch0 = srcs[0]
        others = srcs[1:]
        zenc = enc0.zipped_encoder([e for e, _ in others], picks)
        fixed = zenc.schema().is_fixed

        def compose():                      # fury_row_project takes at most 64 fields per call
            col = {}
            for s, (e, b) in enumerate(srcs):
                slots = [k for src, k in picks if src == s]
                for at in range(0, len(slots), 64):
                    got = e.project_batch(b, slots[at:at + 64])
                    col.update({(s, k): c for k, c in zip(slots[at:at + 64], got)})
            return zenc.encode_batch([col[p] for p in picks], n)

        want = compose() if can_compose else enc0.zip_fields(batch0, others, picks)
        zip_bytes = want.rows.numel()
        out = torch.empty(max(zip_bytes, 16), dtype=torch.uint8, device=dev)
        offs = None if fixed else torch.empty(n + 1, dtype=torch.int64, device=dev)
        zp = enc0.bind_zip_fields(batch0, others, picks, out, offs)
        zp()
        enc0.device_status()
        if can_compose:
            assert torch.equal(out[:zip_bytes], want.rows), f"{name} {case}: zipped rows differ"
            if not fixed:
                assert torch.equal(offs, want.row_offsets), f"{name} {case}: offsets differ"
        if check:
            check(out[:zip_bytes], offs)
        tout = torch.empty_like(out)
        toffs = None if fixed else torch.empty(n + 1, dtype=torch.int64, device=dev)
        take = zenc.bind_take(want, torch.arange(n, device=dev), tout, toffs)
        legs = {"zip": zp, "compose": compose, "take": take}
        legs = {k: v for k, v in legs.items() if k in want_legs and (k != "compose" or can_compose)}
        rounds = timed(legs)
        enc0.device_status()
        med = {k: statistics.median(v) for k, v in rounds.items()}
        line = {"workload": name, "rows": n, "case": case, "sources": len(srcs), "picks": len(picks),
                "source_bytes": [b.rows.numel() for _, b in srcs], "zipped_bytes": zip_bytes,
                "compose": "timed" if "compose" in med else
                           ("no such route: project cannot read nested fields" if not can_compose
                            else "not timed"),
                **{f"{k}_ms": round(med[k], 4) for k in med},
                **{f"{k}_min_ms": round(min(rounds[k]), 4) for k in med},
                **{f"{k}_max_ms": round(max(rounds[k]), 4) for k in med}}
        if "zip" in med:
            line["zip_GBps"] = round(2 * zip_bytes / (med["zip"] * 1e-3) / 1e9, 1)
            for k in ("compose", "take"):
                if k in med:
                    line[f"{k}_over_zip"] = round(med[k] / med["zip"], 3)
            if "compose" in med:
                line["zip_max_le_compose_min"] = max(rounds["zip"]) <= min(rounds["compose"])
        emit(line)
        del out, tout, want, zp, take, srcs, batch0, others, check, compose, legs
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
