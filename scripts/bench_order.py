"""The order of rows (fury_row_compare, fury_row_order_words, argsort_rows) against the routes there
were before it: milliseconds, rows per second and bytes touched per call (not part of bench.py).

Batches of `--rows` rows, no nulls, keys drawn uniformly from `--distinct` values:
  int64          Struct-100 (816-byte rows) ordered by its first field, an INT64
  int32_int32    (a INT32, b INT32, pad INT64) ordered by (a, b), a from 1000 values
  string8 / string24 / string200
                 (id INT64, k STRING) ordered by k, a STRING of that many bytes whose first 12 are the
                 key number's digits and the rest random
  string24_int64 (k STRING of 24 bytes, v INT64) ordered by (k, v), k from 1000 values
Legs:
  compare        bind_compare of row j against row perm[j] (indices on the right side) into a
                 preallocated int8 tensor; no host synchronisation
  order_words    order_words_into of chunk 0 of the first key, no indices, with out_more
  argsort        argsort_rows: the refinement rounds, their torch sorts and host synchronisations
  project_sort   int64: bind_project of the key into a preallocated column, then
                 torch.sort(stable=True); int32_int32: both keys projected, a stable sort by b, then a
                 stable sort by a of the result.  The only device routes before this operator; the
                 string cases have none.
Each timed call has its own pair of HIP events and follows a 512 MiB copy that empties the Infinity
Cache of the batch.  The legs are interleaved over `--rounds` rounds of `--iters` calls; the median call
of the median round is reported, with the fastest and slowest round beside it.  Before timing, the
argsort permutation is checked: against project_sort's where that exists, else through is_sorted of
the sorted batch and a stable-order check of equal neighbours.

One JSON line per case: compare_bytes / words_bytes = the bytes the kernel must touch (per row and
side: the index if any, the row offset of a variable-length schema, one bitmap word and one slot per
key, the payload of STRING keys up to the first difference -- counted in full -- and the output),
GBps of each against its milliseconds, argsort_rounds = the order_words calls one argsort made, and
argsort's ratio to project_sort where that exists.

    python scripts/bench_order.py [--rows 1000000] [--out profiles/order_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

CASES = ["int64", "int32_int32", "string8", "string24", "string200", "string24_int64"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000])
    ap.add_argument("--distinct", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--cases", nargs="+", default=CASES)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "bench_order.py measures on the GPU; there is no fallback"
    import fury_amd.order as O
    from bench import make_device_columns
    from fury_amd import KeySide
    from fury_amd import _native as N
    from fury_amd import types as T
    from fury_amd.encoder import Encoders
    from fury_amd.workloads import SCHEMAS, Column
    dev = torch.device("cuda:0")
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
        """Median call of every round per leg, the legs interleaved.  legs: name -> (call, iters)."""
        rounds = {name: [] for name in legs}
        for call, _ in legs.values():
            call()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for name, (call, iters) in legs.items():
                ev = []
                for _ in range(iters):
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

    def digits12(kid):
        p = 10 ** torch.arange(11, -1, -1, device=dev, dtype=torch.int64)
        return ((kid.unsqueeze(1) // p) % 10 + 48).to(torch.uint8)

    def strings(kid, distinct, width, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        table = torch.randint(0, 256, (distinct, max(width, 12)), dtype=torch.uint8, device=dev, generator=g)
        table[:, :12] = digits12(torch.arange(distinct, device=dev))
        table = table[:, 12 - min(width, 12):][:, :width] if width < 12 else table
        n = kid.numel()
        return Column(values=table[kid].reshape(-1).contiguous(),
                      offsets=(torch.arange(n + 1, dtype=torch.int64, device=dev) * width).to(torch.int32))

    def columns(case, n, g):
        """(fields, device columns, keys, STRING payload bytes per row)."""
        kid = torch.randint(0, args.distinct, (n,), device=dev, generator=g)
        if case == "int64":
            fields = SCHEMAS["struct100"]
            cols = make_device_columns("struct100", fields, n, 0, dev)
            cols[0] = Column(values=kid * -7046029254386353131 + 1)
            return fields, cols, [0], 0
        if case == "int32_int32":
            fields = [T.not_null_field("a", T.INT32), T.not_null_field("b", T.INT32), T.not_null_field("pad", T.INT64)]
            cols = [Column(values=(kid % 1000).to(torch.int32)), Column(values=(kid * 2654435761 % 2 ** 31).to(torch.int32)),
                    Column(values=torch.arange(n, dtype=torch.int64, device=dev))]
            return fields, cols, ["a", "b"], 0
        if case == "string24_int64":
            fields = [T.field("k", T.STRING), T.not_null_field("v", T.INT64)]
            cols = [strings(kid % 1000, 1000, 24, 24), Column(values=kid * -7046029254386353131 + 1)]
            return fields, cols, ["k", "v"], 24
        width = int(case[len("string"):])
        fields = [T.not_null_field("id", T.INT64), T.field("k", T.STRING)]
        cols = [Column(values=torch.arange(n, dtype=torch.int64, device=dev)), strings(kid, args.distinct, width, width)]
        return fields, cols, ["k"], width

    for case in args.cases:
        for n in args.rows:
            g = torch.Generator(device=dev).manual_seed(n)
            fields, cols, keys, payload = columns(case, n, g)
            enc = Encoders.bean(fields, device=dev)
            sch = enc.schema()
            batch = enc.encode_batch(cols, n)
            del cols
            perm = torch.randperm(n, device=dev, generator=g)
            cmp = torch.empty(n, dtype=torch.int8, device=dev)
            words = torch.empty(n, dtype=torch.int64, device=dev)
            more = torch.empty(1, dtype=torch.int32, device=dev)
            compare = O.bind_compare(KeySide(enc, batch, keys), KeySide(enc, batch, keys, perm), cmp)

            def order_words():
                O.order_words_into(enc, batch, keys[0], 0, words, more)

            def argsort():
                return O.argsort_rows(enc, batch, keys)
            legs = {"compare": (compare, args.iters), "order_words": (order_words, args.iters),
                    "argsort": (argsort, args.iters)}
            # one argsort, its rounds counted, and the check of its permutation
            calls = [0]
            inner = O.order_words_into

            def counting(*a, **k):
                calls[0] += 1
                return inner(*a, **k)
            O.order_words_into = counting
            got = argsort()
            O.order_words_into = inner
            if case in ("int64", "int32_int32"):
                col = enc.project_batch(batch, keys)
                proj = enc.bind_project(batch, keys, col)
                views = [c.values.view(torch.int64 if case == "int64" else torch.int32) for c in col]

                def project_sort():
                    proj()
                    order = torch.sort(views[-1], stable=True).indices
                    for v in reversed(views[:-1]):
                        order = order[torch.sort(v[order], stable=True).indices]
                    return order
                assert torch.equal(project_sort(), got), "argsort_rows is not project + stable sort"
                legs["project_sort"] = (project_sort, args.iters)
            else:
                srt = enc.take(batch, got)
                assert O.is_sorted(enc, srt, keys), "the sorted batch is not sorted"
                at = torch.arange(n - 1, device=dev)
                tie = O.compare_rows(KeySide(enc, srt, keys, at), KeySide(enc, srt, keys, at + 1)) == 0
                assert bool((got[:-1][tie] < got[1:][tie]).all()), "equal rows left their source order"
                del srt, at, tie
            rounds = timed(legs)
            enc.device_status()
            med = {k: statistics.median(v) for k, v in rounds.items()}
            var = 0 if sch.is_fixed else 8
            compare_bytes = n * (2 * (var + 16 * len(keys) + payload) + 8 + 1)
            words_bytes = n * (var + 16 + min(payload, 16) + 8)
            line = {"case": case, "rows": n, "distinct": args.distinct, "keys": len(keys),
                    "row_bytes": batch.rows.numel(), "compare_bytes": compare_bytes, "words_bytes": words_bytes,
                    "argsort_rounds": calls[0]}
            for k in med:
                line[f"{k}_ms"] = round(med[k], 4)
                line[f"{k}_min_ms"] = round(min(rounds[k]), 4)
                line[f"{k}_max_ms"] = round(max(rounds[k]), 4)
            line["compare_GBps"] = round(compare_bytes / (med["compare"] * 1e-3) / 1e9, 1)
            line["order_words_GBps"] = round(words_bytes / (med["order_words"] * 1e-3) / 1e9, 1)
            line["argsort_Mrows_per_s"] = round(n / (med["argsort"] * 1e-3) / 1e6, 1)
            if "project_sort" in med:
                line["argsort_vs_project_sort"] = round(med["argsort"] / med["project_sort"], 3)
            emit(line)
            del legs, compare, batch, perm, cmp, words, more, got
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
