"""Per-group aggregates (fury_row_aggregate) against the route there was before it: rows per second
per shape of the group ids (not part of bench.py).

Batch: the C3 mixed workload (a INT32, b INT64, c FLOAT64, s1..s3 STRING, 10% nulls) at every `--rows`
count.  Id shapes: one group (group_ids=None); 37 groups drawn at random; the same 37 groups with the
ids sorted, as the rows lie after `partition`; all-distinct ids (a permutation, G = rows).
  aggregate       bind_aggregate of SUM(c) into preallocated out / count; no host synchronisation
  aggregate4      one call of SUM(b), SUM(c), MIN(a) and COUNT(*)
  argmax_s1       ARGMAX(s1): the compare-and-swap cell (no baseline: the old route sorts the batch)
  project_scatter what the library offered before: bind_project of c into a preallocated column, the
                  nulls zeroed through the validity bits, then index_add_ on the same ids
  project_scatter4  bind_project of a, b, c, then index_add_ twice, scatter_reduce("amin") and bincount
  hash            bind_hash of the field c: the time to read the same row headers once
Each timed call has its own pair of HIP events and follows a 512 MiB copy that empties the Infinity
Cache of the batch.  The legs are interleaved over `--rounds` rounds of `--iters` calls; the median call
of the median round is reported, with the fastest and slowest round beside it (`--baseline-iters` calls
per round for the project_scatter legs, whose calls take up to seconds).  Before timing, the
integer results are checked against torch on the projected columns and the float sum within rule 3's
bound.

One JSON line per (rows, shape): ms per leg, Mrows_per_s of aggregate, and the ratios
vs_project_scatter (> 1: aggregate is faster) and vs_hash (aggregate / hash).

    python scripts/bench_aggregate.py [--rows 1000000 10000000] [--out profiles/aggregate_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--baseline-iters", type=int, default=2,
                    help="calls per round of the project_scatter legs (a call takes up to seconds)")
    ap.add_argument("--shapes", nargs="+", default=["one", "37_random", "37_partitioned", "distinct"])
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "bench_aggregate.py measures on the GPU; there is no fallback"
    from bench import make_device_columns
    from fury_amd import Agg, bind_aggregate
    from fury_amd import _native as N
    from fury_amd.encoder import Encoders
    from fury_amd.workloads import SCHEMAS
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
        """Median call of every round per leg, the legs interleaved.  legs: name -> call; every leg
        has run at least twice before (the checks), which is the warm-up."""
        rounds = {name: [] for name in legs}
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for name, call in legs.items():
                ev = []
                for _ in range(args.baseline_iters if name.startswith("project") else args.iters):
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

    def valid_of(col, n):
        idx = torch.arange(n, device=dev)
        return ((col.validity[idx >> 3].to(torch.int32) >> (idx & 7).to(torch.int32)) & 1).bool()

    fields = SCHEMAS["mixed"]
    for n in args.rows:
        enc = Encoders.bean(fields, device=dev)
        batch = enc.encode_batch(make_device_columns("mixed", fields, n, 0, dev), n)
        for shape in args.shapes:
            g = torch.Generator(device=dev).manual_seed(37)
            if shape == "one":
                ids, G = None, 1
            elif shape.startswith("37"):
                ids, G = torch.randint(0, 37, (n,), device=dev, generator=g), 37
                if shape == "37_partitioned":
                    ids = ids.sort().values
            else:
                ids, G = torch.randperm(n, device=dev, generator=g), n
            index = torch.zeros(n, dtype=torch.int64, device=dev) if ids is None else ids
            out1, cnt1 = (torch.empty(G, dtype=torch.int64, device=dev) for _ in range(2))
            out4 = [torch.empty(G, dtype=torch.int64, device=dev) for _ in range(4)]
            arg, cnt_arg = (torch.empty(G, dtype=torch.int64, device=dev) for _ in range(2))
            four = [Agg("sum", "b"), Agg("sum", "c"), Agg("min", "a"), Agg("count", None)]
            legs = {"aggregate": bind_aggregate(enc, batch, ids, G, [Agg("sum", "c")], [out1], [cnt1]),
                    "aggregate4": bind_aggregate(enc, batch, ids, G, four, out4),
                    "argmax_s1": bind_aggregate(enc, batch, ids, G, [Agg("argmax", "s1")], [arg], [cnt_arg])}
            # the route before: the value columns in HBM, then torch's scatter kernels
            col1 = enc.project_batch(batch, ["c"])
            proj1 = enc.bind_project(batch, ["c"], col1)
            sum1 = torch.empty(G, dtype=torch.float64, device=dev)
            col3 = enc.project_batch(batch, ["a", "b", "c"])
            proj3 = enc.bind_project(batch, ["a", "b", "c"], col3)
            acc_b = torch.empty(G, dtype=torch.int64, device=dev)
            acc_c = torch.empty(G, dtype=torch.float64, device=dev)
            acc_a = torch.empty(G, dtype=torch.int32, device=dev)

            def project_scatter():
                proj1()
                v = torch.where(valid_of(col1[0], n), col1[0].values.view(torch.float64), 0.0)
                sum1.zero_().index_add_(0, index, v)

            def project_scatter4():
                proj3()
                a, b, c = (x.values for x in col3)
                acc_b.zero_().index_add_(0, index, torch.where(valid_of(col3[1], n), b.view(torch.int64), 0))
                acc_c.zero_().index_add_(0, index, torch.where(valid_of(col3[2], n), c.view(torch.float64), 0.0))
                big = torch.iinfo(torch.int32).max
                acc_a.fill_(big).scatter_reduce_(0, index, torch.where(valid_of(col3[0], n), a.view(torch.int32), big),
                                                 "amin")
                return torch.bincount(index, minlength=G)

            hashes = torch.empty(n, dtype=torch.uint32, device=dev)
            legs.update(project_scatter=project_scatter, project_scatter4=project_scatter4,
                        hash=enc.bind_hash(batch, ["c"], hashes))
            # the results agree before anything is timed
            for call in legs.values():
                call()
                call()
            enc.device_status()
            sizes = project_scatter4()
            torch.cuda.synchronize()
            assert torch.equal(out4[0], acc_b) and torch.equal(out4[3], sizes)
            has_a = torch.zeros(G, dtype=torch.bool, device=dev).index_fill_(0, index[valid_of(col3[0], n)], True)
            assert torch.equal(out4[2][has_a], acc_a.to(torch.int64)[has_a]) and bool((out4[2][~has_a] == 0).all())
            mass = torch.zeros(G, dtype=torch.float64, device=dev).index_add_(
                0, index, torch.where(valid_of(col1[0], n), col1[0].values.view(torch.float64).abs(), 0.0))
            slack = 2.0 * cnt1.to(torch.float64) * 2.0 ** -52 * mass           # both sums carry rule 3's error
            assert bool(((out1.view(torch.float64) - sum1).abs() <= slack).all()), "SUM(c) outside rule 3's bound"
            assert bool((arg[cnt_arg > 0] >= 0).all()) and bool((arg[cnt_arg == 0] == -1).all())
            rounds = timed(legs)
            enc.device_status()
            med = {k: statistics.median(v) for k, v in rounds.items()}
            line = {"rows": n, "shape": shape, "groups": G, "row_bytes": batch.rows.numel()}
            for k in med:
                line[f"{k}_ms"] = round(med[k], 4)
                line[f"{k}_min_ms"] = round(min(rounds[k]), 4)
                line[f"{k}_max_ms"] = round(max(rounds[k]), 4)
            line["Mrows_per_s"] = round(n / (med["aggregate"] * 1e-3) / 1e6, 1)
            line["vs_project_scatter"] = round(med["project_scatter"] / med["aggregate"], 3)
            line["vs_project_scatter4"] = round(med["project_scatter4"] / med["aggregate4"], 3)
            line["vs_hash"] = round(med["aggregate"] / med["hash"], 3)
            emit(line)
            del legs, col1, col3, proj1, proj3, ids, index
            torch.cuda.empty_cache()
        del batch
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
