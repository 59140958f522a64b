"""WHERE masks (fury_row_predicate) against the routes there were before it: milliseconds per call and
effective GB/s of row-header bytes touched, one leg per line (not part of bench.py).

Batch: the C3 mixed workload (a INT32, b INT64, c FLOAT64, s1..s3 STRING, 10% nulls) at every `--rows`
count.  The predicate legs are bind_predicate calls into a preallocated mask and count, no host
synchronisation:
  pred_fixed        a < median(a): one fixed-width term
  pred_eq           s1 = <the s1 of one row>: one string term, the like-for-like pair of compare_rows_eq
  pred_three        a BETWEEN the quartiles AND s1 = <the same literal>: three clauses, two fields; a row
                    outside the range is decided before its string is read, so this leg does other work
                    than compare_rows_eq and no ratio of the two is reported
  pred_starts_with  s1 LIKE 'a%'
  pred_contains     s1 LIKE '%ab%'
The routes of the parent commit, measured in the same run:
  project_torch     pred_fixed by hand: bind_project of a into a preallocated column, the comparison
                    and the validity bits in torch, then RowEncoder._mask_words to pack the bool tensor
  compare_rows_eq   s1 = literal by hand: bind_compare of every row against a one-row batch that
                    holds the literal, then `== 0` and _mask_words
  hbm_copy          the box's copy rate beside them: fury_hbm_copy of 512 MiB (read + write bytes)
Each timed call has its own pair of HIP events and follows a 512 MiB copy that empties the Infinity
Cache of the batch.  The legs are interleaved over `--rounds` rounds of `--iters` calls; the median call
of the median round is reported, with the fastest and slowest round beside it.  Before timing, every
predicate mask is checked against its hand-made route (the fixed term and the string equality) or
against Python on the projected strings (the pattern legs, on the first 20000 rows).

header_bytes = rows x (8 for the row offset + 8 for the bitmap word + 8 per distinct field of the
predicate): what the kernel must read of the row headers; payload bytes come on top for string terms.

    python scripts/bench_predicate.py [--rows 1000000] [--out profiles/predicate_bench.jsonl]
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
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "bench_predicate.py measures on the GPU; there is no fallback"
    from bench import make_device_columns
    import fury_amd as F
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

    def valid_of(col, n):
        idx = torch.arange(n, device=dev)
        return ((col.validity[idx >> 3].to(torch.int32) >> (idx & 7).to(torch.int32)) & 1).bool()

    fields = SCHEMAS["mixed"]
    for n in args.rows:
        enc = Encoders.bean(fields, device=dev)
        batch = enc.encode_batch(make_device_columns("mixed", fields, n, 0, dev), n)
        words = (n + 31) // 32
        # the literals, from the batch itself
        col_a = enc.project_batch(batch, ["a"])
        va = col_a[0].values.view(torch.int32)[valid_of(col_a[0], n)].sort().values
        lo, med, hi = (int(va[(va.numel() * q) // 4]) for q in (1, 2, 3))
        s1 = enc.project_batch(batch, ["s1"])[0]
        offs, data, ok = s1.offsets.cpu().numpy(), s1.values.cpu().numpy(), valid_of(s1, n).cpu().numpy()
        r = next(i for i in range(n // 2, n) if ok[i] and offs[i + 1] - offs[i] >= 12)
        literal = bytes(data[offs[r]:offs[r + 1]])
        one = enc.take(batch, torch.tensor([r], device=dev))

        preds = {"pred_fixed": ([F.lt("a", med)], 1),
                 "pred_eq": ([F.eq("s1", literal)], 1),
                 "pred_three": ([F.between("a", lo, hi), F.eq("s1", literal)], 2),
                 "pred_starts_with": ([F.starts_with("s1", "a")], 1),
                 "pred_contains": ([F.contains("s1", "ab")], 1)}
        masks = {k: torch.empty(words, dtype=torch.int32, device=dev) for k in preds}
        counts = {k: torch.empty(1, dtype=torch.int64, device=dev) for k in preds}
        legs = {k: F.bind_predicate(enc, batch, p, masks[k], counts[k]) for k, (p, _) in preds.items()}

        # the routes before: a projected column and torch, or fury_row_compare against the literal's row
        proj = enc.bind_project(batch, ["a"], col_a)
        kept = {}

        def project_torch():
            proj()
            bits = valid_of(col_a[0], n) & (col_a[0].values.view(torch.int32) < med)
            kept["fixed"] = enc._mask_words(bits, n, None)

        cmp = torch.empty(n, dtype=torch.int8, device=dev)
        zeros = torch.zeros(n, dtype=torch.int64, device=dev)
        compare = F.bind_compare(F.KeySide(enc, batch, ["s1"]), F.KeySide(enc, one, ["s1"], zeros), cmp)

        def compare_rows_eq():
            compare()
            kept["eq"] = enc._mask_words(cmp == 0, n, None)

        legs.update(project_torch=project_torch, compare_rows_eq=compare_rows_eq, hbm_copy=flush)
        # the results agree before anything is timed
        for call in legs.values():
            call()
            call()
        enc.device_status()
        torch.cuda.synchronize()
        assert torch.equal(masks["pred_fixed"].view(torch.uint8), kept["fixed"]), "pred_fixed differs from project + torch"
        eq_mask = masks["pred_eq"]
        assert torch.equal(eq_mask.view(torch.uint8), kept["eq"]), "s1 = literal differs from compare_rows"
        in_range = torch.empty(words, dtype=torch.int32, device=dev)
        F.predicate_into(enc, batch, [F.between("a", lo, hi)], in_range)
        assert torch.equal(masks["pred_three"], in_range & eq_mask)
        head = min(n, 20000)
        strings = [bytes(data[offs[i]:offs[i + 1]]) if ok[i] else None for i in range(head)]
        for k, test in (("pred_starts_with", lambda v: v.startswith(b"a")), ("pred_contains", lambda v: b"ab" in v)):
            got = masks[k].view(torch.uint8).cpu().numpy()
            want = [v is not None and test(v) for v in strings]
            assert [bool(got[i >> 3] >> (i & 7) & 1) for i in range(head)] == want, k
            assert int(counts[k]) == sum(bin(int(x) & 0xFFFFFFFF).count("1") for x in masks[k].cpu()), k

        rounds = timed(legs)
        enc.device_status()
        for k, v in rounds.items():
            ms = statistics.median(v)
            line = {"rows": n, "leg": k, "ms": round(ms, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
            if k == "hbm_copy":
                line["bytes"] = 2 * fsrc.numel()
                line["GBps"] = round(line["bytes"] / (ms * 1e-3) / 1e9, 1)
            else:
                nf = preds[k][1] if k in preds else 1
                line["header_bytes"] = n * (8 + 8 + 8 * nf)
                line["header_GBps"] = round(line["header_bytes"] / (ms * 1e-3) / 1e9, 1)
                line["Mrows_per_s"] = round(n / (ms * 1e-3) / 1e6, 1)
                if k in preds:
                    line["selected"] = int(counts[k])
            emit(line)
        med_ms = {k: statistics.median(v) for k, v in rounds.items()}
        emit({"rows": n, "leg": "ratios", "row_bytes": batch.rows.numel(),
              "project_torch_over_pred_fixed": round(med_ms["project_torch"] / med_ms["pred_fixed"], 3),
              "compare_rows_eq_over_pred_eq": round(med_ms["compare_rows_eq"] / med_ms["pred_eq"], 3)})
        del legs, batch
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
