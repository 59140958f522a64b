"""Group ids (fury_row_group) against the routes there were before it: rows per second and bytes
touched per route (not part of bench.py).

Batches: (a) Struct-100 (816-byte rows) grouped by one INT64 key, (b) C3 mixed grouped by ["a", "s1"]
(an INT32 and a 12-byte STRING), (c) a two-field schema (id INT64, k STRING) grouped by its 64-byte
STRING key.  Each at every `--rows` count and with 100, 65536 and rows / 2 distinct keys: every row
draws a key number uniformly, and the key columns are an injective function of it (no nulls), so the
expected groups are known from the key numbers.
  group           bind_group into preallocated out_first / out_group_ids / out_group_rows /
                  out_num_groups, the call hashing the keys itself; no host synchronisation
  group_hashed    the same with the caller's hashes (hash_rows, made outside the timed call)
  project_unique  (a) only: bind_project of the key into a preallocated column, then
                  torch.unique(return_inverse=True) -- sorted ids, not first-occurrence ids, and no
                  first rows; the only route for a fixed-width key before this operator
  self_join       join_pairs of the batch with itself under null_equal=True, where the candidate pairs
                  (the sum of the squared group sizes) number at most `--max-pairs`; otherwise the
                  count is recorded as the result: the route does not fit
Each timed call has its own pair of HIP events and follows a 512 MiB copy that empties the Infinity
Cache of the batch.  The legs are interleaved over `--rounds` rounds of `--iters` calls (self_join:
2 calls a round; it synchronises with the host twice per call); the median call of the median round
is reported, with the fastest and slowest round beside it.  Before timing, out_first is checked
against the first occurrence of every key number and the group count against torch.unique.

One JSON line per case: batch_bytes = the key bytes of the batch the call must read (per row: the
row offset of a variable-length schema, one bitmap word and one slot per key, the payload of STRING
keys), table_bytes = the 8-byte slots of the table (written by the memset, probed), out_bytes = the
four outputs; ms per leg, Mrows_per_s and GBps (the three byte counts together) of group.

    python scripts/bench_group.py [--rows 1000000 16000000] [--out profiles/group_bench.jsonl]
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
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 16_000_000])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--max-pairs", type=int, default=1 << 28)
    ap.add_argument("--cases", nargs="+", default=["struct100_int64", "mixed_int32_string", "string64"])
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "bench_group.py measures on the GPU; there is no fallback"
    from bench import make_device_columns
    from fury_amd import KeySide, bind_group, join_pairs
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

    def stats(rounds):
        med = {k: statistics.median(v) for k, v in rounds.items()}
        out = {}
        for k in med:
            out[f"{k}_ms"] = round(med[k], 4)
            out[f"{k}_min_ms"] = round(min(rounds[k]), 4)
            out[f"{k}_max_ms"] = round(max(rounds[k]), 4)
        return med, out

    def digits12(kid):
        """The key number as 12 ASCII digits: [n, 12] uint8."""
        p = 10 ** torch.arange(11, -1, -1, device=dev, dtype=torch.int64)
        return ((kid.unsqueeze(1) // p) % 10 + 48).to(torch.uint8)

    def columns(case, n, kid, distinct):
        """(fields, device columns, keys, payload bytes per row) with the key columns made from kid."""
        if case == "struct100_int64":
            fields = SCHEMAS["struct100"]
            cols = make_device_columns("struct100", fields, n, 0, dev)
            cols[0] = Column(values=kid * -7046029254386353131 + 1)         # odd multiplier: injective
            return fields, cols, [0], 0
        if case == "mixed_int32_string":
            fields = SCHEMAS["mixed"]
            cols = make_device_columns("mixed", fields, n, 0, dev)
            names = [f.name for f in fields]
            cols[names.index("a")] = Column(values=(kid % 1000).to(torch.int32))
            cols[names.index("s1")] = Column(
                values=digits12(kid).reshape(-1),
                offsets=(torch.arange(n + 1, dtype=torch.int64, device=dev) * 12).to(torch.int32))
            return fields, cols, ["a", "s1"], 12
        fields = [T.not_null_field("id", T.INT64), T.field("k", T.STRING)]
        g = torch.Generator(device=dev).manual_seed(64)
        table = torch.randint(0, 256, (distinct, 64), dtype=torch.uint8, device=dev, generator=g)
        table[:, :12] = digits12(torch.arange(distinct, device=dev))       # distinct whatever the draw
        cols = [Column(values=torch.arange(n, dtype=torch.int64, device=dev)),
                Column(values=table[kid].reshape(-1),
                       offsets=(torch.arange(n + 1, dtype=torch.int64, device=dev) * 64).to(torch.int32))]
        return fields, cols, ["k"], 64

    for case in args.cases:
        for n in args.rows:
            for distinct in (100, 65536, n // 2):
                g = torch.Generator(device=dev).manual_seed(distinct)
                kid = torch.randint(0, distinct, (n,), device=dev, generator=g)
                fields, cols, keys, payload = columns(case, n, kid, distinct)
                enc = Encoders.bean(fields, device=dev)
                sch = enc.schema()
                batch = enc.encode_batch(cols, n)
                del cols
                first = torch.empty(n, dtype=torch.int64, device=dev)
                ids = torch.empty(n, dtype=torch.int64, device=dev)
                rows = torch.empty(n, dtype=torch.int64, device=dev)
                num = torch.empty(1, dtype=torch.int64, device=dev)
                hashes = enc.hash_rows(batch, keys, seed=7)
                call = bind_group(enc, batch, keys, first, ids, rows, num)
                hashed = bind_group(enc, batch, keys, first, ids, rows, num, hashes=hashes)
                # the expectation: the first occurrence of every key number
                pos = torch.arange(n, device=dev)
                want = torch.full((distinct,), n, dtype=torch.int64, device=dev).scatter_reduce(
                    0, kid, pos, "amin")[kid]
                groups = int(torch.unique(kid).numel())
                for c in (hashed, call):
                    first.fill_(-1)
                    c()
                    enc.device_status()
                    assert torch.equal(first, want), "out_first is not the first occurrence of the key"
                    assert int(num) == groups and int(ids.max()) == groups - 1
                    assert torch.equal(rows[ids], first) and bool((rows[groups:] == -1).all())
                legs = {"group": (call, args.iters), "group_hashed": (hashed, args.iters)}
                if case == "struct100_int64":
                    col = enc.project_batch(batch, keys)
                    proj = enc.bind_project(batch, keys, col)
                    values = col[0].values.view(torch.int64)

                    def project_unique():
                        proj()
                        return torch.unique(values, return_inverse=True)
                    uniq, inverse = project_unique()
                    assert uniq.numel() == groups and torch.equal(uniq[inverse][want], uniq[inverse])
                    legs["project_unique"] = (project_unique, args.iters)
                sizes = torch.bincount(kid, minlength=distinct)
                candidates = int((sizes * sizes).sum())
                if candidates <= args.max_pairs:
                    side = KeySide(enc, batch, keys)

                    def self_join():
                        return join_pairs(side, side, null_equal=True, seed=7)
                    li, ri = self_join()
                    assert li.numel() == candidates                  # no collision survives the compare
                    del li, ri
                    legs["self_join"] = (self_join, 2)
                rounds = timed(legs)
                enc.device_status()
                med, out = stats(rounds)
                cap = 2
                while cap < 2 * n:
                    cap *= 2
                batch_bytes = n * ((0 if sch.is_fixed else 8) + 16 * len(keys) + payload)
                table_bytes, out_bytes = 8 * cap, 24 * n + 8
                line = {"case": case, "rows": n, "distinct": distinct, "groups": groups, "keys": len(keys),
                        "row_bytes": batch.rows.numel(), "batch_bytes": batch_bytes, "table_bytes": table_bytes,
                        "out_bytes": out_bytes, **out,
                        "Mrows_per_s": round(n / (med["group"] * 1e-3) / 1e6, 1),
                        "GBps": round((batch_bytes + table_bytes + out_bytes) / (med["group"] * 1e-3) / 1e9, 1),
                        "self_join_candidates": candidates}
                if "project_unique" in med:
                    line["vs_project_unique"] = round(med["project_unique"] / med["group"], 3)
                if "self_join" in med:
                    line["vs_self_join"] = round(med["self_join"] / med["group"], 3)
                else:
                    line["self_join"] = f"{candidates} candidate pairs exceed {args.max_pairs}: does not fit"
                emit(line)
                del legs, call, hashed, batch, first, ids, rows, num, hashes, want, kid
                torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
