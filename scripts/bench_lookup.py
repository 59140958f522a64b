"""Key index and lookup (fury_row_index_build / fury_row_lookup) against the routes there were before
them: probe rows per second and bytes touched per route (not part of bench.py).

Key sets: (a) Struct-100 (816-byte rows), one INT64 key, (b) C3 mixed, keys ["a", "s1"] (an INT32 and a
12-byte STRING), (c) a two-field schema (id INT64, k STRING) with its 64-byte STRING key.  The build
side has `--build` rows of distinct keys (key numbers 0 .. B - 1 in a random order); the probe side
has `--rows` rows whose key numbers are drawn uniformly from 0 .. B / hit - 1 for each hit rate of
`--hits`, so about that share of the probe rows finds a build row.  The key columns are an injective
function of the key number (no nulls); the other columns of a probe batch are generated once per
case and row count.
  build           build_index_into into a preallocated table, the call hashing the keys itself
  lookup          bind_lookup into a preallocated out_rows, the call hashing the probe keys itself
  lookup_hashed   the same with the caller's hashes on both sides (hash_rows, made outside the timed call)
  both            build + lookup in one timed region: what a one-off join pays
  join_pairs      route (a) at the parent commit: join_pairs(probe, build); with distinct build keys it
                  gives the same matches (2 calls a round: it synchronises with the host twice per call)
  sorted          route (b), the INT64 key only: bind_project of both keys, torch.sort of the build keys,
                  torch.searchsorted of the probe keys and an equality check
Each timed call has its own pair of HIP events and follows a 512 MiB copy that empties the Infinity
Cache of the batches.  The legs are interleaved over `--rounds` rounds of `--iters` calls; the median
call of the median round is reported, with the fastest and slowest round beside it.  Before timing,
out_rows of both lookup forms is checked against the build row of every key number.

One JSON line per case.  lookup_bytes = what a lookup must touch: per probe row the row offset of a
variable-length schema, one bitmap word and one slot per key, the payload of STRING keys, 8 bytes of
hash (written, then read), one 8-byte table slot and the 8-byte result; per probe row that finds a
build row, that row's offset, header words and payload once more.  build_bytes = the same per build
row plus the table's 8-byte slots (written by the memset, probed).  GBps = bytes / time.

    python scripts/bench_lookup.py [--rows 1000000 16000000] [--out profiles/lookup_bench.jsonl]
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
    ap.add_argument("--build", type=int, nargs="+", default=[65_536, 1_000_000])
    ap.add_argument("--hits", type=float, nargs="+", default=[0.1, 0.5, 1.0])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--cases", nargs="+", default=["struct100_int64", "mixed_int32_string", "string64"])
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "bench_lookup.py measures on the GPU; there is no fallback"
    from bench import make_device_columns
    from fury_amd import KeyIndex, KeySide, bind_lookup, build_index_into, index_slots, join_pairs
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
        """The key number as 12 ASCII digits: [n, 12] uint8."""
        p = 10 ** torch.arange(11, -1, -1, device=dev, dtype=torch.int64)
        return ((kid.unsqueeze(1) // p) % 10 + 48).to(torch.uint8)

    def other_columns(case, n):
        """(fields, device columns without their key values, keys, payload bytes per row)."""
        if case == "struct100_int64":
            fields = SCHEMAS["struct100"]
            return fields, make_device_columns("struct100", fields, n, 0, dev), [0], 0
        if case == "mixed_int32_string":
            fields = SCHEMAS["mixed"]
            return fields, make_device_columns("mixed", fields, n, 0, dev), ["a", "s1"], 12
        fields = [T.not_null_field("id", T.INT64), T.field("k", T.STRING)]
        return fields, [Column(values=torch.arange(n, dtype=torch.int64, device=dev)), None], ["k"], 64

    def with_keys(case, fields, cols, kid):
        """The columns with the key columns made from the key numbers kid."""
        n = kid.numel()
        cols = list(cols)
        if case == "struct100_int64":
            cols[0] = Column(values=kid * -7046029254386353131 + 1)         # odd multiplier: injective
        elif case == "mixed_int32_string":
            names = [f.name for f in fields]
            cols[names.index("a")] = Column(values=(kid % 1000).to(torch.int32))
            cols[names.index("s1")] = Column(
                values=digits12(kid).reshape(-1),
                offsets=(torch.arange(n + 1, dtype=torch.int64, device=dev) * 12).to(torch.int32))
        else:
            # 64 bytes per key: 12 digits, then 52 bytes that are a function of the key number
            tail = ((kid.unsqueeze(1) * 2654435761 + torch.arange(52, device=dev) * 40503) >> 7) & 0xFF
            cols[1] = Column(values=torch.cat([digits12(kid), tail.to(torch.uint8)], 1).reshape(-1),
                             offsets=(torch.arange(n + 1, dtype=torch.int64, device=dev) * 64).to(torch.int32))
        return cols

    for case in args.cases:
        for B in args.build:
            fields, bcols, keys, payload = other_columns(case, B)
            enc = Encoders.bean(fields, device=dev)
            sch = enc.schema()
            g = torch.Generator(device=dev).manual_seed(B)
            bkid = torch.randperm(B, device=dev, generator=g)
            build = enc.encode_batch(with_keys(case, fields, bcols, bkid), B)
            del bcols
            row_of_key = torch.empty(B, dtype=torch.int64, device=dev)
            row_of_key[bkid] = torch.arange(B, device=dev)
            bside = KeySide(enc, build, keys)
            slots = index_slots(B)
            table, table_h = (torch.empty(slots, dtype=torch.int64, device=dev) for _ in range(2))
            bh = enc.hash_rows(build, keys, seed=7)
            build_index_into(bside, table_h, hashes=bh)
            index, index_h = KeyIndex(bside, table, None, False), KeyIndex(bside, table_h, None, True)
            for n in args.rows:
                _, pcols, _, _ = other_columns(case, n)
                for hit in args.hits:
                    g = torch.Generator(device=dev).manual_seed(n + B)
                    kid = torch.randint(0, max(B, int(B / hit)), (n,), device=dev, generator=g)
                    probe = enc.encode_batch(with_keys(case, fields, pcols, kid), n)
                    pside = KeySide(enc, probe, keys)
                    out = torch.empty(n, dtype=torch.int64, device=dev)
                    ph = enc.hash_rows(probe, keys, seed=7)

                    def build_call():
                        build_index_into(bside, table)
                    look = bind_lookup(index, pside, out)
                    look_h = bind_lookup(index_h, pside, out, hashes=ph)

                    def both():
                        build_index_into(bside, table)
                        look()
                    want = torch.where(kid < B, row_of_key[kid.clamp(max=B - 1)], torch.full_like(kid, -1))
                    found = int((want >= 0).sum())
                    build_call()
                    for c in (look, look_h):
                        out.fill_(-2)
                        c()
                        enc.device_status()
                        assert torch.equal(out, want), "out_rows is not the build row of the key"
                    legs = {"build": (build_call, args.iters), "lookup": (look, args.iters),
                            "lookup_hashed": (look_h, args.iters), "both": (both, args.iters)}

                    def joined():
                        return join_pairs(pside, bside, seed=7)
                    pj, bi = joined()
                    assert pj.numel() == found and torch.equal(bi, want[pj])
                    del pj, bi
                    legs["join_pairs"] = (joined, 2)
                    if case == "struct100_int64":
                        bcol, pcol = enc.project_batch(build, keys), enc.project_batch(probe, keys)
                        pb, pp = enc.bind_project(build, keys, bcol), enc.bind_project(probe, keys, pcol)
                        bv, pv = bcol[0].values.view(torch.int64), pcol[0].values.view(torch.int64)

                        def sorted_route():
                            pb()
                            pp()
                            sk, order = torch.sort(bv)
                            pos = torch.searchsorted(sk, pv).clamp_(max=B - 1)
                            return torch.where(sk[pos] == pv, order[pos], torch.full_like(pos, -1))
                        assert torch.equal(sorted_route(), want)
                        legs["sorted"] = (sorted_route, args.iters)
                    rounds = timed(legs)
                    enc.device_status()
                    med = {k: statistics.median(v) for k, v in rounds.items()}
                    per_row = (0 if sch.is_fixed else 8) + 16 * len(keys) + payload
                    lookup_bytes = n * (per_row + 8 + 8 + 8) + found * per_row
                    build_bytes = B * (per_row + 8) + 8 * slots
                    line = {"case": case, "build_rows": B, "rows": n, "hit": hit, "found": found, "keys": len(keys),
                            "probe_row_bytes": probe.rows.numel(), "build_row_bytes": build.rows.numel(),
                            "lookup_bytes": lookup_bytes, "build_bytes": build_bytes}
                    for k in med:
                        line[f"{k}_ms"] = round(med[k], 4)
                        line[f"{k}_min_ms"] = round(min(rounds[k]), 4)
                        line[f"{k}_max_ms"] = round(max(rounds[k]), 4)
                    line["Mrows_per_s"] = round(n / (med["lookup"] * 1e-3) / 1e6, 1)
                    line["lookup_GBps"] = round(lookup_bytes / (med["lookup"] * 1e-3) / 1e9, 1)
                    line["build_GBps"] = round(build_bytes / (med["build"] * 1e-3) / 1e9, 1)
                    line["join_pairs_vs_both"] = round(med["join_pairs"] / med["both"], 3)
                    line["join_pairs_vs_lookup"] = round(med["join_pairs"] / med["lookup"], 3)
                    if "sorted" in med:
                        line["sorted_vs_both"] = round(med["sorted"] / med["both"], 3)
                        line["sorted_vs_lookup"] = round(med["sorted"] / med["lookup"], 3)
                    emit(line)
                    del legs, look, look_h, probe, pside, out, ph, want, kid
                    torch.cuda.empty_cache()
                del pcols
            del build, bside, table, table_h, index, index_h, bh
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
