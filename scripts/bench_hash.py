"""Key hash (fury_row_hash) against the projected decode of the same key fields -- the first half of
the only route there was before -- and partition_by against its two halves (not part of bench.py).

Workloads: Struct-100 (816-byte rows) and C3 mixed (3 numbers + 3 strings), 1M rows each.  Cases: one
INT64 key, four fixed-width keys, 64 keys (Struct-100); one INT64 key, one STRING key, a STRING and an
INT64 key (mixed).  Per case these legs are timed in the same process:
  hash           bind_hash into preallocated hashes and part ids (16 partitions), no host
                 synchronisation
  project        bind_project of the same fields into preallocated columns (values + validity; the
                 count pass, scan and payload copy for a STRING key)
  project_torch  fixed-width single keys only: project, then the multiplicative hash one-liner in torch
                 on the decoded column
and per workload, for the first key set, 16 partitions:
  partition_by   RowEncoder.partition_by (allocates, sizes the output with one host read)
  separate       bind_hash, then RowEncoder.partition with the ids: the same work as two calls
  hash_then_into bind_hash + bind_partition into preallocated buffers: no host read at all
Each timed call has its own pair of HIP events and follows a 512 MiB copy that empties the Infinity
Cache of the batch.  The legs are interleaved over `--rounds` rounds of `--iters` calls; the median
call of the median round is reported, with the fastest and slowest round beside it.  Before timing,
the hashes are checked against fury_hash_bytes on a sample of rows.

One JSON line per case: min_bytes = the bytes the hash must touch (per row: the 8-byte header words
of the keys, the row offset of a variable-length schema, the payload bytes of STRING keys, 8 bytes of
output), ms per leg, hash_GBps = min_bytes / time, vs_project = project / hash, and
not_slower_than_project: the median hash round is at most the slowest project round.

    python scripts/bench_hash.py [--rows 1000000] [--out profiles/hash_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

PARTS = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "bench_hash.py measures on the GPU; there is no fallback"
    import fury_amd
    from bench import make_device_columns
    from fury_amd import _native as N
    from fury_amd import types as T
    from fury_amd.encoder import Encoders
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

    def stats(rounds):
        med = {k: statistics.median(v) for k, v in rounds.items()}
        out = {}
        for k in med:
            out[f"{k}_ms"] = round(med[k], 4)
            out[f"{k}_min_ms"] = round(min(rounds[k]), 4)
            out[f"{k}_max_ms"] = round(max(rounds[k]), 4)
        return med, out

    def check_sample(enc, fields, batch, keys, hashes, seed):
        """The device's hashes of a few rows against fury_hash_bytes on their decoded values."""
        idx = enc._select(keys)
        rows = torch.tensor([0, 1, n // 2, n - 1], device=dev)
        cols = enc.project_batch(enc.take(batch, rows), keys)
        for j in range(rows.numel()):
            h = seed
            for k, c in zip(idx, cols):
                valid = c.validity is None or (int(c.validity[j >> 3]) >> (j & 7)) & 1
                if not valid:
                    h = fury_amd.hash_null(h)
                elif fields[k].type_id == T.STRING:
                    o = c.offsets.cpu().tolist()
                    h = fury_amd.hash_bytes(c.values[o[j]:o[j + 1]].cpu().numpy().tobytes(), h)
                else:
                    w = T.type_width(fields[k].type_id)
                    raw = c.values.view(torch.uint8)[j * w:(j + 1) * w].cpu().numpy().tobytes()
                    h = fury_amd.hash_bytes(raw, h)
            assert int(hashes[int(rows[j])]) & 0xFFFFFFFF == h, f"row {int(rows[j])}: hash differs"

    cases = {"struct100": [("int64", [0]), ("fixed4", [0, 1, 50, 99]), ("fixed64", list(range(64)))],
             "mixed": [("int64", ["b"]), ("string", ["s1"]), ("string_int64", ["s1", "b"])]}
    for name in ("struct100", "mixed"):
        fields = SCHEMAS[name]
        enc = Encoders.bean(fields, device=dev)
        sch = enc.schema()
        fixed = sch.is_fixed
        batch = enc.encode_batch(make_device_columns(name, fields, n, 0, dev), n)
        nbytes = batch.rows.numel()
        hashes = torch.empty(n, dtype=torch.uint32, device=dev)
        ids = torch.empty(n, dtype=torch.int32, device=dev)
        for case, keys in cases[name]:
            idx = enc._select(keys)
            hash_call = enc.bind_hash(batch, keys, hashes, ids, 42, PARTS)
            cols = enc.project_batch(batch, keys)               # sized for the STRING keys
            project = enc.bind_project(batch, keys, cols)
            legs = {"hash": hash_call, "project": project}
            if len(idx) == 1 and T.type_width(fields[idx[0]].type_id) > 0:
                col = cols[0].values

                def project_torch():
                    project()
                    return (col.to(torch.int64) * 0x9E3779B1 >> 7) % PARTS
                legs["project_torch"] = project_torch
            hash_call()
            enc.device_status()
            check_sample(enc, fields, batch, keys, hashes.view(torch.int32).cpu().tolist(), 42)
            assert torch.equal(ids, (hashes.view(torch.int32).to(torch.int64) & 0xFFFFFFFF).remainder(PARTS)
                               .to(torch.int32))
            words = {k >> 6 for k in idx} | {sch.bitmap_bytes // 8 + k for k in idx}
            payload = sum(int(c.offsets[n]) for k, c in zip(idx, cols)
                          if fields[k].type_id in (T.STRING, T.BINARY))
            min_bytes = n * (8 * len(words) + (0 if fixed else 8) + 8) + payload
            rounds = timed(legs)
            enc.device_status()
            med, out = stats(rounds)
            emit({"workload": name, "rows": n, "case": case, "keys": len(idx), "row_bytes": nbytes,
                  "min_bytes": min_bytes, **out,
                  "hash_GBps": round(min_bytes / (med["hash"] * 1e-3) / 1e9, 1),
                  "vs_project": round(med["project"] / med["hash"], 3),
                  "not_slower_than_project": med["hash"] <= max(rounds["project"])})
            del cols, project, legs
        # partition_by against its two halves
        case, keys = cases[name][0]
        out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        offs = None if fixed else torch.empty(n + 1, dtype=torch.int64, device=dev)
        part_rows = torch.empty(PARTS + 1, dtype=torch.int64, device=dev)
        hash_ids = enc.bind_hash(batch, keys, None, ids, 42, PARTS)
        into = enc.bind_partition(batch, ids, PARTS, out, offs, part_rows)

        def partition_by():
            return enc.partition_by(batch, keys, PARTS, seed=42)

        def separate():
            hash_ids()
            return enc.partition(batch, ids, PARTS)

        def hash_then_into():
            hash_ids()
            into()

        got, pr = partition_by()
        hash_then_into()
        assert torch.equal(pr, part_rows) and torch.equal(got.rows, out[:got.rows.numel()])
        rounds = timed({"partition_by": partition_by, "separate": separate,
                        "hash_then_into": hash_then_into, "hash_ids": hash_ids, "partition_into": into})
        med, stat = stats(rounds)
        emit({"workload": name, "rows": n, "case": f"partition_by_{case}", "num_parts": PARTS,
              "row_bytes": nbytes, **stat,
              "by_vs_separate": round(med["separate"] / med["partition_by"], 3),
              "hash_share_of_into": round(med["hash_ids"] / med["hash_then_into"], 3)})
        del batch, out, into, got
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
