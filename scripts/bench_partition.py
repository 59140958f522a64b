"""Partition and concat (fury_row_partition / fury_row_concat) against a plain copy of the same bytes
and against the only route there was before (not part of bench.py).

Workloads: Struct-100 (816-byte rows) and C3 mixed (3 numbers + 3 strings), 1M rows each.  Cases:
uniform ids over 2, 16, 256 and 4096 partitions (one ranking pass up to 255 partitions, two from 256
on), one skewed case (90 % of the rows in partition 0 of 16), and concat of the batch's 8 equal parts.
Per case three legs are timed in the same process:
  partition  bind_partition into preallocated buffers: everything the call launches (histograms,
             scans, scatters, part rows, offsets scan, copy), no host synchronisation
  composed   torch.sort(ids, stable=True), bincount + cumsum for the part rows, then bind_take at the
             sorted row numbers
  copy       fury_hbm_copy of the same number of bytes (rounded up to its 16 KB block): the roofline
and for concat: concat_into, torch.cat of the rows plus the offset arithmetic in torch, and the copy.
Each timed call has its own pair of HIP events and follows a 512 MiB copy that empties the Infinity
Cache of the batch.  The legs are interleaved over `--rounds` rounds of `--iters` calls; the median
call of the median round is reported, with the fastest and slowest round beside it.  Before timing,
the partitioned batch is checked byte for byte against the composed route's.

One JSON line per case: bytes moved, ms per leg, GBps = 2 x bytes / time, the ratio to the copy
(copy / partition) and to the composed route (composed / partition), and beats_composed: the slowest
partition round is faster than the fastest composed round.

    python scripts/bench_partition.py [--rows 1000000] [--out profiles/partition_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

COPY_BLOCK = 16 << 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "bench_partition.py measures on the GPU; there is no fallback"
    from bench import make_device_columns
    from fury_amd import _native as N
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

    def report(name, case, extra, nbytes, rounds, ours):
        med = {k: statistics.median(v) for k, v in rounds.items()}
        emit({"workload": name, "rows": n, "case": case, **extra, "bytes": nbytes,
              **{f"{k}_ms": round(med[k], 4) for k in med},
              **{f"{k}_min_ms": round(min(rounds[k]), 4) for k in med},
              **{f"{k}_max_ms": round(max(rounds[k]), 4) for k in med},
              **{f"{k}_GBps": round(2 * nbytes / (med[k] * 1e-3) / 1e9, 1) for k in med},
              "vs_copy": round(med["copy"] / med[ours], 3),
              "vs_composed": round(med["composed"] / med[ours], 3),
              "beats_composed": max(rounds[ours]) < min(rounds["composed"])})

    def copy_leg(nbytes):
        cb = max((nbytes + COPY_BLOCK - 1) // COPY_BLOCK * COPY_BLOCK, COPY_BLOCK)
        csrc = torch.zeros(cb, dtype=torch.uint8, device=dev)
        cdst = torch.empty_like(csrc)

        def copy():
            assert N.lib().fury_hbm_copy(cdst.data_ptr(), csrc.data_ptr(), cb, None) == 0
        copy.keep = (csrc, cdst)
        return copy

    g = torch.Generator(device=dev)
    g.manual_seed(20240607)
    for name in ("struct100", "mixed"):
        fields = SCHEMAS[name]
        enc = Encoders.bean(fields, device=dev)
        fixed = enc.schema().is_fixed
        batch = enc.encode_batch(make_device_columns(name, fields, n, 0, dev), n)
        nbytes = batch.rows.numel()
        cases = [(f"uniform_{p}", p, torch.randint(0, p, (n,), generator=g, device=dev,
                                                   dtype=torch.int32)) for p in (2, 16, 256, 4096)]
        skew = torch.randint(0, 16, (n,), generator=g, device=dev, dtype=torch.int32)
        skew[torch.rand(n, generator=g, device=dev) < 0.9] = 0
        cases.append(("skewed_16", 16, skew))
        for case, parts, ids in cases:
            out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            offs = None if fixed else torch.empty(n + 1, dtype=torch.int64, device=dev)
            part_rows = torch.empty(parts + 1, dtype=torch.int64, device=dev)
            partition = enc.bind_partition(batch, ids, parts, out, offs, part_rows)

            out2 = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            offs2 = None if fixed else torch.empty(n + 1, dtype=torch.int64, device=dev)
            part_rows2 = torch.zeros(parts + 1, dtype=torch.int64, device=dev)
            keys = torch.empty_like(ids)
            order = torch.empty(n, dtype=torch.int64, device=dev)
            take = enc.bind_take(batch, order, out2, offs2)

            def composed():
                torch.sort(ids, stable=True, out=(keys, order))
                torch.cumsum(torch.bincount(ids, minlength=parts), 0, out=part_rows2[1:])
                take()

            partition()
            composed()
            enc.device_status()
            assert torch.equal(out, out2), f"{name} {case}: partitioned rows differ"
            assert torch.equal(part_rows, part_rows2), f"{name} {case}: part rows differ"
            if not fixed:
                assert torch.equal(offs, offs2), f"{name} {case}: offsets differ"
            rounds = timed({"partition": partition, "copy": copy_leg(nbytes), "composed": composed})
            enc.device_status()
            report(name, case, {"num_parts": parts}, nbytes, rounds, "partition")
            del out, out2, partition, take
        # concat of the batch's 8 equal parts, each a batch of its own
        k = 8
        cuts = [n * i // k for i in range(k + 1)]
        pieces = [enc.slice_rows(batch, cuts[i], cuts[i + 1]) for i in range(k)]
        pieces = [type(p)(p.rows.clone(), None if fixed else p.row_offsets.clone(), p.nrows,
                          p.schema_hash) for p in pieces]
        out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        offs = None if fixed else torch.empty(n + 1, dtype=torch.int64, device=dev)
        out2 = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        offs2 = None if fixed else torch.empty(n + 1, dtype=torch.int64, device=dev)

        def concat():
            enc.concat_into(pieces, out, offs)

        def composed():
            torch.cat([p.rows for p in pieces], out=out2)
            if not fixed:
                ends = torch.cumsum(torch.stack([p.row_offsets[-1] for p in pieces]), 0)
                torch.cat([pieces[0].row_offsets] +
                          [p.row_offsets[1:] + ends[i] for i, p in enumerate(pieces[1:])], out=offs2)

        concat()
        composed()
        enc.device_status()
        assert torch.equal(out, batch.rows) and torch.equal(out2, batch.rows), f"{name}: concat differs"
        if not fixed:
            assert torch.equal(offs, batch.row_offsets) and torch.equal(offs2, batch.row_offsets)
        rounds = timed({"concat": concat, "copy": copy_leg(nbytes), "composed": composed})
        enc.device_status()
        report(name, "concat_8", {"num_sources": k}, nbytes, rounds, "concat")
        del batch, pieces, out, out2
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
