"""Nested-value extraction (fury_row_extract) against the only route to a nested field there was
before -- decode_batch of the whole parent batch --, against fury_row_filter of the same batch with an
all-ones mask (the same pass structure, whole rows moved) and against a plain copy of the bytes moved
(not part of bench.py).

Workloads, `--rows` rows each (a 4096-row pattern of row values, encoded once and repeated with take):
  foo    RowEncoderTest.Foo {int f1; String f2; List<String> f3; Map<String,Integer> f4; Bar f5}:
         extract f5 (a struct) and f3 (a list of strings)
  deep   id INT64, outer STRUCT{a INT32, inner STRUCT{s STRING, v LIST<INT64>}, fx STRUCT{p INT64,
         q INT32}, m MAP<STRING, INT32>}: extract outer.inner (two levels)
Per case these legs are timed in the same process:
  extract         bind_extract into preallocated buffers: everything the call launches (locate, two
                  scans, compact, copy), no host synchronisation
  extract_decode  the same call followed by child_encoder(path).decode_batch of the extracted batch
  decode          decode_batch of the parent batch
  filter          filter_into of the parent batch with an all-ones mask
  copy            fury_hbm_copy of the extracted bytes (rounded up to its 16 KB block)
Each timed call has its own pair of HIP events and follows a 512 MiB copy that empties the Infinity
Cache of the batch.  The legs are interleaved over `--rounds` rounds of `--iters` calls; the median
call of the median round is reported, with the fastest and slowest round beside it.  Before timing,
the bound call's output is checked byte for byte against RowEncoder.extract of the same batch and of
the pattern alone.

One JSON line per case: extracted values and bytes, parent bytes, ms per leg and the three ratios
(time of the yardstick / time of extract; > 1: extract is faster).

    python scripts/bench_extract.py [--rows 1000000] [--legs extract,filter] [--out profiles/extract_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_BLOCK = 16 << 10
PATTERN = 4096
LEGS = ("extract", "extract_decode", "decode", "filter", "copy")


def deep_fields():
    from fury_amd import types as T
    inner = T.struct_field("inner", [T.field("s", T.STRING), T.array_field("v", T.INT64)])
    fx = T.struct_field("fx", [T.field("p", T.INT64), T.field("q", T.INT32)])
    m = T.map_field("m", T.field("key", T.STRING), T.field("value", T.INT32))
    return [T.field("id", T.INT64), T.struct_field("outer", [T.field("a", T.INT32), inner, fx, m])]


def foo_beans(n):
    return [{"f1": i, "f2": None if i % 3 == 0 else f"s{i}" * (i % 5),
             "f3": [f"x{j}" for j in range(i % 4)],
             "f4": [(f"k{j}", j) for j in range(i % 3)] if i % 5 else None,
             "f5": None if i % 7 == 0 else {"f1": i, "f2": "b" * (i % 11)}} for i in range(n)]


def deep_beans(n):
    def f(i):
        inner = None if i % 3 == 2 else {"s": None if i % 6 == 1 else "t" * (i % 9),
                                         "v": None if i % 8 == 3 else [i * j for j in range(i % 5)]}
        fx = None if i % 4 == 3 else {"p": i * 1000003, "q": None if i % 2 else -i}
        m = None if i % 7 == 4 else [(f"k{j}", i + j) for j in range(i % 4)]
        return {"id": i, "outer": None if i % 5 == 1 else {"a": i, "inner": inner, "fx": fx, "m": m}}
    return [f(i) for i in range(n)]


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
    assert torch.cuda.is_available(), "bench_extract.py measures on the GPU; there is no fallback"
    from fury_amd import _native as N
    from fury_amd.beans import beans_to_columns
    from fury_amd.encoder import Encoders, RowBatch, column_to_device
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

    workloads = (("foo", SCHEMAS["foo"], foo_beans, (("f5",), ("f3",))),
                 ("deep", deep_fields(), deep_beans, (("outer", "inner"),)))
    for name, fields, beans, paths in workloads:
        enc = Encoders.bean(fields, device=dev)
        host = beans_to_columns(fields, beans(PATTERN))
        pat = enc.encode_batch([column_to_device(c, dev) for c in host], PATTERN)
        batch = enc.take(pat, torch.arange(n, device=dev) % PATTERN)
        src_bytes = batch.rows.numel()
        ones = torch.full((((n + 31) // 32) * 4,), 255, dtype=torch.uint8, device=dev)
        fout = torch.empty(max(src_bytes, 16), dtype=torch.uint8, device=dev)
        foffs = torch.empty(n + 1, dtype=torch.int64, device=dev)
        fcnt = torch.zeros(1, dtype=torch.int64, device=dev)
        for path in paths:
            child = enc.child_encoder(path)
            got, _ = enc.extract(batch, path)
            count, ext_bytes = got.nrows, got.rows.numel()
            small, _ = enc.extract(pat, path)       # the batch is the pattern repeated
            assert count >= small.nrows and torch.equal(got.rows[:small.rows.numel()], small.rows)
            child.decode_batch(small)
            out = torch.empty(max(ext_bytes, 16), dtype=torch.uint8, device=dev)
            offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
            cnt = torch.zeros(1, dtype=torch.int64, device=dev)
            extract = enc.bind_extract(batch, path, out, offs, cnt)
            extract()
            enc.device_status()
            assert int(cnt.item()) == count and torch.equal(out[:ext_bytes], got.rows)
            assert torch.equal(offs[:count + 1], got.row_offsets)
            view = RowBatch(out[:ext_bytes], offs[:count + 1], count, child.schema_hash)
            cb = max((ext_bytes + COPY_BLOCK - 1) // COPY_BLOCK * COPY_BLOCK, COPY_BLOCK)
            csrc = torch.zeros(cb, dtype=torch.uint8, device=dev)
            cdst = torch.empty_like(csrc)

            def extract_decode():
                extract()
                return child.decode_batch(view)

            def copy():
                assert N.lib().fury_hbm_copy(cdst.data_ptr(), csrc.data_ptr(), cb, None) == 0

            legs = {"extract": extract, "extract_decode": extract_decode,
                    "decode": lambda: enc.decode_batch(batch),
                    "filter": lambda: enc.filter_into(batch, ones, fout, foffs, fcnt),
                    "copy": copy}
            rounds = timed({k: legs[k] for k in want_legs})
            enc.device_status()
            med = {k: statistics.median(v) for k, v in rounds.items()}
            d = {"workload": name, "rows": n, "path": ".".join(path),
                 "end": "collection" if child.schema().collection else "struct",
                 "values": count, "extracted_bytes": ext_bytes, "parent_bytes": src_bytes,
                 **{f"{k}_ms": round(med[k], 4) for k in med},
                 **{f"{k}_min_ms": round(min(rounds[k]), 4) for k in med},
                 **{f"{k}_max_ms": round(max(rounds[k]), 4) for k in med}}
            if "extract" in med:
                d["extract_GBps"] = round(2 * ext_bytes / (med["extract"] * 1e-3) / 1e9, 1)
                for k, label in (("decode", "decode_over_extract"), ("filter", "filter_over_extract"),
                                 ("copy", "copy_over_extract")):
                    if k in med:
                        d[label] = round(med[k] / med["extract"], 3)
                if "decode" in med and "extract_decode" in med:
                    d["decode_over_extract_decode"] = round(med["decode"] / med["extract_decode"], 3)
            emit(d)
            del out, csrc, cdst, got, view
        del batch, fout
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
