"""In-place update against the decode + encode round trip of the same batch (not part of bench.py).

Struct-100, 1M rows: selections of k = 1, 3, 8, 32 fields, adjacent (slots 0..k-1) and spread evenly
over the 100 slots.  Per selection three things are timed:
  update     fury_row_update of the k fields from fresh columns (no validity: every value valid)
  project    fury_row_project of the same selection -- the update's read-side mirror
and once per run
  roundtrip  fury_row_decode of the whole batch + fury_row_encode of all 100 columns back into it:
             what a caller had to run for the same job before fury_row_update existed.
Every leg is a bound call (argument block built once); each timed call has its own pair of HIP
events and follows a 512 MiB copy that empties the Infinity Cache of the batch.  The legs are
interleaved over `--rounds` rounds of `--iters` calls in one process; the median call of the median
round is reported, with the fastest and slowest round beside it.  Before timing, every update is
checked: the full decode of the updated batch equals the old columns with the selected ones replaced.

One JSON line per leg with the bytes model beside the time:
  segments_per_row   128-byte segments of the row buffer holding a byte the selection touches
                     (bitmap words + slots; the batch's rows packed back to back), per row
  model_bytes        update: 128 * segments written (a partial-line store is counted as its line)
                     + 8 * bitmap words read per row + the input column bytes
  GBps_model         model_bytes / time
and a last line with the copy rate (fury_hbm_copy) and the crossover against the round trip.

    python scripts/bench_update.py [--rows 1000000] [--out profiles/update_struct100.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    import statistics

    import torch
    assert torch.cuda.is_available(), "bench_update.py measures on the GPU; there is no fallback"
    from bench import copy_rate, make_device_columns
    from bench_project import column_bytes, same, segments_per_row
    from fury_amd import _native as N
    from fury_amd.encoder import Encoders
    from fury_amd.workloads import SCHEMAS, gen_columns_torch
    dev = torch.device("cuda:0")
    n = args.rows
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    copy = copy_rate(dev, torch.cuda.current_stream(dev))
    emit({"copy_rate": copy})
    fsrc = torch.zeros(512 << 20, dtype=torch.uint8, device=dev)
    fdst = torch.empty_like(fsrc)

    def flush():
        assert N.lib().fury_hbm_copy(fdst.data_ptr(), fsrc.data_ptr(), fsrc.numel(), None) == 0

    fields = SCHEMAS["struct100"]
    enc = Encoders.bean(fields, device=dev)
    schema = enc.schema()
    current = make_device_columns("struct100", fields, n, 0, dev)     # what the batch holds
    fresh = gen_columns_torch("struct100", fields, n, seed=99, start=0, device=dev)
    batch = enc.encode_batch(current, n)
    full = enc.alloc_columns(n, validity=False)
    decode = enc.bind_decode(batch, full)
    encode = enc.bind_encode(full, n, batch.rows)
    current = list(current)

    def roundtrip():
        decode()
        encode()

    legs = {"roundtrip": roundtrip}
    meta = {"roundtrip": {"k": 100, "shape": "decode + encode", "segments_per_row": schema.fixed_size / 128.0,
                          "model_bytes": 2 * (n * schema.fixed_size + column_bytes(fields, range(100), n, False))}}
    for k in (1, 3, 8, 32):
        for shape in ("adjacent", "spread"):
            idx = list(range(k)) if shape == "adjacent" else [(2 * j + 1) * 100 // (2 * k) for j in range(k)]
            assert len(set(idx)) == k
            cols = [fresh[j] for j in idx]
            upd = enc.bind_update(batch, idx, cols)
            upd()
            enc.device_status()
            for j in idx:
                current[j] = fresh[j]
            decode()
            enc.device_status()
            assert same(torch, full, current), f"k={k} {shape}: the updated batch differs"
            outs = enc.alloc_projected(idx, n, validity=False)
            seg = segments_per_row(schema, idx)
            nbw = len({j >> 6 for j in idx})
            name = f"k{k}_{shape}"
            legs["update_" + name] = upd
            legs["project_" + name] = enc.bind_project(batch, idx, outs)
            common = {"k": k, "shape": shape, "segments_per_row": round(seg, 3)}
            meta["update_" + name] = {**common, "model_bytes": int(n * 128 * seg) + 8 * nbw * n +
                                      column_bytes(fields, idx, n, False)}
            meta["project_" + name] = {**common, "model_bytes": int(n * 128 * seg) +
                                       column_bytes(fields, idx, n, False)}
    # interleaved rounds: per leg the median call of every round
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
    enc.device_status()
    med = {name: statistics.median(v) for name, v in rounds.items()}
    rt = med["roundtrip"]
    for name, v in rounds.items():
        m = meta[name]
        emit({"workload": "struct100", "rows": n, "leg": name, **m, "ms": round(med[name], 4),
              "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
              "GBps_model": round(m["model_bytes"] / (med[name] * 1e-3) / 1e9, 1),
              "vs_roundtrip": round(med[name] / rt, 3)})
    cross = {}
    for shape in ("adjacent", "spread"):
        ks = sorted((meta[x]["k"], max(rounds[x])) for x in legs
                    if x.startswith("update_") and meta[x]["shape"] == shape)
        lose = [k for k, slowest in ks if slowest >= min(rounds["roundtrip"])]
        cross[shape] = lose[0] if lose else None
    emit({"workload": "struct100", "rows": n, "roundtrip_ms": round(rt, 4),
          "roundtrip_min_ms": round(min(rounds["roundtrip"]), 4),
          "roundtrip_max_ms": round(max(rounds["roundtrip"]), 4), "crossover_k": cross,
          "what": "crossover_k: the smallest measured k at which the update's slowest round is no "
                  "faster than the round trip's fastest round (null: the update wins at every "
                  "measured k, by more than the spread between rounds)"})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
