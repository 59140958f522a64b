"""Projected decode against the full decode of the same batch (not part of bench.py).

Struct-100, 1M rows: selections of k = 1, 3, 8, 32, 100 fields, adjacent (slots 0..k-1) and spread
evenly over the 100 slots; then `mixed`, 1M rows, projecting [a, s2].  Every leg is a bound call
(argument block built once); each timed call has its own pair of HIP events and follows a 512 MiB
copy that empties the Infinity Cache of the batch.  The legs of a workload are interleaved over
`--rounds` rounds of `--iters` calls in one process; the median call of the median round is reported.
The outputs of every projected leg are checked against the full decode's columns before timing.

One JSON line per leg with the bytes model beside the time:
  segments_per_row   128-byte segments of the row buffer holding a byte the selection reads
                     (bitmap words + slots; the batch's rows packed back to back), per row
  model_bytes        128 * segments + column bytes written (+ payload read and written, offsets)
  GBps_model         model_bytes / time
and a last line per workload with the copy rate (fury_hbm_copy) and the crossover k.

    python scripts/bench_project.py [--rows 1000000] [--out profiles/project_struct100.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAX_SELECT = 64      # fields per fury_row_project call; wider selections run as several calls


def segments_per_row(schema, idx, offs=None, sample=4096):
    """128-byte segments touched per row by the header words of `idx`, counted over `sample`
    consecutive rows (neighbouring rows share segments)."""
    import numpy as np
    words = sorted({k >> 6 for k in idx} | {schema.bitmap_bytes // 8 + k for k in idx})
    if offs is None:
        base = np.arange(sample, dtype=np.int64) * schema.fixed_size
    else:
        base = np.asarray(offs[:sample], dtype=np.int64)
    seg = (base[:, None] + 8 * np.asarray(words, dtype=np.int64)[None, :]) >> 7
    return len(np.unique(seg)) / len(base)


def column_bytes(fields, idx, n, validity):
    from fury_amd.types import BOOL, type_width
    total = 0
    for k in idx:
        t = fields[k].type_id
        total += (n + 7) // 8 if t == BOOL else n * max(type_width(t), 0)
        if validity:
            total += (n + 7) // 8
    return total


def time_legs(torch, legs, rounds, iters, flush):
    """legs: name -> callable.  Interleaved rounds; ms per call, median and min over the rounds.
    Every timed call has its own pair of events and follows `flush()` (a 512 MiB copy), so the
    segments a small selection touches (k <= 8 adjacent: under 256 MB) are not served from the
    Infinity Cache by the call before it -- a user projects a batch once."""
    times = {k: [] for k in legs}
    for call in legs.values():
        call()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, call in legs.items():
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
            times[name].append(statistics.median(a.elapsed_time(b) for a, b in ev))
    return {k: (statistics.median(v), min(v)) for k, v in times.items()}


def same(torch, a, b):
    for x, y in zip(a, b):
        for p, q in ((x.values, y.values), (x.validity, y.validity), (x.offsets, y.offsets)):
            if p is not None and q is not None and not torch.equal(p.view(torch.uint8)[:q.numel() * q.element_size()],
                                                                 q.view(torch.uint8)):
                return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_project.py measures on the GPU; there is no fallback"
    from bench import copy_rate, make_device_columns
    from fury_amd.encoder import Encoders
    from fury_amd.workloads import SCHEMAS
    dev = torch.device("cuda:0")
    n = args.rows
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    copy = copy_rate(dev, torch.cuda.current_stream(dev))
    emit({"copy_rate": copy})
    from fury_amd import _native as N
    fsrc = torch.zeros(512 << 20, dtype=torch.uint8, device=dev)
    fdst = torch.empty_like(fsrc)

    def flush():
        assert N.lib().fury_hbm_copy(fdst.data_ptr(), fsrc.data_ptr(), fsrc.numel(), None) == 0

    # ---- Struct-100 -------------------------------------------------------------------------
    fields = SCHEMAS["struct100"]
    enc = Encoders.bean(fields, device=dev)
    batch = enc.encode_batch(make_device_columns("struct100", fields, n, 0, dev), n)
    full = enc.alloc_columns(n, validity=False)
    enc.decode_into(batch, full)
    torch.cuda.synchronize()
    legs = {"full": enc.bind_decode(batch, full)}
    meta = {"full": {"k": 100, "shape": "full decode", "calls": 1,
                     "segments_per_row": enc.schema().fixed_size / 128.0,
                     "model_bytes": n * enc.schema().fixed_size + column_bytes(fields, range(100), n, False)}}
    for k in (1, 3, 8, 32, 100):
        for shape in ("adjacent", "spread"):
            if k == 100 and shape == "spread":
                continue
            idx = list(range(k)) if shape == "adjacent" else [(2 * j + 1) * 100 // (2 * k) for j in range(k)]
            assert len(set(idx)) == k
            chunks = [idx[i:i + MAX_SELECT] for i in range(0, k, MAX_SELECT)]
            outs = [enc.alloc_projected(c, n, validity=False) for c in chunks]
            calls = [enc.bind_project(batch, c, o) for c, o in zip(chunks, outs)]
            for c in calls:
                c()
            enc.device_status()
            for c, o in zip(chunks, outs):
                assert same(torch, o, [full[j] for j in c]), f"k={k} {shape}: output differs"
            name = f"k{k}_{shape}"
            legs[name] = (lambda cs: lambda: [c() for c in cs])(calls)
            seg = sum(segments_per_row(enc.schema(), c) for c in chunks)
            meta[name] = {"k": k, "shape": shape, "calls": len(chunks), "segments_per_row": round(seg, 3),
                          "model_bytes": int(n * 128 * seg) + column_bytes(fields, idx, n, False)}
    res = time_legs(torch, legs, args.rounds, args.iters, flush)
    full_ms = res["full"][0]
    cross = None
    for name, (med, mn) in res.items():
        m = meta[name]
        emit({"workload": "struct100", "rows": n, "leg": name, **m, "ms": round(med, 4),
              "min_ms": round(mn, 4), "GBps_model": round(m["model_bytes"] / (med * 1e-3) / 1e9, 1),
              "vs_full": round(med / full_ms, 3)})
    for shape in ("adjacent", "spread"):
        ks = sorted((meta[x]["k"], res[x][0]) for x in res if meta[x]["shape"] == shape)
        lose = [k for k, ms in ks if ms >= full_ms]
        cross = {**(cross or {}), shape: (lose[0] if lose else None)}
    emit({"workload": "struct100", "rows": n, "full_ms": round(full_ms, 4),
          "full_fraction_of_copy": round(meta["full"]["model_bytes"] / (full_ms * 1e-3) / 1e9 / copy["GBps"], 3),
          "crossover_k": cross,
          "what": "crossover_k: the smallest measured k at which the projection is no faster than "
                  "the full decode (null: it wins at every measured k)"})

    # ---- mixed: [a, s2] -----------------------------------------------------------------------
    fields = SCHEMAS["mixed"]
    enc = Encoders.bean(fields, device=dev)
    batch = enc.encode_batch(make_device_columns("mixed", fields, n, 0, dev), n)
    full = enc.decode_batch(batch)
    sel = ["a", "s2"]
    idx = enc._select(sel)
    out = enc.project_batch(batch, sel)
    assert same(torch, out, [full[j] for j in idx]), "mixed [a, s2]: output differs"
    legs = {"full": enc.bind_decode(batch, full), "project_a_s2": enc.bind_project(batch, sel, out)}
    res = time_legs(torch, legs, args.rounds, args.iters, flush)
    row_bytes = int(batch.rows.numel())
    pay_all = sum(int(full[j].values.numel()) for j in (3, 4, 5))
    pay = int(out[1].values.numel())
    offs = batch.row_offsets[:4097].cpu().numpy()
    seg = segments_per_row(enc.schema(), idx, offs, 4096)
    seg_count = segments_per_row(enc.schema(), [idx[1]], offs, 4096)
    model = {"full": row_bytes + 8 * (n + 1) + column_bytes(fields, range(6), n, True) + pay_all + 3 * 4 * (n + 1),
             # count pass (s2's words) + write pass (all words) + row offsets twice + payload in and
             # out + the columns
             "project_a_s2": int(n * 128 * (seg + seg_count)) + 2 * 8 * (n + 1) + 2 * pay +
                             column_bytes(fields, idx, n, True) + 4 * (n + 1)}
    for name, (med, mn) in res.items():
        emit({"workload": "mixed", "rows": n, "leg": name, "select": sel if name != "full" else None,
              "segments_per_row": round(seg, 3) if name != "full" else None,
              "model_bytes": model[name], "ms": round(med, 4), "min_ms": round(mn, 4),
              "GBps_model": round(model[name] / (med * 1e-3) / 1e9, 1),
              "vs_full": round(med / res["full"][0], 3)})
    enc.device_status()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
