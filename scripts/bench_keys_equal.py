"""Key equality (fury_row_keys_equal): pairs per second and bytes touched per second (not part of
bench.py).

Key sets: (a) one INT64 key of Struct-100 (816-byte rows), (b) the keys ["a", "s1"] of C3 mixed (an
INT32 and a STRING), (c) a 64-byte STRING key of a two-field schema (id INT64, k STRING).  Each is
run at every `--pairs` count with identity pairs (no indices: pair j is row j of both sides) and with
random pairs (both sides indexed; half of the pairs name equal rows, half random ones).  The batch of
a key set has as many rows as the largest pair count -- 1M generated rows repeated by take -- and the
right side is a copy of it in memory of its own (no cache line serves both sides), so identity pairs
are all equal: every payload is read to its end.
  keys_equal     bind_keys_equal into a preallocated out_equal and out_mask, no host synchronisation
  project_torch  (a) only, the only route there was before: bind_project of the key on both sides
                 into preallocated columns, then a torch gather of both columns and a compare
Each timed call has its own pair of HIP events and follows a 512 MiB copy that empties the Infinity
Cache of the batch.  The legs are interleaved over `--rounds` rounds of `--iters` calls; the median
call of the median round is reported, with the fastest and slowest round beside it.  Before timing,
the result is checked against the pair construction (equal rows compare equal) and, for (a), against
the torch route.

One JSON line per case: min_bytes = the bytes the call must touch (per pair and side: the index
when there is one, the row offset of a variable-length schema, one bitmap word and one slot per key,
the payload bytes of STRING keys of pairs whose lengths agree; 1 byte and 1 bit of output), ms per
leg, Mpairs_per_s and GBps of keys_equal, and for (a) vs_project_torch = project_torch / keys_equal.

    python scripts/bench_keys_equal.py [--pairs 1000000 16000000] [--out profiles/keys_equal_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

BASE_ROWS = 1_000_000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[1_000_000, 16_000_000])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "bench_keys_equal.py measures on the GPU; there is no fallback"
    from bench import make_device_columns
    from fury_amd import KeySide, bind_keys_equal
    from fury_amd import _native as N
    from fury_amd import types as T
    from fury_amd.encoder import Encoders, RowBatch
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

    def string64(n):
        """(id INT64, k STRING): 64 random bytes per key, 4096 distinct keys."""
        fields = [T.not_null_field("id", T.INT64), T.field("k", T.STRING)]
        g = torch.Generator(device=dev).manual_seed(64)
        keys = torch.randint(0, 256, (4096, 64), dtype=torch.uint8, device=dev, generator=g)
        pick = torch.randint(0, 4096, (n,), device=dev, generator=g)
        cols = [Column(values=torch.arange(n, dtype=torch.int64, device=dev)),
                Column(values=keys[pick].reshape(-1),
                       offsets=(torch.arange(n + 1, dtype=torch.int64, device=dev) * 64).to(torch.int32))]
        return fields, cols

    nmax = max(args.pairs)
    cases = [("struct100_int64", "struct100", [0]), ("mixed_int32_string", "mixed", ["a", "s1"]),
             ("string64", None, ["k"])]
    for case, name, keys in cases:
        if name is None:
            fields, cols = string64(BASE_ROWS)
        else:
            fields = SCHEMAS[name]
            cols = make_device_columns(name, fields, BASE_ROWS, 0, dev)
        enc = Encoders.bean(fields, device=dev)
        sch = enc.schema()
        batch = enc.encode_batch(cols, BASE_ROWS)
        del cols
        if nmax > BASE_ROWS:                       # the 1M rows, repeated
            batch = enc.take(batch, torch.arange(nmax, device=dev) % BASE_ROWS)
        nrows = batch.nrows
        twin = RowBatch(batch.rows.clone(), None if batch.row_offsets is None else batch.row_offsets.clone(),
                        nrows, batch.schema_hash)
        idx = enc._select(keys)
        strings = [k for k in idx if fields[k].type_id in (T.STRING, T.BINARY)]
        key_cols = enc.project_batch(batch, keys)
        g = torch.Generator(device=dev).manual_seed(7)
        for pairs in args.pairs:
            for kind in ("identity", "random"):
                if kind == "identity":
                    # rows [0, pairs) of the batch, both sides
                    view = enc.slice_rows(batch, 0, pairs) if pairs < nrows else batch
                    other_view = enc.slice_rows(twin, 0, pairs) if pairs < nrows else twin
                    li = ri = None
                    same = torch.ones(pairs, dtype=torch.bool, device=dev)
                else:
                    view, other_view = batch, twin
                    li = torch.randint(0, nrows, (pairs,), device=dev, generator=g)
                    other = torch.randint(0, nrows, (pairs,), device=dev, generator=g)
                    same = torch.rand(pairs, device=dev, generator=g) < 0.5
                    ri = torch.where(same, li, other)
                eq = torch.empty(pairs, dtype=torch.uint8, device=dev)
                mask = torch.empty((pairs + 31) // 32, dtype=torch.int32, device=dev)
                call = bind_keys_equal(KeySide(enc, view, keys, li), KeySide(enc, other_view, keys, ri), eq, mask,
                                       null_equal=True)
                call()
                enc.device_status()
                assert bool(eq[same].all()), "rows compared with themselves must be equal"
                bits = (mask.view(torch.uint8).reshape(-1, 1) >> torch.arange(8, device=dev, dtype=torch.uint8)) & 1
                assert torch.equal(bits.reshape(-1)[:pairs], eq), "out_mask and out_equal differ"
                legs = {"keys_equal": call}
                L = torch.arange(pairs, device=dev) if li is None else li
                R = torch.arange(pairs, device=dev) if ri is None else ri
                if case == "struct100_int64":
                    ca = enc.project_batch(view, keys)
                    cb = enc.project_batch(other_view, keys)
                    pa, pb = enc.bind_project(view, keys, ca), enc.bind_project(other_view, keys, cb)
                    va, vb = ca[0].values.view(torch.int64), cb[0].values.view(torch.int64)

                    def project_torch():
                        pa()
                        pb()
                        return va == vb if li is None else va[li] == vb[ri]
                    assert torch.equal(project_torch().to(torch.uint8), eq), "the two routes differ"
                    legs["project_torch"] = project_torch
                # payload bytes: of the pairs whose lengths agree, both sides
                payload = 0
                for k, c in zip(idx, key_cols):
                    if k in strings:
                        lens = (c.offsets[1:] - c.offsets[:-1]).to(torch.int64)
                        agree = lens[L] == lens[R]
                        if c.validity is not None:
                            v = ((c.validity[L >> 3].to(torch.int32) >> (L & 7).to(torch.int32)) & 1) & \
                                ((c.validity[R >> 3].to(torch.int32) >> (R & 7).to(torch.int32)) & 1)
                            agree &= v.bool()
                        payload += 2 * int(lens[L][agree].sum())
                per_side = (0 if li is None else 8) + (0 if sch.is_fixed else 8) + 16 * len(idx)
                min_bytes = pairs * (2 * per_side + 1) + (pairs + 7) // 8 + payload
                rounds = timed(legs)
                enc.device_status()
                med, out = stats(rounds)
                line = {"case": case, "pairs": pairs, "kind": kind, "rows": nrows, "keys": len(idx),
                        "row_bytes": batch.rows.numel(), "equal_share": round(float(eq.float().mean()), 3),
                        "min_bytes": min_bytes, **out,
                        "Mpairs_per_s": round(pairs / (med["keys_equal"] * 1e-3) / 1e6, 1),
                        "GBps": round(min_bytes / (med["keys_equal"] * 1e-3) / 1e9, 1)}
                if "project_torch" in med:
                    line["vs_project_torch"] = round(med["project_torch"] / med["keys_equal"], 3)
                emit(line)
                del legs, call, eq, mask
        del batch, twin, key_cols
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
