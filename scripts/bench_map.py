"""Map split and join (fury_row_map_split / fury_row_map_join) against the only route to a map's key
and value arrays and back there was before -- decode_batch of the map field, then encode_batch of the
same columns -- and against fury_hbm_copy of the same output bytes, the copy bound (not part of
bench.py).

The batch: `--rows` rows of the one-field schema of `m` MAP<INT32, STRUCT{x INT64, y STRING}> of the
explode test schema (tests/test_explode_abi.py: explode_fields), a 4096-row pattern of row values
encoded once and repeated with take.  `m` is null in one row of 7 and holds 0 .. 12 entries; one value
in 4 is null.
Legs, timed in the same process, all from the same one-field rows to the same one-field rows:
  split       bind_split_map into preallocated buffers: everything the call launches (locate, compact,
              the scans, one copy over both sides), no host synchronisation
  split_keys / split_values  the same call with the other side skipped: what two calls, one per
              side, would cost against the one call that shares locate and compact
  join        bind_join_map of split's two batches into preallocated buffers (rank, rows, scan, write)
  split_join  the two calls back to back
  compose     decode_batch of the rows + encode_batch of the decoded columns as a caller runs them
              today: allocations, the prepare / measure passes and their host reads included
  copy        fury_hbm_copy of as many bytes as the rows have (rounded down to its 16 KB unit)
Each timed call has its own pair of HIP events and follows a 512 MiB copy that empties the Infinity
Cache of the batches.  The legs are interleaved over `--rounds` rounds of `--iters` calls; the median
call of the median round is reported, with the fastest and slowest round beside it.  Before timing,
join(split) and the compose route are checked byte for byte against the source rows.

One JSON line: the batch's bytes, ms per leg, GBps = (row bytes read + written by an ideal split or
join: twice) / time, and the ratios time of the yardstick / time of split_join (compose_over_split_join
> 1: split + join is faster; copy_over_split_join: the fraction of ONE copy's bound the two calls
together reach, at most 0.5).

    python scripts/bench_map.py [--rows 1000000] [--out profiles/map_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PATTERN = 4096
LEGS = ("split", "split_keys", "split_values", "join", "split_join", "compose", "copy")


def map_field():
    from fury_amd import types as T
    val = T.struct_field("value", [T.field("x", T.INT64), T.field("y", T.STRING)])
    return T.map_field("m", T.field("key", T.INT32), val)


def beans(n):
    return [{"m": None if i % 7 == 3 else
             [(j - 7, None if j % 4 == 1 else {"x": i * 1000003 + j, "y": None if j % 5 == 0 else "y" * (j % 9)})
              for j in range(i % 13)]} for i in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--legs", default=",".join(LEGS), help="comma-separated subset of the legs")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    want_legs = [x for x in args.legs.split(",") if x]
    assert set(want_legs) <= set(LEGS), f"legs are {LEGS}"

    import torch
    assert torch.cuda.is_available(), "bench_map.py measures on the GPU; there is no fallback"
    from fury_amd import _native as N
    from fury_amd.beans import beans_to_columns
    from fury_amd.encoder import Encoders, column_to_device
    dev = torch.device("cuda:0")
    n = args.rows

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

    fields = [map_field()]
    enc = Encoders.bean(fields, device=dev)
    cols = [column_to_device(c, dev) for c in beans_to_columns(fields, beans(PATTERN))]
    rows = enc.take(enc.encode_batch(cols, PATTERN), torch.arange(n, device=dev) % PATTERN)
    del cols
    row_bytes = rows.rows.numel()
    keys, vals, _, valid = enc.split_map(rows, "m")
    count, kt, vt = keys.nrows, keys.rows.numel(), vals.rows.numel()

    i64 = lambda k: torch.empty(k, dtype=torch.int64, device=dev)         # noqa: E731
    u8 = lambda k: torch.empty(max(k, 16), dtype=torch.uint8, device=dev)  # noqa: E731
    kout, vout, ko, vo, cnt, idx = u8(kt), u8(vt), i64(n + 1), i64(n + 1), i64(1), i64(n)
    vbits = torch.zeros(((n + 31) // 32) * 4, dtype=torch.uint8, device=dev)
    split = enc.bind_split_map(rows, "m", kout, ko, vout, vo, cnt, idx, vbits)
    split()
    enc.device_status()
    assert int(cnt.item()) == count and torch.equal(kout[:kt], keys.rows) and \
        torch.equal(vout[:vt], vals.rows), "the bound split differs from split_map"
    from fury_amd.encoder import RowBatch
    kb, vb = RowBatch(kout[:kt], ko, n, 0), RowBatch(vout[:vt], vo, n, 0)      # num_values = nrows
    out, offs = u8(row_bytes), i64(n + 1)
    join = enc.bind_join_map(kb, vb, out, offs, vbits, n)
    join()
    enc.device_status()
    assert torch.equal(out[:row_bytes], rows.rows) and torch.equal(offs, rows.row_offsets), \
        "join(split) differs from the source rows"

    k2, v2, o2 = u8(kt), u8(vt), i64(n + 1)
    split_keys = enc.bind_split_map(rows, "m", k2, o2, None, None, cnt, None, None)
    split_values = enc.bind_split_map(rows, "m", None, None, v2, o2, cnt, None, None)

    def split_join():
        split()
        join()

    def compose():
        return enc.encode_batch(enc.decode_batch(rows), n)

    got = compose()
    assert torch.equal(got.rows, rows.rows) and torch.equal(got.row_offsets, rows.row_offsets), \
        "decode + encode differs from the source rows"
    del got
    cdst = torch.empty_like(out)
    copy_bytes = row_bytes & ~0x3FFF           # fury_hbm_copy takes multiples of 16 KB
    assert copy_bytes > 0, "too few rows for the copy leg"

    def copy():
        assert N.lib().fury_hbm_copy(cdst.data_ptr(), rows.rows.data_ptr(), copy_bytes, None) == 0

    legs = {"split": split, "split_keys": split_keys, "split_values": split_values, "join": join,
            "split_join": split_join, "compose": compose, "copy": copy}
    legs = {k: v for k, v in legs.items() if k in want_legs}
    rounds = timed(legs)
    enc.device_status()
    med = {k: statistics.median(v) for k, v in rounds.items()}
    line = {"workload": "explode_fields", "rows": n, "field": "m", "maps": count,
            "row_bytes": row_bytes, "key_bytes": kt, "value_bytes": vt,
            **{f"{k}_ms": round(med[k], 4) for k in med},
            **{f"{k}_min_ms": round(min(rounds[k]), 4) for k in med},
            **{f"{k}_max_ms": round(max(rounds[k]), 4) for k in med}}
    for k in ("split", "join", "copy"):
        if k in med:
            line[f"{k}_GBps"] = round(2 * row_bytes / (med[k] * 1e-3) / 1e9, 1)
    if "split_join" in med:
        for k in ("compose", "copy"):
            if k in med:
                line[f"{k}_over_split_join"] = round(med[k] / med["split_join"], 3)
        if "compose" in med:
            line["split_join_max_le_compose_min"] = max(rounds["split_join"]) <= min(rounds["compose"])
    s = json.dumps(line)
    print(s, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
