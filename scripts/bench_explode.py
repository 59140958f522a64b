"""Element explosion (fury_row_explode) against the only route to the elements of a list there was
before -- decode_batch of the whole parent batch --, against fury_row_extract of the same field (the
same bytes moved as whole arrays) and against a plain copy of the bytes moved (not part of bench.py).

Cases, `--rows` rows each of {id INT64, items LIST<STRUCT{a INT32, s STRING}>, note STRING} (a
4096-row pattern of row values, encoded once and repeated with take):
  uniform  row i holds i mod 8 elements
  skewed   one row in 4096 holds 4096 elements, the others none
Per case these legs are timed in the same process:
  explode          bind_explode into preallocated buffers with elem_capacity = rows bytes / 8, the bound
                   the host knows without a synchronisation: everything the call launches (count,
                   locate, compact, three scans, copy)
  explode_exact    the same with elem_capacity = the element count (what a caller that has run the
                   count form passes)
  explode_project  explode followed by the element encoder's project_batch of field a
  decode           decode_batch of the parent batch
  extract          bind_extract of items
  copy             fury_hbm_copy of the bytes explode moves (rounded up to its 16 KB block)
Each timed call has its own pair of HIP events and follows a 512 MiB copy that empties the Infinity
Cache of the batch.  The legs are interleaved over `--rounds` rounds of `--iters` calls; the median
call of the median round is reported, with the fastest and slowest round beside it.  Before timing,
the bound call's outputs are checked against RowEncoder.explode of the same batch, byte for byte.

One JSON line per case: elements, entries and bytes, ms per leg, ns per element and the ratios (time
of the yardstick / time of explode; > 1: explode is faster).

    python scripts/bench_explode.py [--rows 1000000] [--legs explode,decode] [--cases uniform]
                                    [--out profiles/explode_bench.jsonl]
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
LEGS = ("explode", "explode_exact", "explode_project", "decode", "extract", "copy")


def fields():
    from fury_amd import types as T
    item = T.struct_field("item", [T.field("a", T.INT32), T.field("s", T.STRING)])
    return [T.field("id", T.INT64), T.Field("items", T.LIST, True, (item,)), T.field("note", T.STRING)]


def _item(i, j):
    return None if (i + j) % 13 == 0 else {"a": i * 131 + j, "s": None if j % 5 == 0 else "s" * (j % 7)}


def uniform_beans(n):
    return [{"id": i, "items": None if i % 11 == 3 else [_item(i, j) for j in range(i % 8)],
             "note": "n" * (i % 9)} for i in range(n)]


def skewed_beans(n):
    return [{"id": i, "items": [_item(i, j) for j in range(4096 if i % 4096 == 0 else 0)],
             "note": "n" * (i % 9)} for i in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--legs", default=",".join(LEGS), help="comma-separated subset of the legs")
    ap.add_argument("--cases", default="uniform,skewed", help="comma-separated subset of the cases")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    want_legs = [x for x in args.legs.split(",") if x]
    assert set(want_legs) <= set(LEGS), f"legs are {LEGS}"
    want_cases = [x for x in args.cases.split(",") if x]
    assert set(want_cases) <= {"uniform", "skewed"}, "cases are uniform, skewed"

    import torch
    assert torch.cuda.is_available(), "bench_explode.py measures on the GPU; there is no fallback"
    from fury_amd import _native as N
    from fury_amd.beans import beans_to_columns
    from fury_amd.encoder import Encoders, RowBatch, column_to_device
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

    enc = Encoders.bean(fields(), device=dev)
    child = enc.element_encoder("items")
    for name, beans in (("uniform", uniform_beans), ("skewed", skewed_beans)):
        if name not in want_cases:
            continue
        host = beans_to_columns(fields(), beans(PATTERN))
        pat = enc.encode_batch([column_to_device(c, dev) for c in host], PATTERN)
        batch = enc.take(pat, torch.arange(n, device=dev) % PATTERN)
        src_bytes = batch.rows.numel()
        got, glo, gev, gvalid, gpar, gord = enc.explode(batch, "items")
        count, out_bytes, E = got.nrows, got.rows.numel(), int(glo[n].item())
        bound = src_bytes // 8
        assert E <= bound

        def buffers(ecap):
            i64 = lambda k: torch.empty(k, dtype=torch.int64, device=dev)   # noqa: E731
            return dict(lo=i64(n + 1), ev=torch.zeros(((n + 31) // 32) * 4, dtype=torch.uint8, device=dev),
                        out=torch.empty(max(out_bytes, 16), dtype=torch.uint8, device=dev),
                        offs=i64(ecap + 1), cnt=i64(1), par=i64(max(ecap, 1)),
                        ords=torch.empty(max(ecap, 1), dtype=torch.int32, device=dev),
                        val=torch.zeros(((ecap + 31) // 32) * 4 + 4, dtype=torch.uint8, device=dev))

        def bind(b, ecap):
            return enc.bind_explode(batch, "items", b["lo"], b["ev"], b["out"], b["offs"], b["cnt"],
                                    b["par"], b["ords"], b["val"][:((ecap + 31) // 32) * 4],
                                    elem_capacity=ecap)

        calls = {}
        for leg, ecap in (("explode", bound), ("explode_exact", E)):
            b = buffers(ecap)
            calls[leg] = bind(b, ecap)
            calls[leg]()
            enc.device_status()
            assert int(b["cnt"].item()) == count and torch.equal(b["out"][:out_bytes], got.rows)
            assert torch.equal(b["offs"][:count + 1], got.row_offsets) and torch.equal(b["lo"], glo)
            assert torch.equal(b["par"][:count], gpar) and torch.equal(b["ords"][:count], gord)
            assert torch.equal(b["val"][:(E + 7) // 8], gvalid)
            assert torch.equal(b["ev"][:(n + 7) // 8], gev)
            if leg == "explode":
                view = RowBatch(b["out"][:out_bytes], b["offs"][:count + 1], count, child.schema_hash)
        child.project_batch(view, ["a"])

        arrays, _ = enc.extract(batch, "items")
        xout = torch.empty(max(arrays.rows.numel(), 16), dtype=torch.uint8, device=dev)
        xoffs = torch.empty(n + 1, dtype=torch.int64, device=dev)
        xcnt = torch.zeros(1, dtype=torch.int64, device=dev)
        extract = enc.bind_extract(batch, "items", xout, xoffs, xcnt)
        cb = max((out_bytes + COPY_BLOCK - 1) // COPY_BLOCK * COPY_BLOCK, COPY_BLOCK)
        csrc = torch.zeros(cb, dtype=torch.uint8, device=dev)
        cdst = torch.empty_like(csrc)

        def explode_project():
            calls["explode"]()
            return child.project_batch(view, ["a"])

        def copy():
            assert N.lib().fury_hbm_copy(cdst.data_ptr(), csrc.data_ptr(), cb, None) == 0

        legs = {"explode": calls["explode"], "explode_exact": calls["explode_exact"],
                "explode_project": explode_project, "decode": lambda: enc.decode_batch(batch),
                "extract": extract, "copy": copy}
        rounds = timed({k: legs[k] for k in want_legs})
        enc.device_status()
        med = {k: statistics.median(v) for k, v in rounds.items()}
        d = {"case": name, "rows": n, "elements": E, "entries": count, "elem_capacity": bound,
             "exploded_bytes": out_bytes, "extracted_bytes": arrays.rows.numel(),
             "parent_bytes": src_bytes,
             **{f"{k}_ms": round(med[k], 4) for k in med},
             **{f"{k}_min_ms": round(min(rounds[k]), 4) for k in med},
             **{f"{k}_max_ms": round(max(rounds[k]), 4) for k in med}}
        if "explode" in med:
            d["explode_ns_per_element"] = round(med["explode"] * 1e6 / max(E, 1), 3)
            for k in ("explode_exact", "decode", "extract", "copy"):
                if k in med:
                    d[f"{k}_over_explode"] = round(med[k] / med["explode"], 3)
        if "explode_exact" in med:
            d["explode_exact_ns_per_element"] = round(med["explode_exact"] * 1e6 / max(E, 1), 3)
        if "decode" in med and "explode_project" in med:
            d["decode_over_explode_project"] = round(med["decode"] / med["explode_project"], 3)
        emit(d)
        del batch, got, arrays, xout, csrc, cdst, calls, view
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
