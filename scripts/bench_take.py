"""Row selection (fury_row_take / fury_row_filter) against a plain copy of the same bytes and against
the only route there was before: decode, index every column with torch, encode (not part of bench.py).

Workloads: Struct-100 (816-byte rows) and C3 mixed (3 numbers + 3 strings), 1M rows each.  Cases:
filter at 10 %, 50 % and 100 % of the rows selected (random mask) and take with a random permutation.
Per case three legs are timed in the same process:
  select     filter_into / bind_take into preallocated buffers: everything the call launches (mask
             compaction, sizes, scan, copy), no host synchronisation
  copy       fury_hbm_copy of the same number of bytes (rounded up to its 16 KB block): the roofline
  roundtrip  decode_batch of the whole batch, torch indexing of every column (validity bits and string
             payloads included), encode_batch of the result
Each timed call has its own pair of HIP events and follows a 512 MiB copy that empties the Infinity
Cache of the batch.  The legs are interleaved over `--rounds` rounds of `--iters` calls; the median
call of the median round is reported, with the fastest and slowest round beside it.  Before timing,
the selected batch is checked byte for byte against the round trip's batch.

One JSON line per case: selected rows and bytes, ms per leg, GBps = 2 x selected bytes / time (read +
write; the 8-16 bytes of offsets per row are not counted), the ratio to the copy and to the round trip.

    python scripts/bench_take.py [--rows 1000000] [--out profiles/take_bench.jsonl]
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


def pack_bits(torch, m):
    """A bool tensor as an LSB-first bitmap of whole 32-bit words."""
    n = m.numel()
    w = torch.zeros(((n + 31) // 32) * 32, dtype=torch.uint8, device=m.device)
    w[:n] = m
    k = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=m.device)
    return (w.reshape(-1, 8) * k).sum(dim=1, dtype=torch.int32).to(torch.uint8)


def unpack_bits(torch, b, n):
    k = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=b.device)
    return ((b.reshape(-1, 1) & k) != 0).reshape(-1)[:n]


def index_column(torch, f, c, n, idx):
    """Column `c` (n entries of field `f`) gathered at rows `idx`, with torch ops only."""
    from fury_amd.types import BINARY, BOOL, STRING, type_width
    from fury_amd.workloads import Column
    val = None if c.validity is None else pack_bits(torch, unpack_bits(torch, c.validity, n)[idx])
    if f.type_id == BOOL:
        return Column(values=pack_bits(torch, unpack_bits(torch, c.values, n)[idx]), validity=val)
    w = type_width(f.type_id)
    if w > 0:
        return Column(values=c.values.view(torch.uint8)[:n * w].reshape(n, w)[idx].reshape(-1), validity=val)
    assert f.type_id in (STRING, BINARY), f"no torch gather for field {f.name}"
    offs = c.offsets[:n + 1].to(torch.int64)
    lens = (offs[1:] - offs[:-1])[idx]
    new = torch.zeros(idx.numel() + 1, dtype=torch.int64, device=idx.device)
    torch.cumsum(lens, 0, out=new[1:])
    total = int(new[-1].item())
    at = torch.repeat_interleave(offs[:-1][idx] - new[:-1], lens) + torch.arange(total, device=idx.device)
    return Column(values=c.values.view(torch.uint8)[at], validity=val, offsets=new.to(torch.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "bench_take.py measures on the GPU; there is no fallback"
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

    g = torch.Generator(device=dev)
    g.manual_seed(20240607)
    for name in ("struct100", "mixed"):
        fields = SCHEMAS[name]
        enc = Encoders.bean(fields, device=dev)
        fixed = enc.schema().is_fixed
        batch = enc.encode_batch(make_device_columns(name, fields, n, 0, dev), n)
        src_bytes = batch.rows.numel()
        cases = [(f"filter_{p}", torch.rand(n, generator=g, device=dev) < p / 100.0 if p < 100
                  else torch.ones(n, dtype=torch.bool, device=dev)) for p in (10, 50, 100)]
        cases.append(("take_permutation", torch.randperm(n, generator=g, device=dev)))
        for case, sel in cases:
            is_filter = sel.dtype == torch.bool
            idx = torch.nonzero(sel).reshape(-1) if is_filter else sel
            m = idx.numel()

            def roundtrip():
                cols = enc.decode_batch(batch)
                return enc.encode_batch([index_column(torch, f, c, n, idx) for f, c in zip(fields, cols)], m)

            want = roundtrip()
            sel_bytes = want.rows.numel()
            out = torch.empty(max(src_bytes, 16), dtype=torch.uint8, device=dev)
            if is_filter:
                mask = pack_bits(torch, sel)
                offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
                cnt = torch.zeros(1, dtype=torch.int64, device=dev)

                def select():
                    enc.filter_into(batch, mask, out, None if fixed else offs, cnt)
            else:
                offs = torch.empty(m + 1, dtype=torch.int64, device=dev)
                select = enc.bind_take(batch, idx, out, None if fixed else offs)
            select()
            enc.device_status()
            assert not is_filter or int(cnt.item()) == m
            assert torch.equal(out[:sel_bytes], want.rows), f"{name} {case}: selected rows differ"
            if not fixed:
                assert torch.equal(offs[:m + 1], want.row_offsets), f"{name} {case}: offsets differ"
            cb = max((sel_bytes + COPY_BLOCK - 1) // COPY_BLOCK * COPY_BLOCK, COPY_BLOCK)
            csrc = torch.zeros(cb, dtype=torch.uint8, device=dev)
            cdst = torch.empty_like(csrc)

            def copy():
                assert N.lib().fury_hbm_copy(cdst.data_ptr(), csrc.data_ptr(), cb, None) == 0

            rounds = timed({"select": select, "copy": copy, "roundtrip": roundtrip})
            enc.device_status()
            med = {k: statistics.median(v) for k, v in rounds.items()}
            rate = {k: round(2 * sel_bytes / (med[k] * 1e-3) / 1e9, 1) for k in med}
            emit({"workload": name, "rows": n, "case": case, "selected_rows": m,
                  "selected_bytes": sel_bytes,
                  **{f"{k}_ms": round(med[k], 4) for k in med},
                  **{f"{k}_min_ms": round(min(rounds[k]), 4) for k in med},
                  **{f"{k}_max_ms": round(max(rounds[k]), 4) for k in med},
                  **{f"{k}_GBps": rate[k] for k in med},
                  "vs_copy": round(med["copy"] / med["select"], 3),
                  "speedup_vs_roundtrip": round(med["roundtrip"] / med["select"], 2),
                  "beats_roundtrip": max(rounds["select"]) < min(rounds["roundtrip"])})
            del out, csrc, cdst, want
        del batch
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
