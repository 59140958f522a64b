"""bench.py's --dump-outputs and --full.

CPU: dump_outputs writes float32 / float64 arrays, whole when they fit the budget, else a seeded
sample plus block sums that cover every element, the same from call to call and within budget.
GPU: a plain `bench.py --dump-outputs DIR` run writes the rows and the decoded columns its last
timed step computed -- the rows the oracle encodes from the same seeded columns, the columns the
oracle decodes from them -- and its line carries none of the figures that --full adds; a --full
run carries all of them."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ROWS = 3001          # odd, several workgroups, small enough that every array is dumped whole


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_whole_then_sampled(tmp_path):
    import torch
    import bench
    g = torch.Generator().manual_seed(5)
    named = [("bytes", torch.randint(0, 256, (100_003,), dtype=torch.uint8, generator=g)),
             ("offs", torch.arange(0, 3 * 20_001, 3, dtype=torch.int32)),
             ("tiny", torch.arange(7, dtype=torch.uint8))]
    bench.dump_outputs(str(tmp_path / "whole"), named)
    w = _load(tmp_path / "whole")
    assert sorted(w) == ["bytes", "offs", "tiny"]
    assert w["bytes"].dtype == np.float32 and w["offs"].dtype == np.float64
    for name, t in named:
        assert np.array_equal(w[name], t.numpy().astype(np.float64)), name

    budget = 64_000
    for k in "ab":
        bench.dump_outputs(str(tmp_path / k), named, budget=budget)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["bytes", "bytes.blocksum", "offs", "offs.blocksum", "tiny"]
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert sum(v.nbytes for v in a.values()) <= budget
    for name, t in named[:2]:
        x = t.numpy().astype(np.int64)
        s = a[name]
        assert 0 < s.size < x.size and s.size % bench.DUMP_CHUNK == 0
        # every sampled run is a run of the buffer (the last one zero-padded past its end)
        runs = np.pad(x, (0, -x.size % bench.DUMP_CHUNK)).reshape(-1, bench.DUMP_CHUNK)
        have = {r.tobytes() for r in runs}
        assert all(r.astype(np.int64).tobytes() in have for r in s.reshape(-1, bench.DUMP_CHUNK))
        assert a[name + ".blocksum"].dtype == np.float64
    # the block sums cover every element: changing any one of them changes a sum
    for i in (0, 50_001, 100_002):
        t = named[0][1].clone()
        t[i] ^= 1
        bench.dump_outputs(str(tmp_path / "c"), [("bytes", t)] + named[1:], budget=budget)
        c = _load(tmp_path / "c")
        assert (c["bytes.blocksum"] != a["bytes.blocksum"]).sum() == 1, i
        assert np.array_equal(c["offs.blocksum"], a["offs.blocksum"])
    x = named[0][1].numpy().astype(np.int64)
    want = (np.pad(x, (0, -x.size % 1000)) * (np.arange(101_000) % 1000 % 251 + 1))
    assert np.array_equal(bench._blocksums(named[0][1], 1000).numpy(),
                          want.reshape(-1, 1000).sum(1))


def _bench(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps",
                        "2", "--warmup", "1", "--rows", str(ROWS)] + list(args),
                       capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    out = p.stdout.strip().splitlines()
    assert len(out) == 1, out
    return json.loads(out[0])


def _columns(fields, dump, n, path=""):
    from fury_amd.types import LIST
    from fury_amd.workloads import Column
    cols = []
    for f in fields:
        p = path + f.name

        def get(what, dtype):
            a = dump.get(f"{p}.{what}")
            return None if a is None else a.astype(dtype)
        c = Column(values=get("values", np.uint8), validity=get("validity", np.uint8),
                   offsets=get("offsets", np.int32))
        if f.type_id == LIST:
            c.child = _columns(f.children[:1], dump, int(c.offsets[n]), p + ".")
        cols.append(c)
    return cols


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["struct100", "mixed", "nested"])
def test_plain_run_dumps_the_last_steps_outputs(oracle, tmp_path, workload):
    from fury_amd.workloads import SCHEMAS, gen_columns
    from tests.helpers import assert_columns_equal
    line = _bench("--workload", workload, "--dump-outputs", str(tmp_path / "d"))
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["full"] is False
    assert "cpu_baseline" not in line and "e2e_pcie" not in line
    assert "copy_GBps" not in line["roofline"]
    dump = _load(tmp_path / "d")
    assert all(a.dtype in (np.float32, np.float64) for a in dump.values())
    assert sum(a.nbytes for a in dump.values()) <= 64 << 20
    fields = SCHEMAS[workload]
    host = gen_columns(workload, fields, ROWS, seed=1234)      # the bench's seed
    want, want_offs = oracle.encode(fields, host, ROWS)
    assert np.array_equal(dump["rows"].astype(np.uint8), want), "rows differ from the oracle"
    if want_offs is not None and workload != "struct100":
        assert np.array_equal(dump["row_offsets"].astype(np.int64), want_offs)
    ref = oracle.decode(fields, want, want_offs if workload != "struct100" else None, ROWS)
    assert_columns_equal(fields, _columns(fields, dump, ROWS), ref, ROWS)


@pytest.mark.gpu
def test_full_run_adds_the_other_figures():
    line = _bench("--full", "--cpu-seconds", "0.2")
    assert line["full"] is True and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["cpu_baseline"]["value"] > 0 and line["e2e_pcie"]["GBps_algorithmic"] > 0
    assert line["roofline"]["copy_GBps"] > 0 and 0 < line["roofline"]["frac_of_copy"]
