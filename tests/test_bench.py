"""bench.py's plain run (GPU): one result line with the headline keys only, `--steps` timed steps,
and `--dump-outputs` files that hold exactly what the oracle decodes from the same seeded batch."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import spec_amd
from oracle import oracle as O
from spec_amd import workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 3000  # below bench.DUMP_RECORDS: every record is in the dump


def test_full_and_dump_are_off_by_default():
    import bench

    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


@pytest.mark.gpu
def test_plain_run_headline_and_dump(tmp_path, dev):
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--records", str(N), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["unit"] == "Mmsg/s" and d["higher_is_better"] is True and d["dtype"] == "u8" and "metric" in d
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(N / (d["ms_per_step"] * 1e-3) / 1e6, rel=0.02)
    # everything else belongs to --full
    assert not {"roofline", "checks", "correct", "cpu_baseline", "verify", "encode", "native_shard"} & set(d)

    s = spec_amd.FLAT16
    cols, heaps = workload.flat16(N, workload.SEED)
    stream, ends = O.encode_flat_batch(s.tags, s.kinds, cols, [heaps.get(f) for f in range(len(s))], N)
    want, want_status = O.decode_flat_batch(s.tags, s.kinds, stream, ends, s.widths)
    assert sorted(os.listdir(out)) == sorted(
        [f"col{f:02d}.npy" for f in range(len(s))] + ["status.npy", "sample_index.npy", "column_sums.npy"])
    assert np.array_equal(np.load(out / "sample_index.npy"), np.arange(N, dtype=np.float64))
    total = 0
    for f in range(len(s)):
        got = np.load(out / f"col{f:02d}.npy")
        total += got.nbytes
        assert got.dtype == np.float32 and np.array_equal(got, want[f].astype(np.float32)), f
    got = np.load(out / "status.npy")
    assert got.dtype == np.float32 and np.array_equal(got, want_status.astype(np.float32))
    sums = np.load(out / "column_sums.npy")
    assert sums.dtype == np.float64
    assert np.array_equal(sums, np.concatenate([w.sum(0, dtype=np.float64) for w in want] + [[float(want_status.sum())]]))
    assert total + got.nbytes + sums.nbytes + 8 * N <= 64 << 20
