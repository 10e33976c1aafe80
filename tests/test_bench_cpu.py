"""CPU tests (no GPU) of bench.py's own plumbing: the options a plain run and a --full run are told apart by, and what --dump-outputs writes
(bench.dump_outputs over a host tensor: the whole index array when it is small, a fixed seeded sample beside its positions when it is not)."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_help_offers_full_and_dump_outputs():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode(errors="replace")
    out = p.stdout.decode()
    assert "--full" in out and "--dump-outputs" in out and "--steps" in out


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_writes_small_index_arrays_whole(tmp_path):
    import torch
    import bench
    idx = torch.arange(1, 1001, 3, dtype=torch.int64)                   # the step's buffer: its first nsel entries are the answer
    nsel = 300
    bench.dump_outputs(str(tmp_path), torch, idx, nsel, 12345)
    got = _load(tmp_path)
    assert sorted(got) == ["count", "indices"]
    assert got["indices"].dtype == np.float64 and np.array_equal(got["indices"], np.arange(1, 1001, 3)[:nsel].astype(np.float64))
    assert got["count"].dtype == np.float64 and got["count"].tolist() == [12345.0]


def test_dump_outputs_samples_large_index_arrays_alike_every_time(tmp_path):
    import torch
    import bench
    nsel = bench.DUMP_WHOLE_MAX + 17
    idx = torch.arange(1, nsel + 1, dtype=torch.int64) * 7                # index i holds 7 * (i + 1): the sample says which positions it read
    runs = []
    for k in range(2):
        d = tmp_path / str(k)
        bench.dump_outputs(str(d), torch, idx, nsel, nsel)
        runs.append(_load(d))
        assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 << 20
    a, b = runs
    assert sorted(a) == ["count", "indices_sample", "indices_sample_positions"]
    pos = a["indices_sample_positions"]
    assert a["indices_sample"].dtype == np.float64 and pos.dtype == np.float64 and len(pos) == bench.DUMP_SAMPLE
    assert pos.min() >= 0 and pos.max() < nsel and np.all(np.diff(pos) >= 0)
    assert np.array_equal(a["indices_sample"], 7 * (pos + 1))
    assert all(np.array_equal(a[k], b[k]) for k in a)                     # fixed seed: the same sample from run to run
