"""bench.py --dump-outputs: what the timed path computed in its last step, as .npy files that two builds can compare, and
the plain run's line (only what the headline figure needs; the rest is behind --full)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_samples_within_the_budget_and_repeats(tmp_path):
    import torch
    big = torch.arange(3000 * 6 * 5, dtype=torch.float64).reshape(3000, 6, 5)      # 240 B per request, 720 kB in all
    small = torch.linspace(0, 1, 40, dtype=torch.float32).reshape(4, 10)
    budget = 100_000
    written = bench.dump_outputs({"big": big, "small": small}, str(tmp_path / "a"), budget=budget)
    assert written == {"big": budget // 2 // 240, "small": 4}
    a = np.load(tmp_path / "a" / "big.npy")
    assert a.dtype == np.float64 and a.shape == (written["big"], 6, 5)
    rows = a[:, 0, 0] / 30                                                          # the request each row came from
    assert np.array_equal(rows, np.round(rows)) and np.all(np.diff(rows) > 0)       # whole requests, in order, no repeats
    assert np.array_equal(a, big.numpy()[rows.astype(int)])
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and np.array_equal(s, small.numpy())
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in ("big.npy", "small.npy")) <= budget + 2 * 128
    bench.dump_outputs({"big": big, "small": small}, str(tmp_path / "b"), budget=budget)
    assert np.array_equal(np.load(tmp_path / "b" / "big.npy"), a)                   # the same sample every run
    with pytest.raises(TypeError):
        bench.dump_outputs({"idx": torch.zeros(4, 3, dtype=torch.int64)}, str(tmp_path / "c"))


@pytest.mark.gpu
def test_plain_run_line_and_dumped_tables(tmp_path):
    """A plain run: K timed steps, the line without the --full fields, and the tables of the last step equal to the C
    oracle at the benchmark's seeded points."""
    import fiat_amd
    from oracle import c_oracle, fiat_oracle as fo
    batch = 2000
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                          "--batch", str(batch), "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 7 and line["warmup"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "tabulations/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert abs(line["value"] - batch / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]
    assert not {"roofline", "cpu_baseline", "ms_per_step_cold", "allgather"} & set(line)
    assert line["max_rel_err_vs_oracle"] is None
    assert sorted(os.listdir(tmp_path)) == ["Lagrange.npy"]
    got = np.load(tmp_path / "Lagrange.npy")
    assert got.dtype == np.float64 and got.shape == (batch, 4, 20, 23)
    el = fiat_amd.Lagrange(fiat_amd.ufc_simplex(3), 3)
    ref = c_oracle.tabulate_batch(fo.UFC_SIMPLEX[3], 3, el.get_coeffs(), 1, bench.synth_points(3, batch, 23, seed=2),
                                  scale=el._expansion_scale, variant=el._expansion_variant)
    err = np.abs(got - ref.reshape(got.shape)).max(axis=(2, 3)) / np.maximum(1.0, np.abs(ref).max(axis=(2, 3)))
    assert err.max() < 1e-12
