"""bench.py --dump-outputs: the arrays of the timed path's last step on disk, so that two builds can be compared output for
output.  The writer itself on the CPU box; the whole bench run against the operator at the same seeded inputs on the GPU box."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from conftest import ROOT


def test_dump_writes_f_and_grad_as_float64(tmp_path):
    f, g = np.linspace(-1, 1, 5), np.arange(35, dtype=np.float64).reshape(5, 7)
    assert bench.dump_outputs(str(tmp_path), f, g) == ["f", "grad"]
    assert sorted(os.listdir(tmp_path)) == ["f.npy", "grad.npy"]
    for name, want in (("f", f), ("grad", g)):
        got = np.load(tmp_path / (name + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, want)


def test_dump_over_the_limit_is_a_fixed_sample_of_rows(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT", 10_000)
    f, g = np.arange(300.0), np.random.default_rng(1).normal(size=(300, 20))
    names = bench.dump_outputs(str(tmp_path / "a"), f, g)
    bench.dump_outputs(str(tmp_path / "b"), f, g)
    assert names == ["f", "grad", "grad_rows"]
    rows = np.load(tmp_path / "a" / "grad_rows.npy")
    assert rows.dtype == np.float64 and np.array_equal(rows, np.load(tmp_path / "b" / "grad_rows.npy"))  # seeded: same rows
    r = rows.astype(np.int64)
    assert np.array_equal(r, rows) and np.all(np.diff(r) > 0) and 0 < len(r) < 300
    assert np.array_equal(np.load(tmp_path / "a" / "grad.npy"), g[r])
    assert np.array_equal(np.load(tmp_path / "a" / "f.npy"), f)
    assert sum(np.load(tmp_path / "a" / (q + ".npy")).nbytes for q in names) <= 10_000
    # a later run under the limit in the same directory leaves no row list that would mislabel its full gradient
    monkeypatch.setattr(bench, "DUMP_LIMIT", 64 * 10**6)
    assert bench.dump_outputs(str(tmp_path / "a"), f, g) == ["f", "grad"]
    assert sorted(os.listdir(tmp_path / "a")) == ["f.npy", "grad.npy"]


@pytest.mark.gpu
@pytest.mark.parametrize("gpus", [1, 2])
def test_bench_dump_is_the_operator_at_the_seeded_inputs(tmp_path, gpus):
    # the timed passes' f and gradient (rank rows gathered in node order for N = 2, both ranks on device 0 of a 1-GPU box)
    # against gml_objgrad_batch on a handle drawn from the same seeds: the workload's inputs are the same from run to run
    n, K = 256, 50000
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--steps", "4", "--warmup", "1",
                        "--spins", str(n), "--samples", str(K), "--no-cpu", "--no-learn", "--no-f64", "--no-i8x", "--no-weighted",
                        "--no-sparse-theta", "--dump-outputs", str(tmp_path / "out")],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 4 and line["ms_per_step"] > 0 and line["dump_outputs"]["files"] == ["f", "grad"]
    f = np.load(tmp_path / "out" / "f.npy")
    g = np.load(tmp_path / "out" / "grad.npy")
    assert f.dtype == g.dtype == np.float64 and f.shape == (n,) and g.shape == (n, n)

    import gml_amd as gml
    synthetic = __import__("importlib").import_module("gml_amd.synthetic")
    J = synthetic.block_ising_model(n, block=16, seed=0)
    with gml.Problem(model=J, num_samples=K, seed=0) as p:
        f0, g0 = p.objgrad("RISE", np.arange(n), J, precision="i8w")
    assert np.abs(f - f0).max() <= 1e-12 * np.abs(f0).max()
    assert np.abs(g - g0).max() <= 1e-12


def test_full_is_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3"])
    assert not bench.parse_args().full
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3", "--full", "--no-cpu"])
    a = bench.parse_args()
    assert a.full and a.no_cpu and not a.no_learn


@pytest.mark.gpu
def test_plain_run_is_the_headline_only():
    # no --full: set up, warm up, the timed steps, the line -- none of the legs that take runs of their own
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
                        "--spins", "256", "--samples", "50000"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 4 and line["warmup"] == 1 and line["dtype"] == "i8w" and line["higher_is_better"] is True
    assert line["unit"] == "node-evals/s" and line["value"] > 0
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 - 256) <= 1e-6 * 256  # node evaluations per second of the timed steps
    assert line["roofline"]["fwd_ms"] > 0 and line["roofline"]["bwd_ms"] > 0 and "pcie_inclusive_ms_per_step" not in line["roofline"]
    assert line["f64"] is None and line["i8x"] is None and line["cpu_baseline"] is None
    for key in ("value_f64", "value_i8x", "sparse_theta", "learn_wall_s", "learn_from_host", "projection_8gpu", "weighted",
                "ms_per_step_weighted"):
        assert key not in line, key
