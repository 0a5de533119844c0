"""bench.py's command line: a plain run measures the headline only, --full
switches the other legs on, --dump-outputs writes the last timed step's
outputs as float32 .npy files that repeat from run to run."""
import json
import os
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bench

# keys only a --full run carries (the legs that take runs or steps of their own)
FULL_ONLY = ("roofline", "roofline_dispatch", "kernel_profile", "kernel_timing", "eval", "dp_exchange",
             "roofline_e2e", "cpu_baseline")
CONTRACT = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")


def test_plain_run_is_the_default():
    a = bench.parse_args([])
    assert a.full is False and a.dump_outputs is None
    assert bench.parse_args(["--full"]).full is True
    assert bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"]).steps == 7


@pytest.mark.parametrize("argv", [["--phase-timing"], ["--dump-prof-records", "x.json"], ["--steps", "0"]])
def test_rejected_arguments(argv, capsys):
    with pytest.raises(SystemExit) as e:
        bench.parse_args(argv)
    assert e.value.code == 2
    if argv[0] != "--steps":
        assert "--full" in capsys.readouterr().err
        assert bench.parse_args(["--full"] + argv) is not None


def test_sample_is_fixed_and_ordered():
    ts = [torch.arange(0, 1000, dtype=torch.float64).reshape(10, 100), torch.arange(1000, 1500).to(torch.bfloat16)]
    whole = bench._sample_flat(ts, n=4096)
    assert whole.dtype == np.float32 and whole.shape == (1500,)
    np.testing.assert_array_equal(whole[:1000], np.arange(1000, dtype=np.float32))
    a, b = bench._sample_flat(ts, n=64), bench._sample_flat(ts, n=64)
    assert a.shape == (64,) and a.dtype == np.float32
    np.testing.assert_array_equal(a, b)
    assert np.all(np.diff(a) >= 0) and np.isin(a, whole).all()  # elements of the source, in source order


def test_dump_outputs_writes_float32_npy(tmp_path):
    p0 = torch.nn.Parameter(torch.linspace(-1, 1, 12).reshape(3, 4))
    p1 = torch.nn.Parameter(torch.ones(5, dtype=torch.bfloat16))
    p0.grad = torch.full_like(p0, 0.5)  # p1 has no gradient: zeros
    step = SimpleNamespace(stepper=None, params=[p0, p1])
    names = bench.dump_outputs(tmp_path / "out", step, torch.tensor(2.5, dtype=torch.float64))
    assert names == ["grads_sample", "loss", "params_sample"]
    got = {n: np.load(tmp_path / "out" / f"{n}.npy") for n in names}
    assert all(a.dtype == np.float32 for a in got.values())
    np.testing.assert_array_equal(got["loss"], [2.5])
    np.testing.assert_array_equal(got["grads_sample"], [0.5] * 12 + [0.0] * 5)
    np.testing.assert_allclose(got["params_sample"][:12], np.linspace(-1, 1, 12), atol=1e-6)
    step.stepper = SimpleNamespace(static_losses={"loss_vfl": torch.tensor(1.25)})
    assert "loss_vfl" in bench.dump_outputs(tmp_path / "out", step, torch.tensor(2.5))
    np.testing.assert_array_equal(np.load(tmp_path / "out" / "loss_vfl.npy"), [1.25])


@pytest.mark.gpu
def test_plain_bench_run_dumps_repeatable_outputs(tmp_path, hip_lib):
    """One small plain run: the contract keys and nothing of --full on the
    result line, K timed steps, and the dumped arrays of two runs with the same
    arguments agree (same inputs; the step's kernels are deterministic up to
    the deformable-attention value gradient's atomics, hence the tolerance on
    everything but the shapes)."""
    root = Path(bench.__file__).resolve().parent
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    # the two runs side by side: the test takes as long as one of them
    procs = [subprocess.Popen([sys.executable, str(root / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                               "--batch", "2", "--img-h", "256", "--img-w", "256", "--dump-outputs",
                               str(tmp_path / d)], env=env, cwd=tmp_path, stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for d in "ab"]
    results = []
    for p in procs:
        out, err = p.communicate(timeout=300)
        assert p.returncode == 0, err[-3000:]
        lines = [ln for ln in out.splitlines() if ln.strip()]
        assert len(lines) == 1, out
        results.append(json.loads(lines[0]))

    res = results[0]
    for k in CONTRACT:
        assert k in res, k
    assert res["steps"] == 2 and res["warmup"] == 1 and res["full"] is False
    assert res["ms_per_step"] > 0 and abs(res["value"] - 2 * 1e3 / res["ms_per_step"]) <= 0.01 * res["value"]
    assert not [k for k in FULL_ONLY if k in res]
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == sorted(f"{n}.npy" for n in res["dumped_outputs"])
    assert {"loss.npy", "grads_sample.npy", "params_sample.npy"} <= set(files)
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= 64 * 2**20
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float32 and a.shape == b.shape and np.isfinite(a).all()
        np.testing.assert_allclose(a, b, rtol=0.05, atol=0.05 * max(float(np.abs(a).max()), 1e-6), err_msg=f)
