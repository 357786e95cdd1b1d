"""bench.py --dump-outputs on host tensors (CPU only): float32 / float64 arrays, at most 64 MB in all, the same bytes for the
same step, and a seeded sample (not the whole tensor) once an output is over its budget."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import bench  # noqa: E402  (the repository root is on sys.path: tests/conftest.py)


def _step(batch):
    g = torch.Generator().manual_seed(5)
    model = torch.nn.Sequential(torch.nn.Conv2d(3, 48, 3), torch.nn.Linear(1000, 6000))
    return ({"out": torch.rand((batch, 3, 256, 256), generator=g).to(torch.bfloat16), "loss": torch.tensor(0.25),
             "aux": torch.tensor(0.125)}, model)


def _read(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_types_budget_and_repeatability(tmp_path):
    buf, model = _step(8)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), buf, model)
    bench.dump_outputs(str(b), buf, model)
    ra, rb = _read(a), _read(b)
    assert set(ra) == {"output", "loss", "aux_loss", "params_sample"}
    assert all(v.dtype in (np.float32, np.float64) for v in ra.values())
    assert ra["output"].shape == (8, 3, 256, 256)                           # under budget: the whole output, its own shape
    assert np.array_equal(ra["output"], buf["out"].float().numpy())
    assert float(ra["loss"]) == 0.25 and float(ra["aux_loss"]) == 0.125
    n_params = sum(p.numel() for p in model.parameters())
    assert ra["params_sample"].shape == (min(n_params, bench.DUMP_BUDGET["params_sample"] // 4),)
    assert all(np.array_equal(ra[k], rb[k]) for k in ra)
    assert sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a)) <= 64 << 20


def test_dump_outputs_samples_a_large_output(tmp_path):
    buf, model = _step(64)                                                  # 50 MB as float32: over the output's budget
    bench.dump_outputs(str(tmp_path), buf, model)
    out = np.load(tmp_path / "output.npy")
    assert out.shape == (bench.DUMP_BUDGET["output"] // 4,)
    assert set(np.unique(out)) <= set(np.unique(buf["out"].float().numpy()))
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= 64 << 20


def test_steps_must_be_positive():
    """--steps sets the timed loop and ms_per_step divides by it: zero is refused before anything touches a device."""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert res.returncode == 2 and "--steps" in res.stdout
