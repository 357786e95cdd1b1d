"""bench.py's plain run against --full: a plain run times the headline only and reports the --full fields as null."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import bench  # noqa: E402  (the repository root is on sys.path: tests/conftest.py)


def test_full_is_off_by_default():
    assert not bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"]).full
    assert bench.parse(["--full"]).full


def test_profile_json_needs_the_profiled_pass():
    """The per-kernel table comes from the --full profiled pass: asked for without it, the run is refused, not left empty."""
    for argv in (["--profile-json", "t.json"], ["--full", "--no-roofline", "--profile-json", "t.json"]):
        with pytest.raises(SystemExit) as e:
            bench.parse(argv)
        assert e.value.code == 2
    assert bench.parse(["--full", "--profile-json", "t.json"]).profile_json == "t.json"


@pytest.mark.gpu
def test_plain_run_reports_the_headline_only():
    batch, patch, steps = 2, 128, 3
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                          "--batch", str(batch), "--patch", str(patch)],
                         cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    line = json.loads(res.stdout.strip().splitlines()[-1])
    assert line["unit"] == "Mpixels/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert line["steps"] == steps and line["warmup"] == 1
    assert line["value"] == pytest.approx(batch * patch * patch / line["ms_per_step"] / 1e3, rel=1e-2)
    for k in ("roofline", "step_roofline", "mdta_contraction", "inference_forward", "fp32_line", "cpu_baseline"):
        assert line[k] is None, k
    assert "c2_bs8" not in line and "c4_moce" not in line
