"""GPU: bench.py's plain run (no --full) prints only the headline, --steps sets the timed steps, and --dump-outputs writes the
last timed step's output, the same for two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--num-block", "1", "--batch", "4"] + list(extra)
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-6000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_headline_only_and_dumped_outputs_repeat(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    d = _run("--steps", "3", "--warmup", "1", "--dump-outputs", str(a))
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "tiles/s" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0 and abs(d["value"] - 4 * 3 / (d["ms_per_step"] * 3 / 1e3)) / d["value"] < 1e-3
    assert "f16 operands" in d["dtype"]
    for k in ("roofline", "parity", "cpu_baseline", "train_step", "predict", "summary"):
        assert k not in d, k
    _run("--steps", "2", "--warmup", "1", "--dump-outputs", str(b))
    names = sorted(os.listdir(a))
    assert names == ["feature_sample.npy", "feature_tile0.npy"] and sorted(os.listdir(b)) == names
    total = 0
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype == np.float32 and x.shape == y.shape and np.isfinite(x).all()
        np.testing.assert_allclose(x, y, rtol=1e-5, atol=1e-6)
        total += x.nbytes
    assert np.load(a / "feature_tile0.npy").shape == (64, 256, 256) and total <= 64 << 20
