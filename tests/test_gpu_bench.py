"""bench.py as the driver runs it, at a small config: ONE JSON line whose `steps` / `ms_per_step` / `value` agree, nothing but
the headline measured (no roofline, CPU baseline or gradient exchange without --full), and --dump-outputs writing the losses
of the line and a gradient sample as float32 .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from stereoscene_amd import synthetic as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--config", "small_d48", "--dump-outputs", str(tmp_path)],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["n_gpus"] == 1 and rec["ms_per_step"] > 0
    assert rec["unit"] == "voxels/s" and rec["higher_is_better"] is True and rec["dtype"] == "f32"
    X, Y, Z = S.CONFIGS["small_d48"]["occ_size"]
    assert rec["value"] == pytest.approx(X * Y * Z / (rec["ms_per_step"] * 1e-3), rel=1e-3)
    assert rec["roofline"] is None and rec["cpu_baseline"] is None and "gradient_exchange" not in rec
    names = sorted(os.listdir(tmp_path))
    assert names == sorted([f"{k}.npy" for k in rec["losses"]] + ["grad_sample.npy"])
    assert sum(os.path.getsize(tmp_path / n) for n in names) <= 64 << 20
    for k, v in rec["losses"].items():
        a = np.load(tmp_path / f"{k}.npy")
        assert a.dtype == np.float32 and float(a) == pytest.approx(v, rel=1e-4, abs=1e-6)
    g = np.load(tmp_path / "grad_sample.npy")
    assert g.dtype == np.float32 and g.ndim == 1 and np.isfinite(g).all() and np.abs(g).max() > 0
