"""bench.py's command line: a plain run is the headline alone (`--full` adds the other measurements), and `--dump-outputs DIR`
writes what the last timed step returned as float32 .npy files.  CPU: the parser and the writer on a toy model."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_plain_run_is_the_default():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    b = bench.parse(["--full", "--dump-outputs", "out"])
    assert b.full and b.dump_outputs == "out"


def _toy():
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.ReLU(), torch.nn.Linear(32, 4))
    y = m(torch.randn(8, 16))
    losses = {"loss_a": y.square().mean(), "loss_b": y.abs().mean(), "metric_c": y.detach().max()}
    (losses["loss_a"] + losses["loss_b"]).backward()
    return m, losses


def test_dump_writes_losses_and_every_gradient_when_small(tmp_path):
    m, losses = _toy()
    bench.dump_outputs(str(tmp_path), losses, m)
    assert sorted(os.listdir(tmp_path)) == ["grad_sample.npy", "loss_a.npy", "loss_b.npy", "metric_c.npy"]
    for k, v in losses.items():
        a = np.load(tmp_path / f"{k}.npy")
        assert a.dtype == np.float32 and a.shape == () and a == np.float32(float(v.detach()))
    g = np.load(tmp_path / "grad_sample.npy")
    want = torch.cat([p.grad.reshape(-1) for p in m.parameters()]).numpy()
    assert g.dtype == np.float32 and np.array_equal(g, want)


def test_dump_samples_large_gradients_at_fixed_indices(tmp_path):
    m, losses = _toy()
    n = sum(p.numel() for p in m.parameters())
    bench.dump_outputs(str(tmp_path / "a"), losses, m, sample=100)
    bench.dump_outputs(str(tmp_path / "b"), losses, m, sample=100)
    a, b = np.load(tmp_path / "a" / "grad_sample.npy"), np.load(tmp_path / "b" / "grad_sample.npy")
    assert a.shape == (100,) and np.array_equal(a, b)
    idx = torch.randint(n, (100,), generator=torch.Generator().manual_seed(0)).sort().values
    assert np.array_equal(a, torch.cat([p.grad.reshape(-1) for p in m.parameters()])[idx].numpy())
    assert bench.DUMP_GRAD_SAMPLE * 4 <= 32 << 20         # the real model's dump stays far below 64 MB
