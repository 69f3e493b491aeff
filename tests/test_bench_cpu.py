"""bench.py's command line and its --dump-outputs writer, on CPU (no kernel runs)."""
import os
import sys
import types
import zlib

import numpy as np
import pytest
import torch

import bench
from vicasplat_amd.model.encoder.common.gaussian_adapter import Gaussians


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_headline_only_and_full_keeps_every_leg(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.full, a.mode, a.steps, a.warmup, a.dump_outputs) == (False, "infer", 7, 2, None)
    a = _parse(monkeypatch, "--gpus", "1", "--full")
    assert (a.full, a.mode) == (True, "both")
    a = _parse(monkeypatch, "--full", "--mode", "infer", "--dump-outputs", "d")
    assert (a.full, a.mode, a.dump_outputs) == (True, "infer", "d")
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--mode", "train", "--dump-outputs", "d")


def _fake_step(seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, dtype=torch.float32: torch.randn(*s, generator=g, dtype=dtype)
    B, V, H = 2, 3, 64
    gs = Gaussians(means=r(B, V, H, H, 3), covariances=r(B, V, H, H, 3, 3), scales=r(B, V, H, H, 3), rotations=r(B, V, H, H, 4),
                   harmonics=r(B, V, H, H, 3, 25).half(), opacities=r(B, V, H, H, 1))
    out = dict(gaussians=gs, pred_extrins=r(B, V - 1, 8), pred_intrins=None, raw_gaussians=r(B * V, H, H, 86).unflatten(0, (B, V)),
               gaussian_camera_extrins=r(B, V, 4, 4, dtype=torch.float64), gaussian_camera_intrins=None, gaussian_centers=gs.means,
               confidence=None, context_view_depths=None)
    dec = types.SimpleNamespace(color=r(B, 4, 3, 128, 128), depth=r(B, 4, 128, 128).transpose(2, 3))
    return out, dec


def test_dump_outputs_writes_every_array_whole_or_as_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 4096)
    out, dec = _fake_step(0)
    bench.dump_outputs(str(tmp_path / "a"), out, dec)
    names = sorted(f[:-4] for f in os.listdir(tmp_path / "a"))
    assert names == sorted(["gaussians_means", "gaussians_covariances", "gaussians_scales", "gaussians_rotations", "gaussians_harmonics",
                            "gaussians_opacities", "pred_extrins", "raw_gaussians", "gaussian_camera_extrins", "color", "depth"])
    ld = lambda d, n: np.load(tmp_path / d / (n + ".npy"))
    # small arrays whole, in their own shape; float64 stays float64, everything else is float32
    assert np.array_equal(ld("a", "pred_extrins"), out["pred_extrins"].numpy())
    assert ld("a", "gaussian_camera_extrins").dtype == np.float64 and ld("a", "gaussians_harmonics").dtype == np.float32
    # large ones: DUMP_SAMPLE elements at sorted flat indices from a generator seeded by name and size (non-contiguous input included)
    for n, t in (("depth", dec.depth), ("raw_gaussians", out["raw_gaussians"]), ("gaussians_harmonics", out["gaussians"].harmonics)):
        flat = np.sort(np.random.default_rng([zlib.crc32(n.encode()), t.numel()]).choice(t.numel(), size=4096, replace=False))
        assert np.array_equal(ld("a", n), t.float().contiguous().reshape(-1).numpy()[flat]), n
    # same shapes, other values: the same indices are read
    out2, dec2 = _fake_step(1)
    bench.dump_outputs(str(tmp_path / "b"), out2, dec2)
    flat = np.sort(np.random.default_rng([zlib.crc32(b"color"), dec.color.numel()]).choice(dec.color.numel(), size=4096, replace=False))
    assert np.array_equal(ld("b", "color"), dec2.color.reshape(-1).numpy()[flat])
