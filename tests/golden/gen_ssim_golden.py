"""Generates the SSIM fixtures from the real implementations:

  * ssim_metric.npz -- scikit-image `structural_similarity(gt, hat, win_size=11, gaussian_weights=True, data_range=1.0)` per image and
                       channel-averaged, as src/evaluation/metrics.py:46-62 calls it, on uint8 image pairs (random, smooth, near-identical,
                       flat-bright, non-square).  scikit-image runs in a child interpreter: SKIMAGE_PYTHON (default: this one).  Before
                       0.19 it has no `channel_axis`; `multichannel=True` on channel-last arrays means the same.
  * ssim_loss.npz   -- the reference's own `ssim` of src/loss/loss_ssim.py (imported on CPU through ref_import.py) in float64 on
                       2 x 3 x 40 x 52 uint8 pairs at data_range 1.0: the 4-tuple for size_average True / False and nonnegative_ssim,
                       and the autograd gradients of ssim and of structure (retrun_seprate) with respect to X and Y.  The "near" pair is
                       near-identical, so the 0.98 clamps of the contrast and structure maps are active.

Images are stored as uint8; every consumer compares them as float32 / 255 (the generator feeds exactly those values, in float64).

    PYTHONDONTWRITEBYTECODE=1 SKIMAGE_PYTHON=<python with scikit-image> python tests/golden/gen_ssim_golden.py
"""
from __future__ import annotations

import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def as_float(u8: np.ndarray) -> np.ndarray:
    return (u8.astype(np.float32) / np.float32(255.0)).astype(np.float64)


def _smooth(rng, shape, k=4):
    """Box-blurred noise (k passes of a 3-tap mean along both axes), stretched to 0..255."""
    a = rng.random(shape)
    for _ in range(k):
        a = (np.roll(a, 1, -1) + a + np.roll(a, -1, -1)) / 3
        a = (np.roll(a, 1, -2) + a + np.roll(a, -1, -2)) / 3
    a = (a - a.min()) / (a.max() - a.min())
    return a * 255


def metric_cases() -> dict:
    rng = np.random.default_rng(7)
    u8 = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)
    cases = {}
    cases["random_48x48"] = (u8(rng.random((1, 3, 48, 48)) * 255), u8(rng.random((1, 3, 48, 48)) * 255))
    s = _smooth(rng, (1, 3, 64, 80))
    cases["smooth_64x80"] = (u8(s), u8(s + rng.normal(0, 12, s.shape)))
    s = _smooth(rng, (1, 3, 37, 53), k=2)
    cases["near_37x53"] = (u8(s), u8(s + rng.integers(-2, 3, s.shape)))
    f = np.full((1, 3, 40, 40), 250.0)
    g = f + 2
    g[..., 10:14, 20:30] = 255
    cases["flat_40x40"] = (u8(f), u8(g))
    s = _smooth(rng, (2, 3, 32, 44))
    cases["batch2_32x44"] = (u8(s), u8(np.concatenate([s[:1] * 0.8 + 20, 255 - s[1:]])))
    return cases


def skimage_child(src: str, dst: str) -> None:
    """Runs in the scikit-image interpreter: per-image structural_similarity of every case in `src`."""
    import inspect

    from skimage.metrics import structural_similarity
    z = np.load(src)
    has_axis = "channel_axis" in inspect.signature(structural_similarity).parameters
    out = {}
    for key in sorted(k[:-2] for k in z.files if k.endswith("_x")):
        x, y = as_float(z[key + "_x"]), as_float(z[key + "_y"])
        vals = []
        for gt, hat in zip(x, y):
            if has_axis:
                v = structural_similarity(gt, hat, win_size=11, gaussian_weights=True, channel_axis=0, data_range=1.0)
            else:
                v = structural_similarity(gt.transpose(1, 2, 0), hat.transpose(1, 2, 0), win_size=11, gaussian_weights=True,
                                          multichannel=True, data_range=1.0)
            vals.append(v)
        out[key + "_ssim"] = np.array(vals, np.float64)
    import skimage
    out["skimage_version"] = np.array(skimage.__version__)
    np.savez(dst, **out)


def gen_metric() -> None:
    cases = metric_cases()
    arrays = {}
    for k, (x, y) in cases.items():
        arrays[k + "_x"], arrays[k + "_y"] = x, y
    with tempfile.TemporaryDirectory() as td:
        src, dst = os.path.join(td, "in.npz"), os.path.join(td, "out.npz")
        np.savez(src, **arrays)
        py = os.environ.get("SKIMAGE_PYTHON", sys.executable)
        subprocess.check_call([py, os.path.abspath(__file__), "--skimage", src, dst])
        res = dict(np.load(dst))
    arrays.update(res)
    np.savez_compressed(os.path.join(HERE, "ssim_metric.npz"), **arrays)
    print("ssim_metric.npz", {k: v for k, v in res.items()})


def gen_loss() -> None:
    import torch
    sys.path.insert(0, HERE)
    import ref_import
    ref_import.install()
    from src.loss.loss_ssim import ssim

    rng = np.random.default_rng(11)
    u8 = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)
    shape = (2, 3, 40, 52)
    s = _smooth(rng, shape, k=3)
    pairs = {
        "rand": (u8(s), u8(0.7 * s + 0.3 * _smooth(rng, shape, k=1))),
        # near-identical on the left half (clamped structure / contrast maps), noisier on the right (unclamped)
        "near": (u8(s), u8(s + np.where(np.arange(shape[-1]) < shape[-1] // 2, rng.integers(-1, 2, shape), rng.normal(0, 10, shape)))),
        "anti": (u8(s), u8(255 - s)),
    }
    out = {}
    for name, (xu, yu) in pairs.items():
        out[name + "_x"], out[name + "_y"] = xu, yu
        X = torch.tensor(as_float(xu), requires_grad=True)
        Y = torch.tensor(as_float(yu), requires_grad=True)
        avg = ssim(X, Y, data_range=1.0, size_average=True, retrun_seprate=True)
        img = ssim(X, Y, data_range=1.0, size_average=False, retrun_seprate=True)
        out[name + "_avg"] = torch.stack([v.detach() for v in avg]).numpy()
        out[name + "_img"] = torch.stack([v.detach() for v in img]).numpy()
        out[name + "_plain_img"] = torch.stack([v.detach() for v in ssim(X, Y, data_range=1.0, size_average=False)]).numpy()
        out[name + "_nn_img"] = ssim(X, Y, data_range=1.0, size_average=False, nonnegative_ssim=True)[0].detach().numpy()
        if name != "anti":
            gx, gy = torch.autograd.grad(avg[0], (X, Y), retain_graph=True)
            out[name + "_gx_ssim"], out[name + "_gy_ssim"] = gx.numpy(), gy.numpy()
            gx, gy = torch.autograd.grad(avg[3], (X, Y))
            out[name + "_gx_struct"], out[name + "_gy_struct"] = gx.numpy(), gy.numpy()
        print(name, out[name + "_avg"], out[name + "_nn_img"])
    np.savez_compressed(os.path.join(HERE, "ssim_loss.npz"), **out)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--skimage":
        skimage_child(sys.argv[2], sys.argv[3])
    else:
        gen_metric()
        gen_loss()
