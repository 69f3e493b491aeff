"""Float64 restatements of the two SSIM definitions the package implements on the GPU (vicasplat_amd.callers), written from their
specifications; the tests compare both the HIP kernels and these restatements against fixtures recorded from the real implementations.

  * `ssim_metric_f64` -- definition A, the evaluation metric: scikit-image structural_similarity(gt, hat, win_size=11,
    gaussian_weights=True, channel_axis=0, data_range=1.0) as src/evaluation/metrics.py:46-62 calls it.  Pure numpy (no scipy).
  * `ssim_loss_f64`   -- definition B, the SSIM loss of src/loss/loss_ssim.py:129-190 with its 4-tuple (ssim, brightness, contrast,
    structure).  torch float64, differentiable, so that torch autograd gives the reference gradients.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

METRIC_RADIUS = 5           # int(truncate * sigma + 0.5) with truncate 3.5, sigma 1.5


def metric_taps_f64(sigma: float = 1.5, radius: int = METRIC_RADIUS) -> np.ndarray:
    """scipy.ndimage.gaussian_filter's 1-D kernel: exp(-x^2 / (2 sigma^2)), x = -radius..radius, normalised to sum 1."""
    x = np.arange(-radius, radius + 1, dtype=np.float64)
    g = np.exp(-0.5 / (sigma * sigma) * x * x)
    return g / g.sum()


def gaussian_filter_reflect(img: np.ndarray, taps: np.ndarray | None = None) -> np.ndarray:
    """Separable correlation of the last two axes of `img` (float64) with `taps`, half-sample symmetric boundary (scipy mode 'reflect':
    index -1 reads 0, index n reads n - 1), the first of the two axes first."""
    taps = metric_taps_f64() if taps is None else np.asarray(taps, np.float64)
    r = len(taps) // 2
    out = np.asarray(img, np.float64)
    for axis in (-2, -1):
        n = out.shape[axis]
        pad = [(0, 0)] * out.ndim
        pad[axis] = (r, r)
        p = np.pad(out, pad, mode="symmetric")
        acc = np.zeros_like(out)
        for j, w in enumerate(taps):
            acc += w * np.take(p, np.arange(j, j + n), axis=axis)
        out = acc
    return out


def ssim_metric_f64(gt: np.ndarray, pred: np.ndarray) -> float:
    """Definition A on one image [C, H, W] (float64): the mean over channels of the mean SSIM map with 5 pixels cropped from every edge."""
    x, y = np.asarray(gt, np.float64), np.asarray(pred, np.float64)
    if min(x.shape[-2:]) < 2 * METRIC_RADIUS + 1:
        raise ValueError("win_size exceeds image extent")
    cov_norm = 121.0 / 120.0
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    ux, uy = gaussian_filter_reflect(x), gaussian_filter_reflect(y)
    uxx, uyy, uxy = gaussian_filter_reflect(x * x), gaussian_filter_reflect(y * y), gaussian_filter_reflect(x * y)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    r = METRIC_RADIUS
    return float(np.mean([s[c, r:-r, r:-r].mean(dtype=np.float64) for c in range(s.shape[0])]))


def loss_window_f32(size: int = 11, sigma: float = 1.5) -> torch.Tensor:
    """The loss window: float32 Gaussian taps over coords -(size // 2)..size // 2, normalised to sum 1 (loss_ssim.py:12-26)."""
    coords = torch.arange(size, dtype=torch.float) - size // 2
    g = torch.exp(-(coords ** 2) / (2 * sigma ** 2))
    return g / g.sum()


def ssim_loss_f64(X: torch.Tensor, Y: torch.Tensor, data_range: float = 255, size_average: bool = True, win: torch.Tensor | None = None,
                  K=(0.01, 0.03), nonnegative_ssim: bool = False, retrun_seprate: bool = False):
    """Definition B in float64 on [N, C, H, W]: valid separable convolution with the 1-D window `win` (default loss_window_f32()),
    no covariance correction; returns (ssim, brightness, contrast, structure) like the loss (zeros for the last three unless
    retrun_seprate).  Gradients follow torch autograd on this expression."""
    X, Y = X.double(), Y.double()
    w = (loss_window_f32() if win is None else win.reshape(-1)).double().to(X.device)
    C = X.shape[1]
    kv = w.view(1, 1, -1, 1).repeat(C, 1, 1, 1)
    kh = w.view(1, 1, 1, -1).repeat(C, 1, 1, 1)

    def filt(t):
        return F.conv2d(F.conv2d(t, kv, groups=C), kh, groups=C)

    c1, c2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    m1, m2 = filt(X), filt(Y)
    v1 = filt(X * X) - m1 * m1
    v2 = filt(Y * Y) - m2 * m2
    v12 = filt(X * Y) - m1 * m2
    lum = (2 * m1 * m2 + c1) / (m1 * m1 + m2 * m2 + c1)
    s_map = lum * (2 * v12 + c2) / (v1 + v2 + c2)
    s = s_map.flatten(2).mean(-1)
    b = c = t = torch.zeros_like(s)
    if retrun_seprate:
        eps2 = torch.finfo(torch.float32).eps ** 2
        v1c, v2c = v1.clamp(min=eps2), v2.clamp(min=eps2)
        s12 = torch.sign(v12) * torch.minimum(torch.sqrt(v1c * v2c), torch.abs(v12))
        c3 = c2 / 2
        s1s2 = torch.sqrt(v1c) * torch.sqrt(v2c)
        b = lum.flatten(2).mean(-1)
        c = ((2 * s1s2 + c2) / (v1c + v2c + c2)).clamp(max=0.98).flatten(2).mean(-1)
        t = ((s12 + c3) / (s1s2 + c3)).clamp(max=0.98).flatten(2).mean(-1)
    if nonnegative_ssim:
        s = torch.relu(s)
    if size_average:
        return s.mean(), b.mean(), c.mean(), t.mean()
    return s.mean(1), b.mean(1), c.mean(1), t.mean(1)
