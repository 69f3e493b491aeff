"""Float64 restatement of LPIPS-VGG (lpips.LPIPS(net="vgg", version="0.1") in eval mode, as callers.LossLpips restates it) for the tests:
the VGG-16 taps, the heads, the value, and the heads' analytic gradient with the zero-norm convention of csrc/lpips.hip (at a pixel whose
channel vector is all zero, d n / d f = I / (r + eps): the rank-one term is dropped; torch autograd gives NaN there).  CPU, torch float64."""
from __future__ import annotations

import torch
import torch.nn.functional as F

SLICES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))      # torchvision vgg16.features conv indices per slice
CHANNELS = ((3, 64, 64), (64, 128, 128), (128, 256, 256, 256), (256, 512, 512, 512), (512, 512, 512, 512))
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
EPS = 1e-10


def fake_state_dict(seed: int = 0, bias: float = 0.02) -> dict:
    """Key names and shapes of lpips.LPIPS(net='vgg').state_dict(): seeded He-scaled conv weights, small positive biases (so the ReLUs are
    not dead) and rand (non-negative) lin weights.  Float32, as a real state dict."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for s_, (idxs, ch) in enumerate(zip(SLICES, CHANNELS)):
        for j, li in enumerate(idxs):
            sd[f"net.slice{s_ + 1}.{li}.weight"] = torch.randn(ch[j + 1], ch[j], 3, 3, generator=g) * (2.0 / (9 * ch[j])) ** 0.5
            sd[f"net.slice{s_ + 1}.{li}.bias"] = bias * torch.rand(ch[j + 1], generator=g)
        sd[f"lin{s_}.model.1.weight"] = torch.rand(1, ch[-1], 1, 1, generator=g)
    return sd


def features(sd: dict, x: torch.Tensor, normalize: bool, pool_args: list | None = None, relu_masks: list | None = None) -> list:
    """The five taps relu1_2 .. relu5_3 of x [N, 3, H, W], float64.  pool_args: the window positions (0..3, pool_first_max's) the four
    max-pools take instead of their own float64 maxima -- frozen decisions: a gradient check of a float32 forward against this one
    must not count a window whose two largest values are closer than float32 rounding and which the two forwards therefore order
    differently (the routed gradient moves to the other element).  relu_masks: likewise the 13 ReLUs' decisions (z > 0 of the float32
    forward) for pre-activations within rounding of 0."""
    x = x.double()
    if normalize:
        x = 2 * x - 1
    shift = torch.tensor(SHIFT, dtype=torch.float32).double().view(1, 3, 1, 1)     # float32 buffers in lpips' ScalingLayer
    scale = torch.tensor(SCALE, dtype=torch.float32).double().view(1, 3, 1, 1)
    x = (x - shift) / scale
    taps, k = [], 0
    for s_, idxs in enumerate(SLICES):
        if s_ > 0:
            x = F.max_pool2d(x, 2, 2) if pool_args is None else pool_at(x, pool_args[s_ - 1])
        for li in idxs:
            w, b = sd[f"net.slice{s_ + 1}.{li}.weight"].double(), sd[f"net.slice{s_ + 1}.{li}.bias"].double()
            z = F.conv2d(x, w, b, padding=1)
            x = F.relu(z) if relu_masks is None else torch.where(relu_masks[k], z, torch.zeros_like(z))
            k += 1
        taps.append(x)
    return taps


def lins(sd: dict) -> list:
    return [sd[f"lin{s_}.model.1.weight"].double() for s_ in range(5)]


def head(taps0: list, taps1: list, lin: list, per_tap: bool = False):
    """Per-image distance [N] (or [5, N] with per_tap): sum over taps of the spatial mean of sum_c w_c (n0_c - n1_c)^2."""
    out = []
    for f0, f1, w in zip(taps0, taps1, lin):
        n0 = f0 / (f0.pow(2).sum(1, keepdim=True).sqrt() + EPS)
        n1 = f1 / (f1.pow(2).sum(1, keepdim=True).sqrt() + EPS)
        out.append(((n0 - n1) ** 2 * w.view(1, -1, 1, 1)).sum(1).mean(dim=(1, 2)))
    out = torch.stack(out)
    return out if per_tap else out.sum(0)


def value(sd: dict, in0: torch.Tensor, in1: torch.Tensor, normalize: bool) -> torch.Tensor:
    return head(features(sd, in0, normalize), features(sd, in1, normalize), lins(sd))


def head_grad(taps0: list, taps1: list, lin: list, g: torch.Tensor):
    """Analytic gradient of sum_n g[n] head(...)[n] with respect to every tap of both images (lists of 5), zero-norm convention."""
    d0, d1 = [], []
    for f0, f1, w in zip(taps0, taps1, lin):
        hw = f0.shape[-1] * f0.shape[-2]
        r0, r1 = f0.pow(2).sum(1, keepdim=True).sqrt(), f1.pow(2).sum(1, keepdim=True).sqrt()
        t0, t1 = r0 + EPS, r1 + EPS
        u = 2 * g.view(-1, 1, 1, 1) * w.view(1, -1, 1, 1) * (f0 / t0 - f1 / t1) / hw       # dL/dn0 = -dL/dn1

        def back(f, r, t, uu):
            p = (uu * f).sum(1, keepdim=True)
            rank1 = torch.where(r > 0, f * p / (r.clamp_min(1e-300) * t * t), torch.zeros_like(f))
            return uu / t - rank1

        d0.append(back(f0, r0, t0, u))
        d1.append(back(f1, r1, t1, -u))
    return d0, d1


def pool_first_max(x: torch.Tensor):
    """2 x 2 stride-2 max-pool [N, C, H, W] with the tie rule of torch and csrc/lpips.hip: the FIRST maximum in row-major window order.
    Returns (pooled, window index 0..3 of the chosen element)."""
    win = _windows(x)
    best = win[..., 0].clone()
    arg = torch.zeros_like(best, dtype=torch.long)
    for k in range(1, 4):
        take = win[..., k] > best
        best = torch.where(take, win[..., k], best)
        arg = torch.where(take, torch.full_like(arg, k), arg)
    return best, arg


def _windows(x: torch.Tensor) -> torch.Tensor:
    N, C, H, W = x.shape
    return x.reshape(N, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, H // 2, W // 2, 4)


def pool_at(x: torch.Tensor, arg: torch.Tensor) -> torch.Tensor:
    """The 2 x 2 pool that takes window position arg (0..3) of every window (differentiable: the gradient goes to that element)."""
    return _windows(x).gather(-1, arg.unsqueeze(-1)).squeeze(-1)


def pool_backward(dy: torch.Tensor, x: torch.Tensor, g_add: torch.Tensor | None = None):
    """(x > 0) * (g_add + dy routed to the first maximum of each window): what vs_lpips_maxpool_backward computes, NCHW."""
    N, C, H, W = x.shape
    _, arg = pool_first_max(x)
    routed = torch.zeros(N, C, H // 2, W // 2, 4, dtype=dy.dtype)
    routed.scatter_(-1, arg.unsqueeze(-1), dy.unsqueeze(-1))
    routed = routed.view(N, C, H // 2, W // 2, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, H, W)
    if g_add is not None:
        routed = routed + g_add
    return torch.where(x > 0, routed, torch.zeros_like(routed))
