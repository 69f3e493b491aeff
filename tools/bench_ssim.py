"""SSIM timing on an evaluation-sized batch: 288 views of 3 x 256 x 256 pairs (csrc/ssim.hip).

Prints one JSON line: the median time of callers.compute_ssim (the metric: one forward over every plane), the median time of the loss
forward + backward (callers.ssim with retrun_seprate, gradients of 1 - ssim + 1 - structure with respect to both images), the effective
bandwidth of the metric forward (it reads both images once: 2 x 288 x 3 x 256^2 x 4 bytes), and, for scale, the time of one view through
the float64 numpy restatement on the CPU (what a per-image host metric costs, without the device-to-host copy).
    python tools/bench_ssim.py [--views 288] [--iters 20]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ssim_f64  # noqa: E402
from vicasplat_amd import callers  # noqa: E402


def median_ms(fn, iters):
    ts = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=288)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    d = torch.device("cuda:0")
    g = torch.Generator(device=d).manual_seed(0)
    gt = torch.rand(a.views, 3, a.res, a.res, generator=g, device=d)
    pred = (gt * 0.8 + 0.2 * torch.rand(a.views, 3, a.res, a.res, generator=g, device=d)).contiguous()
    Y = pred.clone().requires_grad_(True)

    def fwd():
        callers.compute_ssim(gt, pred)

    def fwd_bwd():
        s, _, _, t = callers.ssim(gt, Y, data_range=1.0, retrun_seprate=True)
        torch.autograd.grad((1 - s) + (1 - t), Y)

    for _ in range(3):
        fwd()
        fwd_bwd()
    torch.cuda.synchronize()
    ms_f = median_ms(fwd, a.iters)
    ms_fb = median_ms(fwd_bwd, a.iters)
    x0, y0 = gt[0].double().cpu().numpy(), pred[0].double().cpu().numpy()
    ssim_f64.ssim_metric_f64(x0, y0)
    t0 = time.perf_counter()
    for _ in range(3):
        ssim_f64.ssim_metric_f64(x0, y0)
    cpu_ms = (time.perf_counter() - t0) / 3 * 1e3
    nbytes = 2 * gt.numel() * 4
    print(json.dumps({"views": a.views, "shape": [3, a.res, a.res], "metric_fwd_ms": round(ms_f, 4), "loss_fwd_bwd_ms": round(ms_fb, 4),
                      "metric_fwd_GBps": round(nbytes / (ms_f * 1e-3) / 1e9, 1), "cpu_f64_ms_per_view": round(cpu_ms, 2),
                      "cpu_ms_for_all_views_est": round(cpu_ms * a.views, 1), "gpu_speedup_vs_cpu_est": round(cpu_ms * a.views / ms_f, 1)}))


if __name__ == "__main__":
    main()
