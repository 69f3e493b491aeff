"""LPIPS-VGG timing, HIP kernels against the torch backend on the same device (seeded He-scaled VGG weights; the cost does not depend on them).

  * the metric: callers.compute_lpips on `--pairs` pairs of 3 x 256 x 256 (metrics.py:37-44), against LossLpips.distance (torch backend);
  * the training term: LossLpips(backend="hip") forward + backward (gradient of the prediction) on each of `--views`, against
    LossLpips(backend="torch").
Prints one JSON line: median ms, algorithmic TFLOP/s (40.09 GFLOP per image forward at 256^2; the loss counts the forward of both images and
the prediction's data-gradient chain, 3 x 40.09), for the HIP path the executed-MFMA fraction (split operands execute three MFMAs per
product: 3 x TFLOP/s over the 2.5 PFLOP/s dense f16 peak), and torch.cuda.max_memory_allocated of each leg.
    python tools/bench_lpips.py [--pairs 288] [--views 96 288] [--iters 5] [--skip-torch]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import lpips_f64  # noqa: E402
from vicasplat_amd import callers  # noqa: E402

GF_PER_IMAGE = sum(2 * (256 * 256 >> (2 * s)) * co * 9 * ci for s, chans in enumerate(lpips_f64.CHANNELS)
                   for ci, co in zip(chans[:-1], chans[1:])) / 1e9      # 40.09
PEAK_F16_TFLOPS = 2500.0


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


def leg(fn, iters, gflop, split):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    ms = median_ms(fn, iters)
    tf = gflop / ms          # GFLOP / ms = TFLOP/s
    out = {"ms": round(ms, 2), "tflops": round(tf, 1), "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 2**30, 2)}
    if split:
        out["executed_mfma_fraction"] = round(3 * tf / PEAK_F16_TFLOPS, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=288)
    ap.add_argument("--views", type=int, nargs="+", default=[96, 288])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--skip-torch", action="store_true")
    a = ap.parse_args()
    d = torch.device("cuda:0")
    sd = lpips_f64.fake_state_dict(0)
    net = callers.LpipsVgg(sd, device=d)
    hip = callers.LossLpips(sd, backend="hip", device=d)
    ref = callers.LossLpips(sd).to(d)
    g = torch.Generator(device=d).manual_seed(0)
    n = max([a.pairs] + a.views)
    gt = torch.rand(n, 3, 256, 256, generator=g, device=d)
    pred = (0.8 * gt + 0.2 * torch.rand(n, 3, 256, 256, generator=g, device=d)).contiguous()
    res = {"gflop_per_image_fwd": round(GF_PER_IMAGE, 2), "metric": {"pairs": a.pairs}, "loss": {}}
    P = a.pairs
    res["metric"]["hip"] = leg(lambda: callers.compute_lpips(gt[:P], pred[:P], net), a.iters, 2 * GF_PER_IMAGE * P, True)
    if not a.skip_torch:
        with torch.no_grad():
            res["metric"]["torch"] = leg(lambda: ref.distance(gt[:P], pred[:P]), a.iters, 2 * GF_PER_IMAGE * P, False)
        res["metric"]["speedup"] = round(res["metric"]["torch"]["ms"] / res["metric"]["hip"]["ms"], 2)
    for v in a.views:
        tgt = gt[:v].view(1, v, 3, 256, 256)
        x = pred[:v].view(1, v, 3, 256, 256).clone().requires_grad_()

        def step(loss):
            return lambda: torch.autograd.grad(loss(x, tgt, 0), x)

        r = {"hip": leg(step(hip), a.iters, 3 * GF_PER_IMAGE * v, True)}
        if not a.skip_torch:
            r["torch"] = leg(step(ref), a.iters, 3 * GF_PER_IMAGE * v, False)
            r["speedup"] = round(r["torch"]["ms"] / r["hip"]["ms"], 2)
        res["loss"][f"views_{v}"] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
