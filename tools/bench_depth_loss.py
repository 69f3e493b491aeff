"""Depth-smoothness loss timing at the training shape: 24 scenes x 12 targets = 288 views of 256 x 256 (csrc/depth_loss.hip).

Prints one JSON line: per configuration (sigma_image None / 4.0 -- config/loss/depth.yaml has null, the bilateral weights need a value --,
first / second derivative) the median time of forward + backward of callers.depth_smoothness_loss (gradient with respect to depth) on the
HIP backend and on the torch backend (about 25 element-wise passes and autograd, on the same device), the forward alone, the two losses,
and the HIP path's time against the bytes it has to move at the HBM rate (BYTE_FLOOR: DESIGN 5).
    python tools/bench_depth_loss.py [--views 288] [--res 256] [--iters 50]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vicasplat_amd import callers  # noqa: E402

SIGMA = 4.0
HBM_PEAK, HBM_COPY = 8.0e12, 6.3e12      # bytes / s of an MI355X: the specified peak, and what a float4 copy reaches
# per pixel: the forward reads the depth (4) and, with the bilateral weights, the three colour planes (12), and writes the gradient image (4);
# the backward scales that image by the upstream gradient (4 read, 4 written).  The floor of the issue counts the forward alone.
FLOOR_FWD = lambda image: 4 + (12 if image else 0) + 4
BACKWARD = 8


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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--backends", default="hip,torch", help="comma-separated; `hip` alone for a kernel trace")
    a = ap.parse_args()
    d = torch.device("cuda:0")
    g = torch.Generator(device=d).manual_seed(0)
    N, S = a.views, a.res
    depth = (0.5 + 5.5 * torch.rand(N, S, S, generator=g, device=d)).requires_grad_(True)
    near, far = 1.5 + 1.5 * torch.rand(N, generator=g, device=d), 60 + 40 * torch.rand(N, generator=g, device=d)
    image = torch.rand(N, 3, S, S, generator=g, device=d)
    res = {"views": N, "shape": [S, S], "configs": {}}
    for sigma in (None, SIGMA):
        for second in (False, True):
            r = {}
            for backend in a.backends.split(","):
                call = lambda: callers.depth_smoothness_loss(depth, near, far, image, 0.25, sigma, second, backend=backend)

                def fwd():
                    with torch.no_grad():
                        return call()

                def fwd_bwd():
                    torch.autograd.grad(call(), depth)

                for _ in range(3):
                    fwd()
                    fwd_bwd()
                torch.cuda.synchronize()
                r[backend + "_fwd_ms"] = round(median_ms(fwd, a.iters), 4)
                r[backend + "_fwd_bwd_ms"] = round(median_ms(fwd_bwd, a.iters), 4)
                r[backend + "_loss"] = float(fwd())
            px = N * S * S
            r["floor_MB"] = round(FLOOR_FWD(sigma is not None) * px / 1e6, 1)
            r["moved_MB"] = round((FLOOR_FWD(sigma is not None) + BACKWARD) * px / 1e6, 1)
            floor_ms = FLOOR_FWD(sigma is not None) * px / HBM_PEAK * 1e3
            r["floor_ms_at_peak"] = round(floor_ms, 4)
            r["hip_fwd_bwd_over_floor"] = round(r["hip_fwd_bwd_ms"] / floor_ms, 2)
            r["hip_fwd_bwd_over_floor_at_copy_rate"] = round(r["hip_fwd_bwd_ms"] / (floor_ms * HBM_PEAK / HBM_COPY), 2)
            r["hip_fwd_bwd_GBps_moved"] = round(r["moved_MB"] / r["hip_fwd_bwd_ms"], 1)
            if "torch_fwd_bwd_ms" in r:
                r["speedup_fwd_bwd"] = round(r["torch_fwd_bwd_ms"] / r["hip_fwd_bwd_ms"], 2)
            res["configs"][f"sigma={sigma},second={second}"] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
