"""Distillation point loss timing at a stage-1 batch: B = 24 pairs of 256 x 256 point maps (csrc/distill.hip).

Prints one JSON line: the median time of forward + backward of callers.Regr3D (normalize_pts, predicted confidences given, gradients with
respect to both predicted point maps and confidences) on the HIP backend and on the torch backend (two torch.quantile sorts, boolean-mask
gathers, element-wise passes and autograd, on the same device), the forward alone, and the effective bandwidth of the HIP path against the
bytes its kernels move (BYTES_PER_PIXEL_VIEW: DESIGN 7).
    python tools/bench_distill.py [--batch 24] [--res 256] [--iters 20]
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

# per pixel and view: select 12 (pseudo-GT point; its three later passes re-read it from L2) + stats 32 (both points, both confidences)
# + loss 28 (both points, pseudo-GT confidence) + backward 32 read, 16 written
BYTES_PER_PIXEL_VIEW = 12 + 32 + 28 + 32 + 16


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
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    d = torch.device("cuda:0")
    g = torch.Generator(device=d).manual_seed(0)
    shape = (a.batch, a.res, a.res)
    rnd = lambda *s: torch.randn(*s, generator=g, device=d)
    gt = [rnd(*shape, 3) * torch.tensor([1.0, 0.7, 1.5], device=d) + torch.tensor([0.2, -0.1, 2.0], device=d) for _ in range(2)]
    pr = [(x * 1.1 + 0.3 * rnd(*shape, 3)).requires_grad_(True) for x in gt]
    cg = [1 + torch.exp(rnd(*shape)) for _ in range(2)]
    pc = [(1 + torch.exp(rnd(*shape))).requires_grad_(True) for _ in range(2)]
    res = {"batch": a.batch, "shape": [a.res, a.res]}
    for backend in ("hip", "torch"):
        fn = callers.Regr3D(backend=backend)

        def fwd():
            with torch.no_grad():
                return fn(gt[0], gt[1], pr[0], pr[1], cg[0], cg[1], pc[0], pc[1], normalize_pts=True)

        def fwd_bwd():
            torch.autograd.grad(fn(gt[0], gt[1], pr[0], pr[1], cg[0], cg[1], pc[0], pc[1], normalize_pts=True), pr + pc)

        for _ in range(3):
            fwd()
            fwd_bwd()
        torch.cuda.synchronize()
        res[backend + "_fwd_ms"] = round(median_ms(fwd, a.iters), 4)
        res[backend + "_fwd_bwd_ms"] = round(median_ms(fwd_bwd, a.iters), 4)
        res[backend + "_loss"] = float(fwd())
    nbytes = BYTES_PER_PIXEL_VIEW * 2 * a.batch * a.res * a.res
    res["hip_fwd_bwd_GBps"] = round(nbytes / (res["hip_fwd_bwd_ms"] * 1e-3) / 1e9, 1)
    res["speedup_fwd_bwd"] = round(res["torch_fwd_bwd_ms"] / res["hip_fwd_bwd_ms"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
