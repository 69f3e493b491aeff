"""Trajectory-metric timing: callers.camera_eval_metrics on the HIP backend (csrc/trajectory.hip, one launch per batch) against the torch
backend (the same algorithm in plain float64 torch, torch's own batched SVD) on the same device.

Shapes: B = 24 scenes of V = 8 context views (the training batch), B = 24 of V = 70 (the demo's video length: two trips over the wave),
B = 1 of V = 8 (the reference's one scene per call).  Per shape: both backends warmed, then windows of `--calls` calls between two device
events, the backends alternating window by window; the median window over its calls is a call's time (launch and glue included: that is
what a test step pays).  Prints one JSON line with both backends and the largest difference of their results; exits non-zero if the HIP
backend is slower at B = 24, V = 8.
    python tools/bench_traj.py [--iters 30] [--calls 20]
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

SHAPES = ((24, 8), (24, 70), (1, 8))


def trajectories(B, V, seed, device):
    """Random walks with slowly turning cameras and their estimates: the truth under a similarity, every pose perturbed.  f32, as the encoder
    hands its poses over."""
    g = torch.Generator().manual_seed(seed)

    def rot(w):
        th = w.norm(dim=-1, keepdim=True).clamp_min(1e-12)[..., None]
        k = w / th[..., 0]
        z = torch.zeros_like(k[..., 0])
        K = torch.stack([z, -k[..., 2], k[..., 1], k[..., 2], z, -k[..., 0], -k[..., 1], k[..., 0], z], -1).unflatten(-1, (3, 3))
        return torch.eye(3, dtype=w.dtype) + th.sin() * K + (1 - th.cos()) * (K @ K)

    y = torch.randn(B, V, 3, generator=g, dtype=torch.float64).cumsum(1)
    Rq = rot(0.3 * torch.randn(B, V, 3, generator=g, dtype=torch.float64))
    for i in range(1, V):
        Rq[:, i] = Rq[:, i - 1] @ Rq[:, i]
    R0, s, t0 = rot(torch.randn(B, 1, 3, generator=g, dtype=torch.float64)), 0.5 + torch.rand(B, 1, 1, generator=g, dtype=torch.float64), torch.randn(B, 1, 3, generator=g, dtype=torch.float64)
    x = s * (y @ R0[:, 0].transpose(1, 2)) + t0 + 0.05 * torch.randn(B, V, 3, generator=g, dtype=torch.float64)
    Rp = R0 @ Rq @ rot(0.1 * torch.randn(B, V, 3, generator=g, dtype=torch.float64))
    P, Q = torch.eye(4, dtype=torch.float64).repeat(B, V, 1, 1), torch.eye(4, dtype=torch.float64).repeat(B, V, 1, 1)
    P[..., :3, :3], P[..., :3, 3], Q[..., :3, :3], Q[..., :3, 3] = Rp, x, Rq, y
    return P.float().to(device), Q.float().to(device)


def window_ms(fn, calls):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    d = torch.device("cuda:0")
    res = {"iters": a.iters, "calls_per_window": a.calls, "shapes": {}}
    for B, V in SHAPES:
        P, Q = trajectories(B, V, 100 * B + V, d)
        fns = {k: (lambda k=k: callers.camera_eval_metrics(P, Q, backend=k, return_valid=True)) for k in ("hip", "torch")}
        outs = {}
        for k, fn in fns.items():
            for _ in range(5):
                outs[k] = fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in fns}
        for _ in range(a.iters):
            for k, fn in fns.items():
                ts[k].append(window_ms(fn, a.calls))
        hip, ref = (torch.stack(outs[k][:3], -1) for k in ("hip", "torch"))
        r = {k + "_us": round(1e3 * float(np.median(v)), 2) for k, v in ts.items()}
        r.update({k + "_us_min_max": [round(1e3 * min(v), 2), round(1e3 * max(v), 2)] for k, v in ts.items()})
        r["valid"] = int(outs["hip"][3].sum())
        r["max_rel_difference"] = float(((hip - ref).abs() / ref.abs().clamp_min(1e-300)).max())
        res["shapes"][f"B={B},V={V}"] = r
    print(json.dumps(res))
    head = res["shapes"]["B=24,V=8"]
    if head["hip_us"] > head["torch_us"]:
        print(f"FAIL: the HIP backend ({head['hip_us']} us) is slower than the torch backend ({head['torch_us']} us) at B = 24, V = 8", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
