"""Vector drawing on the GPU (csrc/draw.hip) against the torch backend on the device in the same process:
  cameras   draw_cameras(256, ...) for 8 + 12 cameras with near and far planes: four layers over three projections, one launch per layer on
            the HIP backend, twelve draw_lines calls of dozens of torch launches each on the torch backend;
  lines     draw_lines with 4 096 random lines of width 2 on 1024 x 1024, round caps, one refinement pass.
Exits non-zero if the HIP backend is slower than the torch backend on either workload, or if the outputs disagree.

Agreement.  Both backends are f32 evaluations of include/vicasplat_draw.h; the general-case criterion of tests/draw_f64.py bounds each
against float64 by 4 x 2^-24 mag + (amb / 64) spread, with at most 10 % of the pixels ambiguous.  The float64 restatement is numpy and takes
minutes at these sizes, so the tool applies the criterion itself to a cut-down instance of the second workload (40 lines on 96 x 96: the
same generator) and, at full size, checks what the criterion implies for two f32 runs: the elements where they differ by more than
8 x 2^-24 x 7 (twice the bound at the largest mag of a unit-range picture) are ambiguous ones -- at most 10 % of the pixels -- and no
difference exceeds the spread of a unit-range picture, 1.

The floor.  A (sample, primitive) test of a round-capped line is about 60 f32 lane-operations, counted from `covers` in csrc/draw.hip with
contraction off: 6 subtractions, 10 products and 6 sums, 3 correctly rounded square roots of about 10 instructions each, 8 compares and
mask operations; a test is made for every sample of a tile (its 180 pass-0 samples inside the image and 64 per refined pixel) against every
record that survives the tile's cull -- counted here with the kernel's own cull rule, restated in torch, and the torch backend's refine mask.
The rate divided by is the f32 vector issue rate, 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz = 78.6e12 lane-operations per second.  The
kernel stops walking a sample's list at the first hit, so on a densely covered picture it can run below this count.

    python tools/bench_draw.py [--lines 4096] [--size 1024]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OPS_PER_TEST = 60
LANE_OPS_PER_SECOND = 256 * 4 * 32 * 2.4e9
U = 2.0 ** -24


def timed(fn, reps: int) -> float:
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


def agree(name: str, hip: torch.Tensor, ref: torch.Tensor) -> bool:
    d = (hip.double() - ref.double()).abs()
    differing = float((d > 8 * U * 7).any(dim=-3).float().mean())
    print(f"{name}: max |hip - torch| {float(d.max()):.3g}; {differing * 100:.3f} % of the pixels differ by more than 8 x 2^-24 x 7")
    return differing <= 0.10 and float(d.max()) <= 1.0


def survivors(rec: torch.Tensor, H: int, W: int, L) -> torch.Tensor:
    """[tiles_y, tiles_x]: how many line records the kernel's cull keeps per tile (the rule of scan_round in csrc/draw.hip, round cap)."""
    sx, sy, ex, ey, w = (rec[:, k][None, None] for k in range(5))
    ty, tx = torch.meshgrid(torch.arange((H + L.VSG_TILE_H - 1) // L.VSG_TILE_H, device=rec.device),
                            torch.arange((W + L.VSG_TILE_W - 1) // L.VSG_TILE_W, device=rec.device), indexing="ij")
    hw_, hh_ = L.VSG_TILE_W + 2, L.VSG_TILE_H + 2
    fx0, fy0 = (tx * L.VSG_TILE_W - 1).float()[..., None], (ty * L.VSG_TILE_H - 1).float()[..., None]
    fx1, fy1 = fx0 + hw_, fy0 + hh_
    e = (0.5 * w).abs()
    dn = ((ex - sx) ** 2 + (ey - sy) ** 2).sqrt()
    directed = dn > 1e-10
    e = torch.where(directed, e, 4 * e)
    mag = sx.abs() + sy.abs() + ex.abs() + ey.abs() + e + 32768.0
    m = e + mag * 2.0 ** -16
    keep = ~((torch.maximum(sx, ex) + m < fx0) | (torch.minimum(sx, ex) - m > fx1) | (torch.maximum(sy, ey) + m < fy0) | (torch.minimum(sy, ey) - m > fy1))
    ux, uy = (ex - sx) / dn, (ey - sy) / dn
    cx, cy = fx0 + 0.5 * hw_ - sx, fy0 + 0.5 * hh_ - sy
    par, cross = ux * cx + uy * cy, ux * cy - uy * cx
    reach = m + 0.5 * (hw_ * hw_ + hh_ * hh_) ** 0.5 + 0.25
    keep &= ~(directed & ((cross.abs() > reach) | (par < -reach) | (par > dn + reach)))
    return keep.sum(-1)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=4096)
    ap.add_argument("--size", type=int, default=1024)
    a = ap.parse_args()
    import draw_f64 as D
    from vicasplat_amd import _lib as L
    from vicasplat_amd.visualization.drawing import draw_cameras, draw_lines
    from vicasplat_amd.visualization.drawing import lines as LN
    from vicasplat_amd.visualization.drawing import rendering
    assert torch.cuda.is_available(), "bench_draw.py needs a GPU"
    dev = torch.device("cuda:0")
    T = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)
    ok = True

    # ---- the criterion itself on a cut-down instance
    image, rec = D.general_image((96, 96), 1), D.general_lines((96, 96), 40, 2, 2.0, 2.0)
    small = draw_lines(T(image), T(rec[:, 0:2]), T(rec[:, 2:4]), T(rec[:, 5:8]), T(rec[:, 4]))
    passed, report = D.check(small.cpu().numpy(), D.render("lines", image, rec, "round", 1))
    print("criterion on 40 lines of width 2 on 96 x 96: " + ("met" if passed else "MISSED") + "  " + "  ".join(f"{k} {v:.3g}" for k, v in report.items()))
    ok &= passed and report["unsure"] <= 0.02 and report["ambiguous"] <= 0.10

    # ---- cameras
    E, K, colour, near, far = (T(v) for v in D.cameras(20, 8))
    colour = torch.ones_like(colour)
    colour[8:, 1:] = 0      # 8 context cameras in white, 12 target cameras in red, as render_cameras colours them
    cam = lambda backend: draw_cameras(256, E, K, colour, near, far, backend=backend)
    t_hip, t_torch = timed(lambda: cam("hip"), 20), timed(lambda: cam("torch"), 2)
    ok &= agree("cameras", cam("hip"), cam("torch")) and t_hip <= t_torch
    print(f"draw_cameras(256) for 8 + 12 cameras: hip {t_hip * 1e3:.3f} ms per call (4 launches), torch backend {t_torch * 1e3:.1f} ms: {t_torch / t_hip:.0f} x")

    # ---- lines
    S, n = a.size, a.lines
    rec = T(D.general_lines((S, S), n, 3, 2.0, 2.0))
    image = T(D.general_image((S, S), 4))
    args = (rec[:, 0:2], rec[:, 2:4], rec[:, 5:8], rec[:, 4])
    hip = draw_lines(image, *args)
    t_hip = timed(lambda: draw_lines(image, *args), 10)
    t_torch = timed(lambda: draw_lines(image, *args, backend="torch"), 1)
    ok &= agree("lines", hip, draw_lines(image, *args, backend="torch")) and t_hip <= t_torch
    from vicasplat_amd import ops
    off = torch.tensor([0, n], dtype=torch.int32, device=dev)
    out = torch.empty_like(image[None])
    t_kernel = timed(lambda: ops.draw_lines(image[None], rec, off, out=out), 20)
    kept = survivors(rec, S, S, L)
    mask = rendering.detect_msaa_pixels(rendering.render((S, S), lambda xy: rendering.topmost(LN.line_coverage(rec, xy, "round"), rec[:, 5:8]), dev,
                                                         num_passes=0)[None])[0]
    th, tw = L.VSG_TILE_H, L.VSG_TILE_W
    pad = torch.zeros(kept.shape[0] * th, kept.shape[1] * tw, dtype=torch.bool, device=dev)
    pad[:S, :S] = mask
    refined = pad.reshape(kept.shape[0], th, kept.shape[1], tw).sum(dim=(1, 3))
    ys = torch.arange(kept.shape[0], device=dev)[:, None] * th
    xs = torch.arange(kept.shape[1], device=dev)[None, :] * tw
    halo = ((ys + th + 1).clamp(max=S) - (ys - 1).clamp(min=0)) * ((xs + tw + 1).clamp(max=S) - (xs - 1).clamp(min=0))
    tests = int(((halo + 64 * refined) * kept).sum())
    floor = tests * OPS_PER_TEST / LANE_OPS_PER_SECOND
    print(f"draw_lines, {n} lines of width 2 on {S} x {S}: hip {t_hip * 1e3:.3f} ms per call (kernel and binding alone {t_kernel * 1e3:.3f} ms), "
          f"torch backend {t_torch * 1e3:.0f} ms: {t_torch / t_hip:.0f} x")
    print(f"  {float(mask.float().mean()) * 100:.1f} % of the pixels refined; {float(kept.float().mean()):.1f} records survive a tile's cull on average "
          f"(most {int(kept.max())}); {tests:.4g} (sample, record) tests x {OPS_PER_TEST} lane-operations at {LANE_OPS_PER_SECOND:.3g} /s = floor "
          f"{floor * 1e3:.3f} ms: the kernel runs at {floor / t_kernel:.2f} of it")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
