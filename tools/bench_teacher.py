"""Distillation-teacher timing at the training shape: the full-size DUSt3R network (24 + 2 x 12 blocks, two DPT heads) with key-seeded golden
weights on 24 scenes of two 256 x 256 anchor frames, as stage 1 runs it once per step (vicasplat_amd.model.distiller, csrc/teacher.hip).

Prints one JSON line:
  * teacher_ms: the median time of one Dust3R.forward per operand class ("split", the default, and "f16"), and per frame (48 frames per call)
    -- to be read beside the encoder's time per frame of the bench line (the encoder runs 192 frames per step where the teacher runs 48);
  * the two classes' outputs against each other (a plausibility check of the full-size routes: finite, and apart by f16 rounding only);
  * tail: the tail kernel (ops.points_conf) against the PyTorch composition it replaces -- PixelwiseTaskWithDPT.postprocess_pts3d, the
    confidence 1 + exp(c) and the einsum + add of distillation_loss -- on the same raw head output [48, 256, 256, 4], f32 and f16, with and
    without the transform; the two are timed alternately in the same process (medians), and the kernel's time is set against the bytes it
    has to move at the HBM rate.
    python tools/bench_teacher.py [--scenes 24] [--res 256] [--iters 5] [--tail-iters 50] [--classes split,f16]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vicasplat_amd import ops, synthetic  # noqa: E402
from vicasplat_amd.model.distiller import get_distiller  # noqa: E402
from vicasplat_amd.model.encoder.heads.dpt import PixelwiseTaskWithDPT  # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s of an MI355X (specified peak)


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def composition(raw, transform):
    """What the package ran before the kernel existed: about a dozen element-wise passes."""
    pts = PixelwiseTaskWithDPT.postprocess_pts3d(raw.permute(0, 3, 1, 2))
    conf = 1 + raw[..., 3].float().exp()
    if transform is not None:
        pts = torch.einsum("bij,bhwj->bhwi", transform[:, :, :3], pts) + transform[:, None, None, :, 3]
    return pts, conf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=24)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--tail-iters", type=int, default=50)
    ap.add_argument("--classes", default="split,f16")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_teacher.py measures on the GPU; there is none here")
    d = torch.device("cuda:0")
    B, S = a.scenes, a.res
    res = {"scenes": B, "frames": 2 * B, "shape": [S, S]}

    # ---- the whole teacher ----
    shapes = json.load(open(os.path.join(ROOT, "tests", "golden", "shapes_teacher_full.json")))
    teacher = get_distiller("dust3r")
    teacher.load_state_dict(synthetic.golden_weights(shapes, seed=0), strict=True)
    teacher = teacher.to(d)
    img, _ = synthetic.synthetic_input(B, 2, S, seed=0)
    ctx = dict(image=img.to(d))
    outs = {}
    res["teacher_ms"], res["teacher_ms_per_frame"] = {}, {}
    for cls in a.classes.split(","):
        teacher.set_compute_dtype(cls)
        for _ in range(2):
            o = teacher(ctx)
        torch.cuda.synchronize()
        ms = float(np.median([timed(lambda: teacher(ctx)) for _ in range(a.iters)]))
        res["teacher_ms"][cls], res["teacher_ms_per_frame"][cls] = round(ms, 2), round(ms / (2 * B), 3)
        outs[cls] = o
        assert all(bool(torch.isfinite(r[k]).all()) for r in o for k in r), cls
    if len(outs) == 2:
        x, y = outs.values()
        res["classes_apart"] = {f"{k}{v + 1}": float((x[v][k] - y[v][k]).abs().max() / x[v][k].abs().max()) for v in (0, 1) for k in ("pts3d", "conf")}
    res["pts3d_abs_max"] = [float(o[v]["pts3d"].abs().max()) for v in (0, 1)]

    # ---- the tail: kernel against the composition, alternately ----
    g = torch.Generator(device=d).manual_seed(0)
    n = 2 * B
    raw32 = torch.randn(n, S, S, 4, generator=g, device=d) * torch.tensor([1.0, 1.0, 1.5, 1.0], device=d)
    E = torch.eye(3, 4, device=d).repeat(n, 1, 1)
    E[:, :, 3] = torch.randn(n, 3, generator=g, device=d)
    res["tail"] = {}
    for name, raw in (("f32", raw32), ("f16", raw32.half())):
        for tr in (None, E):
            pts, conf = torch.empty(n, S, S, 3, device=d), torch.empty(n, S, S, device=d)
            hip = lambda: ops.points_conf(raw, tr, out_pts=pts, out_conf=conf)
            tor = lambda: composition(raw, tr)
            for _ in range(5):
                hip(), tor()
            torch.cuda.synchronize()
            th, tt = [], []
            for _ in range(a.tail_iters):
                th.append(timed(hip))
                tt.append(timed(tor))
            p_ref, c_ref = tor()
            moved = n * S * S * ((16 if name == "f32" else 8) + 12 + 4)
            r = dict(hip_ms=round(float(np.median(th)), 4), torch_ms=round(float(np.median(tt)), 4), moved_MB=round(moved / 1e6, 1),
                     floor_ms_at_peak=round(moved / HBM_PEAK * 1e3, 4), max_abs_diff=float((pts - p_ref).abs().max()))
            r["speedup"] = round(r["torch_ms"] / r["hip_ms"], 2)
            r["hip_GBps"] = round(moved / 1e6 / r["hip_ms"], 1)
            res["tail"][f"{name},transform={tr is not None}"] = r
    res["tail_not_slower"] = all(r["hip_ms"] <= r["torch_ms"] for r in res["tail"].values())
    print(json.dumps(res))
    if not res["tail_not_slower"]:      # the one timing condition: the kernel must not lose against the passes it replaces
        raise SystemExit("bench_teacher.py: the tail kernel is slower than the PyTorch composition it replaces (see `tail` in the line above)")


if __name__ == "__main__":
    main()
