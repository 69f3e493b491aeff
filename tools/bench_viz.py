"""Video-tail timing: the depth range plus the uint8 frames of a 60-frame 256 x 256 video (callers.depth_video_frames: csrc/viz.hip, four
selection passes over the depth maps and one frame kernel) against the same frames built from PyTorch device ops alone -- torch.quantile
twice, log, the x of vis_depth_map, clamp, the index, a table lookup, cat with the white gap, clip * 255 and the cast -- and, when
matplotlib imports, against the reference's own route: the x copied to the host, matplotlib's colour map, the colours copied back, vcat
per frame, and the stack copied to the host.

All three warmed, then windows of `--calls` calls between two device events (the host route: a host clock around calls that end in a
device-to-host copy), alternating window by window; the median window over its calls is a call's time, launch and glue included.  Prints one
JSON line: the three times, the bytes the frames need at the least (depth and rgb read once, frames written once) over 6.3 TB/s as
`floor_us`, and `floor_ratio` = hip_us / floor_us; the frames of the two device routes are compared (pixels may differ where an index sits
within rounding of a step).  Exits non-zero if the kernels are slower than the PyTorch composition.
    python tools/bench_viz.py [--iters 20] [--calls 10] [--frames 60] [--size 256]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vicasplat_amd import callers  # noqa: E402
from vicasplat_amd.visualization.color_map import device_table  # noqa: E402

COPY_RATE = 6.3e12      # bytes / s: the float4 copy rate of the device


def video_inputs(F, S, device, seed=0):
    """Frames in [-0.1, 1.1] and log-uniform depths on [0.5, 50] with 5 % zeros (pixels no Gaussian covers)."""
    g = torch.Generator().manual_seed(seed)
    rgb = torch.rand(F, 3, S, S, generator=g) * 1.2 - 0.1
    depth = torch.exp(torch.rand(F, S, S, generator=g) * (np.log(50.0) - np.log(0.5)) + np.log(0.5))
    depth[torch.rand(F, S, S, generator=g) < 0.05] = 0
    return rgb.to(device), depth.to(device)


def torch_frames(rgb, depth, lut, gap=8):
    """The same outputs from PyTorch device ops alone."""
    flat = depth.reshape(-1)
    far = flat.quantile(0.99).log()
    near = flat[flat > 0].quantile(0.01).log()
    x = 1 - (depth.log() - near) / (far - near)
    idx = (x.clamp(0, 1) * 256).to(torch.int64).clamp_max(255)
    col = lut[idx].permute(0, 3, 1, 2)
    F, _, H, W = rgb.shape
    video = torch.cat([rgb, torch.ones(F, 3, gap, W, device=rgb.device), col], dim=2)
    return (video.clip(min=0, max=1) * 255).type(torch.uint8)


def host_frames(rgb, depth, cmap, gap=8):
    """The reference's route (src/misc/utils.py:13-22, src/visualization/color_map.py:9-27, model_wrapper.py:805-813)."""
    flat = depth.reshape(-1)
    far = flat.quantile(0.99).log()
    near = flat[flat > 0].quantile(0.01).log()
    x = 1 - (depth.log() - near) / (far - near)
    col = torch.tensor(cmap(x.clip(min=0, max=1).cpu().numpy())[..., :3], device=depth.device, dtype=torch.float32).permute(0, 3, 1, 2)
    white = torch.ones(3, gap, rgb.shape[-1], device=rgb.device)
    video = torch.stack([torch.cat([r, white, c], dim=1) for r, c in zip(rgb, col)])
    return (video.clip(min=0, max=1) * 255).type(torch.uint8).cpu().numpy()


def window_ms(fn, calls):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / calls


def host_window_ms(fn, calls):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(calls):
        fn()
    return 1e3 * (time.perf_counter() - t) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--size", type=int, default=256)
    a = ap.parse_args()
    d = torch.device("cuda:0")
    F, S = a.frames, a.size
    rgb, depth = video_inputs(F, S, d)
    lut = device_table("turbo", d)
    fns = {"hip": (lambda: callers.depth_video_frames(rgb, depth), window_ms), "torch": (lambda: torch_frames(rgb, depth, lut), window_ms)}
    try:
        import matplotlib
        cmap = matplotlib.colormaps["turbo"]
        fns["host"] = (lambda: host_frames(rgb, depth, cmap), host_window_ms)
    except ImportError:
        pass
    outs = {}
    for k, (fn, _) in fns.items():
        for _ in range(3):
            outs[k] = fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(a.iters):
        for k, (fn, window) in fns.items():
            ts[k].append(window(fn, a.calls if k != "host" else max(1, a.calls // 5)))
    res = {"frames": F, "size": S, "iters": a.iters, "calls_per_window": a.calls}
    res.update({k + "_us": round(1e3 * float(np.median(v)), 2) for k, v in ts.items()})
    res.update({k + "_us_min_max": [round(1e3 * min(v), 2), round(1e3 * max(v), 2)] for k, v in ts.items()})
    need = depth.numel() * 4 + rgb.numel() * 4 + outs["hip"].numel()
    res["floor_us"] = round(1e6 * need / COPY_RATE, 2)
    res["floor_ratio"] = round(res["hip_us"] / res["floor_us"], 2)
    res["pixels_differing_from_torch"] = int((outs["hip"] != outs["torch"]).any(1).sum())
    res["pixels"] = int(outs["hip"].numel() // 3)
    if "host" in outs:
        res["pixels_differing_from_host"] = int((outs["hip"].cpu().numpy() != outs["host"]).any(1).sum())
    print(json.dumps(res))
    if res["hip_us"] > res["torch_us"]:
        print(f"FAIL: the kernels ({res['hip_us']} us) are slower than the PyTorch composition ({res['torch_us']} us)", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
