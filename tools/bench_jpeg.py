"""Time the JPEG decode of one training step's frames on the GPU path against PIL in the same run.

480 frames (24 scenes x 20 views) of 360 x 640, 4:2:0, quality 90, a smooth field plus mild noise (about 50 KB per frame), encoded with the
installed PIL.  Timed separately: the host parse (pack_jpeg_batch: the marker walk, the restart search and the copy of the compressed
bytes into the pinned packed buffer), the host -> device copy of that buffer, and the kernels behind vsj_decode.  The yardstick is
Image.open(...).load() of the same streams on one core, divided by the 16 CPUs a loader may use.  The pixels must equal PIL's, 0 differing
bytes, and the GPU path (parse + copy + kernels) must not be slower than PIL over 16 CPUs: otherwise the exit code is 1.  One JSON line.

    python tools/bench_jpeg.py [--frames 480] [--repeats 7]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_jpeg.py --repeats 2      # the kernel split (profiles/jpeg.md)
"""
from __future__ import annotations

import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

H, W, CPUS = 360, 640, 16


def make_streams(n: int, seed: int = 0) -> list[bytes]:
    from PIL import Image
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    out = []
    for i in range(n):
        field = np.stack([128 + 90 * np.sin(x / (40 + c * 7) + 0.1 * i + c) * np.cos(y / (33 + c * 5) - 0.07 * i) for c in range(3)], -1)
        img = np.clip(np.rint(field + g.normal(0, 5, (H, W, 3))), 0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", quality=90, subsampling=2)
        out.append(buf.getvalue())
    return out


def pil_decode_all(streams) -> tuple[float, list]:
    from PIL import Image
    t0 = time.perf_counter()
    images = []
    for s in streams:
        im = Image.open(io.BytesIO(s))
        im.load()
        images.append(im)
    return time.perf_counter() - t0, images


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=480)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()

    import torch
    from vicasplat_amd.dataset.jpeg import decode_packed, pack_jpeg_batch
    if not torch.cuda.is_available():
        print("bench_jpeg.py needs a GPU: nothing here is measured on the CPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    streams = make_streams(args.frames)
    nbytes = sum(map(len, streams))

    pil_s, images = min((pil_decode_all(streams) for _ in range(2)), key=lambda r: r[0])

    def once():
        t0 = time.perf_counter()
        packed = pack_jpeg_batch(streams, pin=True)
        t1 = time.perf_counter()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        buffer = packed.tensor.to(dev, non_blocking=True)
        e[1].record()
        out, status = decode_packed(packed, dev, buffer=buffer)
        e[2].record()
        torch.cuda.synchronize()
        return dict(parse=(t1 - t0) * 1e3, copy=e[0].elapsed_time(e[1]), kernels=e[1].elapsed_time(e[2]),
                    wall=(time.perf_counter() - t0) * 1e3), out, status

    for _ in range(2):          # warm-up: code objects, the pinned and the device allocations
        once()
    runs = []
    for _ in range(args.repeats):
        t, out, status = once()
        runs.append(t)
    med = {k: statistics.median(r[k] for r in runs) for k in runs[0]}

    got = out.cpu().numpy()
    differing = sum(int((got[i] != np.asarray(im)).sum()) for i, im in enumerate(images))
    gpu_ms = med["parse"] + med["copy"] + med["kernels"]
    pil_ms = pil_s * 1e3 / CPUS
    pixels = args.frames * H * W * 3
    line = dict(frames=args.frames, height=H, width=W, bytes_per_frame=round(nbytes / args.frames), pil_one_core_ms=round(pil_s * 1e3, 2),
                pil_16_cpus_ms=round(pil_ms, 2), parse_ms=round(med["parse"], 2), copy_ms=round(med["copy"], 3), kernels_ms=round(med["kernels"], 3),
                gpu_path_ms=round(gpu_ms, 2), wall_ms=round(med["wall"], 2), differing_bytes=differing, status_nonzero=int((status != 0).sum()),
                compressed_GBps=round(nbytes / med["kernels"] / 1e6, 2), pixels_GBps=round(pixels / med["kernels"] / 1e6, 2),
                speedup_vs_pil_16_cpus=round(pil_ms / gpu_ms, 2))
    print(json.dumps(line))
    ok = differing == 0 and line["status_nonzero"] == 0 and gpu_ms <= pil_ms
    if not ok:
        print(f"FAILED: differing bytes {differing}, GPU path {gpu_ms:.2f} ms against PIL over {CPUS} CPUs {pil_ms:.2f} ms", file=sys.stderr)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
