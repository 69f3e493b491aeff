"""Time the PNG file output of one evaluation step's frames on the GPU path against PIL in the same run.

480 frames of 256 x 256 RGB (the 192 context and 288 target frames of the bench line's 24-scene step), three classes:
  rendered   the package's own synthetic scene (synthetic.conditioned_weights on synthetic.smooth_input through the encoder once), seen by
             480 cameras through render_cuda
  constant   one colour per frame
  noise      uniform random bytes
Timed separately per class: the kernels behind vse_png_encode (misc.image_io.encode_png_device) and the copy of the lengths and the used
bytes to the host (what encode_png_batch does after them); file writes are excluded on both sides.  The yardstick is
Image.fromarray(prep_image(x)).save(BytesIO) of the same frames on one core, divided by the 16 CPUs a job may use.  PIL must decode the
GPU's files to the exact pixels, and the GPU path (kernels + copies) must not be slower than PIL over 16 CPUs in any class: otherwise the
exit code is 1.  One JSON line.

    python tools/bench_png.py [--frames 480] [--repeats 7]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_png.py --repeats 2 --no-pil      # the kernel split (profiles/png.md)
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

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

RES, CPUS = 256, 16


def rendered_frames(n: int, dev):
    import torch
    from vicasplat_amd import synthetic
    from vicasplat_amd.model.decoder.cuda_splatting import render_cuda
    from vicasplat_amd.model.encoder import default_cfg, get_encoder
    shapes = json.load(open(os.path.join(ROOT, "tests", "golden", "shapes_full.json")))
    enc, _ = get_encoder(default_cfg())
    enc.load_state_dict(synthetic.conditioned_weights(shapes, 0), strict=True)
    enc = enc.to(dev).eval().requires_grad_(False)
    enc.set_compute_dtype("split")
    img, K = synthetic.smooth_input(1, 2, RES, 0)
    with torch.no_grad():
        g = enc(dict(image=img.to(dev), intrinsics=K.to(dev)), compute_viewspace_depth=False)["gaussians"]
        frames = []
        for at in range(0, n, 48):
            v = min(48, n - at)
            E = torch.eye(4, device=dev).repeat(v, 1, 1)
            E[:, 0, 3] = (torch.arange(v, device=dev) + at) * (0.6 / n) - 0.05
            Kt = torch.tensor([[0.9, 0, 0.5], [0, 0.9, 0.5], [0, 0, 1.0]], device=dev).repeat(v, 1, 1)
            near, far = torch.full((v,), 0.01, device=dev), torch.full((v,), 100.0, device=dev)
            col, _ = render_cuda(E, Kt, near, far, (RES, RES), torch.zeros(v, 3, device=dev), g.means.flatten(1, 3)[0],
                                 g.covariances.flatten(1, 3)[0], g.harmonics.flatten(1, 3)[0], g.opacities.flatten(1)[0])
            frames.append(col)
    del enc
    return torch.cat(frames).contiguous()


def pil_encode_all(pixels: np.ndarray) -> tuple[float, int]:
    """(seconds on one core, bytes) of Image.fromarray(x).save(BytesIO) over uint8 [N, H, W, 3]."""
    from PIL import Image
    t0, total = time.perf_counter(), 0
    for x in pixels:
        buf = io.BytesIO()
        Image.fromarray(x).save(buf, "PNG")
        total += buf.tell()
    return time.perf_counter() - t0, total


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=480)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-pil", action="store_true", help="skip the yardstick and the verdict (profiling runs)")
    args = ap.parse_args()

    import torch
    from PIL import Image
    from vicasplat_amd.misc import image_io
    if not torch.cuda.is_available():
        print("bench_png.py needs a GPU: nothing here is measured on the CPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    n = args.frames
    gen = torch.Generator(device=dev).manual_seed(0)
    classes = {"rendered": rendered_frames(n, dev),
               "constant": torch.rand(n, 3, 1, 1, device=dev, generator=gen).expand(n, 3, RES, RES).contiguous(),
               "noise": torch.rand(n, 3, RES, RES, device=dev, generator=gen)}
    torch.cuda.empty_cache()

    def once(frames):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        t0 = time.perf_counter()
        e[0].record()
        out, lengths = image_io.encode_png_device(frames)
        e[1].record()
        sizes = lengths.cpu()
        used = out[torch.arange(out.shape[1], device=dev)[None, :] < lengths[:, None]].cpu()
        e[2].record()
        torch.cuda.synchronize()
        return dict(kernels=e[0].elapsed_time(e[1]), copy=e[1].elapsed_time(e[2]), wall=(time.perf_counter() - t0) * 1e3), sizes, used

    line, ok = dict(frames=n, height=RES, width=RES), True
    for name, frames in classes.items():
        for _ in range(2):          # warm-up: code objects, the allocator's blocks
            once(frames)
        runs = []
        for _ in range(args.repeats):
            t, sizes, used = once(frames)
            runs.append(t)
        med = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
        gpu_ms, gpu_bytes = med["kernels"] + med["copy"], int(sizes.sum())
        line[name] = dict(kernels_ms=round(med["kernels"], 3), copy_ms=round(med["copy"], 3), gpu_path_ms=round(gpu_ms, 3),
                          wall_ms=round(med["wall"], 3), gpu_bytes=gpu_bytes, raw_bytes=n * RES * RES * 3)
        pixels = torch.stack([image_io.prep_image(f) for f in frames]).cpu().numpy()
        files, at = used.numpy().tobytes(), 0
        differing = 0
        for i, size in enumerate(sizes.tolist()):          # PIL reads the GPU's own files back
            if i % 37 == 0 or i == n - 1:
                differing += int((np.asarray(Image.open(io.BytesIO(files[at:at + size]))) != pixels[i]).sum())
            at += size
        line[name]["differing_pixels"] = differing
        ok &= differing == 0 and at == len(files)
        if not args.no_pil:
            pil_s, pil_bytes = pil_encode_all(pixels)
            pil_ms = pil_s * 1e3 / CPUS
            line[name].update(pil_one_core_ms=round(pil_s * 1e3, 1), pil_16_cpus_ms=round(pil_ms, 2), pil_bytes=pil_bytes,
                              bytes_vs_pil=round(gpu_bytes / pil_bytes, 4), speedup_vs_pil_16_cpus=round(pil_ms / gpu_ms, 1))
            ok &= gpu_ms <= pil_ms
    print(json.dumps(line))
    if not ok:
        print("FAILED: a class is slower than PIL over 16 CPUs, or PIL reads other pixels out of the GPU's files", file=sys.stderr)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
