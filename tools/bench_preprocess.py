"""Crop-shim timing: vsp_rescale_crop (csrc/preprocess.hip) on one training step's frames against PIL on the host.

The batch: 480 frames (24 scenes x (8 context + 12 target views)) of 360 x 640, uint8 packed HWC as a decoder delivers them, to 256 x 256
(scaled 256 x 455, crop column 99), every other scene mirrored.  332 MB of source: more than the 256 MiB Infinity Cache holds.
  kernel     warmed, then windows of `--calls` launches between two device events; the median window over its calls is a batch's time
             (the Python glue of crop_shim.rescale_and_crop included: that is what a step pays).
  byte floor (source bytes under the crop window's taps + bytes written) / 6.3 TB/s, the bytes computed from the tables; the kernel's share
             of it is floor / kernel time.  The kernel's integer work is not in the floor.
  PIL        Image.resize((455, 256), Image.LANCZOS) of single frames on one thread of THIS host, in the same run, median over
             `--pil-frames` frames (the tensor <-> PIL conversions of the reference's rescale not included).
Frame 0 and a mirrored frame are compared with PIL's bytes.  Prints one JSON line; exits non-zero if the kernel's batch time exceeds
PIL's batch time / 16 (16 CPU cores: what a training job is taken to have beside its GPUs), or if a byte differs.
    python tools/bench_preprocess.py [--iters 20] [--calls 10] [--pil-frames 24]
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

from vicasplat_amd.dataset.shims import crop_shim  # noqa: E402

SCENES, VIEWS, H, W, SHAPE = 24, 20, 360, 640, (256, 256)
COPY_RATE = 6.3e12      # bytes / s, the measured copy rate of the device
CPUS = 16


def floor_bytes():
    """(source bytes under the crop window, bytes written) per frame, from the tables."""
    h_scaled, w_scaled = crop_shim.scaled_size(H, W, SHAPE)
    row, col = (h_scaled - SHAPE[0]) // 2, (w_scaled - SHAPE[1]) // 2

    def span(n_in, n_out, first, count):
        if n_in == n_out:
            return count
        bounds, _ = crop_shim.resample_tables(n_in, n_out)
        window = bounds[first:first + count]
        return int((window[:, 0] + window[:, 1]).max() - window[:, 0].min())
    return 3 * span(H, h_scaled, row, SHAPE[0]) * span(W, w_scaled, col, SHAPE[1]), 4 * 3 * SHAPE[0] * SHAPE[1]


def window_ms(fn, calls):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / calls


def main():
    import PIL
    from PIL import Image
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--pil-frames", type=int, default=24)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_preprocess.py needs a GPU"
    d = torch.device("cuda:0")
    n = SCENES * VIEWS
    g = torch.Generator(device=d).manual_seed(0)
    frames = torch.randint(0, 256, (SCENES, VIEWS, H, W, 3), dtype=torch.uint8, device=d, generator=g)
    image = frames.permute(0, 1, 4, 2, 3)      # [B, V, 3, h, w]: a view of the packed buffer
    K = torch.eye(3, device=d).repeat(SCENES, VIEWS, 1, 1)
    mirror = (torch.arange(SCENES, device=d) % 2).to(torch.uint8).view(SCENES, 1).expand(SCENES, VIEWS).contiguous()
    fn = lambda: crop_shim.rescale_and_crop(image, K, SHAPE, mirror=mirror)
    for _ in range(3):
        out, _ = fn()
    torch.cuda.synchronize()
    ts = [window_ms(fn, a.calls) for _ in range(a.iters)]
    kernel_ms = float(np.median(ts))

    # PIL on this host, one thread, and the bytes of two frames
    h_scaled, w_scaled = crop_shim.scaled_size(H, W, SHAPE)
    col = (w_scaled - SHAPE[1]) // 2
    differing = 0
    for b, v in ((0, 0), (1, 3)):
        src = frames[b, v].cpu().numpy()
        if b % 2:
            src = np.ascontiguousarray(src[:, ::-1])
        want = np.array(Image.fromarray(src).resize((w_scaled, h_scaled), Image.LANCZOS))[:, col:col + SHAPE[1]]
        differing += int((out[b, v].cpu().numpy() != np.moveaxis(want.astype(np.float32) / np.float32(255), -1, 0)).sum())
    host = [frames[i % SCENES, i % VIEWS].cpu().numpy() for i in range(a.pil_frames)]
    pil = []
    for src in host:
        im = Image.fromarray(src)
        t0 = time.perf_counter()
        im.resize((w_scaled, h_scaled), Image.LANCZOS)
        pil.append(1e3 * (time.perf_counter() - t0))
    pil_ms = float(np.median(pil))

    src_bytes, out_bytes = floor_bytes()
    floor_ms = 1e3 * n * (src_bytes + out_bytes) / COPY_RATE
    res = dict(frames=n, source=[H, W], output=list(SHAPE), iters=a.iters, calls_per_window=a.calls,
               kernel_ms_per_batch=round(kernel_ms, 4), kernel_ms_min_max=[round(min(ts), 4), round(max(ts), 4)],
               source_bytes_per_frame=src_bytes, written_bytes_per_frame=out_bytes, byte_floor_ms=round(floor_ms, 4),
               share_of_byte_floor=round(floor_ms / kernel_ms, 4), pil_ms_per_frame=round(pil_ms, 3),
               pil_ms_per_batch_one_thread=round(pil_ms * n, 1), pil_ms_per_batch_16_cpus=round(pil_ms * n / CPUS, 1),
               speedup_over_16_cpus=round(pil_ms * n / CPUS / kernel_ms, 1), differing_bytes_vs_pil=differing,
               pillow_version=PIL.__version__)
    print(json.dumps(res))
    if differing:
        print(f"FAIL: {differing} output elements differ from PIL's", file=sys.stderr)
        sys.exit(1)
    if kernel_ms > pil_ms * n / CPUS:
        print(f"FAIL: the kernel ({kernel_ms:.3f} ms per batch) is slower than PIL on {CPUS} CPUs ({pil_ms * n / CPUS:.1f} ms)", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
