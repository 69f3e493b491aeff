"""Event-times the split-class 256 -> 256 3x3 convolution of the DPT trunk's residual conv units (dpt.py, _rcu) at the bench step's two large
map sizes, f32 NHWC input, with the unit's epilogues: conv1 = relu_in + bias + relu_out, conv2 = bias + residual (+ the second residual of a
fusion block).  One JSON line per configuration: median / min / max ms over the timed launches and the executed-MFMA rate.

    python tools/bench_conv_trunk.py [--iters 20] [--warmup 5] [--tag NAME]

A/B of two builds: run it once per build with VICASPLAT_HIP_LIB pointing at the other library, alternating."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from vicasplat_amd import ops

SHAPES = [(192, 64, 64, 256), (192, 32, 32, 256)]
CONFIGS = [   # name, relu_in, relu_out, residual, residual2
    ("c1 relu_in+bias+relu_out", True, True, False, False),
    ("c2 bias+res", False, False, True, False),
    ("c2 bias+res+res2", False, False, True, True),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tag", default=os.environ.get("VICASPLAT_HIP_LIB", "tree"))
    a = ap.parse_args()
    d = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    w = ops.pack_conv3x3_weight((torch.randn(256, 256, 3, 3, generator=g) / 48.0).to(d), "split")
    b = torch.randn(256, generator=g).to(d)
    for N, H, W, C in SHAPES:
        x = torch.randn(N, H, W, C, device=d)
        r1, r2, out = torch.randn_like(x), torch.randn_like(x), torch.empty_like(x)
        for name, relu_in, relu_out, res, res2 in CONFIGS:
            run = lambda: ops.conv3x3_nhwc(x, w, b, residual=r1 if res else None, residual2=r2 if res2 else None, relu_in=relu_in,
                                           relu_out=relu_out, out=out)
            for _ in range(a.warmup):
                run()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
            for s, e in ev:
                s.record(); run(); e.record()
            torch.cuda.synchronize()
            ms = sorted(s.elapsed_time(e) for s, e in ev)
            med = ms[len(ms) // 2]
            mfma_flop = 3 * 2.0 * N * H * W * 256 * 9 * C      # three f16 MFMAs per product
            print(json.dumps(dict(tag=a.tag, shape=[N, H, W, C], config=name, ms_median=round(med, 4), ms_min=round(ms[0], 4),
                                  ms_max=round(ms[-1], 4), pflops_mfma=round(mfma_flop / med / 1e12, 3))), flush=True)


if __name__ == "__main__":
    main()
