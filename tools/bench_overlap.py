"""The evaluation-index step on the GPU: one scene of V = 280 frames at 256 x 256 with the shipped configuration's band (min_distance 5,
max_distance 135): vso_view_overlap_counts against the torch backend on the device in the same run, a whole
EvaluationIndexGenerator.test_step against one on the torch backend, and the kernel against its arithmetic floor.  Exits non-zero if
the kernel is slower than the torch backend.

The floor: per ray-pair the kernel issues about 330 f32 vector operations (counted from csrc/overlap.hip with contraction off: 19 correctly
rounded divisions of about 10 instructions each, 2 square roots of about 8, 100 products, sums and compares, the integer row / column
split), each one lane-operation; the rate divided by is the f32 vector issue rate, 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz = 78.6e12
lane-operations per second (half the 157.3 TFLOPS peak, which counts an fma as two).

    python tools/bench_overlap.py [--frames 280] [--size 256]
"""
from __future__ import annotations

import argparse
import os
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
OPS_PER_RAY_PAIR = 330
LANE_OPS_PER_SECOND = 256 * 4 * 32 * 2.4e9


def scene(V: int, dev) -> tuple[torch.Tensor, torch.Tensor]:
    """A seeded walk that turns by 0.01 rad and moves by (0.03, 0, 0.02) per frame."""
    g = torch.Generator().manual_seed(0)
    yaw = 0.01 * torch.arange(V) + 0.002 * torch.randn(V, generator=g)
    E = torch.eye(4).repeat(V, 1, 1)
    E[:, 0, 0], E[:, 0, 2], E[:, 2, 0], E[:, 2, 2] = yaw.cos(), yaw.sin(), -yaw.sin(), yaw.cos()
    E[:, :3, 3] = torch.tensor([0.03, 0.0, 0.02]) * torch.arange(V)[:, None] + 0.002 * torch.randn(V, 3, generator=g)
    K = torch.tensor([[0.9, 0.0, 0.5], [0.0, 1.2, 0.5], [0.0, 0.0, 1.0]]).repeat(V, 1, 1)
    return E.to(dev), K.to(dev)


def timed(fn, reps: int) -> float:
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=280)
    ap.add_argument("--size", type=int, default=256)
    a = ap.parse_args()
    from vicasplat_amd.evaluation import EvaluationIndexGenerator, EvaluationIndexGeneratorCfg, band_pairs
    from vicasplat_amd.geometry.epipolar_lines import view_overlap_counts
    assert torch.cuda.is_available(), "bench_overlap.py needs a GPU"
    dev = torch.device("cuda:0")
    E, K = scene(a.frames, dev)
    shape = (a.size, a.size)
    pairs = band_pairs(a.frames, 5, 135).to(dev)
    P, N = pairs.shape[0], a.size * a.size
    t_hip = timed(lambda: view_overlap_counts(E, K, shape, pairs), 5)
    t_torch = timed(lambda: view_overlap_counts(E, K, shape, pairs, backend="torch"), 1)      # the whole band, sliced by the backend itself
    same = int((view_overlap_counts(E, K, shape, pairs) - view_overlap_counts(E, K, shape, pairs, backend="torch")).abs().max())
    floor = P * N * OPS_PER_RAY_PAIR / LANE_OPS_PER_SECOND
    print(f"{P} pairs x {N} rays: hip {t_hip * 1e3:.2f} ms, torch backend {t_torch * 1e3:.1f} ms, largest count difference {same} rays")
    print(f"arithmetic floor {floor * 1e3:.2f} ms ({OPS_PER_RAY_PAIR} f32 lane-operations per ray-pair at {LANE_OPS_PER_SECOND:.3g} /s): "
          f"the kernel runs at {floor / t_hip:.2f} of it")
    cfg = EvaluationIndexGeneratorCfg(num_target_views=2, min_distance=5, max_distance=135, min_overlap=0.7, max_overlap=1.0,
                                      output_path=Path("."), save_previews=False, seed=123)
    batch = dict(target=dict(image=torch.zeros(1, a.frames, 3, a.size, a.size, device=dev), extrinsics=E[None], intrinsics=K[None]), scene=["bench"])
    gen, gen_torch = EvaluationIndexGenerator(cfg), EvaluationIndexGenerator(cfg, backend="torch")
    t_step = timed(lambda: gen.test_step(batch, 0), 3)
    t_step_torch = timed(lambda: gen_torch.test_step(batch, 0), 1)
    print(f"test_step: hip {t_step * 1e3:.2f} ms -> {gen.index['bench']}; torch backend {t_step_torch * 1e3:.1f} ms")
    return 0 if t_hip <= t_torch else 1


if __name__ == "__main__":
    sys.exit(main())
