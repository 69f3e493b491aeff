"""The teacher's tail kernel (csrc/teacher.hip behind ops.points_conf) against the float64 restatement of tests/teacher_f64.py.  -m gpu.

Shapes (n, H, W) = (1, 1, 1), (3, 3, 5), (2, 16, 65): one pixel, 45 pixels (less than a wave), 2080 pixels (eight full blocks of 256 and a
ragged ninth of 32); f32 and f16 input; without a transform, with one (n different ones; n = 3 in the second shape).  Inputs come from
teacher_f64.tail_edge_input: seeded normal values with the edge values planted at the front of every image -- the zero vector, d = 1e-6 and
1e-3, d = 88 and 89 on either side of the f32 expm1's overflow at 88.72, c in {-inf, -100, 0, 88, 89}.

Criterion per element, no floor: |gpu - f64| <= 4 max(r32, 1) 2^-24 mag, where r32 is the ratio of the torch-f32 composition the kernel
replaces on the same inputs (tests/test_teacher_cpu.py measures the same number) and mag the sum of the absolute terms the output is formed
from (|p|, or |R||p| + |t|; 1 + exp(c)).  Infinities are compared by equality; a NaN is a failure.  The outputs are allocated inside a guard
band of canaries that must come back untouched.

Measured on an MI355X, max |gpu - f64| / (2^-24 mag) (`-s` prints it per case): 0 on the single pixel, 0.87 to 0.93 on 3 x 3 x 5, 0.97 to 0.99
on 2 x 16 x 65, f32 and f16 alike, with and without the transform -- the kernel computes in f64 and rounds once, so it stays below one
unit; the torch-f32 composition has r32 = 43.97 to 44.37 on the same inputs (the d = 88 edge), which puts the bound at 176 to 178 units.
"""
import pytest
import torch

import teacher_f64 as T

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 3, 5), (2, 16, 65)]
GUARD = 64          # floats on either side of an output
CANARY = -7.25


def _guarded(numel):
    buf = torch.full((numel + 2 * GUARD,), CANARY, dtype=torch.float32, device="cuda")
    return buf, buf[GUARD:GUARD + numel]


@pytest.mark.parametrize("with_transform", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("n,H,W", SHAPES)
def test_points_conf_matches_float64(n, H, W, dtype, with_transform):
    from vicasplat_amd import ops
    raw = T.tail_edge_input(n, H, W, dtype, seed=n * 100 + W)
    tr = T.tail_transforms(n, seed=W) if with_transform else None
    ref = T.tail(raw.double(), None if tr is None else tr.double(), f32_overflow=True)
    r32 = T.tail_ratio(*T.tail_torch_f32(raw, tr), ref)
    bp, pts = _guarded(n * H * W * 3)
    bc, conf = _guarded(n * H * W)
    got_p, got_c = ops.points_conf(raw.cuda(), None if tr is None else tr.cuda(), out_pts=pts.view(n, H, W, 3), out_conf=conf.view(n, H, W))
    torch.cuda.synchronize()
    for buf in (bp, bc):
        assert bool((buf[:GUARD] == CANARY).all()) and bool((buf[-GUARD:] == CANARY).all()), "a guard band was written"
    got_p, got_c = got_p.cpu(), got_c.cpu()
    worst = 0.0
    for name, got, want, mag in (("pts", got_p, ref["pts"], ref["mag_pts"]), ("conf", got_c, ref["conf"], ref["mag_conf"])):
        assert not torch.isnan(got).any(), (name, "NaN from finite inputs")
        w32 = want.float()                        # the float64 value as f32 stores it: +-inf from the f32 maximum on
        inf = torch.isinf(w32)
        assert torch.equal(got[inf], w32[inf]), (name, "infinities")
        assert bool(torch.isfinite(got[~inf]).all()), name
        err = (got.double() - want).abs()[~inf]
        lim = 4 * max(r32, 1.0) * 2.0 ** -24 * mag[~inf]
        assert bool((err <= lim).all()), (name, float((err / (2.0 ** -24 * mag[~inf]).clamp_min(1e-300)).max()), r32)
        if (~inf).any():
            pos = mag[~inf] > 0
            if pos.any():
                worst = max(worst, float((err[pos] / (2.0 ** -24 * mag[~inf][pos])).max()))
            assert bool((err[~pos] == 0).all()), (name, "a zero magnitude must give the exact value")
    print(f"points_conf n={n} {H}x{W} {str(dtype)[6:]} transform={with_transform}: gpu {worst:.3f} units of 2^-24 mag, torch f32 {r32:.3f}, "
          f"bound {4 * max(r32, 1.0):.2f}")
    # the planted values, by name: the zero vector is exactly zero without a transform (the translation with one); c = -inf gives 1
    if tr is None:
        assert bool((got_p[:, 0, 0] == 0).all())
    else:
        assert torch.equal(got_p[:, 0, 0], tr[:, :, 3])


def test_points_conf_refuses_what_it_cannot_run():
    from vicasplat_amd import ops
    raw = torch.zeros(1, 2, 2, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.points_conf(raw)
    with pytest.raises(ValueError, match="contiguous f32 or f16"):
        ops.points_conf(torch.zeros(1, 2, 2, 8, device="cuda")[..., :4])
    with pytest.raises(ValueError, match="contiguous f32 or f16"):
        ops.points_conf(raw.cuda().bfloat16())
    with pytest.raises(ValueError, match="transform"):
        ops.points_conf(raw.cuda(), torch.zeros(2, 3, 4, device="cuda"))
