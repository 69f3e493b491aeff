"""The halo-tile body of the split-class 256-wide 3x3 convolution (csrc/conv.hip, conv3x3_256_halo_split_kernel; gemm256.h,
mainloop256_halo_split): a workgroup owns a 16 x 16 block of output pixels of one image and stages + converts the 18 x 18 input patch once
per 32-channel block.  Checked against a float64 convolution computed on the CPU from the same stored values:

  * lattice inputs (small integers scaled by powers of two: every product and every partial sum is exact in f32, bias and residuals
    included): the output equals the float64 result rounded once, bit for bit, and a second call returns the same bits;
  * real-valued inputs: within the split class's per-operator bound (test_split_path_gpu.TOL).

The dispatcher of vs_conv3x3_split_nhwc is unchanged: the 256-wide route takes a convolution from 150 tiles of 256 pixels on and needs an
even number of K-tiles.  So every case below is its per-image shape (the patch, seam and border geometry the case is about) in a batch just
large enough for 150 tiles, two DISTINCT images alternating through the batch -- a halo row that leaked from the neighbouring image would
come from other values -- and the float64 reference is computed once, for the two distinct images only.  Two cases are fall-throughs to the
kernels from before (asserted exact all the same): Cin = 32 (nine K-tiles: odd) and 24 x 40 maps (H, W not multiples of 16: the halo loop
handles no partial patches).  The entry takes dense NHWC tensors (no batch stride), so the NaN guard is before the first and after the last
image; the output lives inside a larger buffer whose sentinel must survive bit for bit."""
import math

import pytest
import torch
import torch.nn.functional as F

from test_split_path_gpu import TOL      # the split class's per-operator bound: max |err| <= 6e-6 of the output scale

pytestmark = pytest.mark.gpu

# (case, images in the batch, H, W, Cin, on the halo loop)
CASES = [
    ("one_patch_16x16", 150, 16, 16, 256, True),       # one patch per image, every border row zero
    ("seam_y_32x16", 76, 32, 16, 256, True),           # a seam between patches in y
    ("seam_x_16x32", 76, 16, 32, 256, True),           # ... and in x
    ("batch_boundary_32x32", 38, 32, 32, 256, True),   # four patches per image, image boundaries inside the batch
    ("two_channel_blocks_cin64", 150, 16, 16, 64, True),   # both patch buffers, the shortest loop with a staged second patch
    ("one_channel_block_cin32", 150, 16, 16, 32, False),   # nine K-tiles: the 256-wide route does not take it
    ("ragged_24x40", 40, 24, 40, 256, False),          # H, W % 16 != 0: today's kernel
]
EPILOGUES = ("none", "bias", "bias+res", "bias+res+res2")
D = 2            # distinct images
SENTINEL = 0x7F8A5A5A      # a NaN payload no kernel produces


def _dev():
    return torch.device("cuda:0")


def _lattice(shape, g, lo, hi, scale):
    return torch.randint(lo, hi + 1, shape, generator=g).float() * scale


def _inputs(kind, H, W, Cin, seed):
    """The distinct images, weights, bias and residuals of one case on the CPU (f32 values; float64 is exact on them)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "lattice":
        # |sum| <= 2304 * 64 units of 2^-9 < 2^24 units; bias / residuals are multiples of 2^-4: every intermediate is exact in f32
        x = _lattice((D, H, W, Cin), g, -8, 8, 2.0 ** -3)
        w = _lattice((256, Cin, 3, 3), g, -8, 8, 2.0 ** -6)
        b = _lattice((256,), g, -64, 64, 2.0 ** -4)
        r1 = _lattice((D, H, W, 256), g, -64, 64, 2.0 ** -4)
        r2 = _lattice((D, H, W, 256), g, -64, 64, 2.0 ** -4)
    else:
        x = torch.randn(D, H, W, Cin, generator=g)
        w = torch.randn(256, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
        b = torch.randn(256, generator=g)
        r1 = torch.randn(D, H, W, 256, generator=g)
        r2 = torch.randn(D, H, W, 256, generator=g)
    return x, w, b, r1, r2


def _guarded(shape, guard, fill_bits, src=None):
    """An f32 tensor of `shape` on the GPU inside a larger buffer: [guard | tensor | guard] floats, the guards filled with the bit pattern."""
    n = math.prod(shape)
    buf = torch.full((guard + n + guard,), fill_bits, dtype=torch.int32, device=_dev())
    view = buf[guard:guard + n].view(torch.float32).view(shape)
    if src is not None:
        view.copy_(src)
    return buf, view


def _run_case(kind, N, H, W, Cin):
    from vicasplat_amd import ops
    d = _dev()
    x, w, b, r1, r2 = _inputs(kind, H, W, Cin, seed=H * 1000 + W * 10 + Cin)
    reps = N // D
    assert reps * D == N
    tile = lambda t: t.to(d).repeat(reps, 1, 1, 1)   # A B A B ...: neighbours in the batch differ
    guard = 2 * W * max(Cin, 256)                      # two image rows (a multiple of 4 floats: the views stay 16-byte aligned)
    NAN_BITS = 0x7FC00000
    _, xg = _guarded((N, H, W, Cin), guard, NAN_BITS, tile(x))        # NaN before the first and after the last image
    wp = ops.pack_conv3x3_weight(w.to(d), "split")
    bg, r1g, r2g = b.to(d), tile(r1), tile(r2)
    xn, wd = x.permute(0, 3, 1, 2).double(), w.double()
    conv = {ri: F.conv2d(F.relu(xn) if ri else xn, wd, None, padding=1).permute(0, 2, 3, 1) for ri in (False, True)}    # float64, CPU
    worst = 0.0
    for relu_in in (False, True):
        for relu_out in (False, True):
            for epi in EPILOGUES:
                ref = conv[relu_in]
                if "bias" in epi:
                    ref = ref + b.double()
                if "res" in epi:
                    ref = ref + r1.double()
                if "res2" in epi:
                    ref = ref + r2.double()
                if relu_out:
                    ref = F.relu(ref)
                obuf, out = _guarded((N, H, W, 256), guard, SENTINEL)
                kw = dict(residual=r1g if "res" in epi else None, residual2=r2g if "res2" in epi else None, relu_in=relu_in, relu_out=relu_out)
                y = ops.conv3x3_nhwc(xg, wp, bg if "bias" in epi else None, out=out, **kw)
                assert y.data_ptr() == out.data_ptr()
                what = (kind, N, H, W, Cin, relu_in, relu_out, epi)
                assert bool((obuf[:guard] == SENTINEL).all()) and bool((obuf[-guard:] == SENTINEL).all()), ("stray write", what)
                assert bool(torch.isfinite(y).all()), ("NaN read from outside the images", what)
                if kind == "lattice":
                    want = tile(ref.float())                    # the float64 result rounded once
                    assert torch.equal(y.view(torch.int32), want.view(torch.int32)), ("not exact", what, float((y - want).abs().max()))
                    y2 = ops.conv3x3_nhwc(xg, wp, bg if "bias" in epi else None, **kw)
                    assert torch.equal(y2.view(torch.int32), y.view(torch.int32)), ("second call differs", what)
                else:
                    e = float((y.double() - tile(ref)).abs().max() / ref.abs().max())
                    worst = max(worst, e)
                    assert e <= TOL, (what, e)
    if kind == "real":
        print(f"conv halo {N}x{H}x{W} Cin={Cin}: worst rel err vs float64 {worst:.2e} (bound {TOL:.0e})")


@pytest.mark.parametrize("case,N,H,W,Cin,halo", CASES, ids=[c[0] for c in CASES])
def test_lattice_inputs_are_exact_and_repeatable(case, N, H, W, Cin, halo):
    assert halo == (N * H * W >= 150 * 256 and H % 16 == 0 and W % 16 == 0 and (9 * Cin // 32) % 2 == 0), "the case table misstates its route"
    _run_case("lattice", N, H, W, Cin)


@pytest.mark.parametrize("case,N,H,W,Cin,halo", CASES, ids=[c[0] for c in CASES])
def test_real_inputs_within_the_split_bound(case, N, H, W, Cin, halo):
    _run_case("real", N, H, W, Cin)
