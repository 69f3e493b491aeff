"""Every forward convolution route of csrc/conv.hip (bodies in gemm256.h) against the float64 reference of tests/conv_f64.py evaluated on the
same stored values, at the smallest shapes that reach each route and each store path of conv_epilogue.  Goes through vicasplat_amd.ops only
(conv3x3_nhwc, conv3x3_head1x1_nhwc, upsample2x_nhwc, split_pack_weight).  -m gpu.

Operand classes: f16, bf16, f32x (the exact-f32 kernels, dtype 3), split.  The route of a 3x3 convolution case is the first part of its id,
written by hand in conv_f64.CASES and held to csrc/routes.h by tests/test_conv_ref_cpu.py (there may be no compiler where this file runs):
    halo256 / tile256   conv3x3_256_halo_split_kernel / conv3x3_256_kernel      tile256x128   conv3x3_256x128_split_kernel
    wave4mi2 / 4 / 8    conv3x3_kernel<., MI>                                   head1x1 / head_dot   the fused heads, conv_f64.head_route
Inputs come from conv_f64.build: two distinct images alternating through the batch (maps of 15 x 17 = 255 pixels put an image seam into every
256-pixel tile and leave the last tile ragged), NaN bit patterns for two image rows before the first and after the last image, the output
inside a larger allocation pre-filled with a NaN payload that must survive bit for bit, `out` / `residual` offset by one element or by 8
bytes where a case says so.

Per case and family: every live element is finite (nothing was read from outside the images, every element was written), everything
outside the output tensor still holds the sentinel, and
    lattice   the result equals the float64 result rounded once to the output type, BIT FOR BIT, and a second call returns the same bits;
    real      max |error| / max |reference| within conv_f64.bound: the constants of the existing tests (3x3: f16 3e-3, bf16 2e-2, f32x 4e-6,
              split 6e-6; fused heads: 4 x 2e-3, 4 x 1.6e-2, split 6e-6; upsampling: 2e-3, 1.6e-2, 4e-6).
Split class: a packed-input run is bit-identical to the f32-input run on tile256, tile256x128 and both fused heads; the packed output of the
upsampling is the packing of its plain f32 result.  Two host-side refusals (VS_CHECK returns before any launch) raise and leave the output
buffer untouched.

Every case prints `FIG <id> <family> <cls> rel=... bound=...`; a failure names the worst element's image, y, x and channel, its 256-, 128- and
64-pixel tile and the route.

Measured on MI355X, largest max |error| / max |reference| of the real family per class and entry, over all epilogues (FIG lines):
              conv3x3    head1x1    head_dot   upsample2x
    f16       4.6e-4     4.4e-4     4.5e-4     4.1e-4
    bf16      3.3e-3     3.5e-3     3.6e-3     3.6e-3
    f32x      9.5e-7     --         --         1.3e-6
    split     1.0e-6     4.3e-7     4.2e-7     --
Lattice cases: 0 everywhere -- every route, class, epilogue, store path and pointer offset returned the float64 result rounded once, and the
same bits on the second call; the packed-input runs and the packed upsampling output matched their f32 counterparts bit for bit.  Every
quantity has a bound in an existing test, so none is derived from these figures.  The file has 213 tests (205 table cases: 97 convolutions,
56 fused heads, 52 upsamplings; 361 case x family runs) and takes 7 s; the slowest test 0.5 s.

FOUND AND FIXED: nothing -- no case failed on the kernels as they are.  That the table is not blind was checked on scratch builds with one
deliberate break each (none committed); the red cases were those of the broken arm and no others:
    mask keeps the value where mask_by == 0, f32 vector path (conv.hip:139)   the 28 f32x / split cases whose `paths` hold f32x4, `mask` only
    W for Win in the 4-wave kernel's row math (conv.hip:777)                  the 8 stride-2 4-wave cases, all four classes
    no output ReLU on the 8-byte path (conv.hip:201)                          the 18 f16 / bf16 cases whose `paths` hold u2 and that run relu_out
    taps above an image's first row not masked, tile kernels (conv.hip:502, 657)   every tile256 / tile256x128 case and the MFMA-form heads
    hidden value of the dot-form head not rounded to 16 bit (conv.hip:708)    the 16 f16 / bf16 head_dot cases, lattice family
    second row pair of the 16-bit upsampling from the wrong source rows (conv.hip:971)   the 26 f16 / bf16 cases with H >= 2
"""
import math

import pytest
import torch

import conv_f64 as C
from conv_f64 import CASES, bound, build, conv_f64, to_device, view_of

pytestmark = pytest.mark.gpu

CONV = [c for c in CASES if c.entry == "conv3x3"]
HEADS = [c for c in CASES if c.entry in ("head1x1", "head_dot")]
UPS = [c for c in CASES if c.entry == "upsample2x"]


def _dev():
    return torch.device("cuda:0")


def _where(c, got, want):
    """The worst element of got against want ([N, Ho, Wo, channels], any dtype): image, y, x, channel, its pixel tiles, the route."""
    e = torch.nan_to_num((got.double() - want.double()).abs(), nan=float("inf"))
    i = int(e.argmax())
    n, Ho, Wo, Cc = got.shape
    img, rem = divmod(i, Ho * Wo * Cc)
    y, rem = divmod(rem, Wo * Cc)
    x, ch = divmod(rem, Cc)
    m = (img * Ho + y) * Wo + x
    return (f"worst at image {img} (distinct {img % C.D}) y {y} x {x} channel {ch}: got {float(got.reshape(-1)[i]):.9g} want {float(want.reshape(-1)[i]):.9g}; "
            f"pixel m = {m} of {n * Ho * Wo}: tile256 {m // 256} tile128 {m // 128} tile64 {m // 64}, column tile64 {ch // 64}; route {c.route}")


def _compare(c, family, got, ref, what):
    """got [N, ...] on the GPU against the float64 reference of the distinct images.  -> max |err| / max |ref| (lattice: after the bit check)."""
    d = got.device
    assert bool(torch.isfinite(got).all()), f"NaN / inf in a live element ({what}): " + _where(c, got, torch.zeros_like(got))
    refd = ref.to(d)[c.idx]
    refmax = float(ref.abs().max())
    err = float((got.double() - refd).abs().max()) / max(refmax, 1e-300)
    if family == "lattice":
        want = ref.float().to(got.dtype).to(d)[c.idx]          # exact in f32 (conv_f64.lattice_units), rounded once to the output type
        assert torch.equal(got.view(C.INT_OF[got.dtype]), want.view(C.INT_OF[got.dtype])), f"lattice result is not the float64 result rounded once ({what}): " + _where(c, got, want)
        err = float((got.double() - want.double()).abs().max()) / max(refmax, 1e-300)          # the figure: distance to the rounded reference, 0
    else:
        assert err <= bound(c.cls, c.entry), f"rel {err:.3e} > bound {bound(c.cls, c.entry):.1e} ({what}): " + _where(c, got, refd)
    return err


def _x_of(c, ops, packed):
    """The input view inside its NaN-guarded buffer; packed: the packed (hi, lo) image of the WHOLE buffer (rows of Cin: the guards stay NaN),
    as test_gemm_routes_gpu._launch packs a whole A buffer."""
    shape = (c.N, c.H, c.W, c.Cin)
    if not packed:
        return view_of(c.xbuf, c.x_at, shape, c.dt)
    rows = c.xbuf.view(torch.float32).view(-1, c.Cin)
    img = ops.split_pack_weight(rows, 0).data[c.x_at // c.Cin:c.x_at // c.Cin + c.N * c.H * c.W].view(shape)
    return ops.SplitWeight(img, 1.0, shape)


def _w_of(c, ops):
    return ops.pack_conv3x3_weight(c.w, "split" if c.cls == "split" else c.dt)


def _conv_call(c, ops, x, w, epi):
    """One call into a fresh copy of the sentinel-filled output allocation.  -> (the whole allocation, the output view)."""
    buf = c.out0.clone()
    out = view_of(buf, c.out_at, c.out_shape, c.dt)
    r1 = view_of(c.rbuf, c.r_at, c.out_shape, c.dt)
    kw = {}
    if "res" in epi:
        kw["residual"] = r1
    if epi == "mask":
        kw["mask_by"] = r1
    if "res2" in epi:
        kw["residual2"] = c.r2_batch
    y = ops.conv3x3_nhwc(x, w, c.bias if "bias" in epi else None, relu_in=epi == "relu_in", relu_out=epi == "relu_out", out=out, stride=c.stride, **kw)
    assert y.data_ptr() == out.data_ptr()
    return buf, out


def _outside_untouched(c, buf):
    end = c.out_at + math.prod(c.out_shape)
    return bool((buf[:c.out_at] == c.sentinel).all()) and bool((buf[end:] == c.sentinel).all())


def _run_conv(case, family, ops):
    cpu = build(case, family)
    c = to_device(cpu, _dev())
    c.r2_batch = c.r2[c.idx].contiguous()
    x, w = _x_of(c, ops, case.packed), _w_of(c, ops)
    worst = 0.0
    for epi in case.epis:
        buf, got = _conv_call(c, ops, x, w, epi)
        assert _outside_untouched(c, buf), f"wrote outside the output tensor ({epi}); route {case.route}"
        worst = max(worst, _compare(c, family, got, conv_f64(cpu, epi), epi))          # the float64 convolution is cached in `cpu`: one per relu_in
        if family == "lattice":
            buf2, _ = _conv_call(c, ops, x, w, epi)
            assert torch.equal(buf2, buf), f"a second call returned other bits ({epi}); route {case.route}"
    print(f"FIG {case.id} {family} {case.cls} rel={worst:.3e} bound={bound(case.cls, case.entry):.1e}")
    return c, x, w


@pytest.mark.parametrize("case", CONV, ids=[c.id for c in CONV])
def test_conv3x3_route_matches_float64(case):
    from vicasplat_amd import ops
    for family in case.families:
        _run_conv(case, family, ops)


# ---- fused heads ---------------------------------------------------------------------------------------------------------------------
def _head_weights(c, ops):
    w = _w_of(c, ops)
    w2 = ops.split_pack_weight(c.w2) if (c.cls == "split" and c.entry == "head1x1") else c.w2.contiguous()
    return w, w2


def _run_head(case, family, ops):
    cpu = build(case, family)
    c = to_device(cpu, _dev())
    x = _x_of(c, ops, case.packed)
    w, w2 = _head_weights(c, ops)
    worst, outs = 0.0, {}
    for relu_out in (False, True):
        for with_bias in (False, True):
            got = ops.conv3x3_head1x1_nhwc(x, w, c.bias if with_bias else None, w2, c.bias2, case.n_out, relu_out=relu_out)
            assert tuple(got.shape) == (case.N, case.H, case.W, case.c2pad)
            what = f"relu_out={relu_out} bias={with_bias}"
            worst = max(worst, _compare(c, family, got, conv_f64(cpu, (relu_out, with_bias)), what))
            assert case.n_out == case.c2pad or float(got[..., case.n_out:].abs().max()) == 0.0, f"columns >= n_out are not 0 ({what}); route {case.route}"
            if family == "lattice":
                again = ops.conv3x3_head1x1_nhwc(x, w, c.bias if with_bias else None, w2, c.bias2, case.n_out, relu_out=relu_out)
                assert torch.equal(again.view(C.INT_OF[got.dtype]), got.view(C.INT_OF[got.dtype])), f"a second call returned other bits ({what}); route {case.route}"
            outs[relu_out, with_bias] = got
    print(f"FIG {case.id} {family} {case.cls} rel={worst:.3e} bound={bound(case.cls, case.entry):.1e}")
    return c, w, w2, outs


@pytest.mark.parametrize("case", HEADS, ids=[c.id for c in HEADS])
def test_fused_head_matches_float64(case):
    from vicasplat_amd import ops
    for family in case.families:
        c, w, w2, outs = _run_head(case, family, ops)
        if case.packed:       # the packed-input kernel against the f32-input kernel on the same values
            x32 = _x_of(c, ops, False)
            for (relu_out, with_bias), got in outs.items():
                plain = ops.conv3x3_head1x1_nhwc(x32, w, c.bias if with_bias else None, w2, c.bias2, case.n_out, relu_out=relu_out)
                assert torch.equal(plain.view(torch.int32), got.view(torch.int32)), f"packed-input run differs from the f32-input run; route {case.route}"


# ---- upsampling ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", UPS, ids=[c.id for c in UPS])
def test_upsample2x_matches_float64(case):
    from vicasplat_amd import ops
    for family in case.families:
        cpu = build(case, family)
        c = to_device(cpu, _dev())
        x = _x_of(c, ops, False)
        add = c.add[c.idx].contiguous()
        worst = 0.0
        for mode in C.UP_MODES:
            got = ops.upsample2x_nhwc(x, None if mode == "none" else add, relu_add=mode == "relu_add")
            worst = max(worst, _compare(c, family, got, conv_f64(cpu, mode), mode))
            if family == "lattice":
                again = ops.upsample2x_nhwc(x, None if mode == "none" else add, relu_add=mode == "relu_add")
                assert torch.equal(again.view(C.INT_OF[got.dtype]), got.view(C.INT_OF[got.dtype]))
        print(f"FIG {case.id} {family} {case.cls} rel={worst:.3e} bound={bound(case.cls, case.entry):.1e}")


@pytest.mark.parametrize("N,H,W,Cc", C.UPSAMPLE_PACKED)
def test_packed_upsample_is_the_packing_of_the_plain_result(N, H, W, Cc):
    from vicasplat_amd import ops
    g = torch.Generator().manual_seed(N * 1000 + H * 100 + W)
    x = torch.randn(N, H, W, Cc, generator=g).to(_dev())
    add = torch.randn(N, 2 * H, 2 * W, Cc, generator=g).to(_dev())
    for a, relu_add in ((None, False), (add, False), (add, True)):
        plain = ops.upsample2x_nhwc(x, a, relu_add)
        packed = ops.upsample2x_nhwc(x, a, relu_add, packed=True)
        want = ops.split_pack_weight(plain.view(-1, Cc), 0).data.view(N, 2 * H, 2 * W, Cc)
        assert tuple(packed.shape) == tuple(plain.shape) and torch.equal(packed.data, want), (a is not None, relu_add)


# ---- split class: packed input == f32 input ------------------------------------------------------------------------------------------
PACKED_CONV = [c for c in CONV if c.packed]


@pytest.mark.parametrize("case", PACKED_CONV, ids=[c.id for c in PACKED_CONV])
def test_packed_input_is_bit_identical_to_f32_input(case):
    from vicasplat_amd import ops
    c = to_device(build(case, "real"), _dev())
    c.r2_batch = None
    xp, x32, w = _x_of(c, ops, True), _x_of(c, ops, False), _w_of(c, ops)
    for epi in case.epis:
        bufp, _ = _conv_call(c, ops, xp, w, epi)
        buf32, _ = _conv_call(c, ops, x32, w, epi)
        assert torch.equal(bufp, buf32), f"packed-input run differs from the f32-input run ({epi}); route {case.route}"


# ---- host-side refusals: VS_CHECK returns before any launch --------------------------------------------------------------------------
def test_a_packed_input_is_refused_where_the_route_is_the_4_wave_kernel():
    from vicasplat_amd import ops
    N, H, W, Cin, Cout = C.REFUSED_PACKED
    d = _dev()
    x = torch.randn(N, H, W, Cin, device=d)
    xp = ops.SplitWeight(ops.split_pack_weight(x.view(-1, Cin), 0).data.view(N, H, W, Cin), 1.0, x.shape)
    w = ops.pack_conv3x3_weight(torch.randn(Cout, Cin, 3, 3, device=d), "split")
    out = torch.full((N, H, W, Cout), C.SENTINEL[torch.float32], dtype=torch.int32, device=d)
    with pytest.raises(RuntimeError, match="packed input"):
        ops.conv3x3_nhwc(xp, w, None, out=out.view(torch.float32))
    assert bool((out == C.SENTINEL[torch.float32]).all())
    assert torch.isfinite(ops.conv3x3_nhwc(x, w, None)).all()          # the f32 input of the same shape is taken


@pytest.mark.parametrize("cls", ["f16", "split"])
def test_a_fused_head_refuses_a_pixel_count_that_is_no_multiple_of_256(cls):
    from vicasplat_amd import ops
    N, H, W = C.REFUSED_HEAD
    d, dt = _dev(), C.STORAGE[cls]
    Cin = 64
    x = torch.randn(N, H, W, Cin, device=d).to(dt)
    wf, w2f = torch.randn(256, Cin, 3, 3, device=d) / 24, torch.randn(16, 256, device=d) / 16
    b2 = torch.zeros(16, device=d)
    if cls == "split":
        w, w2 = ops.pack_conv3x3_weight(wf, "split"), ops.split_pack_weight(w2f)
    else:
        w, w2 = ops.pack_conv3x3_weight(wf, dt), w2f.to(dt)
    with pytest.raises(RuntimeError, match="multiple of 256"):
        ops.conv3x3_head1x1_nhwc(x, w, None, w2, b2, 3)
