"""The fused Gaussian adapter (csrc/adapter.hip), forward and backward, against the float64 reference of tests/pointwise_f64.py on the
edge table, on every kernel route.  -m gpu.

Criterion, per element and per output, with the reference evaluated on the inputs as the kernel reads them (16-bit inputs are rounded
first, so they are exact in f32):  |gpu - ref| <= B 2^-24 mag,  B = 4 max(r32, 1) = 4 for every output (r32 <= 1, see
tests/test_pointwise_ref_cpu.py).  16-bit gradients additionally get half an ulp of their type (2^-11 |ref| f16, 2^-8 |ref| bf16) and
2^-25 for f16 subnormals; likewise one f32 subnormal step (2^-149) and half a bf16 one: the gradient through a scale of 1e-16 (softplus
at -30) is ~1e-44, where the kernel returns the nearest subnormal.  An f16 gradient beyond 65504 is that infinity.  An element of
magnitude 0 (a copy, a derivative past the clamp, the zero quaternion) must be exact.  No input is ambiguous (pointwise_f64: within 1e-3
of the 0.3 clamp or the softplus threshold, within a factor 2 of the 1e-8 / 1e-12 clamps); this is asserted on the inputs, nothing is
excluded.  No bound was widened.

Found by this file: below the 1e-8 clamp (0 < |xyz| < 1e-8) the forward is m = x expm1(d) / 1e-8, whose derivative keeps the expm1'(d)
term, (g . x) e^d / (d 1e-8) x; adapter_backward_kernel dropped it (d_pts off by 0.1 (g . xhat) xhat at |xyz| = 1e-9).  Fixed in the kernel.

For opacity_exponent != 1 the raw opacities stay within +-15: beyond, (1 - p)^(e - 1) or p^(1/e - 1) times p (1 - p) is inf * 0 in f32,
in torch as in the kernel, while the float64 derivative is finite.

Measured on an MI355X, max |gpu - ref| / (2^-24 mag) over all cases of this file (`-s` prints them per case), beside r32:

    output        r32    gpu
    means         0.33   0.32
    covariances   0.33   0.33
    harmonics     0.95   1.00
    opacities     0.64   0.43
    scales        1.00   1.00
    rotations     0.29   0.36
    raw           0.33   0.32
    d_pts         0.33   0.40   (f32; 16-bit: 0.98 of the allowance)
    d_gs          0.98   0.98   (f32; 16-bit: 0.99 of the allowance)
"""
import numpy as np
import pytest
import torch

import pointwise_f64 as pw

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
ACTS = {"softplus": (0.0, 0.0), "exp": (0.0, 0.0), "bounded": (0.5, 15.0)}
FWD = ("means", "covariances", "harmonics", "opacities", "scales", "rotations", "raw")
K_MAX_CH, K_MAX_PIX = 96, 96     # kMaxCh, kMaxPixStride of csrc/adapter.hip


def _dev():
    return torch.device("cuda:0")


def _mask(d_sh):
    return np.linspace(1.0, 0.1, d_sh).astype(np.float32).astype(np.float64)


def _t(a, storage="f32"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DT[storage]).to(_dev())


def _route(pts, gs, d_sh):
    """vs_gaussian_adapter's dispatch, restated from the views the wrapper passes ([N, C, H, W]: pixel stride = stride(3), channel stride
    = stride(1))."""
    ev = 4 if gs.dtype == torch.float32 else 8
    pp, pc, gp, gc = pts.stride(3), pts.stride(1), gs.stride(3), gs.stride(1)
    dense = (pc == 1 and 3 <= pp <= 8 and gc == 1 and 8 + 3 * d_sh <= gp <= K_MAX_PIX and 11 + 3 * d_sh <= K_MAX_CH
             and pts.data_ptr() % 16 == 0 and gs.data_ptr() % 16 == 0 and (64 * pp) % ev == 0 and (64 * gp) % ev == 0)
    return "dense" if dense else "generic"


def _layout(a, storage, layout, pix):
    """[P, C] float64 -> the [1, C, 1, P] view of a buffer in the given layout: 'dense' = channels-last rows of `pix` elements (padding
    NaN: read with the block, never used), 'planar' = NCHW-contiguous (channel stride P, pixel stride 1)."""
    P, C = a.shape
    if layout == "planar":
        return _t(a.T, storage).reshape(C, 1, 1, P).permute(1, 0, 2, 3)
    buf = torch.full((1, 1, P, pix), float("nan"), dtype=DT[storage], device=_dev())
    buf[0, 0, :, :C] = _t(a, storage)
    return buf.permute(0, 3, 1, 2)[:, :C]


def _check(got, ref, names, storage_out="f32", tag=""):
    u = {k: pw.units(got[k], ref, k) for k in names}
    r = {k: pw.ratio(got[k], ref, k, pw.gpu_factor(pw.R32_ADAPTER[k]), storage_out) for k in names}
    print(tag, "units", {k: round(v, 2) for k, v in u.items()}, "of the allowance", {k: round(v, 3) for k, v in r.items()})
    if max(r.values()) > 1.0:      # name the worst element
        k = max(r, key=r.get)
        g = np.asarray(got[k], np.float64).reshape(ref[k].shape)
        i = np.unravel_index(int(np.argmax(np.abs(g - ref[k]) / (pw.bound(ref, k, 1.0, storage_out) + 1e-300))), g.shape)
        raise AssertionError((tag, r, u, k, tuple(int(j) for j in i), float(g[i]), float(ref[k][i]), float(ref[k + "_mag"][i])))


# (storage, layout, gs pixel stride | None = channel count, pts pixel stride, d_sh, P | None = the full table, act, exponent, want_raw, route)
FORWARD = [
    # the whole edge table: dense kernel <1>, <2> (16-bit, channels-last, strides = channel counts) and <0, 32> (f32)
    ("f16", "dense", None, 3, 4, None, "softplus", 1.0, True, "dense"), ("f16", "dense", None, 3, 4, None, "exp", 2.0, True, "dense"),
    ("f16", "dense", None, 3, 4, None, "bounded", -1.0, True, "dense"), ("bf16", "dense", None, 3, 4, None, "softplus", 2.0, True, "dense"),
    ("bf16", "dense", None, 3, 4, None, "exp", -1.0, True, "dense"), ("bf16", "dense", None, 3, 4, None, "bounded", 1.0, True, "dense"),
    ("f32", "dense", None, 3, 4, None, "softplus", 1.0, True, "dense"), ("f32", "dense", None, 3, 4, None, "exp", 0.5, True, "dense"),
    ("f32", "dense", None, 3, 4, None, "bounded", 2.0, True, "dense"), ("f32", "dense", None, 3, 4, None, "softplus", -1.0, False, "dense"),
    # padded pixel strides (a channel slice of a wider channels-last tensor): gs_pix 88 > 83, 96 > 92 (d_sh 28 fills kMaxCh), pts_pix 4, 8
    ("f16", "dense", 88, 4, 25, 129, "softplus", 1.0, True, "dense"), ("bf16", "dense", 96, 8, 28, 65, "softplus", 1.0, True, "dense"),
    ("f32", "dense", 88, 8, 25, 33, "exp", 1.0, True, "dense"), ("f32", "dense", 96, 4, 28, 129, "softplus", 1.0, False, "dense"),
    # NCHW-contiguous (gs_ch = H W = P, gs_pix = 1 < 8 + 3 d_sh): the stride-generic kernel, all three dtypes
    ("f16", "planar", None, 3, 9, 129, "softplus", 1.0, True, "generic"), ("bf16", "planar", None, 3, 4, None, "exp", 2.0, True, "generic"),
    ("f32", "planar", None, 3, 4, None, "softplus", 1.0, True, "generic"), ("f32", "planar", None, 3, 25, 300, "bounded", -1.0, False, "generic"),
    # 11 + 3 * 29 = 98 > kMaxCh: dense layout, generic kernel
    ("f16", "dense", None, 3, 29, 65, "softplus", 1.0, True, "generic"), ("f32", "dense", None, 3, 29, 33, "softplus", 1.0, True, "generic"),
    # pixel counts around the 32- and 64-pixel blocks; np * per odd or not a multiple of 4, so that write_rows' scalar tail runs for
    # per = 3, 4 (np odd: 3 np only), 9, 3 d_sh and 11 + 3 d_sh
    ("f16", "dense", None, 3, 1, 1, "softplus", 1.0, True, "dense"), ("f32", "dense", None, 3, 1, 1, "softplus", 1.0, True, "dense"),
    ("f16", "dense", None, 3, 9, 31, "softplus", 1.0, True, "dense"), ("f32", "dense", None, 3, 9, 31, "exp", 1.0, True, "dense"),
    ("bf16", "dense", None, 3, 25, 33, "softplus", 1.0, True, "dense"), ("f32", "dense", None, 3, 25, 33, "softplus", 1.0, True, "dense"),
    ("f16", "dense", None, 3, 28, 64, "softplus", 1.0, True, "dense"), ("f32", "dense", None, 3, 28, 64, "softplus", 1.0, True, "dense"),
    ("f16", "dense", None, 3, 1, 65, "bounded", 1.0, True, "dense"), ("f32", "dense", None, 3, 9, 65, "softplus", 1.0, False, "dense"),
    ("bf16", "dense", None, 3, 9, 129, "exp", 1.0, False, "dense"), ("f32", "dense", None, 3, 1, 129, "softplus", 1.0, True, "dense"),
]


@pytest.mark.parametrize("storage,layout,gs_pix,pts_pix,d_sh,P,act,exponent,want_raw,route", FORWARD)
def test_adapter_forward_matches_float64(storage, layout, gs_pix, pts_pix, d_sh, P, act, exponent, want_raw, route):
    from vicasplat_amd import ops
    smin, smax = ACTS[act]
    pts, gs = pw.adapter_edge_inputs(act, d_sh, storage, exponent, P=P)
    mask = _mask(d_sh)
    ref = pw.adapter_forward(pts, gs, mask, act, smin, smax, exponent)
    assert not ref["ambiguous"].any()
    pv = _layout(pts, storage, layout, pts_pix)
    gv = _layout(gs, storage, layout, gs_pix or gs.shape[1])
    assert _route(pv, gv, d_sh) == route
    o = ops.gaussian_adapter(pv, gv, _t(mask), scale_act=act, scale_min=smin, scale_max=smax, opacity_exponent=exponent, want_raw=want_raw)
    torch.cuda.synchronize()
    assert (o["raw"] is not None) == want_raw
    names = [k for k in FWD if k != "raw" or want_raw]
    got = {k: o[k].double().cpu().numpy().reshape(ref[k].shape) for k in names}
    _check(got, ref, names, tag=f"fwd {storage} {layout} d_sh={d_sh} P={len(pts)} {act} e={exponent}")
    z = np.flatnonzero((gs[:, 4:8] == 0).all(1))        # the zero quaternion: rotation 0 / 1e-12 = 0, R = I, covariance diag(s^2)
    if z.size:
        assert bool((got["rotations"][z] == 0).all())
        s2 = got["scales"][z].astype(np.float32) ** 2
        assert bool((got["covariances"][z] == np.einsum("pi,ij->pij", s2.astype(np.float64), np.eye(3))).all())


# (storage, act, exponent, d_sh, P, pts channels, with d_raw)
BACKWARD = [(st, act, e, 4, None, 3, raw) for st in ("f32", "f16", "bf16") for act, e in (("softplus", 1.0), ("bounded", 2.0), ("exp", -1.0))
            for raw in (True, False)] + \
           [("f32", "exp", 2.0, 4, None, 4, True), ("f32", "bounded", -1.0, 4, None, 3, False), ("f32", "softplus", 1.0, 1, 1, 3, True),
            ("f16", "softplus", 1.0, 1, 65, 4, True), ("f32", "softplus", 1.0, 28, 129, 4, True), ("bf16", "softplus", 1.0, 28, 65, 3, False),
            ("f32", "softplus", 1.0, 25, 33, 3, False), ("f16", "exp", 1.0, 9, 31, 3, True)]


@pytest.mark.parametrize("storage,act,exponent,d_sh,P,pts_ch,with_raw", BACKWARD)
def test_adapter_backward_matches_float64(storage, act, exponent, d_sh, P, pts_ch, with_raw):
    """adapter_backward_kernel<0> (f32: the class the default model trains in), <1>, <2>."""
    from vicasplat_amd import ops
    smin, smax = ACTS[act]
    pts, gs = pw.adapter_edge_inputs(act, d_sh, storage, exponent, P=P, pts_ch=pts_ch)
    mask = _mask(d_sh)
    cot = pw.adapter_cotangents(gs, d_sh, act, with_raw=with_raw)
    kw = dict(scale_act=act, scale_min=smin, scale_max=smax, opacity_exponent=exponent)
    ref = pw.adapter_backward(pts, gs, mask, **cot, **kw)
    assert not ref["ambiguous"].any()
    n, C = len(pts), gs.shape[1]
    c = {k: None if v is None else _t(v) for k, v in cot.items()}
    d_pts, d_gs = ops.gaussian_adapter_backward(_t(pts, storage).reshape(1, 1, n, pts_ch), _t(gs, storage).reshape(1, 1, n, C), _t(mask), c["d_means"],
                                                c["d_cov"], c["d_harm"], c["d_op"], c["d_raw"], **kw)
    torch.cuda.synchronize()
    assert d_pts.dtype == d_gs.dtype == DT[storage]
    got = dict(d_pts=d_pts[..., :3].double().cpu().numpy(), d_gs=d_gs.double().cpu().numpy())
    _check(got, ref, ("d_pts", "d_gs"), storage, tag=f"bwd {storage} {act} e={exponent} d_sh={d_sh} P={n} raw={with_raw}")
    # channels of pts beyond 3 and the padding columns of both gradient buffers (rows of a multiple of 8 elements) are exactly zero
    bp, bg = d_pts._base, d_gs._base
    assert bp.shape[-1] % 8 == 0 and bg.shape[-1] % 8 == 0 and bg.shape[-1] >= C
    assert float(bp[..., 3:].abs().max()) == 0 and (bg.shape[-1] == C or float(bg[..., C:].abs().max()) == 0)
    z = np.flatnonzero((gs[:, 4:8] == 0).all(1))        # the zero quaternion takes no gradient from the covariance
    if z.size:
        assert bool((got["d_gs"].reshape(n, C)[z, 4:8] == (pw.round_to(cot["d_raw"][z, 7:11], storage) if with_raw else 0)).all())


def test_adapter_backward_rejects_more_channels_than_its_tiles_hold():
    """d_sh = 29 (11 + 3 d_sh = 98 > kMaxCh) runs forward on the generic kernel (FORWARD above) and has no backward."""
    from vicasplat_amd import ops
    pts, gs = pw.adapter_edge_inputs("softplus", 29, "f16", 1.0, P=65)
    cot = pw.adapter_cotangents(gs, 29, "softplus", with_raw=False)
    with pytest.raises(RuntimeError, match="vs_gaussian_adapter_backward: bad argument"):
        ops.gaussian_adapter_backward(_t(pts, "f16").reshape(1, 1, 65, 3), _t(gs, "f16").reshape(1, 1, 65, 95), _t(_mask(29)), _t(cot["d_means"]),
                                      _t(cot["d_cov"]), _t(cot["d_harm"]), _t(cot["d_op"]), None)


@pytest.mark.parametrize("storage,act,exponent", [("f32", "softplus", 1.0), ("f32", "exp", 2.0), ("f16", "bounded", -1.0), ("bf16", "softplus", 1.0)])
def test_adapter_function_unused_outputs_and_scale_rotation_cotangents(storage, act, exponent):
    """autograd.gaussian_adapter: outputs no loss reads arrive as None cotangents; cotangents of `scales` / `rotations` are folded into
    d_raw by GaussianAdapterFn.backward (f32 torch on 7 channels) before the kernel runs."""
    from vicasplat_amd import autograd as A
    smin, smax = ACTS[act]
    d_sh = 4
    pts, gs = pw.adapter_edge_inputs(act, d_sh, storage, exponent, pts_ch=4)
    mask = _mask(d_sh)
    n, C = gs.shape
    kw = dict(scale_act=act, scale_min=smin, scale_max=smax, opacity_exponent=exponent)
    tp, tg = _t(pts, storage).reshape(1, 1, n, 4).requires_grad_(), _t(gs, storage).reshape(1, 1, n, C).requires_grad_()
    means, cov, sh, op, raw, scales, rot = A.gaussian_adapter(tp, tg, _t(mask), **kw)
    cot = pw.adapter_cotangents(gs, d_sh, act, with_raw=False, with_scales_rot=True)
    w = {k: _t(v) for k, v in cot.items() if v is not None}
    # only the covariance is read: every other cotangent is None
    only = dict(d_means=None, d_cov=cot["d_cov"], d_harm=None, d_op=None)
    g_pts, g_gs = torch.autograd.grad((cov * w["d_cov"].reshape(cov.shape)).sum(), (tp, tg), retain_graph=True)
    ref = pw.adapter_backward(pts, gs, mask, **only, **kw)
    got = dict(d_pts=g_pts[..., :3].double().cpu().numpy(), d_gs=g_gs.double().cpu().numpy())
    _check(got, ref, ("d_pts", "d_gs"), storage, tag=f"fn cov-only {storage} {act}")
    assert float(g_pts[..., 3].abs().max()) == 0
    # scales, rotations and opacities are read
    loss = (scales * w["d_scales"].reshape(scales.shape)).sum() + (rot * w["d_rot"].reshape(rot.shape)).sum() + (op * w["d_op"].reshape(op.shape)).sum()
    g_pts, g_gs = torch.autograd.grad(loss, (tp, tg))
    ref = pw.adapter_backward(pts, gs, mask, None, None, None, cot["d_op"], None, cot["d_scales"], cot["d_rot"], **kw)
    got = dict(d_pts=g_pts[..., :3].double().cpu().numpy(), d_gs=g_gs.double().cpu().numpy())
    _check(got, ref, ("d_pts", "d_gs"), storage, tag=f"fn scales+rotations {storage} {act}")
