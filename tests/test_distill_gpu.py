"""The HIP distillation point loss (csrc/distill.hip behind callers.Regr3D) against the float64 reference of tests/distill_f64.py.  -m gpu.

Shapes: 24 x 20 (n = 480: ranks 4.79 and 474.21), 17 x 13, 1 x 101 (integer ranks: a threshold IS a distance), 64 x 64 (four trips of the
selection workgroup, four chunks of the streaming passes); B = 1, 3; normalize_pts off / on; predicted confidences absent / given.
Inputs come from distill_f64.make_inputs, whose quantile brackets are separated by >= 1e-4 relative (asserted): the mask then does not
depend on f32 rounding and must equal the reference's exactly -- it is read off d_pts (zero outside it, non-zero inside for these inputs)
and off the count of valid pixels the forward leaves in its workspace.

Criterion: every element of loss, d_pts, d_conf within 4 r32 2^-24 mag of the reference (distill_f64.R32, no floor: 0.96 / 2.12 / 3.52).
Measured on an MI355X, max |gpu - ref| / (2^-24 mag) (`-s` prints it per case), beside the torch-f32 ratio r32 of tests/test_distill_cpu.py:

    output   r32    bound   gpu
    loss     0.24   0.96    0.18
    d_pts    0.53   2.12    0.66
    d_conf   0.88   3.52    0.88   (the rounding of 1 / (B n), as torch's)

The distill-only step's loss at 256 x 256 (n = 65 536, B = 2): HIP 0.045, torch backend 0.045 units; the two are bit-equal there.
"""
import numpy as np
import pytest
import torch

import distill_f64 as D

pytestmark = pytest.mark.gpu

SHAPES = [(24, 20), (17, 13), (1, 101), (64, 64)]
KEYS = ("gt1", "gt2", "pr1", "pr2", "cg1", "cg2", "pc1", "pc2")


def _dev():
    return torch.device("cuda:0")


def _run(z, norm, conf, backend="hip", up=None):
    """loss and gradients of callers.Regr3D on the device -> dict of float64 numpy arrays (+ the workspace view for the HIP backend)."""
    from vicasplat_amd import callers
    t = {k: torch.tensor(z[k], device=_dev(), requires_grad=k[:2] in ("pr", "pc")) for k in KEYS if k in z}
    loss = callers.Regr3D(backend=backend)(t["gt1"], t["gt2"], t["pr1"], t["pr2"], t["cg1"], t["cg2"], t["pc1"] if conf else None,
                                           t["pc2"] if conf else None, normalize_pts=norm)
    wrt = [t["pr1"], t["pr2"]] + ([t["pc1"], t["pc2"]] if conf else [])
    grads = torch.autograd.grad(loss if up is None else loss * up, wrt)
    names = ("d_pts1", "d_pts2", "d_conf1", "d_conf2")
    out = {k: g.double().cpu().numpy() for k, g in zip(names, grads)}
    out["loss"] = loss.detach().double().cpu().numpy()
    return out


def _ref(z, norm, conf):
    return D.regr3d(z["gt1"], z["gt2"], z["pr1"], z["pr2"], z["cg1"], z["cg2"], z["pc1"] if conf else None, z["pc2"] if conf else None,
                    normalize_pts=norm)


def _check(got, ref, conf, tag, worst):
    for k in ("loss", "d_pts1", "d_pts2") + (("d_conf1", "d_conf2") if conf else ()):
        key = k.rstrip("12")
        u = D.units(got[k], ref, k)
        worst[key] = max(worst.get(key, 0.0), u)
        assert np.isfinite(got[k]).all(), (tag, k)
        assert u <= D.gpu_factor(key), (tag, k, u)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_regr3d_matches_float64(H, W, B):
    from vicasplat_amd import ops
    z = D.make_inputs(B, H, W, 100 + H + B)
    assert D.gap_ok(z["gt1"]) and D.gap_ok(z["gt2"])
    worst = {}
    for norm in (False, True):
        for conf in (False, True):
            ref, got = _ref(z, norm, conf), _run(z, norm, conf)
            _check(got, ref, conf, (norm, conf), worst)
            for v in ("1", "2"):          # the mask, with no exempted element
                assert np.array_equal((got["d_pts" + v] != 0).any(-1), ref["valid" + v]), (norm, conf, v)
    # thresholds and counts as the forward left them
    t = {k: torch.tensor(z[k], device=_dev()) for k in KEYS}
    _, work = ops.regr3d_forward(t["gt1"], t["gt2"], t["pr1"], t["pr2"], t["cg1"], t["cg2"], normalize_pts=True)
    view = ops.regr3d_workspace_view(work, B)
    thr = view["thresholds"].double().cpu().numpy()
    for v in range(2):
        want = ref["thr%d" % (v + 1)]
        assert np.abs(thr[v] - want).max() <= 4 * 2.0 ** -24 * np.abs(want).max(), (v, thr[v], want)
        assert int(view["counts"][v]) == int(ref["valid%d" % (v + 1)].sum())
    print(f"regr3d B={B} {H}x{W}", {k: round(v, 3) for k, v in worst.items()})


def test_ties_across_the_rank_are_all_kept():
    z = D.with_plateau(D.make_inputs(3, 24, 20, 31), "gt1", b=1)
    z = D.with_plateau(z, "gt2", b=0, below=1, above=1)
    ref = _ref(z, True, True)
    lo = D.ranks(480, 0.01)[0]
    assert int(ref["valid1"][1].sum()) == 480 - (lo + 1) - (479 - D.ranks(480, 0.99)[0]) + 3         # the plateau's three low points included
    got = _run(z, True, True)
    for v in ("1", "2"):
        assert np.array_equal((got["d_pts" + v] != 0).any(-1), ref["valid" + v])
    _check(got, ref, True, "ties", {})


def test_zero_residual_and_origin_have_zero_finite_gradients():
    z = D.make_inputs(2, 17, 13, 32)
    ref0 = _ref(z, False, True)
    ij = np.argwhere(ref0["valid1"][0])[5]           # a valid pixel of view 1, element 0
    kl = np.argwhere(ref0["valid2"][1])[7]
    z["pr1"][0, ij[0], ij[1]] = z["gt1"][0, ij[0], ij[1]]          # prediction == target (no normalisation: the residual is exactly 0)
    z["pr2"][1, kl[0], kl[1]] = 0.0                                # a prediction at the origin (under normalisation: |p| has subgradient 0)
    z["pc1"][0, 0, 0] = z["cg1"][0, 0, 0]                          # |.| at 0
    for norm in (False, True):
        ref, got = _ref(z, norm, True), _run(z, norm, True)
        _check(got, ref, True, norm, {})
        assert got["d_conf1"][0, 0, 0] == 0.0
        if not norm:
            assert (got["d_pts1"][0, ij[0], ij[1]] == 0.0).all() and (ref["d_pts1"][0, ij[0], ij[1]] == 0.0).all()
        else:       # at the origin only the direct term remains: -(gt_conf / (count f_pr)) e^
            assert np.isfinite(got["d_pts2"][1, kl[0], kl[1]]).all() and np.abs(got["d_pts2"][1, kl[0], kl[1]]).max() > 0


def test_non_finite_prediction_outside_the_mask_is_ignored():
    """A predicted point at infinity outside the mask: the reference's invalid_to_zeros drops it from the factor; the kernels never read it
    into a sum, and every gradient stays finite (zero at that pixel)."""
    z = D.make_inputs(2, 24, 20, 35)
    ref = _ref(z, True, True)
    i, j = np.argwhere(~ref["valid1"][0])[0]
    z["pr1"][0, i, j] = np.inf
    got = _run(z, True, True)
    _check(got, ref, True, "inf outside the mask", {})
    assert (got["d_pts1"][0, i, j] == 0.0).all()


def test_two_runs_are_bit_identical_and_upstream_scales():
    z = D.make_inputs(3, 64, 64, 33)
    a, b = _run(z, True, True), _run(z, True, True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    c = _run(z, True, True, up=4.0)          # a power of two: exact
    for k in ("d_pts1", "d_pts2", "d_conf1", "d_conf2"):
        assert np.array_equal(c[k], 4.0 * a[k]), k


def test_nan_in_the_pseudo_gt_is_an_error():
    z = D.make_inputs(1, 17, 13, 34)
    z["gt2"][0, 3, 4, 1] = np.nan
    with pytest.raises(RuntimeError, match="vsd_regr3d_forward.*NaN"):
        _run(z, False, False)
    z = D.make_inputs(1, 17, 13, 34)          # the library is usable afterwards
    _check(_run(z, False, False), _ref(z, False, False), False, "after", {})


def test_hip_backend_has_no_cpu_path():
    from vicasplat_amd import callers
    z = D.make_inputs(1, 5, 7, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        callers.Regr3D()(*[torch.tensor(z[k]) for k in KEYS[:6]])


# ---- the full path: tiny encoder with the confidence channel, V = 3, one distill-only step in the split class ----
TINY = dict(enc_depth=2, dec_embed_dim=192, dec_num_heads=3)


def test_distill_only_training_step_on_the_tiny_encoder():
    import dataclasses
    import json
    import os
    from oracle import encoder_ref as er
    from test_encoder_oracle import conf_shapes
    from vicasplat_amd import callers
    from vicasplat_amd.model.encoder import default_cfg, get_encoder
    from vicasplat_amd.model.encoder.train_forward import forward_train
    G = os.path.join(os.path.dirname(__file__), "golden")
    m, _ = get_encoder(dataclasses.replace(default_cfg(**TINY), predict_conf=True))
    m.load_state_dict(er.golden_weights(conf_shapes(json.load(open(os.path.join(G, "shapes_tiny.json")))), seed=0), strict=True)
    m = m.cuda().train()
    B, V = 2, 3
    img, K = er.synthetic_input(B, V, 256, 0)
    g = torch.Generator().manual_seed(1)
    E = torch.eye(4).repeat(B, V, 1, 1)
    c, s = float(np.cos(0.3)), float(np.sin(0.3))
    E[:, 1:, :3, :3] = torch.tensor([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    E[:, 1:, :3, 3] = torch.randn(B, V - 1, 3, generator=g) * 0.2
    frame_idx = segment_idx = torch.tensor([[1, 2], [2, 0]])
    R, t = E[torch.arange(B), frame_idx[:, 0], :3, :3].cuda(), E[torch.arange(B), frame_idx[:, 0], :3, 3].cuda()
    # teacher points whose quantile brackets are separated AFTER the rigid transform (at n = 65 536 random points are not): separated in
    # the first video frame's space, then taken back into the anchor's
    rng = np.random.default_rng(40)
    Rn, tn = R.double().cpu().numpy(), t.double().cpu().numpy()
    z = {}
    for v in ("1", "2"):
        world = D.separate(rng.normal(0, 1, (B, 256, 256, 3)) * [1.0, 0.7, 1.5] + [0.2, -0.1, 2.0])
        z["gt" + v] = np.einsum("bji,bhwj->bhwi", Rn, world - tn[:, None, None]).astype(np.float32)
        z["cg" + v] = (1 + np.exp(rng.normal(0, 1, (B, 256, 256)))).astype(np.float32)
    gts = [(torch.einsum("bij,bhwj->bhwi", R, torch.tensor(z[k]).cuda()) + t[:, None, None]).cpu().numpy() for k in ("gt1", "gt2")]
    assert D.gap_ok(gts[0]) and D.gap_ok(gts[1])
    dist = dict(pseudo_gt1=dict(pts3d=torch.tensor(z["gt1"]).cuda(), conf=torch.tensor(z["cg1"]).cuda()),
                pseudo_gt2=dict(pts3d=torch.tensor(z["gt2"]).cuda(), conf=torch.tensor(z["cg2"]).cuda()),
                frame_idx=frame_idx.cuda(), segment_idx=segment_idx.cuda(), weight=0.5, only=True)
    batch = dict(context=dict(image=img.cuda(), intrinsics=K.cuda(), extrinsics=E.cuda()), target={})
    kept = {}

    def forward_fn(*a, **kw):
        kept["out"] = forward_train(*a, **kw)
        return kept["out"]

    class NoDecoder:
        def forward(self, *a, **kw):
            raise AssertionError("the distillation-only step renders nothing")

    opt, _ = callers.configure_optimizer(m, lr=1e-5, new_param_keywords=None)
    res = callers.training_step(m, NoDecoder(), batch, opt, compute_dtype="split", camera_weight=1.0, distill=dist, forward_fn=forward_fn)
    assert "psnr" not in res and "loss_mse" not in res and torch.isfinite(res["loss"]) and torch.isfinite(res["loss_distill"])
    gw = m.downstream_head1.dpt.head[4].weight.grad
    assert gw is not None and torch.isfinite(gw).all() and float(gw[:3].abs().max()) > 0 and float(gw[3].abs().max()) > 0
    # the term on the same outputs: HIP == torch backend == float64 reference within the bound
    out = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in kept["out"].items()}
    hip = callers.distillation_loss(out, dist["pseudo_gt1"], dist["pseudo_gt2"], dist["frame_idx"], dist["segment_idx"], batch["context"]["extrinsics"], 0.5)
    tor = callers.distillation_loss(out, dist["pseudo_gt1"], dist["pseudo_gt2"], dist["frame_idx"], dist["segment_idx"], batch["context"]["extrinsics"], 0.5,
                                    callers.Regr3D(backend="torch"))
    assert torch.equal(hip, res["loss_distill"])
    xyz, conf = out["gaussian_centers"].float().cpu(), out["confidence"].float().cpu()
    pick = lambda x, j: torch.stack([x[b, segment_idx[b, j]] for b in range(B)]).numpy()
    ref = D.regr3d(gts[0], gts[1], pick(xyz, 0), pick(xyz, 1), z["cg1"], z["cg2"], pick(conf, 0), pick(conf, 1), normalize_pts=True)
    lim = 0.5 * D.gpu_factor("loss") * D.U32 * float(ref["loss_mag"])
    units = lambda x: abs(float(x) - 0.5 * float(ref["loss"])) / (0.5 * D.U32 * float(ref["loss_mag"]))
    print("distill-only step: loss_distill", float(hip), "torch backend", float(tor), "units of 2^-24 mag vs float64: hip", round(units(hip), 3),
          "torch", round(units(tor), 3), "bound", D.gpu_factor("loss"))
    assert abs(float(hip) - float(tor)) <= lim and abs(float(hip) - 0.5 * float(ref["loss"])) <= lim
