"""The distillation teacher on the GPU (vicasplat_amd.model.distiller.Dust3R over the HIP kernels): the tiny teacher against the REAL
reference's float64 fixture and against the float64 restatement of tests/teacher_f64.py, and one distill-only training step whose targets
come from the teacher.  -m gpu.

Bars (the project's numbers for each operand class at this depth, not fitted to these runs):
  split   every output and every block checksum <= 2e-4 of max |f64| (tests/test_split_path_gpu.py's bar against the encoder's goldens);
  f16     outputs <= 8e-3, block checksums <= 6e-3 (F16_TOL of tests/test_encoder_gpu.py: raw quantities and per-block drift);
  a scene alone against the same scene inside a batch of three: 2e-4 (split), 1e-2 (f16), the bars of tests/test_encoder_gpu.py.
The fixture is 2 scenes of 32 x 32 pixels (2 x 2 tokens per frame); the second shape is 3 scenes of 32 x 48 (2 x 3 tokens: non-square
landscape, an odd grid width, so the DPT trunk's crop after the stride-2 level is exercised).

Measured on an MI355X (`-s` prints them), relative to max |f64|, views 1 / 2:
  fixture      split: pts 1.1e-6 / 3.5e-6, conf 4.7e-7 / 2.4e-6, worst block checksum 1.8e-6 (dec10_2); the reference's own f32 run: pts 1.3e-6 /
               2.3e-6, conf 4.5e-7 / 2.2e-6.  f16: pts 1.5e-3 / 3.1e-3, conf 4.3e-4 / 2.5e-3, worst block 2.9e-3 (dec00_2)
  3 x 32 x 48  split: pts 9.9e-7 / 3.3e-6, conf 7.1e-7 / 2.0e-6; scene 1 alone against the batch <= 2.4e-6.  f16: <= 4.9e-3; alone <= 1.2e-3
  transform    inside the kernel against the einsum of the anchor-space points: 1.5 / 1.6 units of 2^-24 mag (bounds 10.5 / 17.8)
  step         loss_distill 4.1478744 against 4.1478747 with the float64 restatement's teacher outputs: 0.10 units of 2^-24 mag (bound 0.96);
               the teacher's targets at 64 x 64 within 5.1e-6 of the restatement's
"""
import json
import os

import numpy as np
import pytest
import torch

import teacher_f64 as T

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
OUTS = (("pts1", 0, "pts3d"), ("conf1", 0, "conf"), ("pts2", 1, "pts3d"), ("conf2", 1, "conf"))
BARS = {"split": dict(out=2e-4, block=2e-4, batch=2e-4), "f16": dict(out=8e-3, block=6e-3, batch=1e-2)}


@pytest.fixture(scope="module")
def weights():
    from vicasplat_amd.synthetic import golden_weights
    return golden_weights(json.load(open(os.path.join(G, "shapes_teacher_tiny.json"))), seed=0)


def _teacher(W, cls):
    from vicasplat_amd.model.distiller import Dust3R
    m = Dust3R(**T.TINY, compute_dtype=cls)
    m.load_state_dict(W, strict=True)
    return m.cuda()


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


@pytest.mark.parametrize("cls", ["split", "f16"])
def test_tiny_teacher_matches_the_reference_float64(weights, cls):
    z = np.load(os.path.join(G, "teacher_tiny.npz"))
    m = _teacher(weights, cls)
    img = T.teacher_input(int(z["cfg_B"]), int(z["cfg_H"]), int(z["cfg_W"]), int(z["cfg_seed"]))
    probes = {}
    m._probe = lambda n, t: probes.__setitem__(n, T.checksum(t).cpu().numpy())
    res = m(dict(image=img.cuda()))
    m._probe = None
    torch.cuda.synchronize()
    errs = {k: _rel(res[v][f].cpu().numpy(), z["f64_" + k]) for k, v, f in OUTS}
    names = [str(n) for n in z["f64_block_names"]]
    drift = {n: float(np.abs(probes[n] - row).max() / row[1]) for n, row in zip(names, z["f64_blocks"])}
    worst = max(drift, key=drift.get)
    print(f"tiny teacher [{cls}] vs reference f64:", {k: f"{v:.2e}" for k, v in errs.items()}, f"block drift max {drift[worst]:.2e} at {worst};",
          "reference's own f32:", {k: f"{float(z['ref_err_' + k]):.1e}" for k, _, _ in OUTS})
    for v in (0, 1):
        assert res[v]["pts3d"].shape == (2, 32, 32, 3) and res[v]["conf"].shape == (2, 32, 32) and res[v]["pts3d"].dtype == torch.float32
        assert float(res[v]["conf"].min()) > 1.0
    assert set(probes) == set(names)
    bar = BARS[cls]
    assert drift[worst] <= bar["block"], (worst, drift[worst])
    assert max(errs.values()) <= bar["out"], errs


@pytest.mark.parametrize("cls", ["split", "f16"])
def test_second_shape_and_batch_against_the_restatement(weights, cls):
    B, H, W = 3, 32, 48
    img = T.teacher_input(B, H, W, 5)
    ref = T.teacher_forward(weights, img, T.TINY["enc_num_heads"], T.TINY["dec_num_heads"], torch.float64)
    m = _teacher(weights, cls)
    res = m(dict(image=img.cuda()))
    errs = {k: _rel(res[v][f].cpu().numpy(), ref[v][f].numpy()) for k, v, f in OUTS}
    one = m(dict(image=img[1:2].cuda()))
    inv = {k: _rel(one[v][f].cpu().numpy(), res[v][f][1:2].cpu().numpy()) for k, v, f in OUTS}
    print(f"tiny teacher [{cls}] 3 x 32 x 48 vs restatement f64:", {k: f"{v:.2e}" for k, v in errs.items()}, "scene 1 alone vs in the batch:",
          {k: f"{v:.2e}" for k, v in inv.items()})
    assert res[0]["pts3d"].shape == (B, H, W, 3)
    assert max(errs.values()) <= BARS[cls]["out"], errs
    assert max(inv.values()) <= BARS[cls]["batch"], inv


def test_transform_is_the_einsum_of_the_loss_within_the_kernels_bound(weights, monkeypatch):
    """With a transform the teacher's points equal its anchor-space points pushed through distillation_loss's einsum + add (in float64),
    element by element within the tail kernel's bound 4 max(r32, 1) 2^-24 mag.  The raw head output of the run with the transform is
    kept (a recorder around ops.points_conf that calls through) and the anchor-space points are formed from those very values, so that the
    comparison is of the tail alone and not of two runs of the network."""
    from vicasplat_amd import ops
    B, H, W = 2, 32, 32
    img = T.teacher_input(B, H, W, 7)
    E = torch.eye(4).repeat(B, 1, 1)
    E[:, :3] = T.tail_transforms(B, seed=3)
    m = _teacher(weights, "split")
    kept = []
    real = ops.points_conf
    monkeypatch.setattr(ops, "points_conf", lambda raw, tr=None, **kw: (kept.append((raw.clone(), tr)), real(raw, tr, **kw))[1])
    res = m(dict(image=img.cuda()), transform=E.cuda())
    monkeypatch.undo()
    assert len(kept) == 2 and all(tr is not None and tuple(tr.shape) == (B, 3, 4) for _, tr in kept)
    for v, (raw, tr) in enumerate(kept):
        anchor, conf = ops.points_conf(raw)      # the reference's outputs: no transform
        assert torch.equal(conf, res[v]["conf"])
        want = torch.einsum("bij,bhwj->bhwi", E[:, :3, :3].double(), anchor.double().cpu()) + E[:, None, None, :3, 3].double()
        ref = T.tail(raw.double().cpu(), E[:, :3].double())
        r32 = T.tail_ratio(*T.tail_torch_f32(raw.cpu(), E[:, :3]), ref)
        lim = 4 * max(r32, 1.0) * 2.0 ** -24 * ref["mag_pts"]
        err = (res[v]["pts3d"].double().cpu() - want).abs()
        print(f"view {v + 1}: transform inside the kernel vs einsum of the anchor-space points: {float((err / (2.0 ** -24 * ref['mag_pts'])).max()):.3f} units, "
              f"bound {4 * max(r32, 1.0):.2f}")
        assert bool((err <= lim).all())


# ---- the step: tiny student with the confidence channel, V = 3, targets from the tiny teacher ----
STUDENT = dict(enc_depth=2, dec_embed_dim=192, dec_num_heads=3)
RES = 64      # 4 x 4 tokens per frame


def test_distill_only_step_from_images_alone(weights):
    import dataclasses
    import distill_f64 as D
    from oracle import encoder_ref as er
    from test_encoder_oracle import conf_shapes
    from vicasplat_amd import callers
    from vicasplat_amd.model.encoder import default_cfg, get_encoder
    from vicasplat_amd.model.encoder.train_forward import forward_train
    m, _ = get_encoder(dataclasses.replace(default_cfg(**STUDENT), predict_conf=True))
    m.load_state_dict(er.golden_weights(conf_shapes(json.load(open(os.path.join(G, "shapes_tiny.json")))), seed=0), strict=True)
    m = m.cuda().train()
    teacher = _teacher(weights, "split")
    B, V = 2, 3
    img, K = er.synthetic_input(B, V, RES, 0)
    g = torch.Generator().manual_seed(1)
    E = torch.eye(4).repeat(B, V, 1, 1)
    c, s = float(np.cos(0.3)), float(np.sin(0.3))
    E[:, 1:, :3, :3] = torch.tensor([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    E[:, 1:, :3, 3] = torch.randn(B, V - 1, 3, generator=g) * 0.2
    ctx = dict(image=img.cuda(), intrinsics=K.cuda(), extrinsics=E.cuda())
    np.random.seed(4)
    dist = callers.distill_targets(teacher, ctx, weight=0.5, only=True)
    assert dist["pts_in_first_frame"] and dist["pseudo_gt1"]["pts3d"].shape == (B, RES, RES, 3) and dist["frame_idx"].shape == (B, 2)
    kept = {}

    def forward_fn(*a, **kw):
        kept["out"] = forward_train(*a, **kw)
        return kept["out"]

    class NoDecoder:
        def forward(self, *a, **kw):
            raise AssertionError("the distillation-only step renders nothing")

    opt, _ = callers.configure_optimizer(m, lr=1e-5, new_param_keywords=None)
    res = callers.training_step(m, NoDecoder(), dict(context=ctx, target={}), opt, compute_dtype="split", camera_weight=1.0, distill=dist,
                                forward_fn=forward_fn)
    assert "psnr" not in res and torch.isfinite(res["loss"]) and torch.isfinite(res["loss_distill"])
    assert all(p.grad is None and not p.requires_grad for p in teacher.parameters())
    gw = m.downstream_head1.dpt.head[4].weight.grad
    assert gw is not None and torch.isfinite(gw).all() and float(gw.abs().max()) > 0
    # the same term with the teacher's outputs taken from the float64 restatement (anchor space, moved by the loss's own einsum in f64)
    fi, si = dist["frame_idx"].cpu(), dist["segment_idx"].cpu()
    anchors = torch.stack([img[b, fi[b]] for b in range(B)])
    r1, r2 = T.teacher_forward(weights, anchors, T.TINY["enc_num_heads"], T.TINY["dec_num_heads"], torch.float64)
    Ea = torch.stack([E[b, fi[b, 0]] for b in range(B)]).double()
    move = lambda p: (torch.einsum("bij,bhwj->bhwi", Ea[:, :3, :3], p) + Ea[:, None, None, :3, 3]).numpy()
    out = kept["out"]
    xyz, conf = out["gaussian_centers"].detach().float().cpu(), out["confidence"].detach().float().cpu()
    pick = lambda x, j: torch.stack([x[b, si[b, j]] for b in range(B)]).numpy()
    ref = D.regr3d(move(r1["pts3d"]), move(r2["pts3d"]), pick(xyz, 0), pick(xyz, 1), r1["conf"].numpy(), r2["conf"].numpy(), pick(conf, 0), pick(conf, 1),
                   normalize_pts=True)
    unit = 0.5 * D.U32 * float(ref["loss_mag"])
    got, want = float(res["loss_distill"]), 0.5 * float(ref["loss"])
    e_t = {k: _rel(dist["pseudo_gt%d" % (v + 1)][f].cpu().numpy(), (move(r[f]) if f == "pts3d" else r[f].numpy()))
           for (k, v, f), r in zip(OUTS, (r1, r1, r2, r2))}
    print("distill-only step from images: loss_distill", got, "with the float64 restatement's teacher outputs", want, "difference",
          round(abs(got - want) / unit, 3), "units of 2^-24 mag, bound", D.gpu_factor("loss"), "; teacher vs restatement:", {k: f"{v:.2e}" for k, v in e_t.items()})
    assert abs(got - want) <= D.gpu_factor("loss") * unit
