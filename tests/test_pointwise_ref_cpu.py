"""The float64 references of tests/pointwise_f64.py are right, and the criterion of the GPU tests built on them has teeth.  No GPU.

1. Pinned: the hand-written float64 forward and chain rule of the Gaussian adapter and of LayerNorm + modulation equal torch float64
   autograd of the plain formulation (heads/postprocess.py:46-56 + MyGaussianAdapter; F.layer_norm * (1 + scale) + shift) to 1e-12 mag
   per element, on the edge sets and on random inputs, for the three scale activations and opacity exponents 1, 2, 0.5, -1.
2. r32: the same code in float32 against float64, max |f32 - f64| / (2^-24 mag) over the edge sets.  Measured (`-s` prints them):

       adapter    means 0.33  covariances 0.33  harmonics 0.95  opacities 0.64  scales 1.00  rotations 0.29  raw 0.33
                  d_pts 0.33  d_gs 0.98
       LayerNorm  y 1.18  dx 1.05  dw 1.06  db 2.31  dscale 1.18  dshift 2.02

   The adapter's are at most 1 (mag is a worst-case bound; one rounding is up to 2^-24 of its result), so B = 4 max(r32, 1) = 4 for all
   its outputs.  LayerNorm's exceed 1 where numpy adds the rows of a column one after the other (db, dshift: up to M - 1 roundings against
   the one that mag counts per sum); recorded rounded up in pointwise_f64.R32_LAYERNORM, B = 4 r32 = 4.4 .. 9.6.
3. Mutation check: each deliberate defect planted in the f32 restatement exceeds that GPU bound on the edge set (the factor is printed);
   the clean restatement stays inside it.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pointwise_f64 as pw

ACTS = [("softplus", 0.0, 0.0), ("exp", 0.0, 0.0), ("bounded", 0.5, 15.0)]
EXPONENTS = [1.0, 2.0, 0.5, -1.0]
D_SH = 4
FWD = ("means", "covariances", "harmonics", "opacities", "scales", "rotations", "raw")


def _mask(d_sh):
    return np.linspace(1.0, 0.1, d_sh).astype(np.float32).astype(np.float64)


def torch_adapter(pts, gs, mask, act, smin, smax, exponent):
    """The plain per-pixel formulation, in the dtype of pts / gs."""
    P, nsh = gs.shape[0], mask.numel()
    xyz = pts[:, :3]
    dist = xyz.norm(dim=-1, keepdim=True)
    centers = xyz / dist.clip(min=1e-8) * torch.expm1(dist)
    o = torch.sigmoid(gs[:, 0])
    if exponent > 0:
        o = 0.5 * (1 - (1 - o) ** exponent + o ** (1 / exponent))
    v = gs[:, 1:4]
    sc = {"softplus": lambda: (0.001 * F.softplus(v)).clamp_max(0.3), "exp": lambda: torch.exp(v).clamp_max(0.3),
          "bounded": lambda: smin + (smax - smin) * torch.sigmoid(v)}[act]()
    rot = F.normalize(gs[:, 4:8], dim=-1)
    qi, qj, qk, qr = rot.unbind(-1)
    two_s = 2 / ((rot * rot).sum(-1) + 1e-8)
    R = torch.stack([1 - two_s * (qj * qj + qk * qk), two_s * (qi * qj - qk * qr), two_s * (qi * qk + qj * qr),
                     two_s * (qi * qj + qk * qr), 1 - two_s * (qi * qi + qk * qk), two_s * (qj * qk - qi * qr),
                     two_s * (qi * qk - qj * qr), two_s * (qj * qk + qi * qr), 1 - two_s * (qi * qi + qj * qj)], -1).reshape(P, 3, 3)
    RS = R * sc[:, None, :]
    return dict(means=centers, covariances=RS @ RS.transpose(-1, -2), harmonics=gs[:, 8:].reshape(P, 3, nsh) * mask, opacities=o, scales=sc,
                rotations=rot, raw=torch.cat([centers, gs], -1))


def _inputs(kind, act, exponent):
    if kind == "edge":
        return pw.adapter_edge_inputs(act, D_SH, "f32", exponent)
    rng = np.random.default_rng(5)
    f = lambda a: a.astype(np.float32).astype(np.float64)
    gs = rng.standard_normal((200, 8 + 3 * D_SH))
    gs[:, 1:4] *= 3
    return f(rng.standard_normal((200, 3)) * 0.7), f(gs)


def _close(got, ref, name, rel):
    err, lim = np.abs(got - ref[name]), rel * ref[name + "_mag"]
    assert bool((err <= lim).all()), (name, float(err.max()), int(np.argmax((err - lim).reshape(-1))))


@pytest.mark.parametrize("kind", ["edge", "random"])
@pytest.mark.parametrize("exponent", EXPONENTS)
@pytest.mark.parametrize("act,smin,smax", ACTS)
def test_adapter_reference_equals_float64_autograd(act, smin, smax, exponent, kind):
    pts, gs = _inputs(kind, act, exponent)
    mask = _mask(D_SH)
    kw = dict(scale_act=act, scale_min=smin, scale_max=smax, opacity_exponent=exponent)
    ref = pw.adapter_forward(pts, gs, mask, **kw)
    if kind == "edge":
        assert not ref["ambiguous"].any()
    tp, tg = torch.from_numpy(pts).requires_grad_(), torch.from_numpy(gs).requires_grad_()
    t = torch_adapter(tp, tg, torch.from_numpy(mask), act, smin, smax, exponent)
    for k in FWD:
        _close(t[k].detach().numpy(), ref, k, 1e-12)
    for with_raw, with_sr in ((True, True), (False, False)):
        cot = pw.adapter_cotangents(gs, D_SH, act, with_raw=with_raw, with_scales_rot=with_sr)
        names = dict(d_means="means", d_cov="covariances", d_harm="harmonics", d_op="opacities", d_raw="raw", d_scales="scales", d_rot="rotations")
        loss = sum((t[names[k]] * torch.from_numpy(v).reshape(t[names[k]].shape)).sum() for k, v in cot.items() if v is not None)
        gp, gg = torch.autograd.grad(loss, (tp, tg), retain_graph=True)
        assert bool(torch.isfinite(gp).all() and torch.isfinite(gg).all())
        bwd = pw.adapter_backward(pts, gs, mask, **cot, **kw)
        _close(gp.numpy(), bwd, "d_pts", 1e-12)
        _close(gg.numpy(), bwd, "d_gs", 1e-12)
        if kind == "edge" and not with_sr:      # the zero quaternion: a finite identity rotation and no gradient from the covariance
            z = np.flatnonzero((gs[:, 4:8] == 0).all(1))
            assert z.size and bool((bwd["d_gs"][z, 4:8] == 0).all())
            assert bool((ref["covariances"][z] == np.einsum("pi,ij->pij", ref["scales"][z] ** 2, np.eye(3))).all())


LN_CASES = [(33, 1024, 5), (9, 768, 3), (33, 192, 9), (7, 4, 7), (9, 2048, 0)]


def _ln_kw(z, mod_rows):
    return dict(scale=z["scale"], mod_rows=mod_rows) if mod_rows else {}


@pytest.mark.parametrize("M,C,mod_rows", LN_CASES)
def test_layernorm_reference_equals_float64_autograd(M, C, mod_rows):
    G = -(-M // mod_rows) if mod_rows else 1
    z = pw.layernorm_edge_inputs(M, C, G)
    T = lambda a: torch.from_numpy(a).requires_grad_()
    x, w, b, sc, sh = T(z["x"]), T(z["w"]), T(z["b"]), T(z["scale"]), T(z["shift"])
    y = F.layer_norm(x, (C,), w, b, 1e-6)
    if mod_rows:
        g = torch.arange(M) // mod_rows
        y = y * (1 + sc[g]) + sh[g]
    ref = pw.layernorm_forward(z["x"], z["w"], z["b"], shift=z["shift"] if mod_rows else None, **_ln_kw(z, mod_rows))
    _close(y.detach().numpy(), ref, "y", 1e-12)
    grads = torch.autograd.grad((y * torch.from_numpy(z["dout"])).sum(), (x, w, b) + ((sc, sh) if mod_rows else ()))
    bwd = pw.layernorm_backward(z["dout"], z["x"], z["w"], z["b"], dx_add=z["dx_add"], **_ln_kw(z, mod_rows))
    _close(grads[0].numpy() + z["dx_add"], bwd, "dx", 1e-12)
    for name, gt in zip(("dw", "db", "dscale", "dshift"), grads[1:]):
        _close(gt.numpy(), bwd, name, 1e-12)


def _adapter_units(act, smin, smax, exponent, mutate=None, B=None):
    """f32 restatement vs float64 over the edge set: {output: r32 units} or, with B, {output: error / GPU bound}."""
    pts, gs = pw.adapter_edge_inputs(act, D_SH, "f32", exponent)
    mask = _mask(D_SH)
    kw = dict(scale_act=act, scale_min=smin, scale_max=smax, opacity_exponent=exponent)
    cot = pw.adapter_cotangents(gs, D_SH, act, with_raw=True, with_scales_rot=True)
    ref = dict(pw.adapter_forward(pts, gs, mask, **kw), **pw.adapter_backward(pts, gs, mask, **cot, **kw))
    got = dict(pw.adapter_forward(pts, gs, mask, dtype=np.float32, mutate=mutate, **kw),
               **pw.adapter_backward(pts, gs, mask, dtype=np.float32, mutate=mutate, **cot, **kw))
    names = FWD + ("d_pts", "d_gs")
    if B is None:
        assert all(np.isfinite(pw.ratio(got[k], ref, k, 1.0)) for k in names)      # elements of magnitude 0 (copies, exact zeros) are exact
        return {k: pw.units(got[k], ref, k) for k in names}
    return {k: pw.ratio(got[k], ref, k, pw.gpu_factor(pw.R32_ADAPTER[k])) for k in names}


def _ln_units(M, C, mod_rows, mutate=None, B=None):
    G = -(-M // mod_rows) if mod_rows else 1
    z = pw.layernorm_edge_inputs(M, C, G)
    kw = _ln_kw(z, mod_rows)
    both = lambda **o: dict(pw.layernorm_forward(z["x"], z["w"], z["b"], shift=z["shift"] if mod_rows else None, **kw, **o),
                            **pw.layernorm_backward(z["dout"], z["x"], z["w"], z["b"], dx_add=z["dx_add"], **kw, **o))
    ref, got = both(), both(dtype=np.float32, mutate=mutate)
    names = [k for k in ("y", "dx", "dw", "db", "dscale", "dshift") if k in ref]
    if B is None:
        return {k: pw.units(got[k], ref, k) for k in names}
    return {k: pw.ratio(got[k], ref, k, pw.gpu_factor(pw.R32_LAYERNORM[k])) for k in names}


def test_f32_restatement_ratios():
    """r32 per output over the edge sets; the recorded values (pointwise_f64.R32_*) cover what is measured."""
    worst = {}
    for act, smin, smax in ACTS:
        for e in EXPONENTS:
            for k, v in _adapter_units(act, smin, smax, e).items():
                worst[k] = max(worst.get(k, 0.0), v)
    print("r32 adapter  ", {k: round(v, 2) for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= pw.R32_ADAPTER[k], (k, v)
    worst = {}
    for M, C, mr in LN_CASES:
        for k, v in _ln_units(M, C, mr).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("r32 layernorm", {k: round(v, 2) for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= pw.R32_LAYERNORM[k], (k, v)


# defect -> the scale activations it applies to
ADAPTER_MUTANTS = {"clamp_grad": ("softplus", "exp"),       # the scale derivative not zeroed past the 0.3 clamp
                   "kp0": None,                             # k'(d) = 0
                   "no_proj": None,                         # quaternion gradient without - q (q . dq)
                   "no_two_s": None,                        # ... without the two_s term (shows where the norm is clamped: |qr| = 4e-13)
                   "rsr": None,                             # R S R^T instead of R S^2 R^T
                   "mask_c": None,                          # SH mask indexed by c (clamped to the table) instead of c % d_sh
                   "k_f16": None}                           # k = expm1(d) / d rounded to f16


@pytest.mark.parametrize("exponent", [1.0, 2.0, -1.0])
@pytest.mark.parametrize("act,smin,smax", ACTS)
def test_adapter_mutants_fail_the_gpu_criterion(act, smin, smax, exponent):
    clean = _adapter_units(act, smin, smax, exponent, B=True)
    assert max(clean.values()) <= 1.0, clean
    seen = {}
    for mut, acts in ADAPTER_MUTANTS.items():
        if acts is not None and act not in acts:
            continue
        r = _adapter_units(act, smin, smax, exponent, mutate=mut, B=True)
        seen[mut] = max(r.values())
        assert seen[mut] > 1.0, (mut, r)
    print(act, exponent, {k: f"{v:.3g}x" for k, v in seen.items()})


LN_MUTANTS = ("var_ex2",          # variance as E[x^2] - mean^2 in f32
              "no_xhat_term",     # dx without mean(dy xhat) xhat
              "dscale_wave8")     # dscale summed into the group of the first of 8 rows


@pytest.mark.parametrize("M,C,mod_rows", [(33, 1024, 5), (9, 768, 3), (33, 192, 9)])
def test_layernorm_mutants_fail_the_gpu_criterion(M, C, mod_rows):
    clean = _ln_units(M, C, mod_rows, B=True)
    assert max(clean.values()) <= 1.0, clean
    seen = {}
    for mut in LN_MUTANTS:
        r = _ln_units(M, C, mod_rows, mutate=mut, B=True)
        seen[mut] = max(r.values())
        assert seen[mut] > 1.0, (mut, r)
    print(M, C, mod_rows, {k: f"{v:.3g}x" for k, v in seen.items()})
