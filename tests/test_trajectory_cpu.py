"""The trajectory metrics (ATE / RPE-trans / RPE-rot, src/evaluation/metrics.py:148-265) on the CPU: the float64 restatement of
tests/trajectory_f64.py against closed forms, invariances and planted defects; callers.camera_eval_metrics(backend="torch") against it;
the binding of vsm_trajectory_metrics and its argument checks; the control flow of callers.test_step and callers.pose_eval_step with a stub
encoder and decoder.  UNVERIFIED against evo (not available offline): what is pinned here is the algorithm as include/vicasplat_metrics.h
states it.

Units are those of trajectory_f64 (2^-52 mag per output).  Measured here (`-s` prints them):
  closed-form square: restatement and torch backend 0 units from sqrt(2/3), sqrt(20)/3, 0; d = (1, 1, 0), R = I, c = 2/3 exactly.
  exact similarity: all three metrics <= 0.81 units (offsets of 1e3: <= 0.44; estimate bit-equal to the truth: <= 0.51), against the 4
  allowed; a similarity applied to either trajectory moves the metrics by <= 1.1 units.
  permutation spread (R64, per output): ate 0.617, rpe_trans 0.577, rpe_rot 0.279, R 8.881, t 1.928, c 3.365.
  torch backend against the restatement: ate 0.36, rpe_trans 0.29, rpe_rot 0.14 units.
  Rotation round trip.  The reference passes every rotation block through scipy's quaternion and back (c2w_to_tumpose,
  metrics.py:148-161), which also re-orthonormalises it; this package uses the blocks as given.  On f32-rounded rotations that moves
  rpe_trans by at most 6.7e-8 of its value and rpe_rot by at most 1.0e-6 degrees -- the f32 rounding of the rotations itself, which
  the round trip projects away --, on float64 rotations by 1.4e-15 and 2.8e-14 degrees; ATE reads no rotation and does not move.  A
  stated deviation, measured, not a bound.
  A general collinear trajectory (not on a coordinate axis) sits inside the ambiguity band of the absolute rank test: numpy gave
  d_2 = 4e-16 > 2^-52 for one.  Documented, not tested; every degenerate case here has d_2 = 0 exactly, V < 3, delta >= V or a non-finite
  element, and every other case d_2 >= 1e-6 d_1 and d_2 + d_3 >= 0.1 d_1 (asserted below on the restatement itself).
"""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import trajectory_f64 as T

VS = (3, 4, 8, 9, 64, 65, 130)


def _all_cases():
    for V in VS:
        for name, (P, Q) in T.families(V).items():
            yield f"{name}_V{V}", P, Q


CASES = list(_all_cases())


def _torch_backend(P, Q, **kw):
    from vicasplat_amd import callers
    out = callers.camera_eval_metrics(torch.tensor(P), torch.tensor(Q), backend="torch", return_valid=True, **kw)
    assert all(isinstance(o, torch.Tensor) for o in out) and all(o.dtype == torch.float64 for o in out[:3]) and out[3].dtype == torch.bool
    return np.stack([o.numpy() for o in out[:3]], -1), out[3].numpy()


def test_closed_form_square():
    P, Q = T.square_case()
    out, valid, (R, t, c), d, mag = T.metrics(P, Q)
    assert valid == 1 and tuple(d) == T.SQUARE["d"] and np.array_equal(R, np.eye(3)) and c == T.SQUARE["c"] and not t.any()
    got_t, valid_t = _torch_backend(P, Q)
    assert valid_t
    for name, got in (("restatement", out), ("torch", got_t)):
        u = [T.units(got[k], T.SQUARE["out"][k], mag[k]) for k in range(3)]
        print(f"square {name}: units {u}")
        assert max(u) <= 4.0, (name, u)


def test_conditions_hold_on_every_case():
    """Non-degenerate cases: d_2 >= 1e-6 d_1 and d_2 + d_3 >= 0.1 d_1, also after rounding the poses to f32; degenerate ones: d_2 = 0 exactly,
    V < 3, delta >= V or a non-finite element.  No case is excluded from any comparison."""
    for tag, P, Q in CASES:
        for cast in (np.float64, np.float32):
            assert T.well_posed(T.metrics(P.astype(cast), Q.astype(cast))), tag
    for V in (1, 2) + VS:
        for name, (P, Q) in T.degenerate_families(V).items():
            ref = T.metrics(P, Q)
            finite = bool(np.isfinite(P).all() and np.isfinite(Q).all())
            assert T.plainly_degenerate(ref, V, 1, finite), (name, V, ref[3])
            assert not ref[0].any() and np.array_equal(ref[2][0], np.eye(3)) and not ref[2][1].any() and ref[2][2] == 1.0
        if V >= 3:
            P, Q = T.families(V)["walk"]
            assert T.plainly_degenerate(T.metrics(P, Q, delta=V), V, V) and T.metrics(P, Q, delta=V - 1)[1] == 1


# the rounding of applying a similarity to the inputs moves every position and rotation entry by a few units; the alignment's condition (at
# most 5 on these cases) and the dozen operations behind an output carry that to the output: 4 x 5 x 12 = 240 -> 256 units
PROPERTY_UNITS = 256.0


def test_similarity_properties():
    g = np.random.default_rng(5)
    worst = 0.0
    for tag, P, Q in CASES:
        ref = T.metrics(P, Q)
        s, R0, t0 = float(g.uniform(0.5, 2.0)), T._rot(g.normal(size=3)), g.normal(size=3)
        moved = T.metrics(T.similarity(P, s, R0, t0), Q)          # a similarity of the estimate changes nothing
        # ... of the truth scales ATE and RPE-trans by s and leaves RPE-rot alone
        scaled = T.metrics(P, T.similarity(Q, s, R0, t0))
        for k in range(3):
            u1 = T.units(moved[0][k], ref[0][k], ref[4][k])
            u2 = T.units(scaled[0][k], ref[0][k] * (s if k < 2 else 1.0), scaled[4][k])
            worst = max(worst, u1, u2)
            assert u1 <= PROPERTY_UNITS and u2 <= PROPERTY_UNITS, (tag, k, u1, u2)
    print(f"similarity properties: worst {worst:.1f} units")


def test_exact_similarity_gives_zero():
    worst = {}
    for V in VS:
        fam = T.families(V)
        for name in ("exact", "exact_far", "identical"):
            out, valid, _, _, mag = T.metrics(*fam[name])
            u = float((out / (T.EPS * mag)).max())
            worst[name] = max(worst.get(name, 0.0), u)
            assert valid == 1 and u <= 4.0, (name, V, out / (T.EPS * mag))
            got, _ = _torch_backend(*fam[name])
            assert float((got / (T.EPS * mag)).max()) <= 4.0, (name, V, got / (T.EPS * mag))
    print("exact similarity, units:", {k: round(v, 2) for k, v in worst.items()})


def test_reflection_takes_the_rotation_branch():
    for V in VS[1:]:
        P, Q = T.families(V)["reflection"]
        out, valid, (R, t, c), d, mag = T.metrics(P, Q)
        assert valid == 1 and np.linalg.det(R) > 0.5 and out[0] > 1e-3 * mag[0] and out[2] <= 4.0 * T.EPS * mag[2], (V, out)
        got, _ = _torch_backend(P, Q)
        assert got[2] <= 4.0 * T.EPS * mag[2] and T.units(got[0], out[0], mag[0]) <= PROPERTY_UNITS


def test_degenerate_scenes_and_the_batch_around_them():
    for V in (1, 2, 3, 8):
        for name, (P, Q) in T.degenerate_families(V).items():
            got, valid = _torch_backend(P, Q)
            assert not valid and not got.any(), (name, V)
    # a NaN scene inside a batch: the others keep their bits
    fam, bad = T.families(8), T.degenerate_families(8)
    names = ["walk", "nan", "planar", "axis", "reflection"]
    Pb = np.stack([(fam[n] if n in fam else bad[n])[0] for n in names])
    Qb = np.stack([(fam[n] if n in fam else bad[n])[1] for n in names])
    got, valid = _torch_backend(Pb, Qb)
    assert valid.tolist() == [True, False, True, False, True] and not got[1].any() and not got[3].any()
    for k in (0, 2, 4):
        alone, _ = _torch_backend(Pb[k], Qb[k])
        assert np.array_equal(alone, got[k]), names[k]
    ref = T.metrics_batch(Pb, Qb)
    assert ref["valid"].tolist() == [1, 0, 1, 0, 1]
    # delta >= V
    P, Q = fam["walk"]
    assert T.metrics(P, Q, delta=8)[1] == 0 and T.metrics(P, Q, delta=7)[1] == 1


def test_torch_backend_matches_the_restatement():
    worst = np.zeros(3)
    for tag, P, Q in CASES:
        ref = T.metrics(P, Q)
        got, valid = _torch_backend(P, Q)
        assert valid
        u = np.abs(got - ref[0]) / (T.EPS * ref[4])
        worst = np.maximum(worst, u)
        assert u.max() <= PROPERTY_UNITS, (tag, u)       # plain float64 sums and torch's own SVD: not the kernel's bound
    print("torch backend against the restatement, units:", dict(zip(T.NAMES, worst.round(2))))
    # sample_stride keeps every other pose; a batch equals its scenes
    P, Q = T.families(9)["walk"]
    a, _ = _torch_backend(P, Q, sample_stride=2)
    b, _ = _torch_backend(P[::2], Q[::2])
    assert np.array_equal(a, b) and not np.array_equal(a, _torch_backend(P, Q)[0])
    f32, _ = _torch_backend(P.astype(np.float32), Q.astype(np.float32))
    assert np.abs(f32 - T.metrics(P.astype(np.float32), Q.astype(np.float32))[0]).max() <= PROPERTY_UNITS * T.EPS * T.metrics(P, Q)[4].max()


def test_permutation_spread_is_within_r64():
    worst = dict.fromkeys(T.OUTPUTS, 0.0)
    for tag, P, Q in CASES:
        s = T.permutation_spread(P, Q)
        worst = {k: max(worst[k], s[k]) for k in T.OUTPUTS}
    print("permutation spread (R64), units:", {k: round(v, 3) for k, v in worst.items()})
    for k in T.OUTPUTS:
        assert worst[k] <= T.R64[k], (k, worst[k])


def test_mutants_are_far_outside_the_gpu_bound():
    """Every planted defect moves some metric on some case by >= 1e3 x the GPU bound; the acos angle exceeds the bound where the estimate equals
    the truth."""
    moved, acos_at_match = dict.fromkeys(T.MUTANTS, 0.0), 0.0
    for tag, P, Q in CASES:
        if "_V130" in tag or "_V65" in tag:
            continue
        for delta in (1, 3):
            if delta >= P.shape[0]:
                continue
            ref = T.metrics(P, Q, delta)
            for m in T.MUTANTS:
                got = T.metrics(P, Q, delta, mutant=m)
                r = max(T.units(got[0][k], ref[0][k], ref[4][k]) / T.gpu_factor(n) for k, n in enumerate(T.NAMES))
                moved[m] = max(moved[m], r)
                if m == "acos" and tag.startswith(("identical", "exact")):
                    acos_at_match = max(acos_at_match, r)
    print("mutants, in GPU bounds:", {k: f"{v:.3g}" for k, v in moved.items()}, f"; acos where the estimate matches: {acos_at_match:.3g}")
    assert acos_at_match > 1.0
    for m in T.MUTANTS:
        assert moved[m] >= 1e3, (m, moved[m])


def test_quaternion_round_trip_is_measured():
    """What the reference's scipy round trip of every rotation block (metrics.py:148-161) moves: printed, recorded in this file's docstring
    and in DESIGN.md; asserted only to stay the small effect it is documented as (the f32 rounding of a rotation is 6e-8)."""
    from scipy.spatial.transform import Rotation

    def round_trip(P):
        out = P.copy()
        q = Rotation.from_matrix(P[:, :3, :3]).as_quat()
        out[:, :3, :3] = Rotation.from_quat(q).as_matrix()
        return out

    worst = {"f32": np.zeros(3), "f64": np.zeros(3)}
    for tag, P, Q in CASES:
        if not tag.startswith(("walk", "planar")):
            continue
        for key, cast in (("f32", np.float32), ("f64", np.float64)):
            p, q = P.astype(cast).astype(np.float64), Q.astype(cast).astype(np.float64)
            ref, got = T.metrics(p, q)[0], T.metrics(round_trip(p), round_trip(q))[0]
            rel = np.abs(got - ref) / np.array([ref[0], ref[1], 1.0])       # rpe_rot: absolute, in degrees
            worst[key] = np.maximum(worst[key], rel)
    print("quaternion round trip (ate rel, rpe_trans rel, rpe_rot deg):", {k: [f"{x:.2g}" for x in v] for k, v in worst.items()})
    assert worst["f32"].max() < 1e-4 and worst["f64"].max() < 1e-10


def test_entry_is_bound_from_the_fifth_header_and_checks_its_arguments():
    from vicasplat_amd import _lib
    inc = os.path.join(os.path.dirname(__file__), "..", "include")
    text = open(os.path.join(inc, "vicasplat_metrics.h")).read()
    sigs = _lib.parse_header(text, prefix="vsm_")
    assert set(sigs) == {"vsm_trajectory_metrics"}
    restype, argtypes, takes_stream = sigs["vsm_trajectory_metrics"]
    i32, vp = C.c_int32, C.c_void_p
    assert restype is C.c_int and argtypes == [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp] and takes_stream
    L = _lib.lib()
    p = C.c_void_p(16)
    err = lambda: L.vs_last_error()
    # every refusal comes before any HIP call: there is no device here
    assert L.vsm_trajectory_metrics(None, p, 5, 1, 8, 1, p, p, None, None) < 0 and b"vsm_trajectory_metrics: null pointer" in err()
    assert L.vsm_trajectory_metrics(p, None, 5, 1, 8, 1, p, p, None, None) < 0 and b"null pointer" in err()
    assert L.vsm_trajectory_metrics(p, p, 5, 1, 8, 1, None, p, None, None) < 0 and b"null pointer" in err()
    assert L.vsm_trajectory_metrics(p, p, 5, 1, 8, 1, p, None, None, None) < 0 and b"null pointer" in err()
    assert L.vsm_trajectory_metrics(p, p, 1, 1, 8, 1, p, p, None, None) < 0 and b"dtype 1" in err()      # f16's code is refused, not misread
    assert L.vsm_trajectory_metrics(p, p, 0, -1, 8, 1, p, p, None, None) < 0 and b"B = -1" in err()
    assert L.vsm_trajectory_metrics(p, p, 0, 1, 0, 1, p, p, None, None) < 0 and b"V = 0" in err()
    assert L.vsm_trajectory_metrics(p, p, 0, 1, 8, 0, p, p, None, None) < 0 and b"delta = 0" in err()
    assert L.vsm_trajectory_metrics(p, p, 0, 0, 8, 1, p, p, None, None) == 0          # B = 0: nothing to do, nothing launched


def test_wrappers_refuse_what_they_cannot_take():
    from vicasplat_amd import callers, ops
    P = torch.eye(4).repeat(2, 5, 1, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.trajectory_metrics(P, P)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        callers.camera_eval_metrics(P, P, backend="hip")
    with pytest.raises(ValueError, match="backend"):
        callers.camera_eval_metrics(P, P, backend="evo")
    with pytest.raises(ValueError, match="one shape"):
        callers.camera_eval_metrics(P, P[:, :4])
    with pytest.raises(ValueError, match="one shape"):
        callers.camera_eval_metrics(P[..., :3, :], P[..., :3, :])
    with pytest.raises(ValueError, match="sample_stride"):
        callers.camera_eval_metrics(P, P, 0)
    ate, rt, rr = callers.camera_eval_metrics(P[0], P[0])          # [V, 4, 4]: 0-d tensors; coincident positions: zeros
    assert ate.shape == rt.shape == rr.shape == () and ate.dtype == torch.float64 and float(ate) == 0.0


# ---- the control flow of test_step / pose_eval_step with a stub encoder and decoder ----
def _stub_batch(B=3, V=5, Vt=2, S=12, seed=0):
    g = torch.Generator().manual_seed(seed)
    fam = [T.walk_case(V, 40 + b) for b in range(B)]
    pred = torch.tensor(np.stack([f[0] for f in fam]), dtype=torch.float32)
    gt = torch.tensor(np.stack([f[1] for f in fam]), dtype=torch.float32)
    ctx = dict(image=torch.rand(B, V, 3, S, S, generator=g) * 2 - 1, intrinsics=torch.eye(3).repeat(B, V, 1, 1), extrinsics=gt,
               near=torch.full((B, V), 0.1), far=torch.full((B, V), 100.0))
    tgt = dict(image=torch.rand(B, Vt, 3, S, S, generator=g), extrinsics=torch.eye(4).repeat(B, Vt, 1, 1), intrinsics=torch.eye(3).repeat(B, Vt, 1, 1),
               near=torch.full((B, Vt), 0.1), far=torch.full((B, Vt), 100.0))
    return dict(context=ctx, target=tgt), pred


class _StubDecoder:
    """Renders a constant image whose level is the mean translation of its cameras: tells which extrinsics it was given."""

    def __init__(self):
        self.seen = []

    def forward(self, gaussians, extrinsics, intrinsics, near, far, image_shape, **kw):
        self.seen.append(extrinsics.detach().clone())
        b, v = extrinsics.shape[:2]
        level = extrinsics[..., :3, 3].mean(-1).clamp(0, 1)
        return types.SimpleNamespace(color=level[..., None, None, None].expand(b, v, 3, *image_shape).clone())


def _stub_encoder(pred, calls):
    from vicasplat_amd.model.types import Gaussians

    def encoder(ctx):
        assert not torch.is_grad_enabled()
        calls.append(ctx)
        z = torch.zeros(pred.shape[0], 1)
        return dict(gaussians=Gaussians(z, z, z, z), gaussian_camera_extrins=pred)
    return encoder


def test_test_step_control_flow(monkeypatch):
    from vicasplat_amd import callers
    batch, pred = _stub_batch()
    B, Vt = batch["target"]["image"].shape[:2]
    monkeypatch.setattr(callers, "compute_ssim", lambda gt, pr: 1 - (gt - pr).abs().flatten(1).mean(1))      # the SSIM kernels need a device
    calls, dec = [], _StubDecoder()
    out = callers.test_step(_stub_encoder(pred, calls), dec, batch)
    assert list(out) == ["psnr_ours", "ssim_ours", "ate_ours", "rpe-trans_ours", "rpe-rot_ours", "pose_valid"] and len(calls) == 1
    assert all(isinstance(v, torch.Tensor) and v.shape == (B,) for v in out.values())
    assert out["ate_ours"].dtype == torch.float64 and out["pose_valid"].dtype == torch.bool and bool(out["pose_valid"].all())
    ref = T.metrics_batch(pred.double().numpy(), batch["context"]["extrinsics"].double().numpy())
    got = np.stack([out[k].numpy() for k in ("ate_ours", "rpe-trans_ours", "rpe-rot_ours")], -1)
    assert (np.abs(got - ref["out"]) <= PROPERTY_UNITS * T.EPS * ref["mag"]).all()
    assert len(dec.seen) == 1 and torch.equal(dec.seen[0], batch["target"]["extrinsics"])
    psnr = callers.compute_psnr(batch["target"]["image"].flatten(0, 1), torch.zeros_like(batch["target"]["image"]).flatten(0, 1))
    assert torch.allclose(out["psnr_ours"], psnr.unflatten(0, (B, Vt)).mean(1))
    # with a net: the key appears, per scene
    net = lambda a, b, normalize=False: (a - b).abs().flatten(1).mean(1).reshape(-1, 1, 1, 1)
    out = callers.test_step(_stub_encoder(pred, calls), dec, batch, lpips_net=net)
    assert "lpips_ours" in out and out["lpips_ours"].shape == (B,) and list(out).index("lpips_ours") == 2
    # align_pose routes through align_poses, and the render uses what it returned
    seen = {}

    def fake_align(decoder, gaussians, target_image, extrinsics, intrinsics, near, far, **kw):
        seen.update(kw, target=target_image, start=extrinsics)
        moved = extrinsics.clone()
        moved[..., :3, 3] += 0.25
        return moved
    monkeypatch.setattr(callers, "align_poses", fake_align)
    dec = _StubDecoder()
    out2 = callers.test_step(_stub_encoder(pred, calls), dec, batch, align_pose=True, align_kwargs=dict(steps=7))
    assert seen["steps"] == 7 and seen["target"] is batch["target"]["image"] and torch.equal(seen["start"], batch["target"]["extrinsics"])
    assert len(dec.seen) == 1 and torch.equal(dec.seen[0][..., :3, 3], batch["target"]["extrinsics"][..., :3, 3] + 0.25)
    assert not torch.equal(out2["psnr_ours"], out["psnr_ours"]) and torch.equal(out2["ate_ours"], out["ate_ours"])
    # a scene the reference's `except` would zero: flagged, zeros, the others untouched
    batch["context"]["extrinsics"] = batch["context"]["extrinsics"].clone()
    batch["context"]["extrinsics"][1, :, :3, 3] = 0.0
    out3 = callers.test_step(_stub_encoder(pred, calls), _StubDecoder(), batch)
    assert out3["pose_valid"].tolist() == [True, False, True] and float(out3["ate_ours"][1]) == 0.0
    assert torch.equal(out3["ate_ours"][[0, 2]], out["ate_ours"][[0, 2]])


def test_pose_eval_step_control_flow(monkeypatch):
    from vicasplat_amd import callers
    batch, pred = _stub_batch(B=2, V=6)
    gt = batch["context"]["extrinsics"]
    calls, dec = [], _StubDecoder()
    out = callers.pose_eval_step(_stub_encoder(pred, calls), dec, batch)          # steps = 0, as the reference ships it: nothing refined
    keys = [f"{n}_{w}_opt" for w in ("after", "before") for n in ("ate", "rpe_trans", "rpe_rot", "pose_valid")]
    assert list(out) == keys and all(v.shape == (2,) for v in out.values()) and not dec.seen
    before = T.metrics_batch(pred.double().numpy(), gt.double().numpy())
    mixed = torch.cat([gt[:, :1], pred[:, 1:]], 1)          # the true first pose in front of the predicted others
    after = T.metrics_batch(mixed.double().numpy(), gt.double().numpy())
    for w, ref in (("before", before), ("after", after)):
        got = np.stack([out[f"{n}_{w}_opt"].numpy() for n in ("ate", "rpe_trans", "rpe_rot")], -1)
        assert (np.abs(got - ref["out"]) <= PROPERTY_UNITS * T.EPS * ref["mag"]).all(), w
    assert not torch.equal(out["ate_after_opt"], out["ate_before_opt"])
    seen = {}

    def fake_align(decoder, gaussians, target_image, extrinsics, intrinsics, near, far, **kw):
        seen.update(kw, target=target_image, start=extrinsics, K=intrinsics)
        return gt[:, 1:].clone()          # a perfect refinement
    monkeypatch.setattr(callers, "align_poses", fake_align)
    out = callers.pose_eval_step(_stub_encoder(pred, calls), dec, batch, steps=3, sample_stride=2)
    assert seen["steps"] == 3 and seen["ssim_structure_weight"] == 1.0 and seen["K"].shape[1] == 5      # the SSIM structure term is on
    assert torch.equal(seen["target"], batch["context"]["image"][:, 1:] * 0.5 + 0.5) and torch.equal(seen["start"], pred[:, 1:])
    assert float(out["ate_after_opt"].max()) < 1e-13 and bool(out["pose_valid_after_opt"].all()) and float(out["ate_before_opt"].min()) > 0
    strided = T.metrics_batch(pred.double().numpy()[:, ::2], gt.double().numpy()[:, ::2])
    assert (np.abs(out["ate_before_opt"].numpy() - strided["out"][:, 0]) <= PROPERTY_UNITS * T.EPS * strided["mag"][:, 0]).all()
