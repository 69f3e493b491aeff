"""The visualisation step on the CPU: the float64 restatement of tests/viz_f64.py against the reference's own results
(tests/golden/viz.npz, written by tests/golden/gen_viz_golden.py) and against torch.quantile; the colour tables; the binding of the vsv_
entries and their refusals; the control flow of callers.validation_step and callers.render_video_generic on stubs; planted defects against
the criteria tests/test_viz_gpu.py applies; the reference's own f32 gap; the exclusion cap of the index band.

Measured here (`-s` prints them), in units of 2^-24 mag:
  reference f32 against float64: near 0.450 / 0.620 / 0.122, far 0.334 / 0.221 / 0.052, x 0.812 / 0.621 / 0.943 (room / wide / narrow).
  band of the index at K = 4: 0.13 % / 0.20 % / 0 % of the 1536 pixels, at three times the width 0.20 % / 0.20 % / 0.13 %; cap 0.5 %.
"""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import viz_f64 as V

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "viz.npz"))
CASES = tuple(V.DEPTH_CASES)


# ---- 1. restatement against the golden ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_range_and_index_against_golden(case):
    d = GOLDEN[f"depth_{case}"]
    ref = V.depth_range(d)
    print(case, "near", V.units(GOLDEN[f"near_{case}"], ref["near"], ref["mag_near"]), "far", V.units(GOLDEN[f"far_{case}"], ref["far"], ref["mag_far"]))
    assert V.range_ok(GOLDEN[f"near_{case}"], GOLDEN[f"far_{case}"], ref)
    err = (V.K * V.EPS * ref["mag_near"], V.K * V.EPS * ref["mag_far"])
    x, bound = V.x_depth(d, ref["near"], ref["far"], range_err=err)
    idx_ref = V.index_of(GOLDEN[f"x_{case}"])          # the reference's own index: x * 256 is exact in f32
    assert V.index_ok(idx_ref, x, bound)
    if case == "room":
        assert d.min() < 0 and (d == 0).any() and (idx_ref == -1).sum() == 1 and (idx_ref[d == 0] == 255).all()
        assert np.array_equal(V.lookup(idx_ref, GOLDEN["turbo"]), GOLDEN["vis_room"])


def test_confidence_against_golden():
    x, bound = V.x_max(GOLDEN["conf"])
    idx_ref = V.index_of(GOLDEN["x_conf"])
    assert V.index_ok(idx_ref, x, bound) and idx_ref.max() == 255
    assert np.array_equal(V.lookup(idx_ref, GOLDEN["magma"]), GOLDEN["vis_conf"])


def test_layouts_and_frames_against_golden():
    a, b, c = GOLDEN["lay_a"], GOLDEN["lay_b"], GOLDEN["lay_c"]
    assert np.array_equal(V.vcat(a, b, c), GOLDEN["lay_vcat"])
    assert np.array_equal(V.vcat(a, b, c, align="end", gap=0), GOLDEN["lay_vcat_right_nogap"])
    assert np.array_equal(V.hcat(a, b, c, align="center", gap=3, gap_color=[0.25, 0.5, 0.75]), GOLDEN["lay_hcat_center"])
    assert np.array_equal(V.hcat(a, b, align="end", gap=1, gap_color=0.0), GOLDEN["lay_hcat_bottom"])
    assert np.array_equal(V.add_border(a, 2, 0.5), GOLDEN["lay_border"])
    rgb, col = GOLDEN["fr_rgb"], GOLDEN["fr_col"]
    M, _, H, W = rgb.shape
    fr = np.full((M, 3, 2 * H + 8, W), 255, np.uint8)
    fr[:, :, :H], fr[:, :, H + 8:] = V.to_u8(rgb), V.to_u8(col)
    assert np.array_equal(fr, GOLDEN["fr_u8"]) and np.array_equal(V.loop_reverse(fr), GOLDEN["fr_loop"])
    assert GOLDEN["fr_loop"].shape[0] == 2 * M - 2


def test_package_layout_against_golden():
    from vicasplat_amd.visualization import layout
    a, b, c = (torch.tensor(GOLDEN[k]) for k in ("lay_a", "lay_b", "lay_c"))
    assert np.array_equal(layout.vcat(a, b, c).numpy(), GOLDEN["lay_vcat"])
    assert np.array_equal(layout.vcat(a, b, c, align="right", gap=0).numpy(), GOLDEN["lay_vcat_right_nogap"])
    assert np.array_equal(layout.hcat(a, b, c, align="center", gap=3, gap_color=[0.25, 0.5, 0.75]).numpy(), GOLDEN["lay_hcat_center"])
    assert np.array_equal(layout.hcat(a, b, align="bottom", gap=1, gap_color=0).numpy(), GOLDEN["lay_hcat_bottom"])
    assert np.array_equal(layout.add_border(a, 2, 0.5).numpy(), GOLDEN["lay_border"])


def test_aabb_and_orthographic_setup_against_golden():
    from vicasplat_amd.visualization.validation_in_3d import compute_equal_aabb_with_margin
    lo, hi = V.equal_aabb_with_margin(GOLDEN["aabb_min_in"], GOLDEN["aabb_max_in"])
    assert np.abs(lo - GOLDEN["aabb_min"]).max() <= 8 * V.EPS * 4 and np.abs(hi - GOLDEN["aabb_max"]).max() <= 8 * V.EPS * 4
    got = compute_equal_aabb_with_margin(torch.tensor(GOLDEN["aabb_min_in"]), torch.tensor(GOLDEN["aabb_max_in"]))
    assert np.array_equal(got[0].numpy(), GOLDEN["aabb_min"]) and np.array_equal(got[1].numpy(), GOLDEN["aabb_max"])
    E, w, h, near, far = V.projection_cameras(GOLDEN["aabb_min"][:1], GOLDEN["aabb_max"][:1], look_axis=1)
    assert np.array_equal(E.astype(np.float32), GOLDEN["ortho_extrinsics_in"])
    s = V.orthographic_setup(E, w, h, near, far, fov_degrees=float(GOLDEN["ortho_fov_degrees"]))
    for k in ("extrinsics", "fov_x", "fov_y", "near", "far"):
        scale = max(1.0, float(np.abs(s[k]).max()))
        assert np.abs(np.asarray(s[k]) - GOLDEN[f"ortho_{k}"]).max() <= 16 * V.EPS * scale, k


# ---- 2. restatement against torch.quantile -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 2, 3, 101, 65537))
def test_quantile_against_torch(n):
    v = np.random.default_rng(n).lognormal(0.0, 2.0, n).astype(np.float32)
    v[::7] *= -1
    for q in (V.Q_NEAR, V.Q_FAR):
        Q, (a, b), mag = V.quantile(v, q)
        t = torch.quantile(torch.tensor(v), float(q))
        assert t.dtype == torch.float32 and abs(float(t) - Q) <= 2 * V.EPS * mag, (n, q, float(t), Q)
        s = np.sort(v)
        lo, hi, w = V.rank_f32(q, n)
        assert a == s[lo] and b == s[hi] and 0 <= lo <= hi <= n - 1
        assert np.float32(V.lerp(np.float32(a), np.float32(b), np.float32(w))) == np.float32(t) or abs(float(t) - Q) <= V.EPS * mag


def test_quantile_at_the_rank_rounding():
    """At the first size where f32(0.99) * f32(m - 1), rounded to f32, and the float64 product have different floors, torch follows the f32 one."""
    m = V.rank_rounding_size()
    v = np.arange(m, dtype=np.float32)
    np.random.default_rng(0).shuffle(v)
    lo, hi, w = V.rank_f32(V.Q_FAR, m)
    assert float(torch.quantile(torch.tensor(v), float(V.Q_FAR))) == V.lerp(float(lo), float(hi), w) != V.quantile(v, V.Q_FAR, rank_f64=True)[0]


# ---- 3. tables ------------------------------------------------------------------------------------------------------------------------
def test_tables():
    from vicasplat_amd.visualization import color_map
    for name in ("turbo", "magma"):
        t = color_map.color_table(name)
        assert t.dtype == np.float32 and t.shape == (256, 3) and np.array_equal(t, GOLDEN[name])
    with pytest.raises(NotImplementedError, match="turbo.*magma"):
        color_map.color_table("inferno")
    with pytest.raises(NotImplementedError, match="turbo.*magma"):
        color_map.apply_color_map_to_image(torch.zeros(2, 2))
    try:
        import matplotlib
    except ImportError:
        return
    for name in ("turbo", "magma"):
        assert np.array_equal(color_map.color_table(name), np.float32(matplotlib.colormaps[name](np.arange(256))[:, :3]))
    x = np.random.default_rng(0).uniform(-0.1, 1.1, 4096).astype(np.float32)      # matplotlib's call is the lookup the kernels restate
    want = np.float32(matplotlib.colormaps["turbo"](np.clip(x, 0, 1))[:, :3])
    assert np.array_equal(V.lookup(V.index_of(x)[None], GOLDEN["turbo"])[:, 0].T, want)


# ---- 4. binding -----------------------------------------------------------------------------------------------------------------------
def test_binding_and_refusals():
    from vicasplat_amd import _lib
    with open(_lib.header_path("vsv_")) as f:
        sigs = _lib.parse_header(f.read(), prefix="vsv_")
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert sigs == {
        "vsv_depth_range_workspace_bytes": (i64, [i64], False),
        "vsv_depth_range": (C.c_int, [vp, i64, vp, vp, vp, i64, vp], True),
        "vsv_color_map_workspace_bytes": (i64, [i32], False),
        "vsv_color_map": (C.c_int, [vp, i32, i32, i32, i32, vp, vp, vp, i32, vp, i64, vp], True),
        "vsv_video_frames": (C.c_int, [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp], True)}
    L = _lib.lib()
    assert (_lib.VSV_THREADS, _lib.VSV_VEC, _lib.VSV_MAX_RANGE_N) == (256, 4, V.MAX_RANGE_N) and _lib.VSV_MAX_BLOCKS >= 1
    assert (_lib.VSV_MODE_DEPTH, _lib.VSV_MODE_MAX, _lib.VSV_MODE_UNIT, _lib.VSV_OUT_F32, _lib.VSV_OUT_U8) == (0, 1, 2, 0, 1)
    p = C.c_void_p(4096)      # never dereferenced: every call below returns before any HIP call

    def refused(rc, text):
        assert rc < 0 and text in L.vs_last_error().decode(), (rc, L.vs_last_error())

    need = L.vsv_depth_range_workspace_bytes(100)
    assert need > 0 and need % 16 == 0 and L.vsv_depth_range_workspace_bytes(V.MAX_RANGE_N) == need
    refused(L.vsv_depth_range_workspace_bytes(V.MAX_RANGE_N + 1), "outside")
    refused(L.vsv_depth_range_workspace_bytes(-1), "outside")
    refused(L.vsv_depth_range(None, 8, p, None, p, need, None), "null pointer")
    refused(L.vsv_depth_range(p, 8, None, None, p, need, None), "null pointer")
    refused(L.vsv_depth_range(p, -1, p, None, p, need, None), "negative")
    refused(L.vsv_depth_range(p, V.MAX_RANGE_N + 1, p, None, p, need, None), "exceeds 16000000")
    refused(L.vsv_depth_range(p, 8, p, None, None, need, None), "null workspace")
    refused(L.vsv_depth_range(p, 8, p, None, p, need - 1, None), "bytes")
    refused(L.vsv_depth_range(p, 8, p, None, C.c_void_p(4100), need, None), "16-byte aligned")
    refused(L.vsv_depth_range(C.c_void_p(4098), 8, p, None, p, need, None), "4-byte aligned")
    assert L.vsv_depth_range(p, 0, p, None, p, need, None) == 0

    assert L.vsv_color_map_workspace_bytes(0) == 0 and L.vsv_color_map_workspace_bytes(2) == 0 and L.vsv_color_map_workspace_bytes(1) == 16
    refused(L.vsv_color_map_workspace_bytes(3), "unknown mode")
    refused(L.vsv_color_map(p, 1, 2, 2, 3, p, p, p, 0, None, 0, None), "unknown mode")
    refused(L.vsv_color_map(p, 1, 2, 2, 0, p, p, p, 2, None, 0, None), "unknown out_dtype")
    refused(L.vsv_color_map(None, 1, 2, 2, 0, p, p, p, 0, None, 0, None), "null pointer")
    refused(L.vsv_color_map(p, 1, 2, 2, 0, p, None, p, 0, None, 0, None), "null pointer")
    refused(L.vsv_color_map(p, 1, 2, 2, 0, p, p, None, 0, None, 0, None), "null pointer")
    refused(L.vsv_color_map(p, 1, 2, 2, 0, None, p, p, 0, None, 0, None), "null range")
    refused(L.vsv_color_map(p, 1, -2, 2, 0, p, p, p, 0, None, 0, None), "negative")
    refused(L.vsv_color_map(p, 1, 2, 2, 1, None, p, p, 0, None, 16, None), "null workspace")
    refused(L.vsv_color_map(p, 1, 2, 2, 1, None, p, p, 0, p, 15, None), "16 needed")
    refused(L.vsv_color_map(p, 1, 2, 2, 1, None, p, p, 0, C.c_void_p(4100), 16, None), "16-byte aligned")
    refused(L.vsv_color_map(p, 2 ** 15, 2 ** 10, 2 ** 6, 0, p, p, p, 0, None, 0, None), "exceed")
    assert L.vsv_color_map(p, 0, 2, 2, 0, p, p, p, 0, None, 0, None) == 0 and L.vsv_color_map(p, 3, 0, 2, 1, None, p, p, 1, p, 16, None) == 0

    refused(L.vsv_video_frames(None, p, 1, 2, 2, 8, p, p, p, None), "null pointer")
    refused(L.vsv_video_frames(p, p, 1, 2, 2, 8, p, p, None, None), "null pointer")
    refused(L.vsv_video_frames(p, p, 1, 2, 2, -1, p, p, p, None), "negative")
    refused(L.vsv_video_frames(p, p, -1, 2, 2, 8, p, p, p, None), "negative")
    refused(L.vsv_video_frames(C.c_void_p(4098), p, 1, 2, 2, 8, p, p, p, None), "4-byte aligned")
    refused(L.vsv_video_frames(p, p, 2 ** 12, 2 ** 10, 2 ** 10, 8, p, p, p, None), "exceed")
    big = 2 ** 31 - 1         # products of sizes near 2^31 must not wrap past the check
    for M, H, W, gap in ((big, big, big, big), (big, big, 4, 0), (4, big, big, 8), (big, 1, big, 0), (2 ** 30, 2 ** 30, 2 ** 4, 0)):
        refused(L.vsv_video_frames(p, p, M, H, W, gap, p, p, p, None), "exceed")
    refused(L.vsv_color_map(p, big, big, big, 0, p, p, p, 0, None, 0, None), "exceed")
    assert L.vsv_video_frames(p, p, 0, 2, 2, 8, p, p, p, None) == 0 and L.vsv_video_frames(p, p, 2, 0, 4, 0, p, p, p, None) == 0


# ---- 5. control flow -------------------------------------------------------------------------------------------------------------------
def _torch_vis(value):      # a stand-in for the colour-map kernels: grey of the value's rank in [0, 1]
    v = value.float()
    return ((v - v.min()) / (v.max() - v.min() + 1e-9)).unsqueeze(-3).expand(*v.shape[:-2], 3, *v.shape[-2:]).clone()


def _stub_world(monkeypatch, S=12, V_=2, Vt=3):
    from vicasplat_amd import callers, ops
    from vicasplat_amd.misc import utils
    from vicasplat_amd.model.types import Gaussians
    from vicasplat_amd.visualization import validation_in_3d
    g = torch.Generator().manual_seed(0)
    eye = torch.eye(4)
    ext = eye.repeat(1, V_, 1, 1).clone()
    ext[0, 1, 0, 3] = 1.0
    ctx = dict(image=torch.rand(1, V_, 3, S, S, generator=g) * 2 - 1, intrinsics=torch.eye(3).repeat(1, V_, 1, 1), extrinsics=ext,
               near=torch.tensor([[0.5, 0.7]]), far=torch.tensor([[50.0, 70.0]]))
    tgt = dict(image=torch.rand(1, Vt, 3, S, S, generator=g), extrinsics=eye.repeat(1, Vt, 1, 1), intrinsics=torch.eye(3).repeat(1, Vt, 1, 1),
               near=torch.full((1, Vt), 0.1), far=torch.full((1, Vt), 100.0))
    z = torch.zeros(1, 1)
    gauss = Gaussians(z, z, z, z)
    calls = dict(encoder=[], decoder=[])

    def encoder(c, **kw):
        assert not torch.is_grad_enabled()
        calls["encoder"].append(kw)
        return dict(gaussians=gauss, context_view_depths=torch.rand(1, V_, S, S, generator=g) + 0.5,
                    confidence=torch.rand(1, V_, S, S, generator=g) + 1 if kw.get("distill") else None)

    class Decoder:
        def forward(self, gaussians, extrinsics, intrinsics, near, far, image_shape, depth_mode=None, **kw):
            assert gaussians is gauss
            calls["decoder"].append(dict(extrinsics=extrinsics.clone(), near=near.clone(), far=far.clone(), depth_mode=depth_mode))
            b, v = extrinsics.shape[:2]
            level = torch.linspace(-0.25, 1.25, v)[None, :, None, None, None]      # frame f has its own level: the order shows in the video
            return types.SimpleNamespace(color=level.expand(b, v, 3, *image_shape).clone(), depth=1 + torch.rand(b, v, *image_shape, generator=g))

    monkeypatch.setattr(utils, "vis_depth_map", _torch_vis)
    monkeypatch.setattr(utils, "confidence_map", _torch_vis)
    monkeypatch.setattr(callers, "compute_ssim", lambda gt, pr: 1 - (gt - pr).abs().flatten(1).mean(1))
    monkeypatch.setattr(validation_in_3d, "render_projections", lambda gs, res, **kw: torch.rand(1, 3, 3, res, res, generator=g))
    monkeypatch.setattr(ops, "depth_range", lambda d: torch.tensor([0.0, 1.0]))

    def video_frames(rgb, depth, rng, lut, gap=8):      # the restatement's packing with the stand-in colours
        assert lut.shape == (256, 3) and depth.shape == rgb[:, 0].shape
        return torch.tensor(V.frames(rgb.numpy(), np.zeros(depth.shape, np.int32), V.ramp_lut(), gap))

    monkeypatch.setattr(ops, "video_frames", video_frames)
    return callers, dict(context=ctx, target=tgt), encoder, Decoder(), calls


def test_render_video_generic_control_flow(monkeypatch):
    callers, batch, encoder, decoder, calls = _stub_world(monkeypatch)
    seen = {}

    def trajectory_fn(t):
        seen["t"] = t.clone()
        return torch.eye(4).repeat(1, len(t), 1, 1), torch.eye(3).repeat(1, len(t), 1, 1)

    F, S = 5, 12
    video = callers.render_video_generic(encoder, decoder, batch, trajectory_fn, num_frames=F)
    lin = torch.linspace(0, 1, F)
    assert torch.equal(seen["t"], (torch.cos(torch.pi * (lin + 1)) + 1) / 2) and len(calls["encoder"]) == 1
    d = calls["decoder"][0]
    assert d["depth_mode"] == "depth" and torch.equal(d["near"], torch.full((1, F), 0.5)) and torch.equal(d["far"], torch.full((1, F), 50.0))
    assert video.dtype == torch.uint8 and video.shape == (2 * F - 2, 3, 2 * S + 8, S)
    levels = video[:, 0, 0, 0].tolist()
    want = [int(np.float32(min(max(x, 0.0), 1.0)) * np.float32(255)) for x in np.linspace(-0.25, 1.25, F, dtype=np.float32)]
    assert levels == want + want[::-1][1:-1] and (video[:, :, S:S + 8] == 255).all()
    plain = callers.render_video_generic(encoder, decoder, batch, trajectory_fn, num_frames=F, smooth=False, loop_reverse=False, save_depth=False)
    assert torch.equal(seen["t"], lin) and plain.shape == (F, 3, S, S) and plain[:, 0, 0, 0].tolist() == want
    # the interpolation step: from the first to the last context camera of scene 0
    video = callers.render_video_interpolation_step(encoder, decoder, batch, num_frames=4, smooth=False)
    E = calls["decoder"][-1]["extrinsics"]
    assert E.shape == (1, 4, 4, 4) and torch.allclose(E[0, 0], batch["context"]["extrinsics"][0, 0], atol=1e-6)
    assert torch.allclose(E[0, -1], batch["context"]["extrinsics"][0, -1], atol=1e-6) and video.shape[0] == 6


def test_validation_step_control_flow(monkeypatch):
    callers, batch, encoder, decoder, calls = _stub_world(monkeypatch)
    S, V_, Vt = 12, 2, 3
    out = callers.validation_step(encoder, decoder, batch)
    assert list(out) == ["psnr", "ssim", "comparison", "projections", "video"] and all(isinstance(v, torch.Tensor) for v in out.values())
    assert out["psnr"].shape == () and out["ssim"].shape == () and len(calls["encoder"]) == 1 and calls["encoder"][0]["compute_viewspace_depth"]
    col = lambda n: n * S + (n - 1) * 8
    assert out["comparison"].shape == (3, col(Vt), 5 * S + 4 * 8)       # columns: 2 of V_ images, 3 of Vt, top-aligned, white below
    assert (out["comparison"][:, col(V_):, :S] == 1).all() and torch.equal(out["comparison"][:, :S, :S], batch["context"]["image"][0, 0] * 0.5 + 0.5)
    assert out["projections"].shape == (3, 256, 3 * 256 + 16) and out["video"].shape == (58, 3, 2 * S + 8, S)
    out = callers.validation_step(encoder, decoder, batch, lpips_net=lambda a, b, normalize=False: (a - b).abs().flatten(1).mean(1).reshape(-1, 1, 1, 1),
                                  video=False, projections=False)
    assert list(out) == ["psnr", "ssim", "lpips", "comparison"]
    # distill-only: the teacher's depth (second view brought into its own camera) and confidence, then the prediction's
    pts = torch.rand(1, S, S, 3) + 1
    teacher = lambda ctx, flag: (dict(pts3d=pts, conf=pts[..., 0]), dict(pts3d=pts + batch["context"]["extrinsics"][:, 1, None, None, :3, 3], conf=pts[..., 1]))
    with pytest.raises(ValueError, match="distiller"):
        callers.validation_step(encoder, decoder, batch, distill_only=True)
    seen = []
    from vicasplat_amd.misc import utils
    monkeypatch.setattr(utils, "vis_depth_map", lambda v: (seen.append(v.clone()), _torch_vis(v))[1])
    out = callers.validation_step(encoder, decoder, batch, distiller=teacher, distill_only=True)
    assert list(out) == ["comparison"] and out["comparison"].shape == (3, col(2), 5 * S + 4 * 8) and calls["encoder"][-1]["distill"]
    assert seen[0].shape == (2, S, S) and torch.allclose(seen[0][0], pts[0, ..., 2]) and torch.allclose(seen[0][1], pts[0, ..., 2], atol=1e-6)


# ---- 6. planted defects -----------------------------------------------------------------------------------------------------------------
def test_planted_defects_are_rejected():
    """Each defect, run through the restatement, fails the criterion of tests/test_viz_gpu.py; the restatement itself passes it."""
    g = np.random.default_rng(1)
    # range
    ramp = V.rank_rounding_case()
    mixed = V.log_uniform((64, 64), 0.5, 50.0, seed=2, zeros=0.3)
    mixed[:8] *= -1
    zeros = np.zeros(100, np.float32)
    sparse = np.array([1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0], np.float32)
    for data, defect in ((ramp, dict(rank_f64=True)), (mixed, dict(far_positive_only=True)), (zeros, dict(no_fallback=True)), (sparse, dict(no_lerp=True))):
        ref, bad = V.depth_range(data), V.depth_range(data, **defect)
        assert V.range_ok(np.float32(ref["near"]), np.float32(ref["far"]), ref), defect
        assert not V.range_ok(np.float32(bad["near"]), np.float32(bad["far"]), ref), defect
    # index
    d = V.log_uniform((48, 64), 0.5, 50.0, seed=3)
    ref = V.depth_range(d)
    near, far = np.float32(ref["near"]), np.float32(ref["far"])
    x, bound = V.x_depth(d, near, far)
    assert V.index_ok(V.index_of(x), x, bound)
    assert not V.index_ok(V.index_of(x, scale=255.0), x, bound)
    assert not V.index_ok(V.index_of(x, rounding=True), x, bound)
    assert not V.index_ok(V.index_of(V.x_depth(d, near, far, no_one_minus=True)[0]), x, bound)
    # bytes and frames (bit-equal given the index), with the ramp table and one NaN depth
    lut = V.ramp_lut()
    rgb = g.uniform(-0.2, 1.2, (2, 3, 6, 8)).astype(np.float32)
    idx = g.integers(0, 256, (2, 6, 8)).astype(np.int32)
    idx[0, 0, 0] = -1
    want = V.frames(rgb, idx, lut, 8)
    assert want[0, :, 6 + 8, 0].tolist() == [0, 0, 0] and (want[:, :, 6:14] == 255).all()
    for defect in (dict(rounding=True), dict(gap_value=0), dict(nan_first_entry=True), dict(scale=256.0)):
        assert not np.array_equal(V.frames(rgb, idx, lut, 8, **defect), want), defect


# ---- 7. the reference's own f32 gap -------------------------------------------------------------------------------------------------------
def test_reference_f32_gap():
    worst_range = worst_x = 0.0
    for case in CASES:
        d = GOLDEN[f"depth_{case}"]
        ref = V.depth_range(d)
        u_near, u_far = V.units(GOLDEN[f"near_{case}"], ref["near"], ref["mag_near"]), V.units(GOLDEN[f"far_{case}"], ref["far"], ref["mag_far"])
        x, bound = V.x_depth(d, GOLDEN[f"near_{case}"], GOLDEN[f"far_{case}"])       # x from the reference's own f32 range: its arithmetic alone
        fin = np.isfinite(x)
        u_x = float((np.abs(GOLDEN[f"x_{case}"].astype(np.float64) - x)[fin] / (bound[fin] / V.K)).max())
        print(f"{case}: near {u_near:.3f} far {u_far:.3f} x {u_x:.3f} units")
        worst_range, worst_x = max(worst_range, u_near, u_far), max(worst_x, u_x)
    assert worst_range <= V.R32 and worst_x <= V.R32 and V.K == 4.0 * max(V.R32, 1.0)


# ---- 8. exclusion cap ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_exclusion_cap(case):
    lo, hi = V.DEPTH_CASES[case]
    d = V.log_uniform((2, 96, 128), lo, hi, seed=20)
    ref = V.depth_range(d)
    err = (V.K * V.EPS * ref["mag_near"], V.K * V.EPS * ref["mag_far"])
    x, bound = V.x_depth(d, ref["near"], ref["far"], range_err=err)
    share, wide = V.band(x, bound).mean(), V.band(x, 3 * bound).mean()
    print(f"{case}: band {100 * share:.3f} %, at three times the width {100 * wide:.3f} %")
    assert share <= wide <= V.EXCLUSION_CAP
