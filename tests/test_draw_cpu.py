"""Vector drawing on the CPU: the torch backend of vicasplat_amd.visualization.drawing and the restatement of tests/draw_f64.py against the
real reference's own results (tests/golden/draw.npz, written by tests/golden/gen_draw_golden.py); the planted defects; the host code of the
camera plot, the wobble and the two extra video trajectories against the golden and closed forms; the binding of the vsg_ entries and
their refusals; the control flow of validation_step's new options on stubs; and, for every general case of tests/test_draw_gpu.py, that
the f32 run of the restatement itself passes the GPU criterion inside both exclusion caps.

Measured here (`-s` prints them): r32 per comparison 0.57 (par_hi), 0.49 (par_lo), 0.76 (perp), 0.88 (cap), 0.85 (inner, outer) -- all below
1, so FACTOR = 4; the f32 run against float64 on the general cases: at most 0.4 % of the pixels ambiguous, none unsure, the largest error 0.42
of 2^-24 mag on unambiguous pixels; torch backend and f32 restatement equal the reference bit for bit on every golden scene.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import draw_f64 as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = lambda a: torch.tensor(np.asarray(a, np.float32))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "draw.npz"))


def _passes(name):
    return (0, 1, 2) if name.startswith("lines_") else (1,)


def _torch_backend(kind, image, world, cap, passes, x_range, y_range):
    from vicasplat_amd.visualization.drawing import draw_lines, draw_points
    if kind == "lines":
        return draw_lines(T(image), T(world["start"]), T(world["end"]), T(world["color"]), T(world["width"]), cap=cap, num_msaa_passes=passes,
                          x_range=x_range, y_range=y_range, backend="torch").numpy()
    return draw_points(T(image), T(world["points"]), T(world["color"]), T(world["radius"]), T(world["inner_radius"]), num_msaa_passes=passes,
                       backend="torch").numpy()


# ---- the golden scenes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(D.golden_scenes()))
def test_torch_backend_and_restatement_reproduce_the_reference(golden, name):
    kind, image, world, cap, xr, yr = D.golden_scenes()[name]
    rec = D.scene_records(kind, image, world, xr, yr)
    for passes in _passes(name):
        want, rgba = golden[f"{name}_p{passes}_out"], golden[f"{name}_p{passes}_rgba"]
        r64 = D.render(kind, image, rec, cap, passes, np.float64)
        bound = D.FACTOR * D.U * r64["mag"]
        got = _torch_backend(kind, image, world, cap, passes, xr, yr)
        assert np.array_equal((np.abs(got - want) <= bound), np.ones_like(want, bool)), (name, passes)
        assert np.array_equal(got, want), (name, passes)      # the same torch operations: the same bits
        for dtype in (np.float32, np.float64):
            r = D.render(kind, image, rec, cap, passes, dtype)
            # coverage, masks and alpha bit for bit; colours within the rounding bound
            assert np.array_equal(r["rgba"][3].astype(np.float32), rgba[3]), (name, passes, dtype)
            if passes:
                assert np.array_equal(r["mask"], golden[f"{name}_p{passes}_mask"]), (name, passes, dtype)
            covered = rgba[3] > 0
            assert (np.abs(r["rgba"][:3].astype(np.float64) - rgba[:3])[:, covered] <= D.FACTOR * D.U * 8).all(), (name, passes, dtype)
            assert (np.abs(r["out"].astype(np.float64) - want) <= bound).all(), (name, passes, dtype)


@pytest.mark.parametrize("defect", D.DEFECTS)
def test_every_planted_defect_changes_a_golden_scene(golden, defect):
    changed = []
    for name, (kind, image, world, cap, xr, yr) in D.golden_scenes().items():
        rec = D.scene_records(kind, image, world, xr, yr, defects=(defect,))
        out = D.render(kind, image, rec, cap, 1, np.float32, defects=(defect,))["out"]
        if np.abs(out - golden[f"{name}_p1_out"]).max() > 1e-3:
            changed.append(name)
    assert changed, defect
    assert "lines_butt" in changed or not defect.startswith("par_")      # the body's thresholds show without caps
    if defect in ("inner_strict", "outer_strict"):
        assert changed == ["points"]


def test_no_defect_no_change(golden):
    for name, (kind, image, world, cap, xr, yr) in D.golden_scenes().items():
        out = D.render(kind, image, D.scene_records(kind, image, world, xr, yr), cap, 1, np.float32)["out"]
        assert np.array_equal(out, golden[f"{name}_p1_out"]), name


# ---- the general cases of the GPU test --------------------------------------------------------------------------------------------------
def _gaps(kind, image, rec, cap):
    g32, g64 = {}, {}
    r32 = D.render(kind, image, rec, cap, 0, np.float32, gaps=g32)
    D.render(kind, image, rec, cap, 0, np.float64, gaps=g64)
    worst = {}
    for k in g64:
        for (d32, _), (d64, e64) in zip(g32[k], g64[k]):
            with np.errstate(all="ignore"):
                r = np.abs(d32 - d64) / (D.U * e64)
            r = r[np.isfinite(r)]
            if r.size:
                worst[k] = max(worst.get(k, 0.0), float(r.max()))
    return worst, r32


def test_r32_is_measured():
    worst = {}
    for name, (kind, shape, build, cap) in D.GENERAL_CASES.items():
        w, _ = _gaps(kind, D.general_image(shape, 5), build(), cap)
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("\n  r32: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert set(worst) == set(D.R32)
    for k, v in worst.items():
        assert v <= D.R32[k], (k, v)
    assert D.FACTOR == 4.0 * max(max(D.R32.values()), 1.0)


@pytest.mark.parametrize("name", list(D.GENERAL_CASES))
def test_general_cases_stay_inside_the_caps(name):
    """The f32 run of the restatement passes the GPU criterion on every general case, with at most 2 % of the pixels unsure and at most
    10 % ambiguous: the caps cannot hide a failure of the kernel."""
    kind, shape, build, cap = D.GENERAL_CASES[name]
    image, rec = D.general_image(shape, 5), build()
    for passes in (0, 1):
        ref = D.render(kind, image, rec, cap, passes, np.float64)
        ok, report = D.check(D.render(kind, image, rec, cap, passes, np.float32)["out"], ref)
        print(f"\n  {name} passes {passes}: " + "  ".join(f"{k} {v:.3g}" for k, v in report.items()))
        assert ok and report["unsure"] <= 0.02 and report["ambiguous"] <= 0.10, (name, report)
        from vicasplat_amd.visualization.drawing import lines, points
        got = (lines._draw_torch(T(image), T(rec), cap, passes) if kind == "lines" else points._draw_torch(T(image), T(rec), passes)).numpy()
        assert D.check(got, ref)[0], name
    # a planted defect does not pass the criterion
    bad = D.render(kind, image, rec, cap, 1, np.float32, defects=("lowest_index",) if kind == "lines" else ("outer_strict", "alpha_sum"))["out"]
    assert not D.check(bad, D.render(kind, image, rec, cap, 1, np.float64))[0]


def test_camera_cases_stay_inside_the_caps():
    from vicasplat_amd.visualization.drawing import cameras as Cm
    from vicasplat_amd.visualization.drawing.lines import line_records
    from vicasplat_amd.visualization.validation_in_3d import compute_equal_aabb_with_margin
    E, K, colour, near, far = (T(v) for v in D.cameras(20, 8))
    lo, hi = compute_equal_aabb_with_margin(*Cm.compute_aabb(E, K, near, far), margin=0.1)
    layers = Cm.camera_layers(E, K, colour, near, far, ((hi - lo).max() * 0.05)[None])
    assert [len(l[0]) for l in layers] == [80, 80, 80, 160]
    start, end, col = layers[-1]
    rec = line_records((64, 64), "cpu", start[:, [1, 2]], end[:, [1, 2]], col, 2, torch.stack((lo[1], hi[1])), torch.stack((lo[2], hi[2]))).numpy()
    image = np.zeros((3, 64, 64), np.float32)
    ok, report = D.check(D.render("lines", image, rec, "round", 1, np.float32)["out"], D.render("lines", image, rec, "round", 1, np.float64))
    assert ok and report["unsure"] <= 0.02 and report["ambiguous"] <= 0.10, report


# ---- the torch backend's surface --------------------------------------------------------------------------------------------------------
def test_backend_surface():
    from vicasplat_amd.visualization.drawing import draw_cameras, draw_lines, draw_points
    image = T(D.lattice_image((16, 24), 0))
    args = ([[2.5, 3.5], [20.0, 4.0]], [[18.5, 12.5], [4.0, 14.0]], [[1, 0, 0], [0, 1, 0]], [2.0, 3.0])
    one = draw_lines(image, *args)
    assert one.shape == image.shape and one is not image and not torch.equal(one, image)
    # a number broadcasts over the components and the lines, as the reference's sanitize_* do
    assert torch.equal(draw_lines(image, args[0], args[1], 0.25, 2), draw_lines(image, args[0], args[1], [[0.25] * 3] * 2, [2.0, 2.0]))
    # a batch: per-image lists, one of them empty (copied through: the stated deviation), shared values broadcast
    batch = torch.stack((image, image.flip(-1), image * 0.5))
    empty = torch.zeros(0, 2)
    out = draw_lines(batch, [T(args[0]), empty, T(args[0][:1])], [T(args[1]), empty, T(args[1][:1])], [T(args[2]), torch.zeros(0, 3), T(args[2][:1])],
                     [T(args[3]), torch.zeros(0), T(args[3][:1])])
    assert torch.equal(out[0], one) and torch.equal(out[1], batch[1])
    assert torch.equal(out[2], draw_lines(batch[2], args[0][:1], args[1][:1], args[2][:1], args[3][:1]))
    pts = draw_points(batch, [T([[5.0, 5.0]]), torch.zeros(0, 2), T([[9.0, 9.0], [12.0, 3.0]])], radius=3, inner_radius=1)
    assert torch.equal(pts[1], batch[1]) and torch.equal(pts[0], draw_points(batch[0], [[5.0, 5.0]], radius=3, inner_radius=1))
    # a NaN in the geometry covers nothing, whichever field it is in (the reference would still draw the start cap for a NaN end)
    for k in range(2):
        bad = [list(args[0][0]), list(args[1][0])]
        bad[k][0] = float("nan")
        assert torch.equal(draw_lines(image, [bad[0], args[0][1]], [bad[1], args[1][1]], args[2], args[3]),
                           draw_lines(image, args[0][1:], args[1][1:], args[2][1:], args[3][1:]))
    with pytest.raises(ValueError, match="cap"):
        draw_lines(image, *args, cap="flat")
    with pytest.raises(ValueError, match="backend"):
        draw_lines(image, *args, backend="triton")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        draw_lines(image, *args, backend="hip")
    with pytest.raises(NotImplementedError, match="font"):
        draw_cameras(16, torch.eye(4)[None], torch.eye(3)[None], torch.ones(1, 3), draw_label=True)


# ---- the camera plot, the wobble, the trajectories ---------------------------------------------------------------------------------------
def test_camera_plot_host_code(golden):
    from vicasplat_amd.visualization.drawing import cameras as Cm
    from vicasplat_amd.visualization.drawing import compute_aabb, draw_cameras, unproject_frustum_corners
    E, K, colour, near, far = (T(golden[k]) for k in ("cam_E", "cam_K", "cam_color", "cam_near", "cam_far"))
    corners = unproject_frustum_corners(E, K, far)
    assert torch.allclose(corners, T(golden["cam_corners"]), atol=1e-6)
    # closed form: the corner (x, y) of camera b at depth d is o + d R ((x - cx) / fx, (y - cy) / fy, 1)
    for b in range(len(E)):
        for p, (x, y) in enumerate(((0, 0), (1, 0), (1, 1), (0, 1))):
            ray = torch.stack(((x - K[b, 0, 2]) / K[b, 0, 0], (y - K[b, 1, 2]) / K[b, 1, 1], torch.tensor(1.0)))
            assert torch.allclose(corners[b, p], E[b, :3, 3] + far[b] * (E[b, :3, :3] @ ray), atol=1e-5), (b, p)
    lo, hi = compute_aabb(E, K, near, far)
    assert torch.equal(lo, T(golden["cam_aabb_lo"])) and torch.equal(hi, T(golden["cam_aabb_hi"]))
    everything = torch.cat((E[:, :3, 3], unproject_frustum_corners(E, K, near).reshape(-1, 3), corners.reshape(-1, 3)))
    assert torch.equal(lo, everything.min(0).values) and torch.equal(hi, everything.max(0).values)
    lo0, hi0 = compute_aabb(E, K)
    assert torch.equal(lo0, E[:, :3, 3].min(0).values) and torch.equal(hi0, E[:, :3, 3].max(0).values)
    # the four layers in the reference's order, the frustums last and in the cameras' colours
    layers = Cm.camera_layers(E, K, colour, near, far, torch.tensor([0.1]))
    assert [l[2] if isinstance(l[2], float) else None for l in layers] == [0.25, 0.25, 0.25, None] and [len(l[0]) for l in layers] == [16, 16, 16, 32]
    assert torch.equal(layers[3][2].reshape(4, 8, 3), colour[:, None].expand(4, 8, 3)) and torch.equal(layers[3][0][:4], E[0, :3, 3].expand(4, 3))
    assert torch.equal(layers[2][0], unproject_frustum_corners(E, K, near).reshape(-1, 3)) and torch.equal(layers[2][1], corners.reshape(-1, 3))
    assert len(Cm.camera_layers(E, K, colour, None, None, torch.tensor([0.1]))) == 1 and len(Cm.camera_layers(E, K, colour, near, None, torch.tensor([0.1]))) == 2
    # end to end against the reference
    assert np.array_equal(draw_cameras(32, E, K, colour).numpy(), golden["cam_plain"])
    planes = draw_cameras(32, E, K, colour, near, far).numpy()
    assert planes.shape == (3, 3, 32, 32) and np.array_equal(planes, golden["cam_planes"])


def test_wobble_against_the_reference_and_closed_form(golden):
    from vicasplat_amd.visualization.camera_trajectory.wobble import generate_wobble, generate_wobble_transformation
    t, radius, E = T(golden["wob_t"]), T(golden["wob_radius"]), T(golden["wob_E"])
    tf = generate_wobble_transformation(radius, t)
    assert np.array_equal(tf.numpy(), golden["wob_tf"]) and np.array_equal(generate_wobble(E, radius, t).numpy(), golden["wob"])
    tf5 = generate_wobble_transformation(radius, t, 5, scale_radius_with_t=False)
    assert np.array_equal(tf5.numpy(), golden["wob_tf5"])
    assert tf.shape == (4, 7, 4, 4) and torch.equal(tf[..., :3, :3], torch.eye(3).expand(4, 7, 3, 3)) and bool((tf[..., 2, 3] == 0).all())
    assert torch.allclose(tf5[..., :2, 3].norm(dim=-1), radius[:, None].expand(4, 7), atol=1e-6)           # a circle of the radius
    assert torch.allclose(tf[..., :2, 3].norm(dim=-1), radius[:, None] * t, atol=1e-6)                      # a spiral that opens with t
    assert torch.allclose(tf[:, 0, :2, 3], torch.zeros(4, 2)) and torch.allclose(tf5[:, 0, :2, 3], torch.stack((torch.zeros(4), -radius), -1))


def test_video_trajectories_on_a_stub_decoder(monkeypatch):
    import test_viz_cpu as TV
    from vicasplat_amd.visualization.camera_trajectory.wobble import generate_wobble_transformation
    callers, batch, encoder, decoder, calls = TV._stub_world(monkeypatch)
    ctx = batch["context"]
    delta = (ctx["extrinsics"][0, 0, :3, 3] - ctx["extrinsics"][0, -1, :3, 3]).norm()
    video = callers.render_video_wobble_step(encoder, decoder, batch)
    E = calls["decoder"][-1]["extrinsics"]
    assert E.shape == (1, 60, 4, 4) and video.shape[0] == 60 + 58         # 60 frames, eased, looped back
    t = (torch.cos(torch.pi * (torch.linspace(0, 1, 60) + 1)) + 1) / 2
    want = ctx["extrinsics"][:, 0, None] @ generate_wobble_transformation((delta * 0.25)[None], t)
    assert torch.equal(E, want) and torch.allclose((E[0, -1, :3, 3] - ctx["extrinsics"][0, 0, :3, 3]).norm(), delta * 0.25, atol=1e-6)
    video = callers.render_video_interpolation_exaggerated_step(encoder, decoder, batch)
    E = calls["decoder"][-1]["extrinsics"]
    assert E.shape == (1, 300, 4, 4) and video.shape[0] == 300          # not eased, not looped
    t = torch.linspace(0, 1, 300)
    centre = callers.interpolate_extrinsics(ctx["extrinsics"][:1, 0], ctx["extrinsics"][:1, -1], t * 5 - 2)
    assert torch.equal(E, centre @ generate_wobble_transformation((delta * 0.5)[None], t, 5, scale_radius_with_t=False))
    # every pose sits on a circle of radius |delta| / 2 around the (extrapolated) interpolation, in that pose's image plane
    offset = torch.linalg.inv(centre[0]) @ E[0]
    assert torch.allclose(offset[:, :2, 3].norm(dim=-1), (delta * 0.5).expand(300), atol=1e-5) and torch.allclose(offset[:, 2, 3], torch.zeros(300), atol=1e-6)
    assert torch.allclose(centre[0, 120, :3, 3], ctx["extrinsics"][0, 0, :3, 3], atol=2e-2)      # t * 5 - 2 = 0 near frame 120
    assert callers.render_video_interpolation_exaggerated_step(encoder, decoder, batch, num_frames=7).shape[0] == 7


def test_validation_step_options_on_stubs(monkeypatch):
    import test_viz_cpu as TV
    callers, batch, encoder, decoder, calls = TV._stub_world(monkeypatch)
    pred = batch["context"]["extrinsics"].clone()
    pred[0, 1, 1, 3] = 0.5
    with_pred = lambda c, **kw: {**encoder(c, **kw), "gaussian_camera_extrins": pred}
    out = callers.validation_step(with_pred, decoder, batch, cameras=True, extended_visualization=True)
    assert list(out) == ["psnr", "ssim", "comparison", "projections", "video", "video_exaggerated", "cameras", "camera_traj"]
    assert out["cameras"].shape == (3, 256, 3 * 256 + 16) and out["camera_traj"].shape == (3, 256, 3 * 256)
    assert out["video_exaggerated"].shape[0] == 300 and out["video_exaggerated"].dtype == torch.uint8
    from vicasplat_amd.visualization import layout, validation_in_3d
    views = validation_in_3d.render_cameras(batch, 256)
    assert views.shape == (3, 3, 256, 256) and torch.equal(out["cameras"], layout.hcat(*views))
    # white context cameras, red target cameras, grey planes
    flat = views.permute(0, 2, 3, 1).reshape(-1, 3)
    for colour in ((1.0, 1.0, 1.0), (1.0, 0.0, 0.0), (0.25, 0.25, 0.25)):
        assert bool((flat == torch.tensor(colour)).all(-1).any()), colour
    ctx = batch["context"]
    plot = callers.camera_trajectory_plot(ctx["extrinsics"][0], ctx["intrinsics"][0], pred[0], ctx["intrinsics"][0], resolution=64)
    assert plot.shape == (3, 64, 192) and float(plot[1].max()) == 0.75 and float(plot[0].max()) == 1.0       # green and red
    # the default call: the keys and outputs of before
    assert list(callers.validation_step(with_pred, decoder, batch)) == ["psnr", "ssim", "comparison", "projections", "video"]
    assert "video_exaggerated" not in callers.validation_step(with_pred, decoder, batch, video=False, extended_visualization=True)
    assert list(callers.validation_step(with_pred, decoder, batch, distiller=lambda c, f: 1 / 0, distill_only=False, video=False, projections=False,
                                        cameras=True)) == ["psnr", "ssim", "comparison", "cameras", "camera_traj"]


def test_first_positives_is_the_reference_slice():
    from vicasplat_amd.callers import first_positives
    g = torch.Generator().manual_seed(0)
    for n, limit in ((50, 10), (50, 60), (7, 7), (9, 1)):
        x = torch.randn(n, generator=g)
        want, got = x[x > 0][:limit], first_positives(x, limit)
        assert got.shape == (limit,) and torch.equal(got[:len(want)], want) and bool((got[len(want):] == 0).all()), (n, limit)


# ---- the binding ------------------------------------------------------------------------------------------------------------------------
def test_the_draw_header_parses_is_bound_and_is_documented():
    from vicasplat_amd import _lib
    assert _lib.DRAW_HEADERS == (("vsg_", "vicasplat_draw.h"),) and "vsg_" not in dict(_lib.HEADERS) and "vsg_" not in dict(_lib.DATA_HEADERS)
    assert _lib.ALL_HEADERS == _lib.HEADERS + _lib.DATA_HEADERS + _lib.DRAW_HEADERS
    assert os.path.samefile(_lib.header_path("vsg_"), os.path.join(ROOT, "include", "vicasplat_draw.h"))
    text = open(_lib.header_path("vsg_")).read()
    sigs = _lib.parse_header(text, prefix="vsg_")
    i32, vp = C.c_int32, C.c_void_p
    assert sigs == {"vsg_draw_lines": (C.c_int, [vp, vp, i32, i32, i32, vp, i32, vp, i32, i32, vp], True),
                    "vsg_draw_points": (C.c_int, [vp, vp, i32, i32, i32, vp, i32, vp, i32, vp], True)}
    L = _lib.lib()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for entry, (restype, argtypes, takes_stream) in sigs.items():
        fn = getattr(L, entry)
        assert fn.restype is restype and fn.argtypes == argtypes and _lib._entries[entry] == (fn, takes_stream)
        assert entry in doc, f"{entry} is not in INTEGRATION.md"
    for other, _ in _lib.HEADERS + _lib.DATA_HEADERS:
        assert not re.findall(r"\b%s[a-z0-9_]+\s*\(" % re.escape(other), re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    consts = _lib.header_constants(_lib.header_path("vsg_"), "VSG_")
    assert len(consts) == 12 and all(getattr(_lib, k) == v for k, v in consts.items())
    assert _lib.VSG_SCAN_CHUNK == _lib.VSG_THREADS and _lib.VSG_LIST_CAP >= _lib.VSG_SCAN_CHUNK and _lib.VSG_THREADS % 64 == 0
    assert (_lib.VSG_TILE_W + 2) * (_lib.VSG_TILE_H + 2) <= _lib.VSG_THREADS and _lib.VSG_MAX_SIDE == 16384
    assert (_lib.VSG_LINE_FLOATS, _lib.VSG_POINT_FLOATS, _lib.VSG_CAP_BUTT, _lib.VSG_CAP_ROUND, _lib.VSG_CAP_SQUARE) == (8, 7, 0, 1, 2)
    from vicasplat_amd import ops
    assert ops._DRAW_CAPS == {"butt": 0, "round": 1, "square": 2} and ops.draw_lines.__doc__ and ops.draw_points.__doc__
    # the semantics are stated in the header's comment
    for phrase in ("par <= n + extra", "inner <= d and d <= radius", "HIGHEST-INDEXED", "1e-10f", "STATED DEVIATION"):
        assert phrase in text, phrase


def test_refusals_come_before_any_gpu_call():
    from vicasplat_amd import _lib
    L = _lib.lib()
    p, q = 4096, 1 << 30      # addresses that are never dereferenced: every call below returns before any HIP call
    ok = dict(image=p, out=q, B=1, H=8, W=8, prims=p, n_prims=3, offsets=p, cap=1, passes=1)

    def lines(**kw):
        return L.vsg_draw_lines(*dict(ok, **kw).values(), None)

    def points(**kw):
        a = dict(ok, **kw)
        del a["cap"]
        return L.vsg_draw_points(*a.values(), None)

    for call in (lines, points):
        for name in ("image", "out", "offsets", "prims"):
            assert call(**{name: None}) < 0 and b"null pointer" in L.vs_last_error(), name
        for name in ("B", "H", "W", "n_prims"):
            assert call(**{name: -1}) < 0 and b"negative" in L.vs_last_error(), name
        assert call(H=16385) < 0 and b"16384" in L.vs_last_error() and call(W=16385) < 0
        assert call(B=65536) < 0 and b"grid limit" in L.vs_last_error()
        assert call(n_prims=1 << 28) < 0 and b"2^28" in L.vs_last_error()
        assert call(passes=2) < 0 and b"num_passes" in L.vs_last_error() and call(passes=-1) < 0
        assert call(out=p + 4) < 0 and b"overlaps" in L.vs_last_error()
        assert call(B=0) == 0 and call(H=0, image=None, out=None) == 0 and call(W=0) == 0      # a zero-size call is a no-op
    assert lines(cap=3) < 0 and b"cap 3" in L.vs_last_error() and lines(cap=-1) < 0
    # the wrappers check before they look for a device
    from vicasplat_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.draw_lines(torch.zeros(1, 3, 4, 4), torch.zeros(1, 8), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="cap"):
        ops.draw_lines(torch.zeros(1, 3, 4, 4), torch.zeros(1, 8), torch.zeros(2, dtype=torch.int32), cap="flat")
