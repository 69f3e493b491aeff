"""The float64 reference of the rasterizer's per-(camera, Gaussian) kernels (oracle/preprocess_f64.py), pinned on the CPU.

  * against float64 autograd of oracle/raster_torch.py, from its inputs and the camera twist to aux["render_inputs"], contracted with
    random records: 2e-5 of mag (d2inv = 1 / (det^2 + 1e-7) against det >= 0.09 moves the conic partials by 1e-7 / 0.0081 = 1.2e-5;
    hw + 1e-7 against hw > 0.2 moves the projection by 5e-7) -- without clamps, and with both clamps active against raster_torch's
    own straight-through convention;
  * against the C oracle (oracle/raster_ref.c): forward decisions bit-identical on every case of tests/preprocess_cases.py, and the
    summed per-camera gradients of the small random scenes of test_raster_gpu.py, records from the float64 render backward of
    oracle/raster_f64.py, at the oracle's float32 level;
  * planted defects: each, applied to the reference on the GPU cases, moves a non-ambiguous element by >= 10 x the GPU bound;
  * the bounds themselves: rho32 of tests/preprocess_cases.py is what the reference costs in float32 on these cases, and the seeds
    keep the exclusion cap (<= 1 % of the visible pairs ambiguous, >= 8 non-ambiguous members of every planted class).

The C oracle's forward stands in for the GPU's decisions here; test_raster_preprocess_gpu.py re-asserts the cap with the GPU's.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import preprocess_cases as pc
from oracle import preprocess_f64 as pf
from oracle import raster_f64 as rf
from oracle import raster_ref as rr
from oracle import raster_torch as rt

_CHAIN = {}


def _oracle_inputs(case, s):
    shs = case["shs"][s] if case["shs"] is not None else None
    if shs is not None and case["sh_rgb_major"]:
        shs = np.ascontiguousarray(np.swapaxes(shs, -1, -2))
    cov6 = np.ascontiguousarray(pf.cov6_of(case["cov"])[s])
    cp = None if shs is not None else case["colors_precomp"][s]
    return case["means"][s], cov6, shs, case["opac"][s], cp


def chain(name):
    """The C oracle's forward and render backward of every camera of a case: decisions (radii, rect, clamp bits), the f32 records
    [C, P, 10] of seeded random image gradients, and the oracle's own 3-D gradients summed over each scene's cameras."""
    if name in _CHAIN:
        return _CHAIN[name]
    case = pc.get(name)
    Cn, (S, P) = len(case["cam_objs"]), case["means"].shape[:2]
    rng = np.random.default_rng(1000 + len(name))
    rec = np.zeros((Cn, P, 10), np.float32)
    radii, rect, bits = np.zeros((Cn, P), np.int64), np.zeros((Cn, P, 4), np.int64), np.zeros((Cn, P), np.uint8)
    geom = dict(xy=np.zeros((Cn, P, 2), np.float32), conic=np.zeros((Cn, P, 3), np.float32), rgb=np.zeros((Cn, P, 3), np.float32),
                depth=np.zeros((Cn, P), np.float32))
    sums = dict(means3D=np.zeros((S, P, 3)), cov3D=np.zeros((S, P, 6)), opacities=np.zeros((S, P)), tau=np.zeros((Cn, 6)),
                shs=None if case["shs"] is None else np.zeros((S, P) + _oracle_inputs(case, 0)[2].shape[1:]))
    for c in range(Cn):
        s = int(case["cam_scene"][c])
        means, cov6, shs, op, cp = _oracle_inputs(case, s)
        gC = rng.standard_normal((3, pc.H, pc.W)).astype(np.float32)
        gD = (0.3 * rng.standard_normal((pc.H, pc.W))).astype(np.float32)
        o = rr.rasterize_forward(case["cam_objs"][c], pc.W, pc.H, pc.BG, means, cov6, shs, op, sh_degree=case["sh_degree"], colors_precomp=cp)
        b = rr.rasterize_backward(case["cam_objs"][c], pc.W, pc.H, pc.BG, means, cov6, shs, op, o, gC, gD, sh_degree=case["sh_degree"],
                                  colors_precomp=cp)
        g = b["_render"]
        rec[c] = np.concatenate([g["mean2D"], g["conic"], g["opacity"][:, None], g["colors"], g["depths"][:, None]], -1)
        radii[c], rect[c] = o["radii"], o["rect"]
        bits[c] = (o["clamped"] * np.array([1, 2, 4], np.uint8)).sum(-1)
        geom["xy"][c], geom["conic"][c], geom["rgb"][c], geom["depth"][c] = o["xy"], o["conic_opacity"][:, :3], o["rgb"], o["depths"]
        sums["means3D"][s] += b["means3D"]; sums["cov3D"][s] += b["cov3D"]; sums["opacities"][s] += b["opacities"]
        sums["tau"][c] = b["tau"]
        if shs is not None:
            sums["shs"][s] += b["shs"]
    vis = radii > 0
    rec[~vis] = 0
    _CHAIN[name] = dict(records=rec, radii=radii, rect=np.where(vis[..., None], rect, 0), visible=vis, clamped=np.where(vis, bits, 0),
                        geom=geom, sums=sums)
    return _CHAIN[name]


_REF = {}


def reference(name, dtype=np.float64, defect=None):
    key = (name, np.dtype(dtype).name, defect)
    if key not in _REF:
        ch = chain(name)
        _REF[key] = pc.reference_backward(pc.get(name), ch["records"], ch["visible"], ch["clamped"], dtype=dtype, defect=defect)
    return _REF[key]


_FWD = {}


def reference_fwd(name, dtype=np.float64):
    key = (name, np.dtype(dtype).name)
    if key not in _FWD:
        _FWD[key] = pc.reference_forward(pc.get(name), dtype=dtype)
    return _FWD[key]


# ---------------------------------------------------------------------------------------------------------------------------------
# pin 1: float64 autograd of raster_torch
# ---------------------------------------------------------------------------------------------------------------------------------
def _torch_case(seed, clamps):
    rng = np.random.default_rng(seed)
    P = 40
    means, cov, op = pc._blob(rng, P)
    sh = pc._sh(rng, P, 16, dc_mean=-0.9 if clamps else 9.0)
    if clamps:           # wide Gaussians beyond 1.3 tanfov in x, in y and in both, reaching the image through their radius
        z = rng.uniform(1.8, 2.4, 12)
        t = rng.uniform(0.8, 0.9, 12) * np.where(np.arange(12) % 2, 1, -1)
        u = rng.uniform(-0.2, 0.2, 12)
        means[0:4] = np.stack([t * z, u * z, z], -1)[0:4]
        means[4:8] = np.stack([u * z, t * z, z], -1)[4:8]
        means[8:12] = np.stack([t * z, -t * z, z], -1)[8:12]
        cov[0:12] = pc._cov(rng, 12, 0.3, 0.6)
    E = pc._c2w(0.05, -0.03, (0.04, -0.02, 0.03))
    return means, cov, sh, op, E


@pytest.mark.parametrize("clamps", [False, True], ids=["no_clamp", "clamps_active"])
@pytest.mark.parametrize("seed", [0, 1])
def test_reference_matches_float64_autograd(seed, clamps):
    means, cov, sh, op, E = _torch_case(seed, clamps)
    P = means.shape[0]
    T = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=True)
    tm, tc, ts, to, tau = T(means), T(cov), T(sh), T(op), T(np.zeros(6))
    K = torch.tensor(pc.K09.astype(np.float64))
    near, far = 0.01, 100.0
    _, _, _, aux = rt.rasterize(tm, tc, ts, to, torch.tensor(E), K, near, far, pc.H, pc.W, pc.BG, tau=tau, sh_degree=3, return_aux=True)
    pix, conic, rgb, zr, _ = aux["render_inputs"]
    vis = aux["visible"].numpy()
    rng = np.random.default_rng(50 + seed)
    rec = rng.standard_normal((1, P, 10)) * vis[None, :, None]
    half = np.array([0.5 * pc.W, 0.5 * pc.H])
    R = lambda a: torch.tensor(a)
    loss = ((pix * R(rec[0, :, 0:2] / half)).sum() + (conic * R(rec[0, :, 2:5])).sum() + (to * R(rec[0, :, 5])).sum()
            + (rgb * R(rec[0, :, 6:9])).sum() + (zr * R(rec[0, :, 9])).sum())
    loss.backward()
    # the same camera in the library's layout, in float64
    Tcw = np.linalg.inv(E)
    Pm = np.zeros((4, 4)); Pm[0, 0] = Pm[1, 1] = 1 / pc.TANFOV; Pm[3, 2] = 1
    Pm[2, 2] = far / (far - near); Pm[2, 3] = -(far * near) / (far - near)
    cams = dict(viewmatrix=Tcw.T.reshape(1, 16), projmatrix=(Pm @ Tcw).T.reshape(1, 16), campos=E[None, :3, 3],
                tanfov=np.array([[pc.TANFOV, pc.TANFOV]]))
    kw = dict(shs=sh[None], sh_degree=3)
    f = pf.forward(means[None], cov[None], op[None], cams, None, pc.W, pc.H, **kw)
    assert np.array_equal(f["visible"][0], vis) and vis.sum() >= 30
    clamped_any = (f["clamped"][0][vis] != 0).any() or (~f["xmul"][0][vis]).any() or (~f["ymul"][0][vis]).any()
    assert clamped_any == clamps
    if clamps:
        assert (~f["xmul"][0] & vis).sum() >= 4 and (~f["ymul"][0] & vis).sum() >= 4 and (f["clamped"][0][vis] != 0).mean() > 0.2
        assert np.array_equal(f["clamped"][0][vis], ((aux["rgb"].detach().numpy() == 0) * np.array([1, 2, 4])).sum(-1)[vis])
    r = pf.backward(rec, vis[None], f["clamped"], means[None], cov[None], op[None], cams, None, pc.W, pc.H, **kw)
    assert not r["ambiguous"].any()
    G = tc.grad.numpy()
    g6 = np.stack([G[:, 0, 0], G[:, 0, 1] + G[:, 1, 0], G[:, 0, 2] + G[:, 2, 0], G[:, 1, 1], G[:, 1, 2] + G[:, 2, 1], G[:, 2, 2]], -1)
    for name, mine, theirs, mag in (("means3D", r["means3D"][0], tm.grad.numpy(), r["mag"]["means3D"][0]),
                                    ("cov6", r["cov6"][0], g6, r["mag"]["cov6"][0]),
                                    ("cov33", r["cov33"][0], 0.5 * (G + G.transpose(0, 2, 1)), r["mag"]["cov33"][0]),
                                    ("shs", r["shs"][0], ts.grad.numpy(), r["mag"]["shs"][0]),
                                    ("opacities", r["opacities"][0], to.grad.numpy(), r["mag"]["opacities"][0]),
                                    ("tau", r["tau"][0], tau.grad.numpy(), r["mag"]["tau"][0])):
        q = pc.ratio(mine, theirs, mag, False)
        print(f"[autograd seed {seed} clamps {clamps}] {name}: {q:.2e} of mag")
        assert q <= 2e-5, (name, q)
        assert np.abs(theirs).max() > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# pin 2: the C oracle
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.CASES)
def test_forward_decisions_match_c_oracle_and_seeds_keep_the_exclusion_cap(name):
    case, ch, f = pc.get(name), chain(name), reference_fwd(name)
    ok = ~f["ambiguous"]
    assert np.array_equal(f["radius"][ok], ch["radii"][ok])
    assert np.array_equal(f["rect"][ok], ch["rect"][ok])
    assert np.array_equal(f["clamped"][ok & ch["visible"]], ch["clamped"][ok & ch["visible"]])
    # same operation order, no contraction: xy, conic, depth bit-identical to the float32 run of the reference
    f32 = reference_fwd(name, np.float32)
    v = ch["visible"] & ok
    for k in ("xy", "conic", "depth"):
        assert np.array_equal(f32[k][v], ch["geom"][k][v]), k
    pc.exclusion_cap(case, ch["visible"], f["ambiguous"] | reference(name)["ambiguous"])


def test_case_properties():
    """what each case was built for, from the decisions"""
    f, case = reference_fwd("pipeline"), pc.get("pipeline")
    lst = np.nonzero(case["cam_scene"] == 3)[0]
    assert len(lst) == 36 and [int((case["cam_scene"] == s).sum()) for s in range(4)] == [0, 1, 2, 36]
    v = f["visible"][lst]                                   # [36, 300] along the list
    assert (v[0::2, :140].mean() > 0.8) and not v[1::2, :140].any() and (v[1::2, 140:280].mean() > 0.8) and not v[0::2, 140:280].any()
    assert v[0, 280:288].all() and not v[1:, 280:288].any() and v[-1, 288:296].all() and not v[:-1, 288:296].any()
    assert not v[:, 296:].any()
    f, case = reference_fwd("clamps"), pc.get("clamps")
    k = case["overflow"]
    sees = np.arange(5) != case["blind_camera"]
    assert not f["visible"][case["blind_camera"]].any()
    assert f["visible"][sees, k].all() and not f["d2inv_nz"][sees, k].any() and f["d2inv_nz"][sees, :k].all()
    for cls in ("clamp_x_neg", "clamp_x_pos", "clamp_xy"):
        assert not f["xmul"][case["classes"][cls]].any() and f["visible"][case["classes"][cls]].all()
    for cls in ("clamp_y_neg", "clamp_y_pos", "clamp_xy"):
        assert not f["ymul"][case["classes"][cls]].any()
    assert f["ymul"][case["classes"]["clamp_x_neg"]].all() and f["xmul"][case["classes"]["clamp_y_pos"]].all()
    assert not f["visible"][case["classes"]["vz_below"]].any() and f["visible"][case["classes"]["vz_above"]].all()
    assert (f["ext"][case["classes"]["opac_below"]] == -1).all() and (f["ext"][case["classes"]["opac_above"]] > 0).all()
    for name in pc.CASES:
        if name.startswith("sh_") and name != "sh_colors_precomp":
            f = reference_fwd(name)
            frac = [float(((f["clamped"][f["visible"]] >> k) & 1).mean()) for k in range(3)]
            assert all(0.15 <= x <= 0.5 for x in frac), (name, frac)
            if pc.get(name)["sh_degree"] > 0:     # the pattern differs between consecutive cameras
                assert all((f["clamped"][c] != f["clamped"][c + 1]).sum() >= 4 for c in range(4)), name


def _c_preprocess_backward(cam, Wd, Hd, bg, means, cov6, shs, op, ofwd, rec, sh_degree):
    """the C oracle's preprocess backward of one camera on the given records [P, 10]"""
    s, keep = rr._mk_in(cam, Wd, Hd, bg, means, cov6, shs, None, op, sh_degree)
    P = s.P
    f = lambda a: np.ascontiguousarray(np.asarray(a, np.float32))
    r = [f(rec[:, 0:2]), f(rec[:, 2:5]), f(rec[:, 6:9]), f(rec[:, 9])]
    out = dict(means3D=np.zeros((P, 3), np.float32), cov3D=np.zeros((P, 6), np.float32), shs=np.zeros_like(keep["shs"]),
               tau=np.zeros(6, np.float32))
    p = rr._p
    rr.lib().ref_preprocess_backward(C.byref(s), p(f(cam.projmatrix_raw)), p(ofwd["radii"]), p(ofwd["clamped"]), p(r[0]), p(r[1]), p(r[2]),
                                     p(r[3]), p(out["means3D"]), p(out["cov3D"]), p(out["shs"]), p(out["tau"]))
    return out


@pytest.mark.parametrize("Wd,Hd,P", [(48, 32, 60), (64, 64, 400), (40, 24, 80)])
def test_reference_matches_c_oracle_on_small_random_scenes(Wd, Hd, P):
    """The scenes, cameras and image gradients of test_raster_gpu.test_backward_matches_oracle; records: the float64 render backward of
    raster_f64 on the oracle's forward, rounded to f32 and given to both.  The oracle is a plain f32 evaluation of the same formulae
    in another order: it is held to the bound the GPU is held to."""
    rng = np.random.default_rng(100 + P)
    means = np.stack([rng.uniform(-0.9, 0.9, P), rng.uniform(-0.6, 0.6, P), rng.uniform(1.5, 4.0, P)], -1).astype(np.float32)
    A = rng.standard_normal((P, 3, 3)) * 0.08
    cov = (A @ A.transpose(0, 2, 1) + 1e-4 * np.eye(3)).astype(np.float32)
    sh = (rng.standard_normal((P, 25, 3)) * rr.SH_MASK[None, :, None]).astype(np.float32)
    sh[:, 0] = rng.standard_normal((P, 3)) * 0.7
    op = rng.uniform(0.2, 0.95, P).astype(np.float32)
    yaw = 0.1
    E = np.eye(4, dtype=np.float32)
    E[:3, :3] = [[math.cos(yaw), 0, math.sin(yaw)], [0, 1, 0], [-math.sin(yaw), 0, math.cos(yaw)]]
    E[:3, 3] = [0.1, -0.05, 0.02]
    objs, cams = pc._cameras([np.eye(4, dtype=np.float32), E])
    bg = np.array([0.2, 0.1, 0.3], np.float32)
    rng = np.random.default_rng(7)
    gC = rng.standard_normal((2, 3, Hd, Wd)).astype(np.float32)
    gD = (rng.standard_normal((2, Hd, Wd)) * 0.3).astype(np.float32)
    c6 = rr.cov6(cov)
    rec = np.zeros((2, P, 10), np.float32)
    vis, bits = np.zeros((2, P), bool), np.zeros((2, P), np.uint8)
    tot = dict(means3D=0.0, cov3D=0.0, shs=0.0)
    taus = []
    for c, cam in enumerate(objs):
        o = rr.rasterize_forward(cam, Wd, Hd, bg, means, c6, sh, op)
        r64 = rf.render_backward(o["xy"], o["conic_opacity"], o["rgb"], o["depths"], o["ranges"], o["point_list"], o["n_contrib"], bg,
                                 gC[c], gD[c], W=Wd, H=Hd, exp=rf.exp_libm)
        rec[c] = np.concatenate([r64["mean2D"], r64["conic"], r64["opacity"][:, None], r64["colors"], r64["depths"][:, None]], -1)
        vis[c], bits[c] = o["radii"] > 0, (o["clamped"] * np.array([1, 2, 4], np.uint8)).sum(-1)
        out = _c_preprocess_backward(cam, Wd, Hd, bg, means, c6, sh, op, o, rec[c], 4)
        for k in tot:
            tot[k] = tot[k] + out[k].astype(np.float64)
        taus.append(out["tau"])
    r = pf.backward(rec, vis, bits, means[None], c6[None], op[None], cams, None, Wd, Hd, shs=sh[None], sh_degree=4)
    ok = ~r["amb_gauss"][0]
    assert ok.mean() > 0.98
    assert float(np.abs(r["shs"][0][:, 16:]).max()) == 0.0
    for fam, mine, theirs, mag, ex in (("means3D", r["means3D"][0], tot["means3D"], r["mag"]["means3D"][0], ~ok[:, None]),
                                       ("cov6", r["cov6"][0], tot["cov3D"], r["mag"]["cov6"][0], ~ok[:, None]),
                                       ("shs", r["shs"][0], tot["shs"], r["mag"]["shs"][0], ~ok[:, None, None]),
                                       ("tau_rho", r["tau"][:, :3], np.stack(taus)[:, :3], r["mag"]["tau"][:, :3], r["amb_cam"][:, None]),
                                       ("tau_theta", r["tau"][:, 3:], np.stack(taus)[:, 3:], r["mag"]["tau"][:, 3:], r["amb_cam"][:, None])):
        q = pc.ratio(theirs, mine, mag, ex)
        print(f"[c oracle {Wd}x{Hd} P={P}] {fam}: {q:.2e} of mag (bound {pc.GPU_MARGIN * pc.RHO32[fam]:.2e})")
        assert q <= pc.GPU_MARGIN * pc.RHO32[fam], (fam, q)


# ---------------------------------------------------------------------------------------------------------------------------------
# the bounds
# ---------------------------------------------------------------------------------------------------------------------------------
def measure_rho32(name, records=None, visible=None, clamped=None):
    """{family: max |ref32 - ref64| / mag over the non-ambiguous elements} of one case, forward and backward."""
    case = pc.get(name)
    if records is None:
        ch = chain(name)
        records, visible, clamped = ch["records"], ch["visible"], ch["clamped"]
        r64, r32 = reference(name), reference(name, np.float32)
    else:
        r64 = pc.reference_backward(case, records, visible, clamped)
        r32 = pc.reference_backward(case, records, visible, clamped, dtype=np.float32)
    f64, f32 = reference_fwd(name), reference_fwd(name, np.float32)
    ex = (f64["ambiguous"] | ~np.asarray(visible, bool))
    rho = {k: pc.ratio(f32[k], f64[k], f64["mag"][k], ex[..., None] if f64[k].ndim == 3 else ex) for k in pf.FAMILIES_FWD}
    a, b = pc.families(case, r64), pc.families(case, r32)
    for k in a:
        rho[k] = pc.ratio(b[k][0], a[k][0], a[k][1], a[k][2])
    return rho


def test_rho32_is_the_measured_float32_cost():
    worst = {k: (0.0, None) for k in pc.RHO32}
    for name in pc.CASES:
        for k, q in measure_rho32(name).items():
            if q > worst[k][0]:
                worst[k] = (q, name)
    print("\n" + "\n".join(f"rho32 {k}: {q:.3e} ({n})" for k, (q, n) in worst.items()))
    for k, (q, n) in worst.items():
        assert q <= pc.RHO32[k], (k, q, n)
        assert pc.RHO32[k] <= 2.0 * q or pc.RHO32[k] == q == 0.0, (k, q, "the recorded rho32 is not the measurement")


# ---------------------------------------------------------------------------------------------------------------------------------
# planted defects
# ---------------------------------------------------------------------------------------------------------------------------------
PLANTED = [("record_prev", "pipeline"), ("record_next", "pipeline"), ("clamp_neighbour", "pipeline"), ("clamp_neighbour", "sh_deg3_M25"),
           ("params_pos31", "pipeline"), ("params_pos31", "chunks"), ("drop_chunk2", "chunks"), ("double_empty_chunk", "chunks"),
           ("no_xmul", "clamps"), ("offdiag", "pipeline"), ("offdiag", "cov33"), ("sh_sign_band2", "sh_deg2_M25"), ("sh_sign_band2", "sh_deg3_M16"), ("sh_sign_band3", "sh_deg3_M16"),
           ("sh_sign_band3", "sh_deg4_M25"),
           ("no_passB_tau", "pipeline"), ("drop_last_wave_tau", "pipeline"), ("sh_shift_half", "pipeline")]


@pytest.mark.parametrize("defect,name", PLANTED)
def test_planted_defect_is_rejected(defect, name):
    case = pc.get(name)
    good, bad = pc.families(case, reference(name)), pc.families(case, pc.reference_backward(
        case, chain(name)["records"], chain(name)["visible"], chain(name)["clamped"], defect=defect))
    moved = {k: pc.ratio(bad[k][0], good[k][0], good[k][1], good[k][2]) / max(pc.GPU_MARGIN * pc.RHO32[k], 1e-300) for k in good}
    k = max(moved, key=moved.get)
    print(f"[{defect} on {name}] largest move: {k}, {moved[k]:.3g} x the GPU bound")
    assert moved[k] >= 10.0, moved
    expect = dict(offdiag="cov6", sh_sign_band2="means3D", sh_sign_band3="means3D", no_passB_tau="tau_rho", drop_last_wave_tau="tau_rho", sh_shift_half="shs",
                  no_xmul="means3D").get(defect)
    if expect:
        assert moved[expect] >= 10.0, (expect, moved[expect])


@pytest.mark.parametrize("name", ["pipeline", "clamps"])
def test_extents_shrunk_by_two_percent_are_rejected(name):
    f = reference_fwd(name)
    v = f["visible"] & ~f["ambiguous"]
    kernel_like = np.where(f["ext"] > 0, 1.01 * f["ext"] + 0.05, -1.0)
    assert pf.extents_ok(kernel_like, f["ext"])[v].all()
    shrunk = np.where(f["ext"] > 0, 0.98 * kernel_like, -1.0)
    assert (~pf.extents_ok(shrunk, f["ext"])[v]).sum() >= 8
    assert (~pf.extents_ok(np.where(f["ext"] > 0, 1.02 * kernel_like, -1.0), f["ext"])[v]).sum() >= 8
