"""preprocess_kernel and preprocess_backward_kernel ("K2") against float64 (oracle/preprocess_f64.py) at their edges.  -m gpu.

K2 is tested in isolation: backward_debug hands back the [C, P, 10] gradient records the render backward left for it, and the
reference consumes those f32 records together with the GPU forward's own `radii > 0` and clamp bits, so neither render-backward
error nor atomic ordering enters K2's bound.  The forward's records (VS_BUF_GEOM) and decisions are compared directly.

Cases (tests/preprocess_cases.py, 48 x 32 images): `pipeline` (scenes with 0 / 1 / 2 / 36 cameras, 300 Gaussians, visibility
1010.. / 0101.. / first-only / last-only / none: the prefetch of list positions k + 1, k + 2 across kParCams = 32, a partial wave,
two blocks), `chunks` (1100 cameras across K2's 512-camera list builds, one scene absent from the second chunk), `clamps` (frustum
clamp in x / y / both, vz and opacity cuts, a Gaussian whose det^2 overflows f32, a camera that sees nothing), `sh_*` (sh_degree
0..4 x M in {16, 25}, rgb-major, M = 36 on the direct-store route, colors_precomp; every channel clamps at 0 for about a third of
the pairs), `cov33`.  Both render-backward routes feed K2 the same way: the checkpoint route everywhere, `pipeline` also on the
whole-list route.

Checked per case, on the pairs no decision of which is within rounding of flipping (at most 1 % of the visible pairs, and at least
8 left in every planted class -- asserted):
  forward   radii, rect, clamp bits equal to the reference's; rect = 0 and radii = 0 at invisible pairs; xy, conic, rgb, depth
            within the bound; the extents contain the float64 half extents and stay inside 1.011 x true + 0.051;
  backward  every element of every output written (a sentinel pre-fills them); |gpu - ref64| <= bound x mag per Gaussian and
            component (per camera for dL_dtau and dL_dmeans2D); dL_dmeans2D zero at invisible pairs; dL_dtau zero for a camera that
            sees nothing; every gradient of a scene without cameras exactly zero; SH gradients of coefficients k >= 16 exactly
            zero; the covariance-path gradient of the overflowing Gaussian exactly zero; the 3 x 3 covariance gradient symmetric.

Bound = 4 x rho32 (tests/preprocess_cases.py: RHO32, GPU_MARGIN).  rho32 is the largest |ref32 - ref64| / mag of the reference run
in float32 on these cases on the CPU (tests/test_raster_preprocess_cpu.py re-measures it); the margin of 4 covers FMA
contraction, K2's reciprocal-multiply forms, v_rsq_f32 in the forward's view direction and a different summation order.

    family           rho32      bound      measured on an MI355X: maximum / mag (case)
    xy               2.7e-07    1.08e-06   2.26e-07 (clamps)
    conic            1.2e-06    4.80e-06   1.16e-06 (chunks)
    rgb              3.3e-07    1.32e-06   2.99e-07 (chunks)
    depth            1.6e-07    6.40e-07   1.52e-07 (pipeline)
    means3D          3.0e-07    1.20e-06   3.58e-07 (pipeline)
    cov6 / cov33     6.4e-07    2.56e-06   9.11e-07 (pipeline)
    shs              5.5e-07    2.20e-06   5.72e-07 (pipeline)
    opacities        1.2e-07    4.80e-07   1.07e-07 (pipeline)
    colors_precomp   9.6e-08    3.84e-07   1.01e-07 (sh_colors_precomp)
    means2D          0          0          0 (every case: a copy)
    tau (rho)        1.9e-07    7.60e-07   7.1e-08 (chunks)
    tau (theta)      1.3e-07    5.20e-07   5.7e-08 (chunks)
"""
import numpy as np
import pytest
import torch

import preprocess_cases as pc
from oracle import preprocess_f64 as pf

pytestmark = pytest.mark.gpu

SENTINEL = 1.2345678e30
RUNS = [(name, "checkpoint") for name in pc.CASES] + [("pipeline", "whole_list")]


def _run(case, route):
    from vicasplat_amd.raster import backward_debug, forward_debug
    d = torch.device("cuda:0")
    T = lambda a: None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=d)
    C = len(case["cam_objs"])
    cams = case["cams"]
    g = forward_debug(T(case["means"]), T(case["cov"]), T(case["opac"]), T(cams["viewmatrix"]), T(cams["projmatrix"]), T(cams["campos"]),
                      T(cams["tanfov"]), T(np.broadcast_to(pc.BG, (C, 3))), case["H"], case["W"], shs=T(case["shs"]),
                      colors_precomp=T(case["colors_precomp"]), sh_degree=case["sh_degree"], sh_rgb_major=case["sh_rgb_major"],
                      cam_scene=torch.tensor(case["cam_scene"], dtype=torch.int32, device=d), count_touched=False,
                      save_for_backward=route == "checkpoint")
    assert (g["_state"]["out"].buffers[12] is not None) == (route == "checkpoint")     # VS_BUF_CHECKPOINT: the route taken
    rng = np.random.default_rng(len(case["name"]))
    gC = rng.standard_normal((C, 3, case["H"], case["W"])).astype(np.float32)
    gD = (0.3 * rng.standard_normal((C, case["H"], case["W"]))).astype(np.float32)
    b = backward_debug(g, T(gC), T(gD), fill=SENTINEL)
    return g, b


@pytest.mark.parametrize("name,route", RUNS, ids=[f"{n}-{r}" for n, r in RUNS])
def test_preprocess_kernels_against_float64(name, route):
    case = pc.get(name)
    S, P = case["means"].shape[:2]
    C = len(case["cam_objs"])
    g, b = _run(case, route)
    N = lambda t: t.cpu().numpy()
    radii, rect, bits, geom = N(g["radii"]).astype(np.int64), N(g["rect"]).astype(np.int64), N(g["clamped"]), N(g["geom"])
    vis = radii > 0
    fails, lines = [], []
    tag = f"[{name} {route}]"

    def check(cond, msg):
        if not cond:
            fails.append(msg)

    # ------------------------------------------------ forward ------------------------------------------------
    f = pc.reference_forward(case)
    ok = ~f["ambiguous"]
    check(np.array_equal(radii[ok], f["radius"][ok]), "radii differ from the reference's")
    check(np.array_equal(rect[ok], f["rect"][ok]), "tile rectangles differ from the reference's")
    check(np.array_equal(bits[ok & vis], f["clamped"][ok & vis]), "clamp bits differ from the reference's")
    inv = ok & ~f["visible"]
    check(not radii[inv].any() and not rect[inv].any() and not bits[~vis].any(), "an invisible pair carries a radius, a rectangle or clamp bits")
    sel = ok & vis & f["visible"]
    for fam, gpu in (("xy", geom[..., 0:2]), ("conic", geom[..., 4:7]), ("rgb", geom[..., 8:11]), ("depth", geom[..., 11])):
        q = pc.ratio(gpu, f[fam], f["mag"][fam], ~sel[..., None] if gpu.ndim == 3 else ~sel)
        lines.append(f"{tag} forward {fam}: {q:.3e} of mag (bound {pc.GPU_MARGIN * pc.RHO32[fam]:.2e})")
        check(q <= pc.GPU_MARGIN * pc.RHO32[fam], f"forward {fam}: {q:.3e} of mag > {pc.GPU_MARGIN * pc.RHO32[fam]:.2e}")
    check(np.array_equal(geom[..., 7][sel], case["opac"][case["cam_scene"]][sel]), "the record's opacity is not the input's")
    sel_e = sel & ~f["amb"]["tau"]
    e_ok = pf.extents_ok(geom[..., 2:4], f["ext"])[sel_e]
    check(e_ok.all(), f"{int((~e_ok).sum())} extents outside [true, 1.011 x true + 0.051]")

    # ------------------------------------------------ backward ------------------------------------------------
    rec = N(b["records"])
    check(not rec[~vis].any(), "a gradient record of an invisible pair is not zero")
    r = pc.reference_backward(case, rec, vis, bits)
    try:
        pc.exclusion_cap(case, vis, f["ambiguous"] | r["ambiguous"])
    except AssertionError as e:
        fails.append(f"exclusion cap: {e}")
    shs = None
    if case["shs"] is not None:
        M = case["shs"].shape[3] if case["sh_rgb_major"] else case["shs"].shape[2]
        shs = N(b["shs"]).reshape(S, P, 3, M) if case["sh_rgb_major"] else N(b["shs"])
    gpu = dict(means3D=N(b["means3D"]), cov6=N(b["cov3D"]), opacities=N(b["opacities"]), means2D=N(b["means2D"]),
               tau_rho=N(b["tau"])[:, :3], tau_theta=N(b["tau"])[:, 3:], shs=shs,
               colors_precomp=None if b["colors_precomp"] is None else N(b["colors_precomp"]))
    for fam, (ref, mag, excl) in pc.families(case, r).items():
        out = gpu[fam]
        check(not (out == np.float32(SENTINEL)).any(), f"{fam}: {int((out == np.float32(SENTINEL)).sum())} elements never written")
        q = pc.ratio(out, ref, mag, excl)
        lines.append(f"{tag} backward {fam}: {q:.3e} of mag (bound {pc.GPU_MARGIN * pc.RHO32[fam]:.2e})")
        check(q <= pc.GPU_MARGIN * pc.RHO32[fam], f"backward {fam}: {q:.3e} of mag > {pc.GPU_MARGIN * pc.RHO32[fam]:.2e}")
    check(not gpu["means2D"][~vis].any(), "dL_dmeans2D is not zero at an invisible pair")
    blind = ~vis.any(1)
    check(not N(b["tau"])[blind].any(), "dL_dtau of a camera that sees nothing is not zero")
    for s in range(S):
        if not (case["cam_scene"] == s).any():
            check(all(not v[s].any() for k, v in gpu.items() if v is not None and k not in ("means2D", "tau_rho", "tau_theta")),
                  f"scene {s} has no camera but a non-zero gradient")
    if shs is not None:
        hi = shs[..., 16:] if case["sh_rgb_major"] else shs[:, :, 16:]
        check(not hi.any(), "SH gradient of a coefficient k >= 16 is not zero")
    if case["cov"].ndim == 4:
        check(np.array_equal(gpu["cov6"], gpu["cov6"].transpose(0, 1, 3, 2)), "the 3 x 3 covariance gradient is not symmetric")
    # what the case was built for, from the GPU's own decisions
    if name == "pipeline":
        check(blind.sum() == 0 and [int((case["cam_scene"] == s).sum()) for s in range(4)] == [0, 1, 2, 36], "pipeline: camera map")
    if name == "clamps":
        k = case["overflow"]
        sees = np.arange(C) != case["blind_camera"]
        check(blind[case["blind_camera"]] and vis[sees, k].all(), "clamps: the blind camera sees something / the huge Gaussian is culled")
        check(not r["decisions"]["d2inv_nz"][sees, k].any(), "clamps: det^2 of the huge Gaussian does not overflow")
        check(not gpu["cov6"][0, k].any(), "clamps: covariance-path gradient of the overflowing Gaussian is not exactly zero")
        check(gpu["means3D"][0, k].any() and gpu["shs"][0, k, 0].any() and rec[sees, k, 9].all(),
              "clamps: mean / colour / depth path of the overflowing Gaussian is zero")
    print("\n" + "\n".join(lines))
    assert not fails, f"{tag} " + "; ".join(fails)
