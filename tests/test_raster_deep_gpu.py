"""Rasterizer render backward on deep and saturated tiles against the float64 reference (oracle/raster_f64.py).  -m gpu.

Every case runs on both backward routes -- the segment replay from the forward's checkpoints (VS_RASTER_SAVE_FOR_BACKWARD, the
route of every differentiated call) and the whole-list back-to-front kernel (flag clear) -- with and without a depth gradient
(render_backward_seg_kernel<true> / <false>).  Colours are precomputed, so dL_dcolors_precomp, dL_dopacities and the per-camera
dL_dmeans2D are the render backward's own records.  Per Gaussian and component, away from decisions that rounding can flip:

    |gpu - ref| <= 1e-3 mag + gamma 2^-24 lim + 1e-6 max(mag)        (colours: 1e-4 mag, gamma 0)

gamma = 0 on the whole-list route (no cancellation), 256 on the checkpoint route (its suffix is out . dL minus a prefix)."""
import numpy as np
import pytest
import torch

from oracle import raster_f64 as rf
from oracle import raster_ref as rr

pytestmark = pytest.mark.gpu

BG = np.array([0.3, 0.2, 0.1], np.float32)
GAMMA = dict(checkpoint=256.0, whole_list=0.0)


def _cams(W, H, shifts):
    K = np.array([[rf.F_NORM, 0, 0.5], [0, rf.F_NORM, 0.5], [0, 0, 1]], np.float32)
    E = np.stack([np.eye(4, dtype=np.float32) for _ in shifts])
    for i, (dx, dy) in enumerate(shifts):
        E[i, 0, 3], E[i, 1, 3] = dx, dy
    n = len(shifts)
    return rr.make_cameras(E, np.broadcast_to(K, (n, 3, 3)).copy(), np.full(n, 0.01, np.float32), np.full(n, 100.0, np.float32))


def _grads(C, H, W, seed):
    rng = np.random.default_rng(seed)
    gC = (1 + 0.1 * rng.standard_normal((C, 3, H, W))).astype(np.float32)
    gD = (0.02 * rng.standard_normal((C, H, W))).astype(np.float32)
    return gC, gD


def _case(name):
    """-> scenes [S] (dicts of raster_f64), cameras [C], cam_scene [C], W, H"""
    if name == "multi":
        a, W, H = rf.deep_scene(seed=5, W=32, H=32)
        b, _, _ = rf.saturated_scene(seed=10, W=32, H=32)
        P = min(len(a["opacities"]), len(b["opacities"]))
        a, b = ({k: v[:P] for k, v in s.items()} for s in (a, b))
        return [a, b], _cams(W, H, [(0, 0), (0.04, -0.02), (0, 0), (-0.03, 0.02)]), np.array([0, 0, 1, 1]), W, H
    sc, W, H = dict(deep=rf.deep_scene, saturated=rf.saturated_scene, segments=rf.segment_scene, onewave=rf.onewave_scene)[name]()
    return [sc], _cams(W, H, [(0, 0)]), np.array([0]), W, H


_REF = {}


def _reference(name, depth, g):
    """float64 records per camera from the GPU's own forward records (decisions are the forward's), cached over the routes."""
    key = (name, depth)
    if key not in _REF:
        scenes, cams, cam_scene, W, H = _case(name)
        gC, gD = _grads(len(cams), H, W, seed=len(name))
        refs = []
        for c in range(len(cams)):
            geom = g["geom"][c].cpu().numpy()
            refs.append(rf.render_backward(geom[:, 0:2], geom[:, 4:8], geom[:, 8:11], geom[:, 11], g["ranges"][c].cpu().numpy(),
                                           g["point_list"].cpu().numpy(), g["n_contrib"][c].cpu().numpy(), BG, gC[c],
                                           gD[c] if depth else None, W=W, H=H))
        _REF[key] = refs
    return _REF[key]


def _sum(refs, name):
    """scene-level record of `name` (summed over the scene's cameras, with its mag / lim) as a reference dict for rf.compare"""
    out = {name: sum(r[name] for r in refs), name + "_mag": sum(r[name + "_mag"] for r in refs),
           name + "_lim": sum(r[name + "_lim"] for r in refs)}
    out["ambiguous"] = np.logical_or.reduce([r["ambiguous"] for r in refs])
    return out


def _run(name, route, depth):
    from vicasplat_amd.raster import backward_debug, forward_debug
    d = torch.device("cuda:0")
    scenes, cams, cam_scene, W, H = _case(name)
    T = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=d)
    C = len(cams)
    g = forward_debug(T(np.stack([s["means"] for s in scenes])), T(np.stack([s["cov6"] for s in scenes])),
                      T(np.stack([s["opacities"] for s in scenes])), T(np.stack([c.viewmatrix for c in cams])),
                      T(np.stack([c.projmatrix for c in cams])), T(np.stack([c.campos for c in cams])),
                      T([[c.tanfovx, c.tanfovy] for c in cams]), T(np.broadcast_to(BG, (C, 3))), H, W,
                      colors_precomp=T(np.stack([s["colors"] for s in scenes])),
                      cam_scene=torch.tensor(cam_scene, dtype=torch.int32, device=d) if len(scenes) > 1 else None,
                      count_touched=False, save_for_backward=route == "checkpoint")
    assert (g["_state"]["out"].buffers[12] is not None) == (route == "checkpoint")     # VS_BUF_CHECKPOINT: the route taken
    gC, gD = _grads(C, H, W, seed=len(name))
    b = backward_debug(g, T(gC), T(gD) if depth else None)
    return scenes, cams, cam_scene, W, H, g, b


def _assert_scene_property(name, g, refs, W, H):
    """the property each scene was built for, read from the forward's own outputs"""
    nc = g["n_contrib"].cpu().numpy()
    rg = g["ranges"].cpu().numpy()
    pop = rg[..., 1] - rg[..., 0]
    if name == "deep":
        assert nc.max() > 2048 and pop.max() >= 3000, (nc.max(), pop.max())
        assert not refs[0]["stopped"].any()
    elif name == "saturated":
        seg = refs[0]["stop_at"][refs[0]["stopped"]] // rf.SEG
        assert (seg == 0).sum() >= 10 and (seg >= 3).sum() >= 10, np.unique(seg, return_counts=True)
        assert refs[0]["colors"].shape[0] > 40 and np.abs(BG).sum() > 0
    elif name == "segments":
        assert pop[0, :5].tolist() == list(rf.SEG_LISTS), pop[0]
        for t, n in enumerate(rf.SEG_LISTS):   # the last entry of every list blends somewhere: the segment boundary is reached
            assert nc[0, :, 16 * t:16 * t + 16].max() == n
        assert pop[0, 7] > rf.SEG and nc[0, :, 112:].max() < rf.SEG      # checkpoint 1 of tile 7 is owed by the list, never written
    elif name == "onewave":
        gx, gy = (W + 15) // 16, (H + 15) // 16
        assert gx * gy * len(refs) >= 4096 and rg.shape[1] == gx * gy == 4160       # render_kernel<., 1> wrote the checkpoints
        assert pop[0, -1] > 0 and nc[0].max() > rf.SEG and refs[0]["stopped"].any()   # partial bottom-right tile in the list
    elif name == "multi":
        assert len(refs) == 4 and nc.max() > rf.SEG


@pytest.mark.parametrize("depth", [True, False], ids=["depth", "nodepth"])
@pytest.mark.parametrize("route", ["checkpoint", "whole_list"])
@pytest.mark.parametrize("name", ["deep", "saturated", "segments", "onewave", "multi"])
def test_render_backward_against_float64(name, route, depth):
    scenes, cams, cam_scene, W, H, g, b = _run(name, route, depth)
    refs = _reference(name, depth, g)
    _assert_scene_property(name, g, refs, W, H)
    gamma = GAMMA[route]
    lines = []
    # forward sanity: the reference and the GPU blend the same entries
    for c, r in enumerate(refs):
        assert np.abs(g["color"][c].cpu().numpy() - r["color"]).max() <= 1e-5
        fT = g["final_T"][c].cpu().numpy()
        assert (np.abs(fT - r["final_T"]) / np.maximum(r["final_T"], 1e-30)).max() <= 5e-4
    fails = []
    ratios = {}
    # per camera: dL_dmeans2D
    for c, r in enumerate(refs):
        ok, msg, q = rf.compare(b["means2D"][c].cpu().numpy(), r, "mean2D", gamma, visible=g["radii"][c].cpu().numpy() > 0)
        ratios.setdefault("mean2D", []).append(q)
        if not ok:
            fails.append(f"cam {c}: {msg}")
    # per scene: dL_dopacities, dL_dcolors_precomp (sums over the scene's cameras)
    for s in range(len(scenes)):
        cs = np.nonzero(cam_scene == s)[0]
        vis = np.logical_or.reduce([g["radii"][c].cpu().numpy() > 0 for c in cs])
        for comp, gpu, gm, rel in (("opacity", b["opacities"][s], gamma, 1e-3), ("colors", b["colors_precomp"][s], 0.0, 1e-4)):
            ok, msg, q = rf.compare(gpu.cpu().numpy(), _sum([refs[c] for c in cs], comp), comp, gm, rel=rel, visible=vis)
            ratios.setdefault(comp, []).append(q)
            if not ok:
                fails.append(f"scene {s}: {msg}")
    for comp, qs in ratios.items():
        lines.append(f"[{name} {route} {'depth' if depth else 'nodepth'}] {comp}: {rf.ratio_summary(np.concatenate(qs))}")
    # 3-D level: the float64 records through the oracle's preprocess backward vs dL_dmeans3D / dL_dcov3D
    for s, sc in enumerate(scenes):
        cs = np.nonzero(cam_scene == s)[0]
        ref3 = dict(means3D=0.0, cov3D=0.0)
        amb = np.zeros(len(sc["opacities"]), bool)
        for c in cs:
            of = rr.rasterize_forward(cams[c], W, H, BG, sc["means"], sc["cov6"], None, sc["opacities"], colors_precomp=sc["colors"])
            assert np.array_equal(of["radii"], g["radii"][c].cpu().numpy())
            o3 = rf.preprocess_backward(cams[c], W, H, BG, sc["means"], sc["cov6"], sc["opacities"], sc["colors"], of, refs[c])
            ref3 = {k: ref3[k] + o3[k] for k in ref3}
            amb |= refs[c]["ambiguous"]
        for k in ("means3D", "cov3D"):
            gpu = b[k][s].cpu().numpy().astype(np.float64)
            nr = np.linalg.norm(ref3[k], axis=1)
            sel = (nr > 1e-3 * nr.max()) & ~amb
            e = np.linalg.norm(gpu - ref3[k], axis=1)[sel] / nr[sel]
            lines.append(f"[{name} {route} {'depth' if depth else 'nodepth'}] 3-D {k}: max rel {e.max():.2e} median {np.median(e):.2e} n={sel.sum()}")
            if e.max() > 2e-3:
                fails.append(f"scene {s} {k}: per-Gaussian relative error {e.max():.3e} > 2e-3 ({int((e > 2e-3).sum())} Gaussians)")
    print("\n" + "\n".join(lines))
    assert not fails, "\n".join(fails)
