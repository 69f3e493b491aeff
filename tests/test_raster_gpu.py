"""Parity of the HIP rasterizer forward (through the C ABI) against the CPU oracle.  -m gpu.

Bar: integer tile data (radii, tile rectangles, tile ranges, sorted ids) BIT-IDENTICAL;
renders float-tolerant (|d color| <= 2e-5 typical; a handful of pixels may differ by one alpha threshold flip
because v_exp_f32 and glibc expf differ in the last ulp) and PSNR-equivalent (|dPSNR| <= 1e-4 dB vs a common target).
"""
import math

import numpy as np
import pytest
import torch

from oracle import raster_ref as rr

pytestmark = pytest.mark.gpu

K09 = np.array([[0.9, 0, 0.5], [0, 0.9, 0.5], [0, 0, 1]], np.float32)


def _dev():
    return torch.device("cuda:0")


def _gpu_cams(cams):
    d = _dev()
    t = lambda a: torch.tensor(np.stack(a), dtype=torch.float32, device=d)
    return dict(viewmatrix=t([c.viewmatrix for c in cams]), projmatrix=t([c.projmatrix for c in cams]),
                campos=t([c.campos for c in cams]), tanfov=t([[c.tanfovx, c.tanfovy] for c in cams]))


def _run_gpu(means, cov6, shs, op, cams, W, H, bg, **kw):
    from vicasplat_amd.raster import forward_debug
    d = _dev()
    g = _gpu_cams(cams)
    C = len(cams)
    return forward_debug(torch.tensor(means, dtype=torch.float32, device=d)[None], torch.tensor(cov6, device=d)[None],
                         torch.tensor(op, dtype=torch.float32, device=d)[None], g["viewmatrix"], g["projmatrix"], g["campos"],
                         g["tanfov"], torch.tensor(bg, dtype=torch.float32, device=d).expand(C, 3).contiguous(), H, W,
                         shs=None if shs is None else torch.tensor(shs, dtype=torch.float32, device=d)[None], sh_degree=4, **kw)


def _compare(o, g, c, color_atol=2e-5, max_bad_frac=2e-4):
    """o: oracle dict of view c; g: gpu dict."""
    vis = o["radii"] > 0
    assert np.array_equal(g["radii"][c].cpu().numpy(), o["radii"]), "radii"
    assert np.array_equal(g["rect"][c].cpu().numpy()[vis].astype(np.int32), o["rect"][vis]), "tile rectangles"
    assert g["ranges"][c].cpu().numpy().shape == o["ranges"].shape
    # ranges are offsets into the per-call list; compare per-tile populations and the concatenated sorted ids
    rg = g["ranges"][c].cpu().numpy()
    assert np.array_equal(rg[:, 1] - rg[:, 0], o["ranges"][:, 1] - o["ranges"][:, 0]), "tile populations"
    pl = g["point_list"].cpu().numpy().astype(np.uint32)
    lo, hi = rg[:, 0].min(), rg[:, 1].max()
    assert np.array_equal(pl[lo:hi], o["point_list"]), "sorted Gaussian ids"
    gm = g["geom"][c].cpu().numpy()
    assert np.array_equal(gm[vis, 0:2], o["xy"][vis]), "pixel centres bit-exact (same op order)"
    assert np.array_equal(gm[vis, 11], o["depths"][vis]), "depth keys bit-exact"
    assert np.array_equal(gm[vis, 4:8], o["conic_opacity"][vis]), "conic bit-exact"
    assert np.allclose(gm[vis, 8:11], o["rgb"][vis], atol=1e-6), "SH colours"
    assert np.array_equal(g["clamped"][c].cpu().numpy()[vis], (o["clamped"][vis] * np.array([1, 2, 4], np.uint8)).sum(-1)), "clamp mask"
    col = g["color"][c].cpu().numpy()
    bad = np.abs(col - o["color"]) > color_atol
    assert bad.mean() <= max_bad_frac, f"{bad.sum()} colour values differ by > {color_atol}"
    assert np.abs(col - o["color"]).max() < 2e-2
    dep = g["depth"][c].cpu().numpy()
    assert (np.abs(dep - o["depth"]) > 1e-4 * max(1.0, np.abs(o["depth"]).max())).mean() <= max_bad_frac
    assert (np.abs(g["opacity"][c].cpu().numpy() - o["opacity"]) > color_atol).mean() <= max_bad_frac
    assert (g["n_contrib"][c].cpu().numpy() != o["n_contrib"]).mean() <= 10 * max_bad_frac
    nt = g["n_touched"][c].cpu().numpy()
    assert (nt != o["n_touched"]).mean() <= 1e-3 and np.abs(nt - o["n_touched"]).max() <= 2


def _random_small(P, seed, spread=0.9):
    rng = np.random.default_rng(seed)
    means = np.stack([rng.uniform(-spread, spread, P), rng.uniform(-0.6, 0.6, P), rng.uniform(1.5, 4.0, P)], -1).astype(np.float32)
    A = rng.standard_normal((P, 3, 3)) * 0.08
    cov = (A @ A.transpose(0, 2, 1) + 1e-4 * np.eye(3)).astype(np.float32)
    sh = (rng.standard_normal((P, 25, 3)) * rr.SH_MASK[None, :, None]).astype(np.float32)
    sh[:, 0] = rng.standard_normal((P, 3)) * 0.7
    op = rng.uniform(0.2, 0.95, P).astype(np.float32)
    return means, cov, sh, op


def _two_cams():
    yaw = 0.1
    E = np.eye(4, dtype=np.float32)
    E[:3, :3] = [[math.cos(yaw), 0, math.sin(yaw)], [0, 1, 0], [-math.sin(yaw), 0, math.cos(yaw)]]
    E[:3, 3] = [0.1, -0.05, 0.02]
    Es = np.stack([np.eye(4, dtype=np.float32), E])
    return rr.make_cameras(Es, np.stack([K09, K09]), np.full(2, 0.01, np.float32), np.full(2, 100.0, np.float32))


@pytest.mark.parametrize("W,H,P", [(48, 32, 60), (64, 64, 500), (50, 37, 300), (256, 256, 5000)])
def test_forward_matches_oracle_small(W, H, P):
    means, cov, sh, op = _random_small(P, seed=P)
    cams = _two_cams()
    bg = np.array([0.2, 0.1, 0.3], np.float32)
    c6 = rr.cov6(cov)
    g = _run_gpu(means, c6, sh, op, cams, W, H, bg)
    tot = 0
    for c, cam in enumerate(cams):
        o = rr.rasterize_forward(cam, W, H, bg, means, c6, sh, op)
        _compare(o, g, c)
        tot += o["R"]
    assert g["R"] == tot


def test_forward_config3_scene_131k():
    """BASELINE.json config 3: re10k_2view-sized scene, ~131k Gaussians, 256x256, 4 target views."""
    sc = rr.synthetic_scene(V=2, res=256, Vt=4, seed=0)
    cams = rr.make_cameras(sc["extrinsics"], sc["intrinsics"], sc["near"], sc["far"])
    shs = np.ascontiguousarray(np.transpose(sc["harmonics"], (0, 2, 1)))
    c6 = rr.cov6(sc["covariances"])
    bg = np.zeros(3, np.float32)
    g = _run_gpu(sc["means"], c6, shs, sc["opacities"], cams, 256, 256, bg)
    rng = np.random.default_rng(0)
    target = rng.uniform(0, 1, (3, 256, 256)).astype(np.float32)
    for c, cam in enumerate(cams):
        o = rr.rasterize_forward(cam, 256, 256, bg, sc["means"], c6, shs, sc["opacities"])
        _compare(o, g, c)
        psnr = lambda img: -10 * math.log10(float(((np.clip(img, 0, 1) - target) ** 2).mean()))
        assert abs(psnr(g["color"][c].cpu().numpy()) - psnr(o["color"])) <= 1e-4


def test_oversize_tile_radix_path():
    # > 8192 Gaussians in ONE tile: exercises the workgroup radix sort (global ping-pong) incl. depth ties
    P = 9000
    rng = np.random.default_rng(1)
    means = np.stack([rng.uniform(-0.02, 0.02, P), rng.uniform(-0.02, 0.02, P), rng.uniform(2.0, 3.0, P)], -1).astype(np.float32)
    means[:, 2] = np.round(means[:, 2] * 64) / 64  # many exact depth ties -> index tie-break matters
    cov = np.tile((1e-6 * np.eye(3, dtype=np.float32))[None], (P, 1, 1))
    sh = np.zeros((P, 25, 3), np.float32); sh[:, 0] = rng.standard_normal((P, 3))
    op = np.full(P, 0.02, np.float32)
    cams = _two_cams()[:1]
    W = H = 32
    bg = np.zeros(3, np.float32)
    g = _run_gpu(means, rr.cov6(cov), sh, op, cams, W, H, bg)
    o = rr.rasterize_forward(cams[0], W, H, bg, means, rr.cov6(cov), sh, op)
    assert (o["ranges"][:, 1] - o["ranges"][:, 0]).max() > 8192
    _compare(o, g, 0, color_atol=1e-4)


@pytest.mark.parametrize("P,tied", [(3000, 1500), (20000, 0), (1500, 0), (5000, 400)])
def test_large_tile_sort_paths(P, tied):
    """One tile holding P Gaussians: bucket + LDS-sort path (spread depths, any size), the radix fallback (more than 512
    keys at one depth) and mixtures; the sorted id list must match the oracle's (depth, index) order exactly."""
    rng = np.random.default_rng(P + tied)
    means = np.stack([rng.uniform(-0.02, 0.02, P), rng.uniform(-0.02, 0.02, P), rng.uniform(1.5, 6.0, P)], -1).astype(np.float32)
    if tied:
        means[rng.permutation(P)[:tied], 2] = 2.75
    cov = np.tile((1e-6 * np.eye(3, dtype=np.float32))[None], (P, 1, 1))
    sh = np.zeros((P, 25, 3), np.float32); sh[:, 0] = rng.standard_normal((P, 3))
    op = np.full(P, 0.01, np.float32)
    cams = _two_cams()[:1]
    W = H = 32
    bg = np.zeros(3, np.float32)
    g = _run_gpu(means, rr.cov6(cov), sh, op, cams, W, H, bg)
    o = rr.rasterize_forward(cams[0], W, H, bg, means, rr.cov6(cov), sh, op)
    assert (o["ranges"][:, 1] - o["ranges"][:, 0]).max() > min(P, 1024) - 1
    _compare(o, g, 0, color_atol=1e-4)


def test_full_size_scene_invariants():
    """BASELINE config-4 size (8 views -> 524 288 Gaussians, 256x256 targets): size-independent properties of the forward
    state, checked on the device -- per-tile lists sorted by (depth, index), every listed Gaussian overlaps its tile,
    populations add up to R, opacity = 1 - final_T, n_contrib <= tile population."""
    d = _dev()
    sc = rr.synthetic_scene(V=8, res=256, Vt=4, seed=3)
    cams = rr.make_cameras(sc["extrinsics"], sc["intrinsics"], sc["near"], sc["far"])
    shs = np.ascontiguousarray(np.transpose(sc["harmonics"], (0, 2, 1)))
    g = _run_gpu(sc["means"], rr.cov6(sc["covariances"]), shs, sc["opacities"], cams, 256, 256, np.zeros(3, np.float32))
    C, P = len(cams), sc["means"].shape[0]
    assert P == 524288
    rg = g["ranges"].long()                       # [C, tiles, 2]
    pop = rg[..., 1] - rg[..., 0]
    assert int(pop.sum()) == g["R"] == g["point_list"].numel()
    assert torch.equal(rg[..., 0].flatten()[1:], rg[..., 1].flatten()[:-1]), "ranges tile the list without gaps"
    pl = g["point_list"].long()
    tile_of = torch.repeat_interleave(torch.arange(C * 256, device=d), pop.flatten())
    cam_of, t_in = tile_of // 256, tile_of % 256
    depth = g["geom"][cam_of, pl, 11]
    same_tile = tile_of[1:] == tile_of[:-1]
    dd = depth[1:] - depth[:-1]
    assert bool((dd[same_tile] >= 0).all()), "depth-sorted inside every tile"
    tie = same_tile & (dd == 0)
    assert bool((pl[1:][tie] > pl[:-1][tie]).all()), "ties broken by Gaussian index"
    rect = g["rect"][cam_of, pl].long()           # min.x min.y max.x max.y (exclusive max)
    tx, ty = t_in % 16, t_in // 16
    assert bool(((tx >= rect[:, 0]) & (tx < rect[:, 2]) & (ty >= rect[:, 1]) & (ty < rect[:, 3])).all())
    assert bool((g["radii"][cam_of, pl] > 0).all())
    # every (visible Gaussian, covered tile) pair is listed exactly once
    r_all = g["rect"].long()
    want = ((r_all[..., 2] - r_all[..., 0]) * (r_all[..., 3] - r_all[..., 1]))[g["radii"] > 0].sum()
    assert int(want) == g["R"]
    assert torch.allclose(g["opacity"], 1.0 - g["final_T"], atol=1e-6)
    tile_pop_px = pop.view(C, 16, 16).repeat_interleave(16, 1).repeat_interleave(16, 2)
    assert bool((g["n_contrib"] <= tile_pop_px).all()) and bool((g["n_contrib"] >= 0).all())
    assert bool(torch.isfinite(g["color"]).all()) and float(g["final_T"].min()) >= 0.0 and float(g["final_T"].max()) <= 1.0


def test_full_size_render_is_linear_in_colour_affine_in_background_and_order_free():
    """BASELINE config-4 size (524 288 Gaussians, 4 target views of 256x256): properties the blend C = sum_i c_i a_i T_i + bg T_final has at ANY
    size, with the geometry (means, covariances, opacities -> a_i, T_i, the tile lists) held fixed --
      * linear in the per-Gaussian colours: render(2 c1 - 0.5 c2, bg = 0) = 2 render(c1) - 0.5 render(c2);
      * affine in the background: render(c, bg) = render(c, 0) + bg * final_T, and opacity / depth / n_contrib do not depend on it;
      * free of the ORDER the Gaussians are stored in: a permuted scene gives the same tile populations, the same sorted depths and -- depth
        ties (broken by index) aside -- the same image."""
    from vicasplat_amd.raster import forward_debug
    d = _dev()
    sc = rr.synthetic_scene(V=8, res=256, Vt=4, seed=5)
    cams = rr.make_cameras(sc["extrinsics"], sc["intrinsics"], sc["near"], sc["far"])
    gc = _gpu_cams(cams)
    C, P = len(cams), sc["means"].shape[0]
    assert P == 524288
    T = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=d)[None]
    rng = np.random.default_rng(0)
    c1, c2 = rng.uniform(0, 1, (P, 3)).astype(np.float32), rng.uniform(0, 1, (P, 3)).astype(np.float32)
    mean_, cov_, op_ = T(sc["means"]), T(rr.cov6(sc["covariances"])), T(sc["opacities"])
    zero = torch.zeros(C, 3, device=d)
    run = lambda col, bg, m=mean_, cv=cov_, o=op_: forward_debug(m, cv, o, gc["viewmatrix"], gc["projmatrix"], gc["campos"], gc["tanfov"], bg, 256, 256,
                                                                 colors_precomp=col)
    r1, r2 = run(T(c1), zero), run(T(c2), zero)
    r12 = run(T(2.0 * c1 - 0.5 * c2), zero)
    assert float((r1["opacity"] > 0.5).float().mean()) > 0.3, "the scene must actually cover the image"
    assert torch.equal(r1["point_list"], r2["point_list"]) and torch.equal(r1["final_T"], r2["final_T"]) and torch.equal(r1["n_contrib"], r2["n_contrib"])
    lin = 2.0 * r1["color"] - 0.5 * r2["color"]
    assert float((r12["color"] - lin).abs().max()) <= 5e-5 * max(1.0, float(lin.abs().max())), float((r12["color"] - lin).abs().max())
    bg = torch.tensor([[0.25, 0.5, 0.75]], device=d).expand(C, 3).contiguous()
    rb = run(T(c1), bg)
    assert torch.equal(rb["final_T"], r1["final_T"]) and torch.equal(rb["opacity"], r1["opacity"]) and torch.equal(rb["depth"], r1["depth"])
    assert torch.equal(rb["n_contrib"], r1["n_contrib"])
    want = r1["color"] + bg[:, :, None, None] * r1["final_T"][:, None]
    assert float((rb["color"] - want).abs().max()) <= 2e-6
    perm = rng.permutation(P)
    rp = run(T(c1[perm]), zero, T(sc["means"][perm]), T(rr.cov6(sc["covariances"])[perm]), T(sc["opacities"][perm]))
    assert rp["R"] == r1["R"]
    pop = lambda r: (r["ranges"][..., 1] - r["ranges"][..., 0])
    assert torch.equal(pop(rp), pop(r1)), "tile populations do not depend on the storage order"
    inv = torch.tensor(perm, device=d)                  # new index j holds old Gaussian perm[j]
    assert torch.equal(rp["radii"], r1["radii"][:, inv])
    # the sorted DEPTH sequence of every tile list is the same; the ids agree wherever the depth is not tied inside its list
    def keyed(r):
        rg = r["ranges"].long()
        tile_of = torch.repeat_interleave(torch.arange(C * 256, device=d), (rg[..., 1] - rg[..., 0]).flatten())
        return tile_of, r["geom"][tile_of // 256, r["point_list"].long(), 11]
    t1, d1 = keyed(r1)
    tp, dp = keyed(rp)
    assert torch.equal(t1, tp) and torch.equal(d1, dp)
    tied = torch.zeros_like(d1, dtype=torch.bool)
    eq = (d1[1:] == d1[:-1]) & (t1[1:] == t1[:-1])
    tied[1:] |= eq; tied[:-1] |= eq
    assert torch.equal(inv[rp["point_list"].long()][~tied], r1["point_list"].long()[~tied])
    tf = float(tied.float().mean())
    assert tf < 0.02, tf
    assert float((rp["color"] - r1["color"]).abs().max()) <= (2e-6 if tf == 0.0 else 2e-2)
    assert float(((rp["color"] - r1["color"]).abs() > 2e-6).float().mean()) <= 1e-4 + 20 * tf


def test_empty_and_culled():
    d = _dev()
    cams = _two_cams()
    bg = np.array([0.1, 0.2, 0.3], np.float32)
    means = np.array([[0, 0, 0.2], [0, 0, -1.0], [50.0, 0, 1.0]], np.float32)  # z<=0.2, behind, far off-screen
    cov = np.tile((1e-4 * np.eye(3, dtype=np.float32))[None], (3, 1, 1))
    sh = np.zeros((3, 25, 3), np.float32)
    g = _run_gpu(means, rr.cov6(cov), sh, np.ones(3, np.float32), cams, 32, 32, bg)
    assert g["R"] == 0 and int(g["radii"].abs().sum()) == 0
    assert torch.allclose(g["color"], torch.tensor(bg, device=d)[None, :, None, None].expand(2, 3, 32, 32))
    assert float(g["depth"].abs().max()) == 0 and float(g["opacity"].abs().max()) == 0
    # P == 0
    g = _run_gpu(np.zeros((0, 3), np.float32), np.zeros((0, 6), np.float32), np.zeros((0, 25, 3), np.float32),
                 np.zeros(0, np.float32), cams, 32, 32, bg)
    assert g["R"] == 0 and torch.allclose(g["color"][0, :, 0, 0].cpu(), torch.tensor(bg))


def test_layout_flags_and_precomputed_colors():
    """[S,P,3,M] SH + [S,P,3,3] covariance (encoder-native) give the same bits as [S,P,M,3] + cov6."""
    from vicasplat_amd.raster import forward_debug
    d = _dev()
    means, cov, sh, op = _random_small(400, seed=11)
    cams = _two_cams()
    gc = _gpu_cams(cams)
    bg = torch.zeros(2, 3, device=d)
    T = lambda a: torch.tensor(a, dtype=torch.float32, device=d)[None]
    a = forward_debug(T(means), T(rr.cov6(cov)), T(op), gc["viewmatrix"], gc["projmatrix"], gc["campos"], gc["tanfov"], bg, 64, 64,
                      shs=T(sh), sh_degree=4)
    b = forward_debug(T(means), T(cov), T(op), gc["viewmatrix"], gc["projmatrix"], gc["campos"], gc["tanfov"], bg, 64, 64,
                      shs=T(np.ascontiguousarray(sh.transpose(0, 2, 1))), sh_degree=4, sh_rgb_major=True)
    assert torch.equal(a["color"], b["color"]) and torch.equal(a["radii"], b["radii"]) and torch.equal(a["point_list"], b["point_list"])
    # colors_precomp path vs oracle
    cp = np.random.default_rng(3).uniform(0, 1, (400, 3)).astype(np.float32)
    g = forward_debug(T(means), T(rr.cov6(cov)), T(op), gc["viewmatrix"], gc["projmatrix"], gc["campos"], gc["tanfov"], bg, 64, 64,
                      colors_precomp=T(cp))
    o = rr.rasterize_forward(cams[1], 64, 64, np.zeros(3, np.float32), means, rr.cov6(cov), None, op, colors_precomp=cp)
    assert np.abs(g["color"][1].cpu().numpy() - o["color"]).max() < 2e-5


def test_render_cuda_call_surface():
    """render_cuda(...) with the reference's argument layout: [b,g,...] per-camera sets and [g,...] shared sets."""
    from vicasplat_amd.model.decoder.cuda_splatting import render_cuda
    from vicasplat_amd.model.decoder import DecoderSplattingCUDACfg, get_decoder
    from vicasplat_amd.model.types import Gaussians
    d = _dev()
    sc = rr.synthetic_scene(V=2, res=64, Vt=3, seed=2)
    T = lambda a: torch.tensor(a, dtype=torch.float32, device=d)
    E, K, near, far = T(sc["extrinsics"]), T(sc["intrinsics"]), T(sc["near"]), T(sc["far"])
    bgc = torch.zeros(3, 3, device=d)
    m, cv, sh, op = T(sc["means"]), T(sc["covariances"]), T(sc["harmonics"]), T(sc["opacities"])
    img_shared, dep_shared = render_cuda(E, K, near, far, (64, 64), bgc, m, cv, sh, op)
    rep = lambda t: t[None].expand(3, *t.shape).contiguous()
    img_rep, dep_rep = render_cuda(E, K, near, far, (64, 64), bgc, rep(m), rep(cv), rep(sh), rep(op))
    assert img_shared.shape == (3, 3, 64, 64) and dep_shared.shape == (3, 64, 64)
    assert torch.equal(img_shared, img_rep) and torch.equal(dep_shared, dep_rep)
    outs = rr.render_views(sc, res=64)
    for c in range(3):
        assert np.abs(img_shared[c].cpu().numpy() - outs[c]["color"]).max() < 5e-4  # camera matrices built independently
    dec = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", [0.0, 0.0, 0.0], False)).to(d)
    out = dec(Gaussians(m[None], cv[None], sh[None], op[None]), E[None], K[None], near[None], far[None], (64, 64))
    assert out.color.shape == (1, 3, 3, 64, 64) and torch.equal(out.color[0], img_shared)


def test_diff_gaussian_rasterization_drop_in():
    from vicasplat_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    d = _dev()
    means, cov, sh, op = _random_small(300, seed=5)
    cam = _two_cams()[1]
    T = lambda a: torch.tensor(a, dtype=torch.float32, device=d)
    st = GaussianRasterizationSettings(image_height=48, image_width=64, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy,
                                       bg=torch.zeros(3, device=d), scale_modifier=1.0, viewmatrix=T(cam.viewmatrix).view(4, 4),
                                       projmatrix=T(cam.projmatrix).view(4, 4), projmatrix_raw=T(cam.projmatrix_raw).view(4, 4),
                                       sh_degree=4, campos=T(cam.campos), prefiltered=False, debug=False)
    image, radii, depth, opacity, n_touched = GaussianRasterizer(st)(
        means3D=T(means), means2D=torch.zeros(300, 3, device=d), shs=T(sh), colors_precomp=None, opacities=T(op)[:, None],
        cov3D_precomp=T(rr.cov6(cov)), theta=None, rho=None)
    o = rr.rasterize_forward(cam, 64, 48, np.zeros(3, np.float32), means, rr.cov6(cov), sh, op)
    assert image.shape == (3, 48, 64) and depth.shape == (1, 48, 64) and opacity.shape == (1, 48, 64)
    assert radii.dtype == torch.int32 and np.array_equal(radii.cpu().numpy(), o["radii"])
    assert np.abs(image.cpu().numpy() - o["color"]).max() < 2e-5
    assert np.array_equal(n_touched.cpu().numpy(), o["n_touched"])
    with pytest.raises(Exception):
        GaussianRasterizer(st)(means3D=T(means), means2D=None, shs=None, colors_precomp=None, opacities=T(op), cov3D_precomp=T(rr.cov6(cov)))


def test_no_cpu_fallback():
    from vicasplat_amd.model.decoder.cuda_splatting import render_cuda
    sc = rr.synthetic_scene(V=2, res=16, Vt=1, seed=2)
    T = lambda a: torch.tensor(a, dtype=torch.float32)
    with pytest.raises(RuntimeError):
        render_cuda(T(sc["extrinsics"]), T(sc["intrinsics"]), T(sc["near"]), T(sc["far"]), (16, 16), torch.zeros(1, 3),
                    T(sc["means"]), T(sc["covariances"]), T(sc["harmonics"]), T(sc["opacities"]))


# ---------------------------------------------------------------------------------------------------------
# backward: HIP kernels vs the C oracle (itself pinned to autograd + finite differences)
# ---------------------------------------------------------------------------------------------------------
def _close(a, b, name, rtol):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    scale = np.abs(b).max() + 1e-12
    assert np.abs(a - b).max() <= rtol * scale, (name, float(np.abs(a - b).max()), float(scale))


@pytest.fixture(params=["0", "4"])
def rbwd_waves(request, monkeypatch):
    """Both render-backward routes (round 6; the backward picks one by the presence of the forward's checkpoints): 0 = the default of every
    differentiated call -- the segment-parallel replay from the forward's blending checkpoints (front to back, a wave per 512-entry segment,
    atomics-free staging); 4 = the whole-list kernel a caller without VS_RASTER_SAVE_FOR_BACKWARD gets (four waves per tile, back to front from
    final_T), reached as that caller does: the flag _Rasterize.forward ORs in is 0, so the forward stores no VS_BUF_CHECKPOINT."""
    if request.param == "4":
        from vicasplat_amd import _lib
        monkeypatch.setattr(_lib, "VS_RASTER_SAVE_FOR_BACKWARD", 0)
    return request.param


@pytest.mark.parametrize("W,H,P", [(48, 32, 60), (64, 64, 400), (40, 24, 80)])     # (40 x 24: partial tiles on both edges)
def test_backward_matches_oracle(W, H, P, rbwd_waves):
    from vicasplat_amd.raster import rasterize
    d = _dev()
    means, cov, sh, op = _random_small(P, seed=100 + P)
    cams = _two_cams()
    gc = _gpu_cams(cams)
    bg = np.array([0.2, 0.1, 0.3], np.float32)
    rng = np.random.default_rng(7)
    gC = rng.standard_normal((2, 3, H, W)).astype(np.float32)
    gD = (rng.standard_normal((2, H, W)) * 0.3).astype(np.float32)
    T = lambda a, g=False: torch.tensor(a, dtype=torch.float32, device=d).requires_grad_(g)
    tm, tc, ts, to = T(means[None], True), T(rr.cov6(cov)[None], True), T(sh[None], True), T(op[None], True)
    theta, rho = torch.zeros(2, 3, device=d, requires_grad=True), torch.zeros(2, 3, device=d, requires_grad=True)
    color, radii, depth, _, _ = rasterize(tm, tc, to, gc["viewmatrix"], gc["projmatrix"], gc["campos"], gc["tanfov"],
                                          T(bg).expand(2, 3).contiguous(), H, W, shs=ts, sh_degree=4, theta=theta, rho=rho)
    ((color * T(gC)).sum() + (depth * T(gD)).sum()).backward()
    c6 = rr.cov6(cov)
    exp = dict(means=0, cov=0, sh=0, op=0)
    taus = []
    for c, cam in enumerate(cams):
        fwd = rr.rasterize_forward(cam, W, H, bg, means, c6, sh, op)
        b = rr.rasterize_backward(cam, W, H, bg, means, c6, sh, op, fwd, gC[c], gD[c])
        exp["means"] = exp["means"] + b["means3D"]; exp["cov"] = exp["cov"] + b["cov3D"]
        exp["sh"] = exp["sh"] + b["shs"]; exp["op"] = exp["op"] + b["opacities"]
        taus.append(b["tau"])
    _close(tm.grad[0].cpu(), exp["means"], "means3D", 2e-3)
    _close(tc.grad[0].cpu(), exp["cov"], "cov3D", 2e-3)
    _close(ts.grad[0].cpu(), exp["sh"], "shs", 2e-3)
    _close(to.grad[0].cpu(), exp["op"], "opacity", 2e-3)
    assert float(ts.grad[0, :, 16:].abs().max()) == 0.0  # band 4: never read, zero gradient
    tau = np.stack(taus)
    _close(rho.grad.cpu(), tau[:, :3], "rho", 5e-3)
    _close(theta.grad.cpu(), tau[:, 3:], "theta", 5e-3)


def test_backward_through_render_cuda_native_layouts(rbwd_waves):
    """[S,P,3,3] covariances + [S,P,3,25] harmonics (encoder-native layouts): gradients land in those layouts."""
    from vicasplat_amd.model.decoder.cuda_splatting import render_cuda
    d = _dev()
    sc = rr.synthetic_scene(V=1, res=32, Vt=2, seed=4)
    T = lambda a, g=False: torch.tensor(a, dtype=torch.float32, device=d).requires_grad_(g)
    m, cv, sh, op = T(sc["means"], True), T(sc["covariances"], True), T(sc["harmonics"], True), T(sc["opacities"], True)
    img, dep = render_cuda(T(sc["extrinsics"]), T(sc["intrinsics"]), T(sc["near"]), T(sc["far"]), (32, 32), torch.zeros(2, 3, device=d), m, cv, sh, op)
    rng = np.random.default_rng(3)
    gC = rng.standard_normal((2, 3, 32, 32)).astype(np.float32)
    (img * T(gC)).sum().backward()
    cams = rr.make_cameras(sc["extrinsics"], sc["intrinsics"], sc["near"], sc["far"])
    shs = np.ascontiguousarray(np.transpose(sc["harmonics"], (0, 2, 1)))
    c6 = rr.cov6(sc["covariances"])
    e_m = e_c = e_s = e_o = 0
    for c, cam in enumerate(cams):
        fwd = rr.rasterize_forward(cam, 32, 32, np.zeros(3, np.float32), sc["means"], c6, shs, sc["opacities"])
        b = rr.rasterize_backward(cam, 32, 32, np.zeros(3, np.float32), sc["means"], c6, shs, sc["opacities"], fwd, gC[c], None)
        e_m = e_m + b["means3D"]; e_c = e_c + b["cov3D"]; e_s = e_s + b["shs"]; e_o = e_o + b["opacities"]
    _close(m.grad.cpu(), e_m, "means", 3e-3)
    _close(op.grad.cpu(), e_o, "opacity", 3e-3)
    _close(sh.grad.cpu(), np.transpose(e_s, (0, 2, 1)), "harmonics [P,3,25]", 3e-3)
    g33 = cv.grad.cpu().numpy()
    assert np.allclose(g33, np.transpose(g33, (0, 2, 1)))  # symmetric spread
    g6 = np.stack([g33[:, 0, 0], 2 * g33[:, 0, 1], 2 * g33[:, 0, 2], g33[:, 1, 1], 2 * g33[:, 1, 2], g33[:, 2, 2]], -1)
    _close(g6, e_c, "covariances", 3e-3)


@pytest.mark.gpu
def test_differentiated_renders_do_not_accumulate_memory():
    """Repeated render + backward (a training loop, or the 100-iteration pose alignment of evaluation) must not grow the live
    device memory: the autograd node may not hold its own outputs (they hold it)."""
    import gc
    from vicasplat_amd.model.decoder.cuda_splatting import render_cuda
    d = _dev()
    sc = rr.synthetic_scene(V=1, res=64, Vt=2, seed=5)
    T = lambda a, g=False: torch.tensor(a, dtype=torch.float32, device=d).requires_grad_(g)
    base = (T(sc["means"]), T(sc["covariances"]), T(sc["harmonics"]), T(sc["opacities"]))
    cam = (T(sc["extrinsics"]), T(sc["intrinsics"]), T(sc["near"]), T(sc["far"]))
    live = []
    for it in range(6):
        m, cv, sh, op = [(b * 1.0).requires_grad_() for b in base]     # fresh graph leaves every iteration, as a model output would be
        big = torch.zeros(1 << 22, device=d, requires_grad=True)      # 16 MB hanging off the graph of the means: leaks show up clearly
        img, dep = render_cuda(*cam, (64, 64), torch.zeros(2, 3, device=d), m + big[:3].sum() * 0, cv, sh, op)
        (img.sum() + dep.sum()).backward()
        del m, cv, sh, op, big, img, dep
        gc.collect()
        torch.cuda.synchronize()
        live.append(torch.cuda.memory_allocated(d))
    assert live[-1] <= live[1], live


# ---------------------------------------------------------------------------------------------------------
# backward at scale (BASELINE config 3 scene: 131 072 Gaussians, 256x256): parity vs the C oracle, run-to-run spread of the
# float-atomic accumulation, finite differences of the camera twist
# ---------------------------------------------------------------------------------------------------------
def _config3_backward(n_views=1, seed_grad=11):
    from vicasplat_amd.raster import rasterize
    d = _dev()
    sc = rr.synthetic_scene(V=2, res=256, Vt=4, seed=0)
    cams = rr.make_cameras(sc["extrinsics"], sc["intrinsics"], sc["near"], sc["far"])[:n_views]
    gc = _gpu_cams(cams)
    shs = np.ascontiguousarray(np.transpose(sc["harmonics"], (0, 2, 1)))
    c6 = rr.cov6(sc["covariances"])
    rng = np.random.default_rng(seed_grad)
    gC = rng.standard_normal((n_views, 3, 256, 256)).astype(np.float32)
    gD = (rng.standard_normal((n_views, 256, 256)) * 0.3).astype(np.float32)
    T = lambda a, g=False: torch.tensor(a, dtype=torch.float32, device=d).requires_grad_(g)

    def run():
        grads = True
        tm, tc, ts, to = T(sc["means"][None], grads), T(c6[None], grads), T(shs[None], grads), T(sc["opacities"][None], grads)
        theta = torch.zeros(n_views, 3, device=d, requires_grad=True)     # zero-valued inputs that only receive dL/dtau
        rho = torch.zeros(n_views, 3, device=d, requires_grad=True)
        color, radii, depth, _, _ = rasterize(tm, tc, to, gc["viewmatrix"], gc["projmatrix"], gc["campos"], gc["tanfov"],
                                              torch.zeros(n_views, 3, device=d), 256, 256, shs=ts, sh_degree=4, theta=theta, rho=rho)
        loss = (color.double() * T(gC).double()).sum() + (depth.double() * T(gD).double()).sum()
        loss.backward()
        return loss.detach(), dict(means=tm.grad[0], cov=tc.grad[0], sh=ts.grad[0], op=to.grad[0], rho=rho.grad, theta=theta.grad)

    return sc, cams, c6, shs, gC, gD, run


def test_backward_config3_scene_131k_matches_oracle(rbwd_waves):
    sc, cams, c6, shs, gC, gD, run = _config3_backward(1)
    _, g = run()
    bg = np.zeros(3, np.float32)
    fwd = rr.rasterize_forward(cams[0], 256, 256, bg, sc["means"], c6, shs, sc["opacities"])
    b = rr.rasterize_backward(cams[0], 256, 256, bg, sc["means"], c6, shs, sc["opacities"], fwd, gC[0], gD[0])
    assert fwd["R"] > 150_000
    # f32 sums of up to thousands of per-pixel terms per Gaussian in a different order than the oracle's serial loop
    _close(g["means"].cpu(), b["means3D"], "means3D", 2e-3)
    _close(g["cov"].cpu(), b["cov3D"], "cov3D", 2e-3)
    _close(g["sh"].cpu(), b["shs"], "shs", 2e-3)
    _close(g["op"].cpu(), b["opacities"], "opacity", 2e-3)
    _close(g["rho"].cpu()[0], b["tau"][:3], "rho", 5e-3)
    _close(g["theta"].cpu()[0], b["tau"][3:], "theta", 5e-3)
    # per-Gaussian error distribution, not only the max: 99.9 % of the mean gradients within 1e-4 of the scale
    gm, bm = g["means"].cpu().numpy().astype(np.float64), b["means3D"].astype(np.float64)
    err = np.abs(gm - bm).max(-1) / (np.abs(bm).max() + 1e-12)
    assert np.quantile(err, 0.999) <= 1e-4, float(np.quantile(err, 0.999))


def test_backward_run_to_run_spread_of_the_atomic_accumulation():
    """The per-Gaussian gradient records are accumulated with f32 atomics (one per wave and component): the order varies from run
    to run, so the result is reproducible only up to f32 re-association.  Bound that spread at the full-size scene."""
    _, _, _, _, _, _, run = _config3_backward(2)
    _, a = run()
    _, b = run()
    for k in a:
        sc_ = float(a[k].abs().max()) + 1e-12
        spread = float((a[k] - b[k]).abs().max()) / sc_
        print(f"run-to-run spread {k}: {spread:.2e}")
        assert spread <= 2e-5, (k, spread)


def test_camera_twist_gradient_finite_differences_at_full_size():
    """dL/d(rho, theta) of the 131 072-Gaussian scene against central differences of the rendered loss: the twist acts on the
    world-to-camera side, w2c' = Exp([rho, theta]) w2c (cam_utils.py:118-137), so the differences move the camera with
    callers.update_pose and re-render (f64 reduction of the image)."""
    from vicasplat_amd import callers
    from vicasplat_amd.model.decoder.cuda_splatting import render_batched
    d = _dev()
    sc = rr.synthetic_scene(V=2, res=256, Vt=4, seed=0)
    T = lambda a: torch.tensor(a, dtype=torch.float32, device=d)
    E, K, near, far = T(sc["extrinsics"][:1]), T(sc["intrinsics"][:1]), T(sc["near"][:1]), T(sc["far"][:1])
    m, cv, sh, op = T(sc["means"])[None], T(sc["covariances"])[None], T(sc["harmonics"])[None], T(sc["opacities"])[None]
    # a SMOOTH cotangent image: with per-pixel noise the rendered loss is dominated by alpha-threshold / radius discontinuities at
    # the scale of a finite-difference step and the difference quotient measures those, not the gradient
    yy, xx = np.meshgrid(np.linspace(0, 1, 256), np.linspace(0, 1, 256), indexing="ij")
    gC = T(np.stack([np.sin(5 * xx + 2 * yy), np.cos(4 * yy - xx), xx - yy])[None].astype(np.float32)).double()
    cs = torch.zeros(1, dtype=torch.int32, device=d)

    def loss_at(ext, rot=None, trans=None):
        img, _ = render_batched(ext, K, near, far, (256, 256), torch.zeros(1, 3, device=d), m, cv, sh, op, cs, rot, trans)
        return (img.double() * gC).sum()

    rot, trans = torch.zeros(1, 3, device=d, requires_grad=True), torch.zeros(1, 3, device=d, requires_grad=True)
    loss_at(E, rot, trans).backward()
    ana = torch.cat([trans.grad[0], rot.grad[0]]).double().cpu().numpy()
    eps = 2e-3
    fd = np.zeros(6)
    for i in range(6):
        dv = torch.zeros(1, 3, device=d)
        dv[0, i % 3] = eps
        z = torch.zeros(1, 3, device=d)
        Ep = callers.update_pose(dv, z, E) if i < 3 else callers.update_pose(z, dv, E)
        Em = callers.update_pose(-dv, z, E) if i < 3 else callers.update_pose(z, -dv, E)
        with torch.no_grad():
            fd[i] = float(loss_at(Ep) - loss_at(Em)) / (2 * eps)
    print("tau analytic", ana, "fd", fd)
    # The rendering function is piecewise smooth: alpha >= 1/255 cut-offs, the T < 1e-4 stop and the integer tile rectangles of
    # 131 072 pixel-sized Gaussians move under a finite step, and no implementation (upstream's included) differentiates those
    # jumps.  The exact check of the formula is the float64 autograd pin of the oracle (tests/test_raster_oracle.py) plus the
    # oracle comparison at this size (test_backward_config3_scene_131k_matches_oracle); here the difference quotient must agree in
    # direction and magnitude (measured: cosine 0.95-0.99, components within 10-40 % of the largest one).
    cos = float(ana @ fd / (np.linalg.norm(ana) * np.linalg.norm(fd)))
    assert cos >= 0.9, (cos, ana, fd)
    assert 0.5 <= np.linalg.norm(ana) / np.linalg.norm(fd) <= 2.0
    assert (np.sign(ana) == np.sign(fd)).all()


def test_camera_lists_many_cameras_two_scenes():
    """preprocess builds each scene's camera list per block in chunks of 2048 cameras, preprocess_backward in chunks of 512: 2200 cameras over two scenes
    with an irregular camera -> scene map (every camera rendered against the oracle's per-view result for ITS scene), forward state
    bit-identical, and the Gaussian gradients of the batched backward equal to the sum of the per-camera oracle gradients."""
    from vicasplat_amd.raster import forward_debug, rasterize
    d = _dev()
    W = H = 32
    P, C = 48, 2200
    rng = np.random.default_rng(5)
    sc = [_random_small(P, seed=70 + s, spread=0.5) for s in range(2)]
    cam_scene = (rng.uniform(size=C) < 0.35).astype(np.int32)        # irregular: ~35 % of the cameras look at scene 1
    cam_scene[:3] = [1, 0, 1]
    Es = np.tile(np.eye(4, dtype=np.float32)[None], (C, 1, 1))
    Es[:, :3, 3] = rng.uniform(-0.05, 0.05, (C, 3)).astype(np.float32)
    cams = rr.make_cameras(Es, np.tile(K09[None], (C, 1, 1)), np.full(C, 0.01, np.float32), np.full(C, 100.0, np.float32))
    g = _gpu_cams(cams)
    T = lambda k: torch.tensor(np.stack([s[k] for s in sc]), dtype=torch.float32, device=d)
    means, cov6, shs, op = T(0), torch.tensor(np.stack([rr.cov6(s[1]) for s in sc]), device=d), T(2), T(3)
    bg = np.array([0.05, 0.1, 0.15], np.float32)
    bgt = torch.tensor(bg, device=d).expand(C, 3).contiguous()
    cs = torch.tensor(cam_scene, device=d)
    out = forward_debug(means, cov6, op, g["viewmatrix"], g["projmatrix"], g["campos"], g["tanfov"], bgt, H, W, shs=shs, sh_degree=4,
                        cam_scene=cs)
    check = [0, 1, 2, 2047, 2048, 2049, C - 1] + list(rng.integers(3, C, 6))
    tot_checked = 0
    for c in check:
        s = int(cam_scene[c])
        o = rr.rasterize_forward(cams[c], W, H, bg, sc[s][0], rr.cov6(sc[s][1]), sc[s][2], sc[s][3])
        assert np.array_equal(out["radii"][c].cpu().numpy(), o["radii"]), f"camera {c}"
        rg = out["ranges"][c].cpu().numpy()
        assert np.array_equal(rg[:, 1] - rg[:, 0], o["ranges"][:, 1] - o["ranges"][:, 0])
        assert np.array_equal(out["point_list"].cpu().numpy().astype(np.uint32)[rg[:, 0].min():rg[:, 1].max()], o["point_list"])
        assert np.abs(out["color"][c].cpu().numpy() - o["color"]).max() < 5e-4
        tot_checked += o["R"]
    assert tot_checked > 0 and out["R"] > 0
    # backward: d(sum of all renders * w) / d(means, opacities) of scene s only sees the cameras mapped to s
    wts = torch.tensor(rng.standard_normal((C, 3, H, W)), dtype=torch.float32, device=d)
    m_, o_ = means.clone().requires_grad_(True), op.clone().requires_grad_(True)
    color, *_ = rasterize(m_, cov6, o_, g["viewmatrix"], g["projmatrix"], g["campos"], g["tanfov"], bgt, H, W, shs=shs, sh_degree=4,
                          cam_scene=cs)
    (color * wts).sum().backward()
    for s in range(2):
        idx = torch.tensor(np.nonzero(cam_scene == s)[0], device=d)
        m1, o1 = means[s:s + 1].clone().requires_grad_(True), op[s:s + 1].clone().requires_grad_(True)
        col1, *_ = rasterize(m1, cov6[s:s + 1], o1, g["viewmatrix"][idx], g["projmatrix"][idx], g["campos"][idx], g["tanfov"][idx],
                             bgt[idx].contiguous(), H, W, shs=shs[s:s + 1], sh_degree=4)
        (col1 * wts[idx]).sum().backward()
        for a, b in ((m_.grad[s], m1.grad[0]), (o_.grad[s], o1.grad[0])):
            assert float((a - b).abs().max()) <= 2e-4 * max(1.0, float(b.abs().max())), s


def test_capacity_mode_renders_without_host_sync_and_flags_overflow():
    """vs_raster_forward's capacity mode (VsRasterIn.capacity > 0): identical outputs and gradients to the exact mode when the capacity
    covers the instances; with a capacity that is too small the render is background only and the device-side flag is raised."""
    from vicasplat_amd import raster
    from vicasplat_amd.raster import rasterize
    d = _dev()
    W = H = 64
    means, cov, sh, op = _random_small(800, seed=3)
    cams = _two_cams()
    g = _gpu_cams(cams)
    bg = torch.tensor([0.2, 0.1, 0.3], device=d).expand(2, 3).contiguous()
    T = lambda a: torch.tensor(a, dtype=torch.float32, device=d)[None]
    args = lambda m, o: (m, torch.tensor(rr.cov6(cov), device=d)[None], o, g["viewmatrix"], g["projmatrix"], g["campos"], g["tanfov"], bg, H, W)
    wts = torch.randn(2, 3, H, W, device=d)

    def run(cap):
        m, o = T(means).requires_grad_(True), T(op).requires_grad_(True)
        with raster.instance_capacity(cap):
            color, radii, depth, *_ = rasterize(*args(m, o), shs=T(sh), sh_degree=4)
        info = raster.last_call()
        (color * wts).sum().backward()
        return color.detach(), depth.detach(), m.grad, o.grad, info

    c0, d0, gm0, go0, i0 = run(None)
    R = i0["num_rendered"]
    assert R > 1500 and int(i0["misc"][0]) == R and int(i0["misc"][2]) == 0
    c1, d1, gm1, go1, i1 = run(R + 1000)
    assert i1["num_rendered"] == R + 1000 and int(i1["misc"][0]) == R and int(i1["misc"][2]) == 0
    assert torch.equal(c0, c1) and torch.equal(d0, d1)
    assert float((gm0 - gm1).abs().max()) <= 1e-5 * max(1.0, float(gm0.abs().max())) and float((go0 - go1).abs().max()) <= 1e-5 * max(1.0, float(go0.abs().max()))
    c2, d2, gm2, go2, i2 = run(R // 2)
    assert int(i2["misc"][2]) == 1 and int(i2["misc"][0]) == R
    assert torch.allclose(c2, bg[:, :, None, None].expand(2, 3, H, W)) and float(d2.abs().max()) == 0
    assert float(gm2.abs().max()) == 0 and float(go2.abs().max()) == 0
