"""The float64 render-backward reference (oracle/raster_f64.py) pinned on the CPU: float64 autograd of oracle/raster_torch.py, finite
differences of its own frozen-decision forward, the C oracle's f32 backward, and planted defects that its GPU bars must reject."""

import numpy as np
import pytest
import torch

from oracle import raster_f64 as rf
from oracle import raster_ref as rr
from oracle import raster_torch as rt

K09 = np.array([[0.9, 0, 0.5], [0, 0.9, 0.5], [0, 0, 1]], np.float32)
BG = np.array([0.2, 0.1, 0.3], np.float32)


def _oracle(sc, W, H, bg=BG):
    cam = rf.identity_camera(W, H)
    return cam, rr.rasterize_forward(cam, W, H, bg, sc["means"], sc["cov6"], None, sc["opacities"], colors_precomp=sc["colors"])


def _small(seed, P, op_lo, op_hi, W=48, H=32):
    rng = np.random.default_rng(seed)
    means = np.stack([rng.uniform(-0.7, 0.7, P), rng.uniform(-0.5, 0.5, P), rng.uniform(1.5, 4.0, P)], -1).astype(np.float32)
    A = rng.standard_normal((P, 3, 3)) * 0.1
    cov = (A @ A.transpose(0, 2, 1) + 2e-3 * np.eye(3)).astype(np.float32)
    sh = np.zeros((P, 25, 3), np.float32)
    sh[:, 0] = rng.standard_normal((P, 3)) * 0.7
    return means, cov, sh, rng.uniform(op_lo, op_hi, P).astype(np.float32)


@pytest.mark.parametrize("seed,op", [(0, (0.2, 0.9)), (1, (0.85, 0.999))])
def test_reference_equals_float64_autograd(seed, op):
    """Render-level records of raster_torch's float64 autograd (leaves the render loop reads) == the reference fed the same float64
    records and the C oracle's lists.  seed 1: opaque enough that pixels meet the T < 1e-4 stop."""
    W, H = 48, 32
    means, cov, sh, opac = _small(seed, 40 if seed == 0 else 160, *op)
    E = np.eye(4)
    tm, tc, ts, to = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (means, cov, sh, opac))
    color, depth, _, aux = rt.rasterize(tm, tc, ts, to, torch.tensor(E), torch.tensor(K09, dtype=torch.float64), 0.01, 100.0, H, W,
                                        BG, sh_degree=0, return_aux=True)
    rng = np.random.default_rng(seed + 10)
    gC = rng.standard_normal((3, H, W)); gD = 0.3 * rng.standard_normal((H, W))
    loss = (color * torch.tensor(gC)).sum() + (depth * torch.tensor(gD)).sum()
    pix, conic, rgb, zr, op_t = aux["render_inputs"]
    g_pix, g_conic, g_rgb, g_z, g_op = torch.autograd.grad(loss, [pix, conic, rgb, zr, to])
    cam = rr.make_cameras(E[None].astype(np.float32), K09[None], np.full(1, 0.01, np.float32), np.full(1, 100.0, np.float32))[0]
    o = rr.rasterize_forward(cam, W, H, BG, means, rr.cov6(cov), sh, opac, sh_degree=0)
    vis = o["radii"] > 0
    assert np.array_equal(vis, aux["visible"].numpy())
    co = np.concatenate([conic.detach().numpy(), opac[:, None].astype(np.float64)], 1)
    ref = rf.render_backward(pix.detach().numpy(), co, rgb.detach().numpy(), zr.detach().numpy(), o["ranges"], o["point_list"],
                             o["n_contrib"], BG, gC, gD, W=W, H=H, exp=rf.exp_libm)
    # the float32 decisions of the lists agree with raster_torch's float64 ones: same image to float64 rounding, nothing ambiguous
    assert not ref["ambiguous"][vis].any()
    assert np.abs(ref["color"] - color.detach().numpy()).max() <= 1e-12
    assert np.abs(ref["depth"] - depth.detach().numpy()).max() <= 1e-11
    if seed == 1:
        assert ref["stopped"].sum() >= 10, "the scene reaches the T < 1e-4 stop"
    hw = np.array([0.5 * W, 0.5 * H])
    exp = dict(mean2D=g_pix.numpy() * hw, conic=g_conic.numpy(), opacity=g_op.numpy(), colors=g_rgb.numpy(), depths=g_z.numpy())
    for k, e in exp.items():
        e = np.where(vis.reshape((-1,) + (1,) * (e.ndim - 1)), e, 0.0)
        assert np.abs(ref[k] - e).max() <= 1e-9 * np.abs(e).max(), k


def test_reference_matches_finite_differences_on_a_saturated_stack():
    """Every record kind against central differences of forward_frozen on a 2 x 2 pixel stack of six Gaussians, with
    three near-opaque ones that put several pairs at the 0.99 clamp (straight-through)."""
    W = H = 16
    xy = np.array([[7.3, 7.6], [8.1, 7.2], [7.7, 8.4], [6.9, 8.0], [8.4, 8.3], [7.5, 7.5]])
    co = np.array([[0.02, 0.003, 0.025, 0.999], [0.20, -0.04, 0.35, 0.6], [0.015, 0.002, 0.02, 0.999], [0.25, 0.0, 0.2, 0.4],
                   [0.02, -0.004, 0.018, 0.999], [0.1, 0.01, 0.12, 0.5]])
    rgb = np.array([[0.9, 0.1, 0.2], [0.2, 0.8, 0.3], [0.5, 0.5, 0.1], [0.1, 0.3, 0.9], [0.7, 0.7, 0.7], [0.3, 0.1, 0.5]])
    dep = np.array([2.0, 3.0, 5.0, 9.0, 20.0, 40.0])
    px, py = np.array([7, 8, 7, 8]), np.array([7, 7, 8, 8])
    ranges = np.zeros((1, 2), np.int32); ranges[0] = (0, 6)
    nc = np.zeros((H, W), np.int32); nc[py, px] = 6
    rng = np.random.default_rng(0)
    gC = np.zeros((3, H, W)); gC[:, py, px] = 1 + 0.1 * rng.standard_normal((3, 4))
    gD = np.zeros((H, W)); gD[py, px] = 0.05 * rng.standard_normal(4)
    ref = rf.render_backward(xy, co, rgb, dep, ranges, np.arange(6), nc, BG, gC, gD, W=W, H=H)
    ids = np.arange(6)
    contrib, clamped, _, amb = rf._decisions(ids, px, py, nc[py, px], xy.astype(np.float32), co.astype(np.float32), rf.exp_v)
    assert contrib.all() and clamped.sum() >= 4 and not amb.any()
    st = co[None, :, 3] * np.exp(-0.5 * (co[None, :, 0] * (xy[None, :, 0] - px[:, None]) ** 2 + co[None, :, 2] * (xy[None, :, 1] - py[:, None]) ** 2)
                                 - co[None, :, 1] * (xy[None, :, 0] - px[:, None]) * (xy[None, :, 1] - py[:, None]))
    gCp, gDp = gC[:, py, px].T, gD[py, px]

    def loss(xy_, co_, rgb_, dep_):
        c, d = rf.forward_frozen(xy_, co_, rgb_, dep_, contrib, clamped, px, py, BG, st_base=st)
        return float((c * gCp).sum() + (d * gDp).sum())

    h = 1e-6
    for name, arr, k_of, scale in (("mean2D", xy, lambda j: j, np.array([0.5 * W, 0.5 * H])), ("conic", co, lambda j: j, None),
                                   ("opacity", co, lambda j: 3, None), ("colors", rgb, lambda j: j, None), ("depths", dep, None, None)):
        ncomp = 1 if arr.ndim == 1 else (1 if name == "opacity" else (2 if name == "mean2D" else 3))
        for g in range(6):
            for j in range(ncomp):
                def bump(s):
                    a = [xy.copy(), co.copy(), rgb.copy(), dep.copy()]
                    i = {"mean2D": 0, "conic": 1, "opacity": 1, "colors": 2, "depths": 3}[name]
                    if a[i].ndim == 1:
                        a[i][g] += s
                    else:
                        a[i][g, k_of(j)] += s
                    return loss(*a)
                fd = (bump(h) - bump(-h)) / (2 * h)
                if scale is not None:
                    fd = fd * scale[j]
                r = ref[name][g] if ref[name].ndim == 1 else ref[name][g, j]
                assert abs(r - fd) <= 1e-6 * max(1.0, abs(fd)), (name, g, j, r, fd)


@pytest.mark.parametrize("builder", [rf.deep_scene, rf.saturated_scene, rf.segment_scene])
def test_reference_agrees_with_the_c_oracle(builder):
    """Fed the C oracle's own records, the reference agrees with its float32 ref_render_backward at float32 tolerance (the oracle
    walks back to front from final_T: no cancellation, so gamma 0)."""
    sc, W, H = builder()
    cam, o = _oracle(sc, W, H)
    rng = np.random.default_rng(1)
    gC = (1 + 0.1 * rng.standard_normal((3, H, W))).astype(np.float32)
    gD = (0.02 * rng.standard_normal((H, W))).astype(np.float32)
    ref = rf.render_backward(o["xy"], o["conic_opacity"], o["rgb"], o["depths"], o["ranges"], o["point_list"], o["n_contrib"], BG,
                             gC, gD, W=W, H=H, exp=rf.exp_libm)
    assert np.abs(ref["color"] - o["color"]).max() <= 1e-5
    assert (np.abs(ref["final_T"] - o["final_T"]) / o["final_T"]).max() <= 5e-4
    b = rr.rasterize_backward(cam, W, H, BG, sc["means"], sc["cov6"], None, sc["opacities"], o, gC, gD, colors_precomp=sc["colors"])
    for k in rf.COMPONENTS:
        ok, msg, _ = rf.compare(b["_render"][k], ref, k, gamma=0, rel=1e-4 if k in ("colors", "depths") else 1e-3,
                                visible=o["radii"] > 0)
        assert ok, msg


@pytest.fixture(scope="module")
def deep():
    sc, W, H = rf.deep_scene()
    _, o = _oracle(sc, W, H)
    rng = np.random.default_rng(2)
    gC = (1 + 0.1 * rng.standard_normal((3, H, W))).astype(np.float32)
    gD = (0.02 * rng.standard_normal((H, W))).astype(np.float32)
    args = (o["xy"], o["conic_opacity"], o["rgb"], o["depths"], o["ranges"], o["point_list"])
    kw = dict(W=W, H=H)
    clean = rf.render_backward(*args, o["n_contrib"], BG, gC, gD, **kw)
    return args, kw, o, gC, gD, clean


def _rejected(bad, clean, vis):
    return any(not rf.compare(bad[k], clean, k, gamma=256, rel=1e-4 if k in ("colors", "depths") else 1e-3, visible=vis)[0]
               for k in ("mean2D", "opacity", "colors"))


@pytest.mark.parametrize("defect", ["drop_segment", "n_contrib", "neighbour_checkpoint", "no_background"])
def test_bars_reject_planted_defects(deep, defect):
    """The comparison the GPU tests use (checkpoint-route gamma, render-level records of the ABI) fails on the deep scene for each
    planted defect; the clean reference passes against itself."""
    args, kw, o, gC, gD, clean = deep
    vis = o["radii"] > 0
    assert o["n_contrib"].max() > 4 * rf.SEG
    tile = int(np.argmax(o["ranges"][:, 1] - o["ranges"][:, 0]))
    if defect == "n_contrib":
        bad = rf.render_backward(*args, np.maximum(o["n_contrib"] - 1, 0), BG, gC, gD, **kw)
    elif defect == "no_background":
        bad = rf.render_backward(*args, o["n_contrib"], BG, gC, gD, defect=("no_background",), **kw)
    else:
        bad = rf.render_backward(*args, o["n_contrib"], BG, gC, gD, defect=(defect, tile, 2), **kw)
    assert not _rejected(clean, clean, vis)
    assert _rejected(bad, clean, vis), defect
