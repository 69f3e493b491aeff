"""Float64 render backward of the rasterizer (numpy), the yardstick of tests/test_raster_deep_gpu.py.

TEST INFRASTRUCTURE ONLY.  Input: ONE camera's forward records -- the per-Gaussian `xy`, `conic_opacity`, `rgb`, `depth` (from the
GPU's forward_debug or from the C oracle), the tile `ranges` / `point_list` and per-pixel `n_contrib` of that forward -- plus `bg`,
dL/dcolor [3,H,W] and optionally dL/ddepth [H,W].

Decisions are the forward's: whether a (pixel, entry) pair blends (`power <= 0`, `alpha >= 1/255`, `position < n_contrib`) and
whether alpha sits at the 0.99 clamp are evaluated with the kernels' f32 expressions in their operation order.  Values are
float64: G, alpha, the transmittance T_k as a product over the earlier contributors, and the suffix
    S_k = sum_{j>k} w_j (c_j . dL + d_j dLd) + T_end (bg . dL)
as a reverse cumulative sum (never as a difference), so that
    dL/dalpha_k = T_k (c_k . dL + d_k dLd) - S_k / (1 - alpha_k)
carries no cancellation.  The clamp is straight-through (upstream's backward and the oracle's).

Beside each per-Gaussian record (mean2D in NDC units, conic = partials w.r.t. (A, B, C), opacity, colors, depths) come:
    mag   sum over pixels of |per-pixel term|: the error scale of a correct f32 sum of the terms;
    lim   sum over pixels of |d term / d(dL/dalpha)| |F|_abs / (1 - alpha), |F|_abs = sum_k w_k |c_k . dL + d_k dLd| + T_end |bg . dL|:
          what a front-to-back form that forms the suffix as (out . dL - prefix) from an f32 image inherits (zero for colors / depths);
and `ambiguous`, the Gaussians owning a pair whose f32 decision is within rounding of flipping (alpha at 1/255, |power| at
rounding level, test_T at 1e-4): f32 implementations may legitimately decide those pairs either way.
"""
from __future__ import annotations

import numpy as np

TILE = 16
SEG = 512                      # entries per checkpoint segment of the HIP forward (vs::kCkSeg)
EPS32 = 2.0 ** -24
THR = np.float32(1.0 / 255.0)  # == 1.0f / 255.0f
COMPONENTS = ("mean2D", "conic", "opacity", "colors", "depths")
_F = np.float32


def exp_v(x):
    """__expf of the HIP kernels: v_exp_f32(x * log2(e)) (exp2 is exact to about an ulp; the product is rounded to f32 first)."""
    x = np.asarray(x, np.float32)
    return np.exp2(x * _F(1.4426950408889634)).astype(np.float32)


def exp_libm(x):
    """expf of the C oracle."""
    return np.exp(np.asarray(x, np.float32)).astype(np.float32)


def _tile_pixels(tile, gx, W, H):
    ty, tx = divmod(tile, gx)
    ys, xs = np.meshgrid(np.arange(TILE), np.arange(TILE), indexing="ij")
    px, py = (tx * TILE + xs).ravel(), (ty * TILE + ys).ravel()
    inside = (px < W) & (py < H)
    return px[inside], py[inside]


def _decisions(ids, px, py, nc, xy, co, exp):
    """The kernels' f32 expressions over the [npix, n] pairs -> contrib (the pair blends), clamped (alpha at 0.99), passing (power <= 0
    and alpha >= 1/255: blends unless the pixel is done), amb (the f32 value of power / alpha is within rounding of a decision)."""
    x, y = xy[ids, 0][None, :], xy[ids, 1][None, :]
    A, B, Cc, op = co[ids, 0][None, :], co[ids, 1][None, :], co[ids, 2][None, :], co[ids, 3][None, :]
    dx = x - px.astype(np.float32)[:, None]
    dy = y - py.astype(np.float32)[:, None]
    with np.errstate(over="ignore", invalid="ignore"):
        power = _F(-0.5) * (A * dx * dx + Cc * dy * dy) - B * dx * dy
        G32 = exp(np.minimum(power, _F(0.0)))
        raw = op * G32
    a32 = np.minimum(_F(0.99), raw)
    pos = np.arange(len(ids))[None, :]
    passing = (power <= 0) & (a32 >= THR)
    contrib = passing & (pos < nc[:, None])
    # FMA contraction of the power and v_exp_f32 vs libm expf move alpha by a few ulp x (1 + |power|); the sign of the power is open
    # only where its terms cancel
    pw = np.abs(power.astype(np.float64))
    near_thr = np.abs(a32.astype(np.float64) - float(THR)) <= 8 * EPS32 * (1.0 + pw) * float(THR)
    scale = (0.5 * (np.abs(A) * dx * dx + np.abs(Cc) * dy * dy) + np.abs(B * dx * dy)).astype(np.float64)
    near_zero = pw < 8 * EPS32 * scale
    return contrib, raw > _F(0.99), passing, near_thr | near_zero


def render_backward(xy, conic_opacity, rgb, depth, ranges, point_list, n_contrib, bg, dL_dcolor, dL_ddepth=None, *, W, H,
                    exp=exp_v, defect=None) -> dict:
    """Float64 render backward of one camera.  Returns {component: record}, {component + '_mag'}, {component + '_lim'} for the
    components of COMPONENTS (mean2D [P,2], conic [P,3], opacity [P], colors [P,3], depths [P]), 'ambiguous' bool [P],
    'color' [3,H,W] / 'depth' [H,W] / 'final_T' [H,W] of the float64 replay, 'n_pairs' (contributing pairs), 'stopped' bool [H,W]
    (the pixel met T < 1e-4) and 'stop_at' [H,W] (list position of that entry, -1 if none).

    `defect` plants a known error on this side, for the tests that show the GPU bars can fail: ('drop_segment', tile, seg) leaves
    out the terms of that 512-entry segment of one tile; ('neighbour_checkpoint', tile, seg) starts that segment of one tile from
    the state (T, colour and depth prefix) of the pixel's horizontal neighbour; ('no_background',) omits T_end (bg . dL)."""
    # decisions on the f32 values (what the forward saw), values from the records as given (float64 records stay exact)
    xy64, co64 = np.asarray(xy, np.float64), np.asarray(conic_opacity, np.float64)
    xy, co = xy64.astype(np.float32), co64.astype(np.float32)
    rgb64 = np.asarray(rgb, np.float64); dep64 = np.asarray(depth, np.float64)
    ranges = np.asarray(ranges).reshape(-1, 2); point_list = np.asarray(point_list).astype(np.int64)
    nc_img = np.asarray(n_contrib).reshape(H, W)
    bg64 = np.asarray(bg, np.float64)
    gC = np.asarray(dL_dcolor, np.float64).reshape(3, H, W)
    gD = None if dL_ddepth is None else np.asarray(dL_ddepth, np.float64).reshape(H, W)
    P = xy.shape[0]
    gx = (W + TILE - 1) // TILE
    acc = {k: np.zeros(P * n) for k, n in (("mean2D", 2), ("conic", 3), ("opacity", 1), ("colors", 3), ("depths", 1))}
    mag = {k: np.zeros_like(v) for k, v in acc.items()}
    lim = {k: np.zeros_like(v) for k, v in acc.items()}
    amb_g = np.zeros(P, bool)
    color = np.zeros((3, H, W)) + bg64[:, None, None]
    depth_img = np.zeros((H, W))
    final_T = np.ones((H, W))
    n_pairs = 0
    stopped = np.zeros((H, W), bool)
    stop_at = np.full((H, W), -1)
    hw = np.array([0.5 * W, 0.5 * H])

    def add(name, k, idx, vals, fac, lim_scale):
        n = acc[name].shape[0] // P
        flat = idx * n + k
        acc[name] += np.bincount(flat.ravel(), weights=vals.ravel(), minlength=P * n)
        mag[name] += np.bincount(flat.ravel(), weights=np.abs(vals).ravel(), minlength=P * n)
        if fac is not None:
            lim[name] += np.bincount(flat.ravel(), weights=(np.abs(fac) * lim_scale).ravel(), minlength=P * n)

    for tile in range(ranges.shape[0]):
        r0, r1 = int(ranges[tile, 0]), int(ranges[tile, 1])
        if r1 <= r0:
            continue
        px, py = _tile_pixels(tile, gx, W, H)
        nc = nc_img[py, px]
        n = r1 - r0
        ids = point_list[r0:r1]
        contrib, clamped, passing, amb = _decisions(ids, px, py, nc, xy, co, exp)
        # a pixel is done (T < 1e-4) at its first passing entry behind its last contributor, if there is one; the forward never
        # evaluated the entries behind that
        pos = np.arange(n)[None, :]
        after = passing & (pos >= nc[:, None])
        done = after.any(1)
        stop_pos = np.where(done, np.argmax(after, 1), n)
        stopped[py, px] = done
        stop_at[py, px] = np.where(done, stop_pos, -1)
        x, y = xy64[ids, 0][None, :], xy64[ids, 1][None, :]
        A, B, Cc, op = (co64[ids, i][None, :] for i in range(4))
        dx, dy = x - px[:, None], y - py[:, None]
        G = np.exp(np.minimum(-0.5 * (A * dx * dx + Cc * dy * dy) - B * dx * dy, 0.0))
        alpha = np.where(clamped, 0.99, op * G)
        a = np.where(contrib, alpha, 0.0)
        om = 1.0 - a
        Tinc = np.cumprod(om, axis=1)
        T = np.concatenate([np.ones((len(px), 1)), Tinc[:, :-1]], axis=1)     # transmittance in front of entry k
        T_end = Tinc[:, -1]
        dLc = gC[:, py, px].T                                                  # [npix, 3]
        dLd = gD[py, px] if gD is not None else np.zeros(len(px))
        c = rgb64[ids]                                                        # [n, 3]
        d = dep64[ids]
        w = w_fwd = a * T
        # the stop test T (1 - alpha) < 1e-4 at rounding level (f32 T drifts ~5e-4 relative over thousands of products)
        testT = np.where(passing & (pos <= stop_pos[:, None]), T * (1.0 - alpha), np.inf)
        amb = (amb & (pos <= stop_pos[:, None])) | (np.abs(testT - 1e-4) <= 5e-4 * 1e-4)
        amb_g[np.unique(np.broadcast_to(ids[None, :], amb.shape)[amb])] = True
        cd = dLc @ c.T + dLd[:, None] * d[None, :]                            # c_k . dL + d_k dLd   [npix, n]
        wcd = w * cd
        bgdot = dLc @ bg64
        if defect is not None and defect[0] == "no_background":
            bgdot = np.zeros_like(bgdot)
        # suffix after k: reverse exclusive cumulative sum, plus the background term
        S = np.concatenate([np.cumsum(wcd[:, ::-1], axis=1)[:, ::-1][:, 1:], np.zeros((len(px), 1))], axis=1)
        S = S + (T_end * bgdot)[:, None]
        if defect is not None and defect[0] == "neighbour_checkpoint" and defect[1] == tile and defect[2] * SEG < n:
            # segment [s0, s1) replayed front to back from the horizontal neighbour's state (T and the colour . dL / depth . dLd prefix),
            # its suffix formed as the pixel's rendered F minus that prefix: what a checkpoint replay with a wrong index map computes
            s0, s1 = defect[2] * SEG, min((defect[2] + 1) * SEG, n)
            key = {(int(p), int(q)): i for i, (p, q) in enumerate(zip(px, py))}
            nb = np.array([key.get((int(p) ^ 1, int(q)), i) for i, (p, q) in enumerate(zip(px, py))])
            pre_c, pre_d = w[:, :s0] @ c[:s0], w[:, :s0] @ d[:s0]
            F = S[:, 0] + wcd[:, 0]                                            # the pixel's out . dL
            Ts0 = T[:, s0].copy()
            T[:, s0:s1] = T[:, s0:s1] / np.where(Ts0 > 0, Ts0, 1.0)[:, None] * Ts0[nb][:, None]
            w = a * T
            wcd = w * cd
            D = ((pre_c[nb] * dLc).sum(1) + pre_d[nb] * dLd)[:, None] + np.cumsum(wcd[:, s0:s1], axis=1)
            S[:, s0:s1] = F[:, None] - D
        dLda = np.where(contrib, T * cd - S / (1.0 - alpha), 0.0)
        Fabs = (w * np.abs(cd)).sum(1) + T_end * np.abs(bgdot)
        lim_scale = np.where(contrib, Fabs[:, None] / (1.0 - alpha), 0.0)
        keep = np.ones(n, bool)
        if defect is not None and defect[0] == "drop_segment" and defect[1] == tile:
            keep[defect[2] * SEG:(defect[2] + 1) * SEG] = False
        km = keep[None, :]
        dLda_k, w_k, ls = dLda * km, w * km, lim_scale * km
        idx = np.broadcast_to(ids[None, :], dLda.shape)
        fm2 = [op * G * (dx * A + dy * B) * hw[0], op * G * (dy * Cc + dx * B) * hw[1]]
        for k in range(2):
            add("mean2D", k, idx, -dLda_k * fm2[k], fm2[k], ls)
        fcn = [-0.5 * op * G * dx * dx, -op * G * dx * dy, -0.5 * op * G * dy * dy]
        for k in range(3):
            add("conic", k, idx, dLda_k * fcn[k], fcn[k], ls)
        add("opacity", 0, idx, dLda_k * G, G, ls)
        for k in range(3):
            add("colors", k, idx, w_k * dLc[:, k:k + 1], None, None)
        add("depths", 0, idx, w_k * dLd[:, None], None, None)
        n_pairs += int(contrib.sum())
        # float64 replay of the forward (decisions frozen)
        color[:, py, px] = (w_fwd @ c).T + T_end[None, :] * bg64[:, None]
        depth_img[py, px] = w_fwd @ d
        final_T[py, px] = T_end
    shapes = dict(mean2D=(P, 2), conic=(P, 3), opacity=(P,), colors=(P, 3), depths=(P,))
    out = dict(ambiguous=amb_g, color=color, depth=depth_img, final_T=final_T, n_pairs=n_pairs, stopped=stopped, stop_at=stop_at)
    for k, s in shapes.items():
        out[k] = acc[k].reshape(s); out[k + "_mag"] = mag[k].reshape(s); out[k + "_lim"] = lim[k].reshape(s)
    return out


def forward_frozen(xy, conic_opacity, rgb, depth, contrib, clamped, px, py, bg, st_base=None):
    """Float64 forward of ONE pixel stack with frozen decisions: xy [n,2], conic_opacity [n,4], rgb [n,3], depth [n] of the entries in
    list order (float64, differentiable by finite differences), contrib / clamped bool [npix, n], px / py [npix].  -> colour [npix,3],
    depth [npix].  st_base [npix, n]: op G at the base point; a clamped alpha is then 0.99 + (op G - st_base), the straight-through
    clamp as a function (its value 0.99 at the base point, its derivative that of op G)."""
    dx = xy[None, :, 0] - px[:, None]; dy = xy[None, :, 1] - py[:, None]
    A, B, Cc, op = (conic_opacity[None, :, i] for i in range(4))
    G = np.exp(-0.5 * (A * dx * dx + Cc * dy * dy) - B * dx * dy)
    alpha = np.where(clamped, 0.99 + (op * G - (op * G if st_base is None else st_base)), op * G)
    a = np.where(contrib, alpha, 0.0)
    om = 1.0 - a
    T = np.concatenate([np.ones((len(px), 1)), np.cumprod(om, 1)[:, :-1]], 1)
    w = a * T
    return w @ rgb + np.cumprod(om, 1)[:, -1:] * np.asarray(bg, np.float64)[None, :], w @ depth


# ---------------------------------------------------------------------------------------------------------------------------------
# comparison against the float64 records
# ---------------------------------------------------------------------------------------------------------------------------------
def bar(ref, name, gamma, rel=1e-3):
    """Per-element allowance of the GPU record `name`: rel mag + gamma 2^-24 lim + 1e-6 max(mag)."""
    m, l = ref[name + "_mag"], ref[name + "_lim"]
    return rel * m + gamma * EPS32 * l + 1e-6 * float(m.max(initial=0.0))


def compare(gpu, ref, name, gamma, rel=1e-3, visible=None, max_amb_frac=1e-3, old_rtol=2e-3):
    """Checks the GPU record `name` (same shape as ref[name]) against the float64 reference.  Non-ambiguous Gaussians: per element
    |gpu - ref| <= bar; ambiguous ones: at most max_amb_frac of the visible Gaussians, held to the max-scaled bar old_rtol max|ref|.
    Returns (ok, message, ratios) with ratios = err / (mag + 2^-24 lim) over the checked elements."""
    g = np.asarray(gpu, np.float64); r = ref[name]
    err = np.abs(g - r)
    amb = ref["ambiguous"]
    vis = np.ones(len(amb), bool) if visible is None else np.asarray(visible, bool)
    lim_ok = err <= bar(ref, name, gamma, rel)
    sel = ~amb & vis
    selb = sel.reshape((-1,) + (1,) * (r.ndim - 1)) if r.ndim > 1 else sel
    selb = np.broadcast_to(selb, r.shape)
    bad = ~lim_ok & selb
    den = ref[name + "_mag"] + EPS32 * ref[name + "_lim"]
    touched = selb & (den > 0)
    ratios = err[touched] / den[touched]
    msgs = []
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bad, err / np.maximum(bar(ref, name, gamma, rel), 1e-300), 0)), r.shape)
        msgs.append(f"{name}: {int(bad.sum())} elements over the bar (worst at {i}: gpu {g[i]:.6e} ref {r[i]:.6e} "
                    f"mag {ref[name + '_mag'][i]:.3e} lim {ref[name + '_lim'][i]:.3e})")
    namb = int((amb & vis).sum())
    if namb > max_amb_frac * max(int(vis.sum()), 1):
        msgs.append(f"{name}: {namb} ambiguous Gaussians of {int(vis.sum())} visible")
    if namb:
        ab = np.broadcast_to((amb & vis).reshape((-1,) + (1,) * (r.ndim - 1)) if r.ndim > 1 else (amb & vis), r.shape)
        if err[ab].max() > old_rtol * (np.abs(r).max() + 1e-30):
            msgs.append(f"{name}: ambiguous Gaussian over the max-scaled bar")
    return not msgs, "; ".join(msgs), ratios


def ratio_summary(ratios) -> str:
    if len(ratios) == 0:
        return "n=0"
    return (f"max {np.max(ratios):.2e} p99.9 {np.quantile(ratios, 0.999):.2e} median {np.median(ratios):.2e} n={len(ratios)}")


# ---------------------------------------------------------------------------------------------------------------------------------
# seeded scenes of the deep-tile tests, laid out in PIXELS for an identity camera (c2w = I, normalised focal f, principal point at
# the centre): a Gaussian at pixel (u, v), view depth z and screen standard deviation s gets the world mean and isotropic covariance
# that project there.  Records: means [P,3], cov6 [P,6], colors [P,3], opacities [P] (float32).
# ---------------------------------------------------------------------------------------------------------------------------------
F_NORM = 0.9


def identity_camera(W, H, f=F_NORM):
    from oracle import raster_ref as rr
    K = np.array([[[f, 0, 0.5], [0, f, 0.5], [0, 0, 1]]], np.float32)
    return rr.make_cameras(np.eye(4, dtype=np.float32)[None], K, np.full(1, 0.01, np.float32), np.full(1, 100.0, np.float32))[0]


def place(u, v, z, s, W, H, f=F_NORM):
    """pixel centre (u, v), depth z, screen sigma s (pixels, before the +0.3 dilation) -> means [P,3], cov6 [P,6] (axis-aligned)."""
    u, v, z, s = (np.asarray(a, np.float64) for a in (u, v, z, s))
    tx, ty = 0.5 / f, 0.5 / f
    x = ((2 * u + 1) / W - 1) * z * tx
    y = ((2 * v + 1) / H - 1) * z * ty
    fx, fy = W / (2 * tx), H / (2 * ty)
    cov = np.zeros((len(u), 6)); cov[:, 0] = cov[:, 5] = (s * z / fx) ** 2; cov[:, 3] = (s * z / fy) ** 2
    return np.stack([x, y, z], -1).astype(np.float32), cov.astype(np.float32)


def _pack(parts):
    means, cov, col, op = (np.concatenate([p[i] for p in parts]).astype(np.float32) for i in range(4))
    return dict(means=means, cov6=cov, colors=col, opacities=op)


def _blob(rng, n, W, H, s_lo, s_hi, op_lo, op_hi, z_lo=2.0, z_hi=60.0, box=None):
    x0, y0, x1, y1 = box if box is not None else (0, 0, W, H)
    u, v = rng.uniform(x0, x1, n) - 0.5, rng.uniform(y0, y1, n) - 0.5
    z = rng.uniform(z_lo, z_hi, n)
    s = np.exp(rng.uniform(np.log(s_lo), np.log(s_hi), n))
    m, c = place(u, v, z, s, W, H)
    return m, c, rng.uniform(0, 1, (n, 3)), rng.uniform(op_lo, op_hi, n)


def deep_scene(seed=0, W=48, H=40):
    """Deep translucent tiles: ~3 000 list entries per tile, footprints from a pixel to the whole tile, opacity 0.01-0.05, so every
    pixel sees part of the list and stays unsaturated deep into it (n_contrib past 2 048 = five segments)."""
    rng = np.random.default_rng(seed)
    return _pack([_blob(rng, 9000, W, H, 0.6, 2.5, 0.01, 0.05), _blob(rng, 300, W, H, 4.0, 10.0, 0.01, 0.02)]), W, H


def saturated_scene(seed=1, W=32, H=32):
    """~40 near-opaque Gaussians (alpha at the 0.99 clamp) interleaved in depth with ~2 000 translucent ones per tile: the left
    column of tiles has opaque Gaussians at the front (pixels stop in segment 0), the lower right tile opaque ones far behind
    (pixels stop in segment >= 3), the rest are spread over all depths."""
    rng = np.random.default_rng(seed)
    parts = [_blob(rng, 5200, W, H, 0.6, 2.0, 0.01, 0.05, z_lo=2.0, z_hi=60.0)]
    parts.append(_blob(rng, 20, W, H, 3.0, 4.0, 0.995, 0.999, z_lo=2.0, z_hi=2.5, box=(2, 2, 10, 14)))
    parts.append(_blob(rng, 16, W, H, 2.5, 4.0, 0.995, 0.999, z_lo=56.0, z_hi=59.0, box=(18, 18, 30, 30)))
    parts.append(_blob(rng, 12, W, H, 1.0, 3.0, 0.995, 0.999, z_lo=3.0, z_hi=58.0, box=(16, 0, 32, 16)))
    return _pack(parts), W, H


SEG_LISTS = (511, 512, 513, 1024, 1025)


def segment_scene(seed=2):
    """A row of 16 x 16 tiles (W = 128, H = 16): tiles 0-4 hold lists of exactly SEG_LISTS entries of small Gaussians that each stay
    inside their tile; tiles 5-6 are spacers; tile 7 holds 1 100 small Gaussians behind 40 opaque tile-sized ones, so every pixel of it
    stops long before entry 512 although its list is longer (its second checkpoint is never written)."""
    rng = np.random.default_rng(seed)
    W, H = 128, 16
    parts = []
    for t, n in enumerate(SEG_LISTS):
        u = rng.integers(4, 12, n) + 16 * t
        v = rng.integers(4, 12, n)
        z = rng.uniform(2.0, 60.0, n)
        z[np.argmax(z)] = 61.0     # the last entry of the list is the deepest, and opaque enough to blend at its centre pixel
        m, c = place(u, v, z, np.full(n, 0.5), W, H)
        op = rng.uniform(0.05, 0.3, n); op[np.argmax(z)] = 0.5
        parts.append((m, c, rng.uniform(0, 1, (n, 3)), op))
    n = 1100
    m, c = place(rng.integers(116, 124, n), rng.integers(4, 12, n), rng.uniform(10.0, 60.0, n), np.full(n, 0.5), W, H)
    parts.append((m, c, rng.uniform(0, 1, (n, 3)), rng.uniform(0.05, 0.3, n)))
    m, c = place(np.full(40, 119.5), np.full(40, 7.5), rng.uniform(2.0, 3.0, 40), np.full(40, 8.0), W, H)
    parts.append((m, c, rng.uniform(0, 1, (40, 3)), np.full(40, 0.999)))
    return _pack(parts), W, H


def onewave_scene(seed=3, W=1032, H=1016):
    """65 x 64 = 4 160 tiles (>= 4 096: the forward runs one wave per tile): a deep and a saturated cluster in interior tiles and a
    deep one in the partial bottom-right tile; the rest of the image is empty."""
    rng = np.random.default_rng(seed)
    parts = [_blob(rng, 2500, W, H, 0.6, 2.0, 0.01, 0.05, box=(160, 160, 192, 192)),
             _blob(rng, 2500, W, H, 0.6, 2.0, 0.01, 0.05, box=(480, 640, 512, 672)),
             _blob(rng, 40, W, H, 3.0, 4.0, 0.995, 0.999, z_lo=40.0, z_hi=45.0, box=(488, 648, 504, 664)),
             _blob(rng, 1200, W, H, 0.6, 1.5, 0.01, 0.05, box=(1024, 1008, 1032, 1016))]
    return _pack(parts), W, H


def preprocess_backward(cam, W, H, bg, means, cov6, opacities, colors, ofwd, rec):
    """3-D gradients (means3D [P,3], cov3D [P,6]) of the render records `rec` (e.g. the float64 ones, rounded to f32) through the C
    oracle's ref_preprocess_backward; ofwd: the oracle's forward of the same camera (radii, clamp mask)."""
    import ctypes as C
    from oracle import raster_ref as rr
    L = rr.lib()
    s, keep = rr._mk_in(cam, W, H, bg, means, cov6, None, colors, opacities, 0)
    P = s.P
    f = lambda a: np.ascontiguousarray(np.asarray(a, np.float32))
    r = {k: f(rec[k]) for k in ("mean2D", "conic", "colors", "depths")}
    out = dict(means3D=np.zeros((P, 3), np.float32), cov3D=np.zeros((P, 6), np.float32), tau=np.zeros(6, np.float32))
    praw = f(cam.projmatrix_raw)
    p = rr._p
    L.ref_preprocess_backward(C.byref(s), p(praw), p(ofwd["radii"]), p(ofwd["clamped"]), p(r["mean2D"]), p(r["conic"]), p(r["colors"]),
                              p(r["depths"]), p(out["means3D"]), p(out["cov3D"]), None, p(out["tau"]))
    return out
