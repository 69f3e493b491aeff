"""Float64 statement of the rasterizer's two per-(camera, Gaussian) kernels (numpy): preprocess_kernel (forward) and
preprocess_backward_kernel ("K2").  The yardstick of tests/test_raster_preprocess_cpu.py and tests/test_raster_preprocess_gpu.py.

TEST INFRASTRUCTURE ONLY.  One code path, parametrised by dtype: float64 is the reference, float32 is "what a plain f32 evaluation
of the same formulae costs on these inputs" (the tests derive their bounds from the gap between the two).

Forward, vectorised over the [C, P] (camera, Gaussian) pairs: pixel xy, the dilated 2-D covariance (a, b, cc), conic, colour
before / after the clamp at zero, depth, the true half extents sqrt(2 ln(255 o) a), sqrt(2 ln(255 o) cc), radius and tile rectangle.
Upstream's quirks are kept as the kernel has them: hw + 1e-7, the +0.3 dilation, max(0.1, mid^2 - det), vz > 0.2, SH bands
above 3 ignored.  VALUES are computed in `dtype`; DECISIONS (visible, ceil of the radius, the four rectangle integers, the clamp
bit per channel, xmul / ymul, tau > 0, det == 0, d2inv != 0) always come from the float32 evaluation in the kernel's operation
order (no contraction), and each is marked ambiguous where that f32 value is within a few ulp -- scaled by the sum of the absolute
terms that formed it, plus the f32 / f64 gap of the value itself -- of flipping.

Backward: consumes the per-pair gradient records [C, P, 10] (slot order of the render-backward kernels: mean2D xy in NDC units,
conic A B C, opacity, colour rgb, depth), the forward's `radii > 0` and clamp bits, and the scene / camera inputs.  Upstream's
formulae as K2 states them: d2inv = 1 / (det^2 + 1e-7), straight-through frustum clamp (xmul / ymul), straight-through colour
clamp through the bits.  Beside every output comes `mag`: the sum of the absolute values of the terms of the final accumulation
(over the scene's cameras; for dL_dtau over the Gaussians), where a term that is itself a sum or difference counts with the absolute
values of its own monomials (2 zz - xx - yy as 2 zz + xx + yy, the conic partials as the sum of their three absolute products, ...)
-- the error scale of a correct f32 evaluation, free of the cancellation a single near-zero term would hide.

Camera arrays are in the layout the library takes: viewmatrix / projmatrix [C, 16] (column-major 4x4), campos [C, 3],
tanfov [C, 2].  cam_scene [C] maps a camera to its scene (None: c % S).
"""
from __future__ import annotations

import numpy as np

TILE = 16
EPS32 = 2.0 ** -24
ULPS = 8.0                      # "a few ulp": half-width of the ambiguity band, in units of EPS32 x (sum of |terms|)
FLT_MAX = float(np.finfo(np.float32).max)
K_PAR_CAMS = 32                 # cameras of a chunk whose parameters K2 stages in LDS
K_CAM_CHUNK = 512               # cameras per list build of K2

C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
      1.445305721320277, -0.5900435899266435)

FAMILIES_FWD = ("xy", "conic", "rgb", "depth")
DEFECTS = ("record_prev", "record_next", "clamp_neighbour", "params_pos31", "drop_chunk2", "double_empty_chunk", "no_xmul",
           "offdiag", "sh_sign_band2", "sh_sign_band3", "no_passB_tau", "drop_last_wave_tau", "sh_shift_half")


def n_coef(sh_degree: int) -> int:
    return 16 if sh_degree >= 3 else (sh_degree + 1) ** 2


def camera_lists(cam_scene, C: int, S: int):
    cs = np.arange(C) % S if cam_scene is None else np.asarray(cam_scene).astype(np.int64)
    return cs, [np.nonzero(cs == s)[0] for s in range(S)]


def cov6_of(cov):
    cov = np.asarray(cov)
    if cov.ndim == 4:     # [S, P, 3, 3]: the kernels read the upper triangle
        return np.stack([cov[..., 0, 0], cov[..., 0, 1], cov[..., 0, 2], cov[..., 1, 1], cov[..., 1, 2], cov[..., 2, 2]], -1)
    return cov


def _gather(dt, means, cov, opac, cams, cs, shs, colors_precomp, sh_rgb_major, sh_degree):
    """Per-pair operands in dtype dt.  Scalars of a camera are [C, 1], of a pair [C, P]."""
    A = lambda x: np.asarray(x, np.float64).astype(dt)
    m, c6, op = A(means)[cs], A(cov6_of(cov))[cs], A(opac)[cs]
    V, Pm = A(cams["viewmatrix"]).reshape(-1, 16), A(cams["projmatrix"]).reshape(-1, 16)
    cp, tf = A(cams["campos"]), A(cams["tanfov"])
    g = dict(p=[m[..., k] for k in range(3)], S6=[c6[..., k] for k in range(6)], op=op,
             vm=[V[:, j:j + 1] for j in range(16)], pm=[Pm[:, j:j + 1] for j in range(16)],
             cp=[cp[:, k:k + 1] for k in range(3)], tfx=tf[:, 0:1], tfy=tf[:, 1:2], sh=None, col=None)
    if shs is not None:
        sh = A(shs)
        if sh_rgb_major:
            sh = np.swapaxes(sh, -1, -2)          # -> [S, P, M, 3]
        n = n_coef(sh_degree)
        full = np.zeros(sh.shape[:2] + (16, 3), dt)
        full[:, :, :n] = sh[:, :, :n]
        g["sh"] = full[cs]                        # [C, P, 16, 3]; rows >= n_coef are zero, as the kernels load them
    else:
        g["col"] = A(colors_precomp)[cs]
    return g


def _basis(dt, x, y, z, deg, absolute=False):
    """The 16 SH basis polynomials in the kernels' grouping (rows above the active degree: None).  absolute: every monomial by its
    absolute value (the error scale of the polynomial)."""
    f = dt.type
    s = -1.0
    if absolute:
        x, y, z, s = abs(x), abs(y), abs(z), 1.0
        c = lambda v: f(abs(v))
    else:
        c = f
    m = f(s)                   # the sign of a subtracted monomial
    b = [None] * 16
    b[0] = c(C0)
    if deg > 0:
        b[1], b[2], b[3] = c(-C1) * y, c(C1) * z, c(-C1) * x
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        b[4], b[5], b[6] = c(C2[0]) * xy, c(C2[1]) * yz, c(C2[2]) * (f(2) * zz + m * xx + m * yy)
        b[7], b[8] = c(C2[3]) * xz, c(C2[4]) * (xx + m * yy)
    if deg > 2:
        b[9] = c(C3[0]) * y * (f(3) * xx + m * yy)
        b[10] = c(C3[1]) * xy * z
        b[11] = c(C3[2]) * y * (f(4) * zz + m * xx + m * yy)
        b[12] = c(C3[3]) * z * (f(2) * zz + m * f(3) * xx + m * f(3) * yy)
        b[13] = c(C3[4]) * x * (f(4) * zz + m * xx + m * yy)
        b[14] = c(C3[5]) * z * (xx + m * yy)
        b[15] = c(C3[6]) * x * (xx + m * f(3) * yy)
    return b


def _geometry(dt, g, W, H):
    """View-space point, its error scales, focal lengths and frustum limits: the part the forward and K2 share."""
    f = dt.type
    px, py, pz = g["p"]
    vm = g["vm"]
    vx = vm[0] * px + vm[4] * py + vm[8] * pz + vm[12]
    vy = vm[1] * px + vm[5] * py + vm[9] * pz + vm[13]
    vz = vm[2] * px + vm[6] * py + vm[10] * pz + vm[14]
    sx = abs(vm[0] * px) + abs(vm[4] * py) + abs(vm[8] * pz) + abs(vm[12])
    sy = abs(vm[1] * px) + abs(vm[5] * py) + abs(vm[9] * pz) + abs(vm[13])
    sz = abs(vm[2] * px) + abs(vm[6] * py) + abs(vm[10] * pz) + abs(vm[14])
    fx, fy = f(W) / (f(2) * g["tfx"]), f(H) / (f(2) * g["tfy"])
    limx, limy = f(1.3) * g["tfx"], f(1.3) * g["tfy"]
    return dict(vx=vx, vy=vy, vz=vz, sx=sx, sy=sy, sz=sz, fx=fx, fy=fy, limx=limx, limy=limy)


def _cov2d(dt, g, J00, J02, J11, J12):
    vm = g["vm"]
    c0, c1, c2, c3, c4, c5 = g["S6"]
    S = ((c0, c1, c2), (c1, c3, c4), (c2, c4, c5))
    M0 = [J00 * vm[4 * k] + J02 * vm[4 * k + 2] for k in range(3)]
    M1 = [J11 * vm[4 * k + 1] + J12 * vm[4 * k + 2] for k in range(3)]
    t0 = [S[k][0] * M0[0] + S[k][1] * M0[1] + S[k][2] * M0[2] for k in range(3)]
    t1 = [S[k][0] * M1[0] + S[k][1] * M1[1] + S[k][2] * M1[2] for k in range(3)]
    f = dt.type
    a = M0[0] * t0[0] + M0[1] * t0[1] + M0[2] * t0[2] + f(0.3)
    b = M0[0] * t1[0] + M0[1] * t1[1] + M0[2] * t1[2]
    cc = M1[0] * t1[0] + M1[1] * t1[1] + M1[2] * t1[2] + f(0.3)
    return M0, M1, t0, t1, a, b, cc


def _forward_core(dt, g, W, H, deg):
    f = dt.type
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    with np.errstate(all="ignore"):
        q = _geometry(dt, g, W, H)
        vx, vy, vz = q["vx"], q["vy"], q["vz"]
        px, py, pz = g["p"]
        pm = g["pm"]
        hx = pm[0] * px + pm[4] * py + pm[8] * pz + pm[12]
        hy = pm[1] * px + pm[5] * py + pm[9] * pz + pm[13]
        hw = pm[3] * px + pm[7] * py + pm[11] * pz + pm[15]
        p_w = f(1) / (hw + f(0.0000001))
        projx, projy = hx * p_w, hy * p_w
        txtz, tytz = vx / vz, vy / vz
        tx = np.fmin(q["limx"], np.fmax(-q["limx"], txtz)) * vz
        ty = np.fmin(q["limy"], np.fmax(-q["limy"], tytz)) * vz
        tz = vz
        J00, J02 = q["fx"] / tz, -(q["fx"] * tx) / (tz * tz)
        J11, J12 = q["fy"] / tz, -(q["fy"] * ty) / (tz * tz)
        M0, M1, t0, t1, a, b, cc = _cov2d(dt, g, J00, J02, J11, J12)
        det = a * cc - b * b
        det_inv = f(1) / det
        conic = np.stack([cc * det_inv, -b * det_inv, a * det_inv], -1)
        mid = f(0.5) * (a + cc)
        disc = mid * mid - det
        sq = np.sqrt(np.fmax(f(0.1), disc))
        lam1, lam2 = mid + sq, mid - sq
        r_real = f(3) * np.sqrt(np.fmax(lam1, lam2))
        radius = np.ceil(r_real)
        pixx = ((projx + f(1)) * f(W) - f(1)) * f(0.5)
        pixy = ((projy + f(1)) * f(H) - f(1)) * f(0.5)
        rv = np.stack([(pixx - radius) / f(TILE), (pixy - radius) / f(TILE),
                       (pixx + radius + f(TILE - 1)) / f(TILE), (pixy + radius + f(TILE - 1)) / f(TILE)], -1)
        lim = np.array([gx, gy, gx, gy])
        f2i = lambda v: np.trunc(np.fmin(np.fmax(v, f(-1.0e6)), f(1.0e6))).astype(np.int64)
        rect = np.minimum(lim, np.maximum(0, f2i(rv)))
        area = (rect[..., 2] - rect[..., 0]) * (rect[..., 3] - rect[..., 1])
        visible = (vz > f(0.2)) & ~(det == 0) & (area > 0)
        # colour
        if g["sh"] is None:
            rgb_raw = g["col"].copy()
            rgb = rgb_raw
            bits = np.zeros(vz.shape, np.uint8)
            rgb_scale = np.abs(rgb_raw)
        else:
            dx, dy, dz = px - g["cp"][0], py - g["cp"][1], pz - g["cp"][2]
            rlen = f(1) / np.sqrt(dx * dx + dy * dy + dz * dz)
            x, y, z = dx * rlen, dy * rlen, dz * rlen
            bas, bas_a = _basis(dt, x, y, z, min(deg, 3)), _basis(dt, x, y, z, min(deg, 3), absolute=True)
            sh = g["sh"]
            rgb_raw = np.zeros(vz.shape + (3,), dt)
            rgb_scale = np.zeros(vz.shape + (3,), dt)
            for k in range(16):
                if bas[k] is None:
                    continue
                bk = np.asarray(bas[k], dt)[..., None] if np.ndim(bas[k]) else bas[k]
                rgb_raw = rgb_raw + bk * sh[:, :, k]
                bka = np.asarray(bas_a[k], dt)[..., None] if np.ndim(bas_a[k]) else bas_a[k]
                rgb_scale = rgb_scale + bka * abs(sh[:, :, k])
            rgb_raw = rgb_raw + f(0.5)
            rgb_scale = rgb_scale + f(0.5)
            neg = rgb_raw < 0
            bits = (neg * np.array([1, 2, 4])).sum(-1).astype(np.uint8)
            rgb = np.fmax(rgb_raw, f(0))
        op = g["op"]
        tau = np.log(f(255) * op)
        tau_pos = tau > 0
        tpos = np.where(tau_pos, tau, f(0))
        ext = np.stack([np.where(tau_pos, np.sqrt(f(2) * tpos * a), f(-1)), np.where(tau_pos, np.sqrt(f(2) * tpos * cc), f(-1))], -1)
        # K2's forms of the decisions it takes itself
        rz = f(1) / vz
        txtz2, tytz2 = vx * rz, vy * rz
        d2 = det * det + f(0.0000001)
        d2inv = f(1) / d2
    return dict(q=q, xy=np.stack([pixx, pixy], -1), a=a, b=b, cc=cc, det=det, conic=conic, rgb_raw=rgb_raw, rgb=rgb, depth=vz,
                ext=ext, tau=tau, r_real=r_real, radius=radius, rv=rv, rect=rect, visible=visible, bits=bits, rgb_scale=rgb_scale,
                txtz=txtz, tytz=tytz, txtz2=txtz2, tytz2=tytz2, d2inv_nz=d2inv != 0, mid=mid, disc=disc, sq=sq,
                hw=hw, tau_pos=tau_pos)


def forward(means, cov, opac, cams, cam_scene, W, H, *, shs=None, colors_precomp=None, sh_degree=0, sh_rgb_major=False,
            dtype=np.float64) -> dict:
    """Values in `dtype`, decisions from float32; all arrays [C, P, ...].  Keys: xy, a, b, cc, conic, rgb_raw, rgb, depth, ext (true
    half extents; -1 where tau <= 0), radius (int, 0 where invisible), rect (int, 0 where invisible), visible, clamped (bits),
    xmul, ymul (True: the frustum clamp is NOT active), tau_pos, det_zero, d2inv_nz; amb: {decision: bool [C, P]}; ambiguous: any
    of them; mag: {family: error scale of the forward values}."""
    dt = np.dtype(dtype)
    means = np.asarray(means)
    S, C = means.shape[0], np.asarray(cams["viewmatrix"]).reshape(-1, 16).shape[0]
    cs, _ = camera_lists(cam_scene, C, S)
    kw = dict(shs=shs, colors_precomp=colors_precomp, sh_rgb_major=sh_rgb_major, sh_degree=sh_degree)
    d32 = _forward_core(np.dtype(np.float32), _gather(np.dtype(np.float32), means, cov, opac, cams, cs, **kw), W, H, sh_degree)
    v64 = _forward_core(np.dtype(np.float64), _gather(np.dtype(np.float64), means, cov, opac, cams, cs, **kw), W, H, sh_degree)
    val = d32 if dt == np.float32 else v64
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    D = lambda k: d32[k].astype(np.float64)
    tol = ULPS * EPS32
    with np.errstate(all="ignore"):
        gap = lambda k: 2.0 * np.abs(np.nan_to_num(D(k) - v64[k], nan=0.0, posinf=0.0, neginf=0.0))
        q64 = v64["q"]
        amb = {}
        amb["vz"] = np.abs(D("depth") - 0.2) <= tol * q64["sz"] + gap("depth")
        amb["det_zero"] = np.abs(D("det")) <= tol * (np.abs(v64["a"] * v64["cc"]) + v64["b"] ** 2) + gap("det")
        # ceil(3 sqrt(lambda)): lambda = mid + sqrt(max(0.1, mid^2 - det)); the discriminant carries the cancellation
        x = v64["r_real"]
        cond = 1.0 + (v64["mid"] ** 2 + np.abs(v64["a"] * v64["cc"]) + v64["b"] ** 2) / (4.0 * v64["sq"] * np.maximum(v64["mid"] + v64["sq"], 1e-30))
        to_int = np.minimum(np.abs(D("r_real") - np.round(D("r_real"))), np.abs(x - np.round(x)))
        amb["radius"] = (to_int <= tol * x * cond + gap("r_real")) | (np.ceil(x) != D("radius"))
        amb["radius"] &= np.isfinite(x)
        # rectangle integers: trunc() flips at the integers 1 .. g (below 1 and above g the clamps decide)
        rv32, rv64 = D("rv"), v64["rv"]
        lim = np.array([gx, gy, gx, gy], np.float64)
        near = np.abs(rv32 - np.round(rv32))
        live = (np.round(rv32) >= 1) & (np.round(rv32) <= lim)
        scale = (np.abs(v64["xy"])[..., [0, 1, 0, 1]] + v64["radius"][..., None] + TILE) / TILE
        amb["rect"] = (live & (near <= tol * scale + 2.0 * np.abs(np.nan_to_num(rv32 - rv64)))).any(-1) | amb["radius"]
        amb["clamp"] = (np.abs(D("rgb_raw")) <= tol * v64["rgb_scale"] + gap("rgb_raw")).any(-1) if shs is not None \
            else np.zeros(amb["vz"].shape, bool)
        for ax, t1, t2, lm, sn, sd in (("xmul", "txtz", "txtz2", "limx", "sx", "sz"), ("ymul", "tytz", "tytz2", "limy", "sy", "sz")):
            t64 = v64[t1]
            sc = (q64[sn] + np.abs(t64) * q64[sd]) / np.abs(q64["vz"])
            lim32 = d32["q"][lm].astype(np.float64)
            dist = np.minimum(np.abs(np.abs(D(t1)) - lim32), np.abs(np.abs(D(t2)) - lim32))
            amb[ax] = dist <= tol * sc + gap(t1)
        amb["tau"] = np.abs(v64["tau"]) <= 2.0 * tol
        amb["d2inv"] = np.abs(np.log(np.maximum(D("det") ** 2, 1e-300) / FLT_MAX)) <= 1e-5
    vis = d32["visible"]
    xmul = ~((d32["txtz2"] < -d32["q"]["limx"]) | (d32["txtz2"] > d32["q"]["limx"]))
    ymul = ~((d32["tytz2"] < -d32["q"]["limy"]) | (d32["tytz2"] > d32["q"]["limy"]))
    out = {k: val[k] for k in ("xy", "a", "b", "cc", "conic", "rgb_raw", "rgb", "depth")}
    out["ext"] = np.where(d32["tau_pos"][..., None], val["ext"], -1.0)
    out.update(radius=np.where(vis, np.nan_to_num(D("radius"), posinf=1e6).clip(-1e6, 1e6), 0).astype(np.int64),
               rect=np.where(vis[..., None], d32["rect"], 0), visible=vis, clamped=d32["bits"], xmul=xmul, ymul=ymul,
               tau_pos=d32["tau_pos"], det_zero=d32["det"] == 0, d2inv_nz=d32["d2inv_nz"], amb=amb)
    out["ambiguous"] = np.logical_or.reduce([amb[k] for k in amb])
    # error scales of the values: |pix| + image size for xy (the NDC -> pixel map adds W / 2), the conic entries' common scale, the
    # SH sum's absolute terms, the view-space sum's absolute terms
    with np.errstate(all="ignore"):
        cmax = np.abs(v64["conic"]).max(-1, keepdims=True)
        out["mag"] = dict(xy=np.abs(v64["xy"]) + 0.5 * np.array([W, H]), conic=np.broadcast_to(cmax, v64["conic"].shape),
                          rgb=np.broadcast_to(v64["rgb_scale"], v64["rgb"].shape), depth=q64["sz"])
    return out


def _apply_record_defects(defect, rec, clamped, lists):
    rec, clamped = rec.copy(), clamped.copy()
    src_r, src_c = rec.copy(), clamped.copy()
    for lst in lists:
        if len(lst) < 2:
            continue
        if defect == "record_prev":
            rec[lst[1:]] = src_r[lst[:-1]]
        elif defect == "record_next":
            rec[lst[:-1]] = src_r[lst[1:]]
        elif defect == "clamp_neighbour":
            clamped[lst[:-1]] = src_c[lst[1:]]
    return rec, clamped


def backward(records, visible, clamped, means, cov, opac, cams, cam_scene, W, H, *, shs=None, colors_precomp=None, sh_degree=0,
             sh_rgb_major=False, dtype=np.float64, defect=None) -> dict:
    """records [C, P, 10], visible bool [C, P] (the forward's radii > 0), clamped uint8 [C, P].  Returns means3D [S,P,3], cov6 [S,P,6],
    cov33 [S,P,3,3] (halves), shs [S,P,M,3] and shs_rgb_major [S,P,3,M] (None without SH; zero for k >= 16), colors_precomp [S,P,3]
    (None with SH), opacities [S,P], means2D [C,P,2], tau [C,6]; `mag`: the same keys, the error scales; `ambiguous` [C,P]: a visible
    pair whose xmul / ymul / d2inv decision is within rounding of flipping; amb_gauss [S,P] / amb_cam [C]: their unions.

    `defect` (one of DEFECTS) plants a known error on this side, for the tests that show the GPU bounds can fail."""
    assert defect is None or defect in DEFECTS, defect
    dt = np.dtype(dtype)
    f = dt.type
    means = np.asarray(means)
    S, P = means.shape[0], means.shape[1]
    C = np.asarray(cams["viewmatrix"]).reshape(-1, 16).shape[0]
    cs, lists = camera_lists(cam_scene, C, S)
    has_sh = shs is not None
    M = 0 if not has_sh else (np.asarray(shs).shape[3] if sh_rgb_major else np.asarray(shs).shape[2])
    deg = min(int(sh_degree), 3)
    rec = np.asarray(records, np.float64).reshape(C, P, 10)
    vis = np.asarray(visible).astype(bool).reshape(C, P)
    clamped = np.asarray(clamped).astype(np.uint8).reshape(C, P)
    if defect in ("record_prev", "record_next", "clamp_neighbour"):
        rec, clamped = _apply_record_defects(defect, rec, clamped, lists)
    rec = np.where(vis[..., None], rec, 0.0).astype(dt)
    if defect == "params_pos31":      # list positions >= 32 of a chunk read the parameters staged for position 31
        cams = {k: np.array(np.asarray(v, np.float64).reshape(C, -1)) for k, v in cams.items()}
        src = {k: v.copy() for k, v in cams.items()}
        for lst in lists:
            for c0 in range(0, C, K_CAM_CHUNK):
                sub = lst[(lst >= c0) & (lst < c0 + K_CAM_CHUNK)]
                if len(sub) > K_PAR_CAMS:
                    for k in cams:
                        cams[k][sub[K_PAR_CAMS:]] = src[k][sub[K_PAR_CAMS - 1]]
    weight = np.ones(C)
    if defect == "drop_chunk2":
        weight[K_CAM_CHUNK:2 * K_CAM_CHUNK] = 0.0
    if defect == "double_empty_chunk":    # a chunk without a camera of the scene walks the previous chunk's list again
        for lst in lists:
            for c0 in range(K_CAM_CHUNK, C, K_CAM_CHUNK):
                if not ((lst >= c0) & (lst < c0 + K_CAM_CHUNK)).any():
                    weight[lst[(lst >= c0 - K_CAM_CHUNK) & (lst < c0)]] += 1.0

    kw = dict(shs=shs, colors_precomp=colors_precomp, sh_rgb_major=sh_rgb_major, sh_degree=sh_degree)
    g = _gather(dt, means, cov, opac, cams, cs, **kw)
    # ---- K2's own decisions, in float32 in its operation order ----
    f32 = np.dtype(np.float32)
    g32 = g if dt == f32 else _gather(f32, means, cov, opac, cams, cs, **kw)
    fwd = forward(means, cov, opac, cams, cam_scene, W, H, **kw)
    xmul, ymul = fwd["xmul"], fwd["ymul"]
    if defect == "no_xmul":
        xmul, ymul = np.ones_like(xmul), np.ones_like(ymul)
    with np.errstate(all="ignore"):
        q32 = _geometry(f32, g32, W, H)
        one = np.float32(1)
        rz = one / q32["vz"]
        tx32 = np.fmin(q32["limx"], np.fmax(-q32["limx"], q32["vx"] * rz)) * q32["vz"]
        ty32 = np.fmin(q32["limy"], np.fmax(-q32["limy"], q32["vy"] * rz)) * q32["vz"]
        tz2 = rz * rz
        _, _, _, _, a32, b32, c32 = _cov2d(f32, g32, q32["fx"] * rz, -(q32["fx"] * tx32) * tz2, q32["fy"] * rz, -(q32["fy"] * ty32) * tz2)
        det32 = a32 * c32 - b32 * b32
        d2nz = (one / (det32 * det32 + np.float32(0.0000001))) != 0
        amb_d2 = np.abs(np.log(np.maximum(det32.astype(np.float64) ** 2, 1e-300) / FLT_MAX)) <= 1e-5
    ambiguous = vis & (fwd["amb"]["xmul"] | fwd["amb"]["ymul"] | amb_d2)

    with np.errstate(all="ignore"):
        q = _geometry(dt, g, W, H)
        vm, pm = g["vm"], g["pm"]
        vx, vy, vz, fx, fy = q["vx"], q["vy"], q["vz"], q["fx"], q["fy"]
        px, py, pz = g["p"]
        g2x, g2y, gA, gB, gC = rec[..., 0], rec[..., 1], rec[..., 2], rec[..., 3], rec[..., 4]
        gop, gcol, gdep = rec[..., 5], rec[..., 6:9], rec[..., 9]
        X, Y = xmul.astype(dt), ymul.astype(dt)
        # ---- 2-D covariance path ----
        rz = f(1) / vz
        txtz, tytz = vx * rz, vy * rz
        tx = np.where(xmul, vx, np.fmin(q["limx"], np.fmax(-q["limx"], txtz)) * vz)
        ty = np.where(ymul, vy, np.fmin(q["limy"], np.fmax(-q["limy"], tytz)) * vz)
        tz2 = rz * rz
        tz3 = tz2 * rz
        J00, J02, J11, J12 = fx * rz, -(fx * tx) * tz2, fy * rz, -(fy * ty) * tz2
        M0, M1, t0, t1, a, b, cc = _cov2d(dt, g, J00, J02, J11, J12)
        det = a * cc - b * b
        d2inv = np.where(d2nz, f(1) / (det * det + f(0.0000001)), f(0))
        d2inv = np.where(np.isfinite(d2inv), d2inv, f(0))
        z_ = np.zeros_like(vz)
        fin = lambda v: np.where(d2nz, v, z_)
        ga = fin(d2inv * (-cc * cc * gA + b * cc * gB - b * b * gC))
        gc = fin(d2inv * (-b * b * gA + a * b * gB - a * a * gC))
        gb = fin(d2inv * (f(2) * b * cc * gA - (det + f(2) * b * b) * gB + f(2) * a * b * gC))
        # Beside every value X comes Xa >= |X|: the sum of the absolute values of the monomials that form X (a term that is itself a
        # difference counts with the absolute values of its parts), so that `mag` is the scale of the rounding error of the whole
        # evaluation, not only of its last sum.
        ab = np.abs
        ga_a = fin(d2inv * (cc * cc * ab(gA) + ab(b * cc) * ab(gB) + b * b * ab(gC)))
        gc_a = fin(d2inv * (b * b * ab(gA) + ab(a * b) * ab(gB) + a * a * ab(gC)))
        gb_a = fin(d2inv * (f(2) * ab(b * cc) * ab(gA) + (ab(a * cc) + f(3) * b * b) * ab(gB) + f(2) * ab(a * b) * ab(gC)))
        c0, c1, c2, c3, c4, c5 = g["S6"]
        Sm = ((c0, c1, c2), (c1, c3, c4), (c2, c4, c5))
        M0a = [ab(J00 * vm[4 * k]) + ab(J02 * vm[4 * k + 2]) for k in range(3)]
        M1a = [ab(J11 * vm[4 * k + 1]) + ab(J12 * vm[4 * k + 2]) for k in range(3)]
        t0a = [ab(Sm[k][0]) * M0a[0] + ab(Sm[k][1]) * M0a[1] + ab(Sm[k][2]) * M0a[2] for k in range(3)]
        t1a = [ab(Sm[k][0]) * M1a[0] + ab(Sm[k][1]) * M1a[1] + ab(Sm[k][2]) * M1a[2] for k in range(3)]
        pairs6 = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
        cov_v, cov_a = [], []
        for (i, j) in pairs6:
            if i == j:
                cov_v.append(M0[i] * M0[i] * ga + M0[i] * M1[i] * gb + M1[i] * M1[i] * gc)
                cov_a.append(M0a[i] * M0a[i] * ga_a + M0a[i] * M1a[i] * gb_a + M1a[i] * M1a[i] * gc_a)
            else:
                cov_v.append(f(2) * M0[i] * M0[j] * ga + (M0[i] * M1[j] + M0[j] * M1[i]) * gb + f(2) * M1[i] * M1[j] * gc)
                cov_a.append(f(2) * M0a[i] * M0a[j] * ga_a + (M0a[i] * M1a[j] + M0a[j] * M1a[i]) * gb_a + f(2) * M1a[i] * M1a[j] * gc_a)
        gM0 = [f(2) * ga * t0[k] + gb * t1[k] for k in range(3)]
        gM1 = [f(2) * gc * t1[k] + gb * t0[k] for k in range(3)]
        gM0a = [f(2) * ga_a * t0a[k] + gb_a * t1a[k] for k in range(3)]
        gM1a = [f(2) * gc_a * t1a[k] + gb_a * t0a[k] for k in range(3)]
        gJ00 = sum(gM0[k] * vm[4 * k] for k in range(3))
        gJ02 = sum(gM0[k] * vm[4 * k + 2] for k in range(3))
        gJ11 = sum(gM1[k] * vm[4 * k + 1] for k in range(3))
        gJ12 = sum(gM1[k] * vm[4 * k + 2] for k in range(3))
        gJ00a = sum(gM0a[k] * ab(vm[4 * k]) for k in range(3))
        gJ02a = sum(gM0a[k] * ab(vm[4 * k + 2]) for k in range(3))
        gJ11a = sum(gM1a[k] * ab(vm[4 * k + 1]) for k in range(3))
        gJ12a = sum(gM1a[k] * ab(vm[4 * k + 2]) for k in range(3))
        gR = [[J00 * gM0[k] for k in range(3)], [J11 * gM1[k] for k in range(3)], [J02 * gM0[k] + J12 * gM1[k] for k in range(3)]]
        gRa = [[ab(J00) * gM0a[k] for k in range(3)], [ab(J11) * gM1a[k] for k in range(3)],
               [ab(J02) * gM0a[k] + ab(J12) * gM1a[k] for k in range(3)]]
        gpc = [X * (-fx * tz2) * gJ02, Y * (-fy * tz2) * gJ12,
               -fx * tz2 * gJ00 - fy * tz2 * gJ11 + (f(2) * fx * tx) * tz3 * gJ02 + (f(2) * fy * ty) * tz3 * gJ12]
        gpc_a = [X * ab(fx * tz2) * gJ02a, Y * ab(fy * tz2) * gJ12a,
                 ab(fx * tz2) * gJ00a + ab(fy * tz2) * gJ11a + ab(f(2) * fx * tx * tz3) * gJ02a + ab(f(2) * fy * ty * tz3) * gJ12a]
        # ---- projected mean path ----
        hx = pm[0] * px + pm[4] * py + pm[8] * pz + pm[12]
        hy = pm[1] * px + pm[5] * py + pm[9] * pz + pm[13]
        hw = pm[3] * px + pm[7] * py + pm[11] * pz + pm[15]
        m_w = f(1) / (hw + f(0.0000001))
        mul1, mul2 = hx * m_w * m_w, hy * m_w * m_w
        gw = [(pm[4 * k] * m_w - pm[4 * k + 3] * mul1) * g2x + (pm[4 * k + 1] * m_w - pm[4 * k + 3] * mul2) * g2y for k in range(3)]
        gw_a = [(ab(pm[4 * k] * m_w) + ab(pm[4 * k + 3] * mul1)) * ab(g2x) + (ab(pm[4 * k + 1] * m_w) + ab(pm[4 * k + 3] * mul2)) * ab(g2y)
                for k in range(3)]
        for r in range(3):
            gpc[r] = gpc[r] + (vm[r] * gw[0] + vm[4 + r] * gw[1] + vm[8 + r] * gw[2])
            gpc_a[r] = gpc_a[r] + (ab(vm[r]) * gw_a[0] + ab(vm[4 + r]) * gw_a[1] + ab(vm[8 + r]) * gw_a[2])
        gpc[2] = gpc[2] + gdep          # depth path
        gpc_a[2] = gpc_a[2] + ab(gdep)
        msk = lambda v: np.where(vis, v, z_)
        gpc, gpc_a = [msk(v) for v in gpc], [msk(v) for v in gpc_a]
        cov_v, cov_a = [msk(v) for v in cov_v], [msk(v) for v in cov_a]
        mean_v = [vm[4 * k] * gpc[0] + vm[4 * k + 1] * gpc[1] + vm[4 * k + 2] * gpc[2] for k in range(3)]
        mean_a = [ab(vm[4 * k]) * gpc_a[0] + ab(vm[4 * k + 1]) * gpc_a[1] + ab(vm[4 * k + 2]) * gpc_a[2] for k in range(3)]
        th_v = [vy * gpc[2] - vz * gpc[1], vz * gpc[0] - vx * gpc[2], vx * gpc[1] - vy * gpc[0]]
        th_a = [ab(vy) * gpc_a[2] + ab(vz) * gpc_a[1], ab(vz) * gpc_a[0] + ab(vx) * gpc_a[2], ab(vx) * gpc_a[1] + ab(vy) * gpc_a[0]]
        for j in range(3):
            r0, r1, r2 = vm[4 * j], vm[4 * j + 1], vm[4 * j + 2]
            th_v[0] = th_v[0] + (r1 * gR[2][j] - r2 * gR[1][j])
            th_v[1] = th_v[1] + (r2 * gR[0][j] - r0 * gR[2][j])
            th_v[2] = th_v[2] + (r0 * gR[1][j] - r1 * gR[0][j])
            th_a[0] = th_a[0] + (ab(r1) * gRa[2][j] + ab(r2) * gRa[1][j])
            th_a[1] = th_a[1] + (ab(r2) * gRa[0][j] + ab(r0) * gRa[2][j])
            th_a[2] = th_a[2] + (ab(r0) * gRa[1][j] + ab(r1) * gRa[0][j])
        th_v, th_a = [msk(v) for v in th_v], [msk(v) for v in th_a]
        rho_v, rho_a = [gpc[0], gpc[1], gpc[2]], [gpc_a[0], gpc_a[1], gpc_a[2]]
        # ---- colour path ----
        sh_v = sh_a = None
        if has_sh:
            keep = ((clamped[..., None] >> np.arange(3)) & 1) == 0
            gch = np.where(keep & vis[..., None], gcol, f(0))                   # [C, P, 3]
            dxo, dyo, dzo = px - g["cp"][0], py - g["cp"][1], pz - g["cp"][2]
            rlen = f(1) / np.sqrt(dxo * dxo + dyo * dyo + dzo * dzo)
            x, y, z = dxo * rlen, dyo * rlen, dzo * rlen
            bas, bas_a = _basis(dt, x, y, z, deg), _basis(dt, x, y, z, deg, absolute=True)
            sh_v, sh_a = np.zeros((C, P, 16, 3), dt), np.zeros((C, P, 16, 3), dt)
            for k in range(16):
                if bas[k] is not None:
                    bk = bas[k][..., None] if np.ndim(bas[k]) else bas[k]
                    bka = bas_a[k][..., None] if np.ndim(bas_a[k]) else bas_a[k]
                    sh_v[:, :, k] = np.where(vis[..., None], bk * gch, f(0))
                    sh_a[:, :, k] = np.where(vis[..., None], bka * ab(gch), f(0))
            sh = g["sh"]
            w = [(sh[:, :, k] * gch).sum(-1) for k in range(16)]
            wa = [ab(sh[:, :, k] * gch).sum(-1) for k in range(16)]
            xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
            ax, ay, az, axy, ayz, axz = ab(x), ab(y), ab(z), ab(xy), ab(yz), ab(xz)
            ddx = ddy = ddz = ddxa = ddya = ddza = z_
            if deg > 0:
                ddx, ddy, ddz = -f(C1) * w[3], -f(C1) * w[1], f(C1) * w[2]
                ddxa, ddya, ddza = f(C1) * wa[3], f(C1) * wa[1], f(C1) * wa[2]
            if deg > 1:
                s7 = f(-1) if defect == "sh_sign_band2" else f(1)
                q = [f(abs(v)) for v in C2]
                ddx = ddx + f(C2[0]) * y * w[4] - f(2) * f(C2[2]) * x * w[6] + s7 * f(C2[3]) * z * w[7] + f(2) * f(C2[4]) * x * w[8]
                ddy = ddy + f(C2[0]) * x * w[4] + f(C2[1]) * z * w[5] - f(2) * f(C2[2]) * y * w[6] - f(2) * f(C2[4]) * y * w[8]
                ddz = ddz + f(C2[1]) * y * w[5] + f(4) * f(C2[2]) * z * w[6] + f(C2[3]) * x * w[7]
                ddxa = ddxa + q[0] * ay * wa[4] + f(2) * q[2] * ax * wa[6] + q[3] * az * wa[7] + f(2) * q[4] * ax * wa[8]
                ddya = ddya + q[0] * ax * wa[4] + q[1] * az * wa[5] + f(2) * q[2] * ay * wa[6] + f(2) * q[4] * ay * wa[8]
                ddza = ddza + q[1] * ay * wa[5] + f(4) * q[2] * az * wa[6] + q[3] * ax * wa[7]
            if deg > 2:
                s13 = f(-1) if defect == "sh_sign_band3" else f(1)
                q = [f(abs(v)) for v in C3]
                ddx = ddx + (f(C3[0]) * w[9] * f(6) * xy + f(C3[1]) * w[10] * yz + f(C3[2]) * w[11] * f(-2) * xy
                             + f(C3[3]) * w[12] * f(-6) * xz + f(C3[4]) * w[13] * (f(-3) * xx + f(4) * zz - yy)
                             + f(C3[5]) * w[14] * f(2) * xz + f(C3[6]) * w[15] * f(3) * (xx - yy))
                ddy = ddy + (f(C3[0]) * w[9] * f(3) * (xx - yy) + f(C3[1]) * w[10] * xz
                             + f(C3[2]) * w[11] * (f(-3) * yy + f(4) * zz - xx) + f(C3[3]) * w[12] * f(-6) * yz
                             + f(C3[4]) * w[13] * f(-2) * xy + f(C3[5]) * w[14] * f(-2) * yz + f(C3[6]) * w[15] * f(-6) * xy)
                ddz = ddz + (f(C3[1]) * w[10] * xy + f(C3[2]) * w[11] * f(8) * yz + f(C3[3]) * w[12] * f(3) * (f(2) * zz - xx - yy)
                             + s13 * f(C3[4]) * w[13] * f(8) * xz + f(C3[5]) * w[14] * (xx - yy))
                ddxa = ddxa + (q[0] * wa[9] * f(6) * axy + q[1] * wa[10] * ayz + q[2] * wa[11] * f(2) * axy + q[3] * wa[12] * f(6) * axz
                               + q[4] * wa[13] * (f(3) * xx + f(4) * zz + yy) + q[5] * wa[14] * f(2) * axz + q[6] * wa[15] * f(3) * (xx + yy))
                ddya = ddya + (q[0] * wa[9] * f(3) * (xx + yy) + q[1] * wa[10] * axz + q[2] * wa[11] * (f(3) * yy + f(4) * zz + xx)
                               + q[3] * wa[12] * f(6) * ayz + q[4] * wa[13] * f(2) * axy + q[5] * wa[14] * f(2) * ayz + q[6] * wa[15] * f(6) * axy)
                ddza = ddza + (q[1] * wa[10] * axy + q[2] * wa[11] * f(8) * ayz + q[3] * wa[12] * f(3) * (f(2) * zz + xx + yy)
                               + q[4] * wa[13] * f(8) * axz + q[5] * wa[14] * (xx + yy))
            dot = x * ddx + y * ddy + z * ddz
            dota = ax * ddxa + ay * ddya + az * ddza
            gd = [msk((ddx - x * dot) * rlen), msk((ddy - y * dot) * rlen), msk((ddz - z * dot) * rlen)]
            gda = [msk((ddxa + ax * dota) * rlen), msk((ddya + ay * dota) * rlen), msk((ddza + az * dota) * rlen)]
            for k in range(3):
                mean_v[k], mean_a[k] = mean_v[k] + gd[k], mean_a[k] + gda[k]
            if defect != "no_passB_tau":
                for r in range(3):
                    rho_v[r] = rho_v[r] + (vm[r] * gd[0] + vm[4 + r] * gd[1] + vm[8 + r] * gd[2])
                    rho_a[r] = rho_a[r] + (ab(vm[r]) * gda[0] + ab(vm[4 + r]) * gda[1] + ab(vm[8 + r]) * gda[2])

    wt = weight.astype(dt)[:, None]

    def per_scene(val, scale):
        """[C, P] per-camera contributions and their error scales -> sums over each scene's cameras [S, P], accumulated camera by
        camera in ascending order in dt."""
        tot = (val * np.ones_like(vz)) * wt
        mg = (scale * np.ones_like(vz)).astype(np.float64) * weight[:, None]
        out, mag = np.zeros((S, P), dt), np.zeros((S, P))
        for s, lst in enumerate(lists):
            for c in lst:
                out[s] += tot[c]
                mag[s] += mg[c]
        return out, mag

    def stack_scene(vals, scales):
        r = [per_scene(v, a) for v, a in zip(vals, scales)]
        return np.stack([a for a, _ in r], -1), np.stack([m for _, m in r], -1)

    res, mag = {}, {}
    res["means3D"], mag["means3D"] = stack_scene(mean_v, mean_a)
    c6, m6 = stack_scene(cov_v, cov_a)
    half = np.array([1, 0.5, 0.5, 1, 0.5, 1])
    idx = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])
    if defect == "offdiag":           # off-diagonal partials not doubled (6-vector) / not halved (3 x 3)
        res["cov6"], res["cov33"] = c6 * half.astype(dt), c6[..., idx]
    else:
        res["cov6"], res["cov33"] = c6, (c6 * half.astype(dt))[..., idx]
    mag["cov6"], mag["cov33"] = m6, (m6 * half)[..., idx]
    res["opacities"], mag["opacities"] = per_scene(msk(gop), ab(msk(gop)))
    if has_sh:
        fv, fa = sh_v.reshape(C, P, 48), sh_a.reshape(C, P, 48)
        o16, m16 = stack_scene([fv[..., e] for e in range(48)], [fa[..., e] for e in range(48)])
        o16, m16 = o16.reshape(S, P, 16, 3), m16.reshape(S, P, 16, 3)
        full, mfull = np.zeros((S, P, M, 3), dt), np.zeros((S, P, M, 3))
        n = min(M, 16)
        full[:, :, :n], mfull[:, :, :n] = o16[:, :, :n], m16[:, :, :n]
        if defect == "sh_shift_half":     # rows of the second half-block (Gaussians 128..255 of a block of 256) land one Gaussian late
            i = np.arange(P)
            second = np.nonzero((i % 256) >= 128)[0]
            src = full.copy()
            full[:, second] = src[:, second - 1]
        res["shs"], mag["shs"] = full, mfull
        res["shs_rgb_major"], mag["shs_rgb_major"] = np.swapaxes(full, -1, -2), np.swapaxes(mfull, -1, -2)
        res["colors_precomp"] = mag["colors_precomp"] = None
    else:
        res["shs"] = mag["shs"] = res["shs_rgb_major"] = mag["shs_rgb_major"] = None
        cpv = [msk(gcol[..., k]) for k in range(3)]
        res["colors_precomp"], mag["colors_precomp"] = stack_scene(cpv, [ab(v) for v in cpv])
    m2 = np.where(vis[..., None], rec[..., 0:2], f(0))
    res["means2D"], mag["means2D"] = m2, np.abs(m2).astype(np.float64)
    # dL_dtau: per camera, summed over the Gaussians
    live = np.ones(P, bool)
    if defect == "drop_last_wave_tau" and P % 64:
        live[(P // 64) * 64:] = False
    tau = np.zeros((C, 6), dt)
    tmag = np.zeros((C, 6))
    for k, (v, a) in enumerate(zip(rho_v + th_v, rho_a + th_a)):
        tau[:, k] = (v * np.ones_like(vz))[:, live].sum(1) * weight.astype(dt)
        tmag[:, k] = (a * np.ones_like(vz)).astype(np.float64)[:, live].sum(1) * weight
    res["tau"], mag["tau"] = tau, tmag
    res["mag"] = mag
    res["ambiguous"] = ambiguous
    amb_g = np.zeros((S, P), bool)
    for s, lst in enumerate(lists):
        if len(lst):
            amb_g[s] = ambiguous[lst].any(0)
    res["amb_gauss"], res["amb_cam"] = amb_g, ambiguous.any(1)
    res["decisions"] = dict(xmul=xmul, ymul=ymul, d2inv_nz=d2nz)
    return res


def extents_ok(ext_gpu, ext_true):
    """The forward's conservative footprint: contains the true half extent, stays inside 1.011 x true + 0.051 (the kernel's x 1.01 + 0.05
    and a 1-ulp hardware log and sqrt); -1 where tau <= 0.  Element-wise bool."""
    e, t = np.asarray(ext_gpu, np.float64), np.asarray(ext_true, np.float64)
    return np.where(t < 0, e == -1.0, (e >= t) & (e <= 1.011 * t + 0.051))
