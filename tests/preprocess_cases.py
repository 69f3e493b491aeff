"""The scenes of tests/test_raster_preprocess_cpu.py and tests/test_raster_preprocess_gpu.py (numpy, seeded), the smallest that reach each
edge of preprocess_kernel / preprocess_backward_kernel, and the bounds both files share.  48 x 32 images: fx != fy in pixels.

A case is a dict: W, H, means [S,P,3], cov ([S,P,6] or [S,P,3,3]), opac [S,P], shs / colors_precomp, sh_degree, sh_rgb_major,
cam_scene [C], cams (the camera arrays in the library's layout), cam_objs (the oracle's Camera objects), classes
{name: bool [C,P]} -- the planted (camera, Gaussian) classes the exclusion cap counts.
"""
import math

import numpy as np

from oracle import preprocess_f64 as pf
from oracle import raster_ref as rr

W, H = 48, 32
K09 = np.array([[0.9, 0, 0.5], [0, 0.9, 0.5], [0, 0, 1]], np.float32)
TANFOV = 0.5 / 0.9
BG = np.array([0.2, 0.1, 0.3], np.float32)

# rho32 per output family: the largest |ref32 - ref64| / mag over every case below, the reference run in float32 against itself in
# float64 on the CPU (test_rho32_is_the_measured_float32_cost re-measures it: each entry must cover the measurement and stay within
# 2 x of it).  The GPU bound is GPU_MARGIN x rho32: FMA contraction, the reciprocal-multiply forms, v_rsq_f32 in the view direction
# and a different summation order cost a few ulp each.
GPU_MARGIN = 4.0
RHO32 = dict(xy=2.7e-7, conic=1.2e-6, rgb=3.3e-7, depth=1.6e-7, means3D=3.0e-7, cov6=6.4e-7, shs=5.5e-7, opacities=1.2e-7,
             colors_precomp=9.6e-8, means2D=0.0, tau_rho=1.9e-7, tau_theta=1.3e-7)


def _rot_y(a):
    return np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])


def _rot_x(a):
    return np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])


def _c2w(yaw=0.0, pitch=0.0, t=(0, 0, 0)):
    E = np.eye(4)
    E[:3, :3] = _rot_y(yaw) @ _rot_x(pitch)
    E[:3, 3] = t
    return E


def _cameras(Es):
    Es = np.stack(Es).astype(np.float32)
    n = len(Es)
    objs = rr.make_cameras(Es, np.tile(K09[None], (n, 1, 1)), np.full(n, 0.01, np.float32), np.full(n, 100.0, np.float32))
    arrs = dict(viewmatrix=np.stack([c.viewmatrix for c in objs]).astype(np.float32),
                projmatrix=np.stack([c.projmatrix for c in objs]).astype(np.float32),
                campos=np.stack([c.campos for c in objs]).astype(np.float32),
                tanfov=np.array([[c.tanfovx, c.tanfovy] for c in objs], np.float32))
    return objs, arrs


def _cov(rng, n, s_lo, s_hi):
    """R diag(s^2) R^T with the standard deviations in [s_lo, s_hi]: s_hi / s_lo <= 5 keeps the anisotropy (of the variances) <= 25 : 1"""
    assert s_hi / s_lo <= 5.0 + 1e-9
    q = rng.standard_normal((n, 4)); q /= np.linalg.norm(q, axis=-1, keepdims=True)
    x, y, z, w = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                  2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(n, 3, 3)
    s = rng.uniform(s_lo, s_hi, (n, 3))
    RS = R * s[:, None, :]
    return RS @ RS.transpose(0, 2, 1)


def _sh(rng, n, M, dc_mean=-0.9):
    """Coefficients for which each channel's colour clamps at zero for roughly a third of the (camera, Gaussian) pairs: the DC term puts
    the mean colour at 0.25, band 1 moves it by ~0.5 with the view direction."""
    sh = np.zeros((n, M, 3))
    sh[:, 0] = dc_mean + 1.2 * rng.standard_normal((n, 3))
    for lo, hi, sd in ((1, 4, 1.0), (4, 9, 0.5), (9, 16, 0.4), (16, M, 0.3)):
        if M > lo:
            sh[:, lo:min(hi, M)] = sd * rng.standard_normal((n, min(hi, M) - lo, 3))
    return sh


def _blob(rng, n, zsign=1.0, s_lo=0.03, s_hi=0.15):
    means = np.stack([rng.uniform(-0.9, 0.9, n), rng.uniform(-0.5, 0.5, n), zsign * rng.uniform(1.5, 4.0, n)], -1)
    return means, _cov(rng, n, s_lo, s_hi), rng.uniform(0.2, 0.95, n)


def _finish(name, means, cov, opac, cam_scene, Es, classes, *, shs=None, colors=None, sh_degree=3, sh_rgb_major=False, cov33=False):
    objs, arrs = _cameras(Es)
    f = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, np.float32))
    cov = np.asarray(cov)
    c = cov if cov33 else np.stack([cov[..., 0, 0], cov[..., 0, 1], cov[..., 0, 2], cov[..., 1, 1], cov[..., 1, 2], cov[..., 2, 2]], -1)
    if shs is not None and sh_rgb_major:
        shs = np.swapaxes(shs, -1, -2)
    return dict(name=name, W=W, H=H, means=f(means), cov=f(c), opac=f(opac), shs=f(shs), colors_precomp=f(colors), sh_degree=sh_degree,
                sh_rgb_major=sh_rgb_major, cam_scene=np.asarray(cam_scene, np.int32), cams=arrs, cam_objs=objs, classes=classes)


def _jitter(rng, n, rot=0.03, tr=0.05):
    return rng.uniform(-rot, rot, n), rng.uniform(-rot, rot, n), rng.uniform(-tr, tr, (n, 3))


# ---------------------------------------------------------------------------------------------------------------------------------
def pipeline(seed=11):
    """S = 4 scenes with 0, 1, 2 and 36 cameras (39 in all, irregular map); P = 300: two blocks, the second with 44 live lanes.  The
    cameras of a scene alternate (by list position) between looking down +z and down -z from the origin; Gaussians 0..139 sit at z > 0,
    140..279 at z < 0, so a Gaussian's visibility along its scene's list runs 1010.. or 0101..; 280..287 are seen by the first camera of
    the 36-camera scene only (it is yawed by 0.6), 288..295 by its last only, 296..299 by no camera."""
    rng = np.random.default_rng(seed)
    S, P, C = 4, 300, 39
    cam_scene = np.full(C, 3); cam_scene[1] = 1; cam_scene[3] = 2; cam_scene[20] = 2
    pos = np.zeros(C, int)
    for s in range(S):
        lst = np.nonzero(cam_scene == s)[0]
        pos[lst] = np.arange(len(lst))
    last = np.nonzero(cam_scene == 3)[0][-1]
    ya, pa, tr = _jitter(rng, C)
    Es = []
    for c in range(C):
        back = pos[c] % 2 == 1
        yaw = ya[c] + (math.pi if back else 0.0)
        if cam_scene[c] == 3 and pos[c] == 0:
            yaw += 0.6
        if c == last:
            yaw -= 0.6
        Es.append(_c2w(yaw, pa[c], tr[c]))
    means, cov, op, shs = [], [], [], []
    for s in range(S):
        a, b = _blob(rng, 140, 1.0), _blob(rng, 140, -1.0)
        m = np.concatenate([a[0], b[0], np.zeros((20, 3))])
        ang = 0.6 + rng.uniform(0.2, 0.45, 8)                     # first-only: inside the yawed first camera's image, 0.8 rad and more off every other axis
        m[280:288] = np.stack([3 * np.sin(ang), rng.uniform(-0.3, 0.3, 8), 3 * np.cos(ang)], -1)
        ang = math.pi - 0.6 - rng.uniform(0.2, 0.45, 8)           # last-only (the last camera of the list looks down -z, yawed by -0.6)
        m[288:296] = np.stack([3 * np.sin(ang), rng.uniform(-0.3, 0.3, 8), 3 * np.cos(ang)], -1)
        m[296:300] = np.stack([rng.uniform(-0.3, 0.3, 4), rng.uniform(9, 12, 4) * np.where(np.arange(4) % 2, 1, -1), rng.uniform(-0.4, 0.4, 4)], -1)
        means.append(m)
        cov.append(np.concatenate([a[1], b[1], _cov(rng, 20, 0.03, 0.1)]))
        op.append(np.concatenate([a[2], b[2], rng.uniform(0.3, 0.9, 20)]))
        shs.append(_sh(rng, P, 16))
    i = np.arange(P)[None, :]
    in3 = (cam_scene == 3)[:, None]
    even = (pos % 2 == 0)[:, None]
    classes = dict(front_even=in3 & even & (i < 140), back_odd=in3 & ~even & (i >= 140) & (i < 280),
                   first_only=in3 & (pos == 0)[:, None] & (i >= 280) & (i < 288), last_only=(np.arange(C) == last)[:, None] & (i >= 288) & (i < 296),
                   beyond_par_cams=in3 & (pos >= pf.K_PAR_CAMS)[:, None] & (i < 280), partial_wave=in3 & (i >= 256) & (i < 280))
    return _finish("pipeline", np.stack(means), np.stack(cov), np.stack(op), cam_scene, Es, classes, shs=np.stack(shs))


def chunks(seed=12):
    """C = 1100 cameras, crossing K2's list chunks at 512 and 1024; S = 3, P = 96.  Scene 0 has no camera in 512..1023; the cameras
    510..513 and 1022..1025 all belong to scene 1 (its list straddles both boundaries); scenes 1 and 2 have far more than 32 cameras in
    every chunk."""
    rng = np.random.default_rng(seed)
    S, P, C = 3, 96, 1100
    c = np.arange(C)
    cam_scene = np.where((c >= 512) & (c < 1024), 1 + c % 2, c % 3)
    cam_scene[510:514] = 1
    cam_scene[1022:1026] = 1
    ya, pa, tr = _jitter(rng, C, rot=0.06, tr=0.12)
    Es = [_c2w(ya[k], pa[k], tr[k]) for k in range(C)]
    sc = [_blob(rng, P) for _ in range(S)]
    chunk = c // pf.K_CAM_CHUNK
    all_p = np.ones((1, P), bool)
    classes = {f"scene{s}_chunk{j}": ((cam_scene == s) & (chunk == j))[:, None] & all_p for s in range(S) for j in range(3)
               if not (s == 0 and j == 1)}
    assert not ((cam_scene == 0) & (chunk == 1)).any()
    return _finish("chunks", np.stack([x[0] for x in sc]), np.stack([x[1] for x in sc]), np.stack([x[2] for x in sc]), cam_scene, Es,
                   classes, shs=np.stack([_sh(rng, P, 16) for _ in range(S)]))


def clamps(seed=13):
    """One scene, 5 cameras near the origin -- camera 2 looks the other way and sees nothing, between cameras that do --, P = 124.  0..15: wide Gaussians whose centres lie beyond 1.3 tanfov in x only (8 per
    sign), 16..31 in y only, 32..47 in both (4 per sign pair) -- all reach the image through their radius; 48..63: small Gaussians with
    vz in 0.12 .. 0.28, eight on either side of 0.2; 64..79: opacities on either side of 1/255; 80: a Gaussian so large that det^2
    overflows float32 (d2inv == 0: no covariance-path gradient); 81..123: ordinary Gaussians."""
    rng = np.random.default_rng(seed)
    P, C = 124, 5
    ya, pa, tr = _jitter(rng, C, rot=0.01, tr=0.004)
    Es = [_c2w(ya[k] + (math.pi if k == 2 else 0.0), pa[k], tr[k]) for k in range(C)]
    m, cv, op = _blob(rng, P)
    z = rng.uniform(1.8, 2.4, 48)
    t = rng.uniform(0.80, 0.90, 48)            # |x / z| or |y / z|: 1.3 tanfov = 0.722
    sg = np.where(np.arange(48) % 2, 1.0, -1.0)
    sg2 = np.where((np.arange(48) // 2) % 2, 1.0, -1.0)
    small = rng.uniform(-0.2, 0.2, 48)
    m[0:16] = np.stack([sg * t * z, small * z, z], -1)[0:16]
    m[16:32] = np.stack([small * z, sg * t * z, z], -1)[16:32]
    m[32:48] = np.stack([sg * t * z, sg2 * t * z, z], -1)[32:48]
    cv[0:48] = _cov(rng, 48, 0.3, 0.6)
    op[0:48] = rng.uniform(0.3, 0.8, 48)
    m[48:64] = np.stack([rng.uniform(-0.03, 0.03, 16), rng.uniform(-0.02, 0.02, 16),
                         np.concatenate([np.linspace(0.12, 0.188, 8), np.linspace(0.212, 0.28, 8)])], -1)
    cv[48:64] = _cov(rng, 16, 0.002, 0.006)
    op[64:72] = np.linspace(0.0020, 0.0038, 8)
    op[72:80] = np.linspace(0.0041, 0.0060, 8)
    m[80] = [0.1, -0.05, 3.5]
    cv[80] = _cov(rng, 1, 0.7e4, 1.4e4)[0]
    op[80] = 0.2
    vm = _cameras(Es)[1]["viewmatrix"].astype(np.float64)
    pc = np.einsum("cji,pj->cpi", vm.reshape(C, 4, 4)[:, :3, :3], m) + vm.reshape(C, 4, 4)[:, None, 3, :3]
    tx, ty = pc[..., 0] / pc[..., 2], pc[..., 1] / pc[..., 2]
    lim = 1.3 * TANFOV
    i = np.arange(P)[None, :]
    sees = (np.arange(C) != 2)[:, None]
    cx, cy = (np.abs(tx) > lim) & sees, (np.abs(ty) > lim) & sees
    classes = dict(clamp_x_neg=cx & ~cy & (tx < 0) & (i < 16), clamp_x_pos=cx & ~cy & (tx > 0) & (i < 16),
                   clamp_y_neg=~cx & cy & (ty < 0) & (i >= 16) & (i < 32), clamp_y_pos=~cx & cy & (ty > 0) & (i >= 16) & (i < 32),
                   clamp_xy=cx & cy & (i >= 32) & (i < 48), vz_below=(pc[..., 2] < 0.2) & (i >= 48) & (i < 64) & sees,
                   vz_above=(pc[..., 2] > 0.2) & (i >= 48) & (i < 64) & sees, opac_below=sees & (i >= 64) & (i < 72),
                   opac_above=sees & (i >= 72) & (i < 80))
    case = _finish("clamps", m[None], cv[None], op[None], np.zeros(C, int), Es, classes, shs=_sh(rng, P, 16, dc_mean=0.5)[None])
    case["overflow"], case["blind_camera"] = 80, 2
    return case


def _arc_cameras(rng, n, span=0.5, dist=3.0):
    """n cameras on an arc around the point (0, 0, 3), all looking at it: the view direction of a Gaussian differs by ~span / n between
    consecutive cameras"""
    Es = []
    for k in range(n):
        a = span * (2 * k / max(n - 1, 1) - 1) + rng.uniform(-0.02, 0.02)
        p = rng.uniform(-0.25, 0.25)
        R = _rot_y(a) @ _rot_x(p)
        E = np.eye(4); E[:3, :3] = R
        E[:3, 3] = np.array([0, 0, dist]) - R @ np.array([0, 0, dist])
        Es.append(E)
    return Es


SH_CASES = [(f"deg{d}_M{M}", d, M, False, False) for d in range(5) for M in (16, 25)] + \
           [("deg3_M25_rgb_major", 3, 25, True, False), ("deg3_M36", 3, 36, False, False), ("deg2_M36_rgb_major", 2, 36, True, False),
            ("colors_precomp", 0, 0, False, True)]


def sh(name, seed=14):
    """One scene, 5 cameras on an arc, P = 40: sh_degree 0..4 x M in {16, 25}, the rgb-major layout, M = 36 (K2's direct-store route:
    128 * 3M > 45 * 256) and colors_precomp."""
    _, deg, M, rgb_major, precomp = next(c for c in SH_CASES if c[0] == name)
    rng = np.random.default_rng(seed)
    P, C = 40, 5
    Es = _arc_cameras(rng, C)
    m, cv, op = _blob(rng, P)
    m[:, 2] = rng.uniform(2.2, 3.8, P)
    kw = dict(colors=rng.uniform(0.0, 1.0, (1, P, 3)), sh_degree=0) if precomp else \
        dict(shs=_sh(rng, P, M)[None], sh_degree=deg, sh_rgb_major=rgb_major)
    return _finish("sh_" + name, m[None], cv[None], op[None], np.zeros(C, int), Es, {}, **kw)


def cov33(seed=15):
    """VS_RASTER_COV_3X3: two scenes, 6 cameras, P = 70, covariances as [S, P, 3, 3]."""
    rng = np.random.default_rng(seed)
    S, P, C = 2, 70, 6
    ya, pa, tr = _jitter(rng, C)
    Es = [_c2w(ya[k], pa[k], tr[k]) for k in range(C)]
    sc = [_blob(rng, P) for _ in range(S)]
    return _finish("cov33", np.stack([x[0] for x in sc]), np.stack([x[1] for x in sc]), np.stack([x[2] for x in sc]),
                   np.array([0, 1, 1, 0, 1, 0]), Es, {}, shs=np.stack([_sh(rng, P, 16) for _ in range(S)]), cov33=True)


CASES = ["pipeline", "chunks", "clamps", "cov33"] + ["sh_" + c[0] for c in SH_CASES]
_CACHE = {}


def get(name):
    if name not in _CACHE:
        _CACHE[name] = sh(name[3:]) if name.startswith("sh_") else globals()[name]()
    return _CACHE[name]


def scene_kw(case):
    return dict(shs=case["shs"], colors_precomp=case["colors_precomp"], sh_degree=case["sh_degree"], sh_rgb_major=case["sh_rgb_major"])


def reference_forward(case, dtype=np.float64):
    return pf.forward(case["means"], case["cov"], case["opac"], case["cams"], case["cam_scene"], case["W"], case["H"], dtype=dtype,
                      **scene_kw(case))


def reference_backward(case, records, visible, clamped, dtype=np.float64, defect=None):
    return pf.backward(records, visible, clamped, case["means"], case["cov"], case["opac"], case["cams"], case["cam_scene"], case["W"],
                       case["H"], dtype=dtype, defect=defect, **scene_kw(case))


def families(case, r):
    """{family: (value, mag, exclusion mask)} of a backward result: per Gaussian and component (per camera for tau and means2D)."""
    ag, ac, ap = r["amb_gauss"], r["amb_cam"], r["ambiguous"]
    m = r["mag"]
    out = dict(means3D=(r["means3D"], m["means3D"], ag[..., None]), opacities=(r["opacities"], m["opacities"], ag),
               means2D=(r["means2D"], m["means2D"], ap[..., None]), tau_rho=(r["tau"][:, :3], m["tau"][:, :3], ac[:, None]),
               tau_theta=(r["tau"][:, 3:], m["tau"][:, 3:], ac[:, None]))
    k = "cov33" if case["cov"].ndim == 4 else "cov6"
    out["cov6"] = (r[k], m[k], ag[..., None, None] if k == "cov33" else ag[..., None])
    if case["shs"] is not None:
        k = "shs_rgb_major" if case["sh_rgb_major"] else "shs"
        out["shs"] = (r[k], m[k], ag[..., None, None])
    else:
        out["colors_precomp"] = (r["colors_precomp"], m["colors_precomp"], ag[..., None])
    return out


def ratio(val, ref, mag, excl):
    """max over the non-excluded elements of |val - ref| / mag (elements of zero mag must agree exactly: they count as inf otherwise)"""
    val, ref, mag = np.asarray(val, np.float64), np.asarray(ref, np.float64), np.asarray(mag, np.float64)
    err = np.abs(val - ref)
    with np.errstate(all="ignore"):
        q = np.where(mag > 0, err / mag, np.where(err == 0, 0.0, np.inf))
    q = np.where(np.broadcast_to(excl, q.shape), 0.0, q)
    return float(q.max()) if q.size else 0.0


def exclusion_cap(case, visible, ambiguous):
    """The condition on a case's seeds: at most 1 % of the visible pairs ambiguous, every planted class keeps >= 8 non-ambiguous
    visible members (the class below the vz cut: invisible ones)."""
    nv = int(visible.sum())
    assert nv > 0
    assert int((ambiguous & visible).sum()) <= 0.01 * nv, (case["name"], int((ambiguous & visible).sum()), nv)
    for k, mask in case["classes"].items():
        n = int((mask & ~ambiguous & (visible | k.startswith("vz_below"))).sum())
        assert n >= 8, (case["name"], k, n)
