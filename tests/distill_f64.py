"""Float64 reference (numpy) of the distillation point loss, Regr3D of src/loss/loss_conf_point.py:188-252 with normalize_pointcloud
'avg_dis' (src/geometry/ptc_geometry.py:270-328): loss, closed-form gradients, and per-output magnitudes in the manner of
tests/pointwise_f64.py (its class V carries them).  Independent of vicasplat_amd/callers.py.  The yardstick of tests/test_distill_gpu.py,
pinned to the real reference (tests/golden/distill_regr3d.npz) and to float64 autograd of a literal transcription by
tests/test_distill_cpu.py.

Quantiles: torch.quantile's default for an f32 input -- rank = q (n - 1) in f32 with q = f32(0.01), f32(0.99); floor, ceil, frac = rank -
floor in f32; torch's lerp (lo + frac (hi - lo) below frac = 0.5, hi - (hi - lo)(1 - frac) from there on) -- on the float64 distances of the
(f32-exact) inputs.  The mask is discrete: it is the f32 mask only while no distance is within rounding of a threshold, which
`gap_ok` states (the order statistics that bracket each quantile differ from each other and from their outer neighbours by >= 1e-4
relative) and `make_inputs` guarantees by retrying seeds.

`mutate=` plants one deliberate defect (MUTANTS); dtype=np.float32 runs the same formulas in f32.
"""
import numpy as np

from pointwise_f64 import U32, V

MUTANTS = ("strict", "count_per_element", "no_eps", "no_norm_grad", "q001", "conf_mean_valid")
# r32: max |torch f32 restatement (callers.Regr3D(backend="torch")) - f64| / (2^-24 mag) per output over the cases of
# tests/test_distill_cpu.py::test_torch_backend_matches_and_r32 (printed there: loss 0.2397, d_pts 0.5216, d_conf 0.8750), rounded up to
# two places.  The GPU bound of an output is 4 r32 2^-24 mag, with no floor: 0.96, 2.12 and 3.52 units.
R32 = dict(loss=0.24, d_pts=0.53, d_conf=0.88)
# What the torch restatement itself is held to on the CPU: its summation order, and with it its last bits, may change with the thread count
# and the torch build, so the CPU tests assert one unit and print the ratio; R32 records what was measured.
F32_LIMIT = 1.0


def gpu_factor(key):
    """B of the GPU criterion |gpu - ref| <= B 2^-24 mag for output `key` ("loss", "d_pts", "d_conf")."""
    return 4.0 * R32[key]


def ranks(n, q):
    """(floor, ceil, frac) of torch.quantile's rank for n samples, in f32 arithmetic."""
    r = np.float32(q) * np.float32(n - 1)
    lo = np.floor(r)
    return int(lo), int(np.ceil(r)), float(np.float32(r - lo))


def lerp(lo, hi, w):
    return lo + w * (hi - lo) if w < 0.5 else hi - (hi - lo) * (1.0 - w)


def thresholds(d, qs=(0.01, 0.99)):
    """d [B, n] float64 -> [B, 2] thresholds."""
    s = np.sort(d, axis=1)
    n = d.shape[1]
    out = np.empty((d.shape[0], 2))
    for j, q in enumerate(qs):
        lo, hi, w = ranks(n, q)
        for b in range(d.shape[0]):
            out[b, j] = lerp(s[b, lo], s[b, hi], w)
    return out


def gap_ok(pts, rel=1e-4):
    """True when, for every batch element of pts [B, H, W, 3], the order statistics bracketing each quantile differ from each other (unless
    the rank is an integer) and from their outer neighbours by >= rel, relative."""
    d = np.sort(np.sqrt((pts.astype(np.float64) ** 2).sum(-1)).reshape(pts.shape[0], -1), axis=1)
    n = d.shape[1]
    for q in (0.01, 0.99):
        lo, hi, _ = ranks(n, q)
        idx = [i for i in (lo - 1, lo, hi, hi + 1) if 0 <= i < n]
        idx = sorted(set(idx))
        for a, b in zip(idx[:-1], idx[1:]):
            if not bool(((d[:, b] - d[:, a]) >= rel * d[:, b]).all()):
                return False
    return True


def separate(pts, rel=1e-3):
    """Scales points [B, H, W, 3] radially, in place, so that gap_ok holds at any n.  Around the 1 % bracket: everything below it by
    1 - 2 rel, its lower statistic by 1 - 1.5 rel, its upper one by 1 - rel; around the 99 % bracket: 1 + rel, 1 + 1.5 rel, and 1 + 2 rel
    above it.  The scale is monotone in the rank, so the order of the distances is kept and neighbours end >= rel / 2 apart."""
    B = pts.shape[0]
    flat = pts.reshape(B, -1, 3)
    n = flat.shape[1]
    (l0, h0, _), (l1, h1, _) = ranks(n, 0.01), ranks(n, 0.99)
    for b in range(B):
        order = np.argsort(np.sqrt((flat[b].astype(np.float64) ** 2).sum(-1)), kind="stable")
        scale = np.ones(n)
        scale[order[:l0]] = 1 - 2 * rel
        scale[order[h0]] = 1 - rel
        scale[order[l0]] = 1 - 1.5 * rel
        scale[order[h1 + 1:]] = 1 + 2 * rel
        scale[order[l1]] = 1 + rel
        scale[order[h1]] = 1 + 1.5 * rel
        flat[b] = (flat[b] * scale[:, None]).astype(pts.dtype)
    return pts


def make_inputs(B, H, W, seed, conf=True):
    """Deterministic f32 inputs with gap_ok pseudo-GT in both views: dict gt1, gt2, pr1, pr2, cg1, cg2 (, pc1, pc2)."""
    for attempt in range(1000):
        rng = np.random.default_rng(seed * 1000 + attempt)
        z = {}
        for v in ("1", "2"):
            z["gt" + v] = (rng.normal(0, 1, (B, H, W, 3)) * [1.0, 0.7, 1.5] + [0.2, -0.1, 2.0]).astype(np.float32)
            z["pr" + v] = (z["gt" + v] * rng.uniform(0.8, 1.3) + rng.normal(0, 0.3, (B, H, W, 3))).astype(np.float32)
            z["cg" + v] = (1 + np.exp(rng.normal(0, 1, (B, H, W)))).astype(np.float32)
            if conf:
                z["pc" + v] = (1 + np.exp(rng.normal(0, 1, (B, H, W)))).astype(np.float32)
        if gap_ok(z["gt1"]) and gap_ok(z["gt2"]):
            return z
    raise RuntimeError("no seed gave well-separated quantile brackets")


def inputs_digest(z):
    """SHA-256 over the bytes of the input arrays, in key order."""
    import hashlib
    h = hashlib.sha256()
    for k in sorted(z):
        h.update(k.encode() + np.ascontiguousarray(z[k]).tobytes())
    return h.hexdigest()


def with_plateau(z, key="gt1", b=0, below=2, above=3):
    """A copy of the inputs in which the points of element b of z[key] whose distance ranks lie in [lo - below, lo + above] around the 1 %
    rank are bit-identical copies of the rank-lo point: a plateau that spans the rank.  The threshold is then the plateau's distance and
    every one of its points is kept (>=), `below` + 1 more than without the tie."""
    z = {k: v.copy() for k, v in z.items()}
    pts = z[key][b].reshape(-1, 3)
    order = np.argsort(np.sqrt((pts.astype(np.float64) ** 2).sum(-1)), kind="stable")
    lo = ranks(len(pts), 0.01)[0]
    pts[order[max(lo - below, 0):lo + above + 1]] = pts[order[lo]]
    z[key][b] = pts.reshape(z[key][b].shape)
    return z


def _sqrt(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        return x.fn(np.sqrt, lambda a: np.where(a > 0, 0.5 / np.sqrt(np.where(a > 0, a, 1)), 0))


def _norm(p):
    return _sqrt(p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1] + p[..., 2] * p[..., 2])


def _zero_like(x, dtype):
    return V(np.zeros_like(x.v, dtype=dtype))


def regr3d(gt1, gt2, pr1, pr2, cg1, cg2, pc1=None, pc2=None, normalize_pts=False, dtype=np.float64, mutate=None):
    """dict: loss, d_pts1, d_pts2 (, d_conf1, d_conf2), each with k + "_mag"; valid1, valid2 [B, H, W] bool; thr1, thr2 [B, 2]."""
    assert mutate is None or mutate in MUTANTS, mutate
    B, H, W, _ = gt1.shape
    dt = dtype
    gts, prs, cgs = [np.asarray(a, np.float64) for a in (gt1, gt2)], [np.asarray(a, np.float64) for a in (pr1, pr2)], [np.asarray(a, np.float64) for a in (cg1, cg2)]
    has_conf = pc1 is not None and pc2 is not None
    qs = (0.001, 0.999) if mutate == "q001" else (0.01, 0.99)
    valid, thr = [], []
    for g in gts:
        d = np.sqrt((g ** 2).sum(-1))
        t = thresholds(d.reshape(B, -1), qs)
        lo, hi = t[:, 0].reshape(B, 1, 1), t[:, 1].reshape(B, 1, 1)
        valid.append(((d > lo) & (d < hi)) if mutate == "strict" else ((d >= lo) & (d <= hi)))
        thr.append(t)
    G = [V(g.astype(dt)) for g in gts]
    P = [V(p.astype(dt)) for p in prs]
    C = [V(c.astype(dt)) for c in cgs]
    zero = lambda x: _zero_like(x, dt)
    if mutate == "count_per_element":
        cnt = [V(v.reshape(B, -1).sum(1).astype(dt).reshape(B, 1, 1)) * dt(B) for v in valid]     # mean of the per-element means
    else:
        cnt = [V(np.asarray(float(v.sum()), dt)) for v in valid]
    fp = fg = None
    if normalize_pts:
        nnz_v = (valid[0].reshape(B, -1).sum(1) + valid[1].reshape(B, -1).sum(1)).astype(np.float64) + (0.0 if mutate == "no_eps" else 1e-8)
        nnz = V(nnz_v.astype(dt))          # an integer + 1e-8: taken as exact (f32 rounds it to the integer)
        rp = [_norm(p) for p in P]
        fac = []
        for X, r in ((P, rp), (G, [_norm(g) for g in G])):
            s = None
            for v in range(2):
                t = V.where(valid[v], r[v], 0.0, dt)
                t = V(t.v.reshape(B, -1), t.m.reshape(B, -1)).sum(axis=1)
                s = t if s is None else s + t
            raw = s / nnz
            clipped = raw.v < 1e-8
            f = V.where(clipped, V.lift(1e-8, dt), raw, dt)
            fac.append((f, clipped))
        (fp, clip_p), (fg, _) = fac
        sh = lambda x: V(x.v.reshape(B, 1, 1, 1), x.m.reshape(B, 1, 1, 1))
        E = [G[v] / sh(fg) - P[v] / sh(fp) for v in range(2)]
    else:
        E = [G[v] - P[v] for v in range(2)]
    en = [_norm(e) for e in E]
    loss = None
    for v in range(2):
        t = V.where(valid[v], C[v] * en[v], 0.0, dt)
        t = V(t.v.reshape(-1), t.m.reshape(-1))
        if mutate == "count_per_element":
            c = np.broadcast_to(cnt[v].v, (B, H, W)).reshape(-1)
            t = (t / V(c.copy())).sum()
        else:
            t = t.sum() / cnt[v]
        loss = t if loss is None else loss + t
    out = dict(valid1=valid[0], valid2=valid[1], thr1=thr[0], thr2=thr[1])
    # gradients (upstream 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ehat = []
        for v in range(2):
            pos = en[v].v > 0
            safe = V(np.where(pos, en[v].v, 1).astype(dt), np.where(pos, en[v].m, 0).astype(dt))
            ehat.append([V.where(pos, E[v][..., k] / safe, 0.0, dt) for k in range(3)])
    w = [V.where(valid[v], C[v] / cnt[v], 0.0, dt) for v in range(2)]                 # gt_conf / count on valid pixels
    if normalize_pts:
        fp3 = V(fp.v.reshape(B, 1, 1), fp.m.reshape(B, 1, 1))
        T = None
        for v in range(2):
            dot = ehat[v][0] * P[v][..., 0] + ehat[v][1] * P[v][..., 1] + ehat[v][2] * P[v][..., 2]
            t = w[v] * dot
            t = V(t.v.reshape(B, -1), t.m.reshape(B, -1)).sum(axis=1)
            T = t if T is None else T + t
        kn = T / (fp * fp * nnz)
        kn = V.where(clip_p, 0.0, kn, dt)
        if mutate == "no_norm_grad":
            kn = zero(kn)
        kn = V(kn.v.reshape(B, 1, 1), kn.m.reshape(B, 1, 1))
    for v in range(2):
        comps = []
        for k in range(3):
            g = -(w[v] * ehat[v][k])
            if normalize_pts:
                g = g / fp3
                pos = rp[v].v > 0
                safe = V(np.where(pos, rp[v].v, 1).astype(dt), np.where(pos, rp[v].m, 0).astype(dt))
                g = g + V.where(valid[v] & pos, kn * (P[v][..., k] / safe), 0.0, dt)
            comps.append(g)
        d = V.stack(comps, -1)
        out[f"d_pts{v + 1}"], out[f"d_pts{v + 1}_mag"] = d.v, d.m
    if has_conf:
        for v, pc in enumerate((pc1, pc2)):
            diff = V(np.asarray(pc, np.float64).astype(dt)) - C[v]
            a = diff.fn(np.abs, np.sign)
            if mutate == "conf_mean_valid":
                t = V.where(valid[v], a, 0.0, dt)
                term = V(t.v.reshape(-1), t.m.reshape(-1)).sum() / cnt[v]
                dc = V.where(valid[v], V(np.sign(diff.v)) / cnt[v], 0.0, dt)
            else:
                term = V(a.v.reshape(-1), a.m.reshape(-1)).sum() / dt(B * H * W)
                dc = V(np.sign(diff.v)) / dt(B * H * W)
            loss = loss + term
            out[f"d_conf{v + 1}"], out[f"d_conf{v + 1}_mag"] = dc.v, dc.m
    out["loss"], out["loss_mag"] = loss.v, loss.m
    return out


def units(got, ref, name):
    """max |got - ref| / (2^-24 mag) over the elements of output `name` (0 where both the error and the magnitude are 0)."""
    err = np.abs(np.asarray(got, np.float64) - ref[name])
    mag = np.asarray(ref[name + "_mag"], np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(err == 0, 0.0, err / (U32 * mag))
    return float(np.max(u))
