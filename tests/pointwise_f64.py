"""Float64 references (numpy) of the two non-matrix operators of the default class, with per-element magnitudes: the fused Gaussian adapter
(csrc/adapter.hip: 'exp' depth post-process + MyGaussianAdapter, forward and chain rule) and LayerNorm with AdaLN modulation
(csrc/norm_rope.hip, csrc/backward.hip).  The yardstick of tests/test_adapter_edges_gpu.py and tests/test_layernorm_edges_gpu.py, pinned
to torch float64 autograd by tests/test_pointwise_ref_cpu.py.

Every output `k` comes with `k + "_mag"`: the sum of the absolute values of the products that form it, carried through every operation
of the formula (class V): an input (exact in f32) has 0; a sum, product or quotient adds |its result| to the magnitudes of its operands
weighted by the absolute partial derivatives; a function f adds |f(v)| to |f'(v)| mag(v).  2^-24 mag is therefore the first-order bound
of the error of the same formula evaluated in f32 with every operation rounded once, including what cancellations amplify (1 - (1 - p)
near p = 0, (e^d d - expm1 d) / d^2 near d = 0, x - mean on a row of mean 300).  Products and quotients also carry the second-order
term 2^-24 mag(a) mag(b): on a constant LayerNorm row xhat and mean(g xhat) are both pure rounding error (exactly 0 in exact
arithmetic), and their product is not small beside the first-order terms.  A pure copy has mag 0 and must be bit exact.

The same code runs in float32 (dtype=np.float32): that is the f32 restatement whose distance from float64, in units of 2^-24 mag, is
r32 (R32_ADAPTER / R32_LAYERNORM, measured by tests/test_pointwise_ref_cpu.py), and `mutate=` plants one deliberate defect in it.
"""
import numpy as np

U32 = 2.0 ** -24
SCALE_CLAMP = 0.3          # clamp_max of the exp / softplus activations
SOFTPLUS_THRESHOLD = 20.0  # F.softplus passes v through above it
DIST_CLAMP = 1e-8          # dist.clip(min=1e-8) of the depth post-process
QUAT_EPS = 1e-12           # F.normalize
TWO_S_EPS = 1e-8           # two_s = 2 / (q.q + 1e-8)

# r32 = max |f32 restatement - f64| / (2^-24 mag) over the edge sets (all activations, opacity exponents 1, 2, 0.5, -1), as printed by
# tests/test_pointwise_ref_cpu.py::test_f32_restatement_ratios, rounded up.  The GPU bound of an output is 4 max(r32, 1) 2^-24 mag.
R32_ADAPTER = dict(means=1.0, covariances=1.0, harmonics=1.0, opacities=1.0, scales=1.0, rotations=1.0, raw=1.0, d_pts=1.0, d_gs=1.0)
R32_LAYERNORM = dict(y=1.2, dx=1.1, dw=1.1, db=2.4, dscale=1.2, dshift=2.1)


def gpu_factor(r32):
    """B of the GPU criterion: 4 x r32 with a floor of r32 = 1 (operation order; the device's expf / log1pf / powf / expm1f)."""
    return 4.0 * max(float(r32), 1.0)


def _f32_exact(a):
    with np.errstate(over="ignore"):
        return a.astype(np.float32).astype(np.float64) == a


class V:
    """value + magnitude (see the module docstring).  Plain numbers and arrays are constants: magnitude 0 if exact in f32, else |c|."""
    __slots__ = ("v", "m")

    def __init__(self, v, m=None):
        self.v = v
        self.m = np.zeros_like(v) if m is None else m

    @staticmethod
    def lift(c, dtype):
        if isinstance(c, V):
            return c
        c64 = np.asarray(c, np.float64)
        return V(c64.astype(dtype), np.where(_f32_exact(c64), 0.0, np.abs(c64)).astype(dtype))

    def _o(self, o):
        return V.lift(o, self.v.dtype)

    def __neg__(self):
        return V(-self.v, self.m)

    def __add__(self, o):
        o = self._o(o); v = self.v + o.v
        return V(v, self.m + o.m + np.abs(v))
    __radd__ = __add__

    def __sub__(self, o):
        o = self._o(o); v = self.v - o.v
        return V(v, self.m + o.m + np.abs(v))

    def __rsub__(self, o):
        return self._o(o) - self

    def __mul__(self, o):
        o = self._o(o); v = self.v * o.v
        return V(v, np.abs(self.v) * o.m + np.abs(o.v) * self.m + U32 * self.m * o.m + np.abs(v))
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = self._o(o); v = self.v / o.v
        return V(v, (self.m + np.abs(v) * o.m + U32 * self.m * o.m / np.abs(o.v)) / np.abs(o.v) + np.abs(v))

    def __rtruediv__(self, o):
        return self._o(o) / self

    def __getitem__(self, i):
        return V(self.v[i], self.m[i])

    def fn(self, f, df):
        v = f(self.v)
        return V(v, np.abs(df(self.v)) * self.m + np.abs(v))

    def pow(self, e):
        """v ** e for an exact exponent (v > 0)."""
        if e == 1.0:
            return self
        return self.fn(lambda a: a ** np.asarray(e, a.dtype), lambda a: e * a ** np.asarray(e - 1.0, a.dtype))

    def sum(self, axis=None, keepdims=False):
        return V(self.v.sum(axis=axis, keepdims=keepdims), (self.m + np.abs(self.v)).sum(axis=axis, keepdims=keepdims))

    @staticmethod
    def where(c, a, b, dtype):
        a, b = V.lift(a, dtype), V.lift(b, dtype)
        return V(np.where(c, a.v, b.v), np.where(c, a.m, b.m))

    @staticmethod
    def stack(vs, axis=-1):
        return V(np.stack([x.v for x in vs], axis), np.stack([x.m for x in vs], axis))


def _sigmoid(x):
    return 1.0 / (1.0 + (-x).fn(np.exp, np.exp))


def _dot(a, b):
    s = a[0] * b[0]
    for x, y in zip(a[1:], b[1:]):
        s = s + x * y
    return s


# R_rc = delta_rc + sign_rc * two_s * u_rc(q), u_rc = sum coef * q_a * q_b  (q = (i, j, k, w) = xyzw)
_U = [[[(1, 1, 1), (1, 2, 2)], [(1, 0, 1), (-1, 2, 3)], [(1, 0, 2), (1, 1, 3)]],
      [[(1, 0, 1), (1, 2, 3)], [(1, 0, 0), (1, 2, 2)], [(1, 1, 2), (-1, 0, 3)]],
      [[(1, 0, 2), (-1, 1, 3)], [(1, 1, 2), (1, 0, 3)], [(1, 0, 0), (1, 1, 1)]]]


def _u(q, r, c):
    s = None
    for coef, a, b in _U[r][c]:
        t = q[a] * q[b]
        s = (t if coef > 0 else -t) if s is None else (s + t if coef > 0 else s - t)
    return s


def _scale_act(v, act, smin, smax, dtype, mutate=None):
    """-> (s, ds/dv) of one pre-activation scale channel."""
    if act == "bounded":
        sg = _sigmoid(v)
        return smin + (smax - smin) * sg, (smax - smin) * sg * (1.0 - sg)
    if act == "exp":
        e = v.fn(np.exp, np.exp)
        keep = e.v < SCALE_CLAMP
        return V.where(keep, e, SCALE_CLAMP, dtype), (e if mutate == "clamp_grad" else V.where(keep, e, 0.0, dtype))
    assert act == "softplus"
    lin = v.v > SOFTPLUS_THRESHOLD
    sp = 0.001 * V.where(lin, v, v.fn(np.exp, np.exp).fn(np.log1p, lambda a: 1.0 / (1.0 + a)), dtype)
    keep = sp.v < SCALE_CLAMP
    d = 0.001 * V.where(lin, 1.0, _sigmoid(v), dtype)
    return V.where(keep, sp, SCALE_CLAMP, dtype), (d if mutate == "clamp_grad" else V.where(keep, d, 0.0, dtype))


def _adapter_core(pts, gs, sh_mask, scale_act, scale_min, scale_max, opacity_exponent, dtype, mutate):
    pts, gs = np.asarray(pts, np.float64), np.asarray(gs, np.float64)
    assert bool(_f32_exact(pts).all() and _f32_exact(gs).all()), "inputs must be exact in f32"
    d_sh = (gs.shape[1] - 8) // 3
    assert gs.shape[1] == 8 + 3 * d_sh and len(sh_mask) == d_sh
    T = type("T", (), {})()
    T.dtype, T.d_sh, T.e = dtype, d_sh, float(opacity_exponent)
    T.x = [V(pts[:, c].astype(dtype)) for c in range(3)]
    T.g = [V(gs[:, c].astype(dtype)) for c in range(gs.shape[1])]
    # centre: xyz / max(|xyz|, 1e-8) * expm1(|xyz|)
    T.d = _dot(T.x, T.x).fn(np.sqrt, lambda a: 0.5 / np.sqrt(np.maximum(a, np.finfo(dtype).tiny)))
    T.far = T.d.v > DIST_CLAMP
    T.em = T.d.fn(np.expm1, np.exp)
    T.k = T.em / V.where(T.far, T.d, DIST_CLAMP, dtype)
    if mutate == "k_f16":
        T.k = V(T.k.v.astype(np.float16).astype(dtype), T.k.m)
    T.means = [x * T.k for x in T.x]
    # opacity
    T.p = _sigmoid(T.g[0])
    T.op = T.p
    if T.e > 0:
        T.op = 0.5 * (1.0 - (1.0 - T.p).pow(T.e) + T.p.pow(1.0 / T.e))
    # scales
    sd = [_scale_act(T.g[1 + c], scale_act, scale_min, scale_max, dtype, mutate) for c in range(3)]
    T.s, T.dsdv = [a for a, _ in sd], [b for _, b in sd]
    # rotation (xyzw) and covariance
    qr = T.g[4:8]
    n = _dot(qr, qr).fn(np.sqrt, lambda a: 0.5 / np.sqrt(np.maximum(a, np.finfo(dtype).tiny)))
    T.unclamped = n.v > QUAT_EPS
    T.qn = V.where(T.unclamped, n, QUAT_EPS, dtype)
    T.q = [c / T.qn for c in qr]
    T.t = 2.0 / (_dot(T.q, T.q) + TWO_S_EPS)
    T.u = [[_u(T.q, r, c) for c in range(3)] for r in range(3)]
    T.R = [[(1.0 - T.t * T.u[r][c]) if r == c else T.t * T.u[r][c] for c in range(3)] for r in range(3)]
    T.RS = [[T.R[r][c] * T.s[c] for c in range(3)] for r in range(3)]
    right = T.R if mutate == "rsr" else T.RS
    T.cov = [[_dot(T.RS[r], right[c]) for c in range(3)] for r in range(3)]
    # spherical harmonics
    mask = np.asarray(sh_mask, np.float64)
    midx = [(min(c, d_sh - 1) if mutate == "mask_c" else c % d_sh) for c in range(3 * d_sh)]
    T.mask = [V.lift(mask[i], dtype) for i in midx]
    T.harm = [T.g[8 + c] * T.mask[c] for c in range(3 * d_sh)]
    # inputs at a decision that rounding can flip
    amb = np.zeros(pts.shape[0], bool)
    d64, n64 = np.sqrt((pts[:, :3] ** 2).sum(1)), np.sqrt((gs[:, 4:8] ** 2).sum(1))
    amb |= (d64 > DIST_CLAMP / 2) & (d64 < DIST_CLAMP * 2)
    amb |= (n64 > QUAT_EPS / 2) & (n64 < QUAT_EPS * 2)
    with np.errstate(over="ignore"):
        for c in range(1, 4):
            v = gs[:, c]
            if scale_act == "softplus":
                amb |= np.abs(v - SOFTPLUS_THRESHOLD) < 1e-3
                amb |= np.abs(0.001 * np.where(v > 20, v, np.log1p(np.exp(np.minimum(v, 50)))) - SCALE_CLAMP) < 1e-3 * SCALE_CLAMP
            elif scale_act == "exp":
                amb |= np.abs(np.exp(v) - SCALE_CLAMP) < 1e-3 * SCALE_CLAMP
    T.ambiguous = amb
    return T


def _pack(out, name, vs, shape=None):
    a = V.stack(vs) if isinstance(vs, list) else vs
    out[name] = a.v if shape is None else a.v.reshape(shape)
    out[name + "_mag"] = (a.m if shape is None else a.m.reshape(shape)).astype(np.float64)


def adapter_forward(pts, gs, sh_mask, scale_act="softplus", scale_min=0.0, scale_max=0.0, opacity_exponent=1.0, *, dtype=np.float64,
                    mutate=None, _keep=False):
    """pts [P, >=3], gs [P, 8 + 3 d_sh] (opacity | scale3 | quaternion xyzw | SH rgb-major) -> dict of means [P,3], covariances [P,3,3],
    harmonics [P,3,d_sh], opacities [P], scales [P,3], rotations [P,4], raw [P, 11 + 3 d_sh], each with `_mag`, and `ambiguous` [P]."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        T = _adapter_core(pts, gs, sh_mask, scale_act, scale_min, scale_max, opacity_exponent, dtype, mutate)
        P, d_sh = len(T.ambiguous), T.d_sh
        out = dict(ambiguous=T.ambiguous)
        _pack(out, "means", T.means)
        _pack(out, "covariances", [T.cov[r][c] for r in range(3) for c in range(3)], (P, 3, 3))
        _pack(out, "harmonics", T.harm, (P, 3, d_sh))
        _pack(out, "opacities", T.op)
        _pack(out, "scales", T.s)
        _pack(out, "rotations", T.q)
        _pack(out, "raw", T.means + T.g)
    if _keep:
        out["_T"] = T
    return out


def adapter_backward(pts, gs, sh_mask, d_means, d_cov, d_harm, d_op, d_raw=None, d_scales=None, d_rot=None, scale_act="softplus",
                     scale_min=0.0, scale_max=0.0, opacity_exponent=1.0, *, dtype=np.float64, mutate=None):
    """Chain rule of adapter_forward for the cotangents d_means [P,3], d_cov [P,3,3], d_harm [P,3,d_sh], d_op [P] and optionally d_raw
    [P, 11 + 3 d_sh], d_scales [P,3], d_rot [P,4] (exact in f32) -> d_pts [P,3], d_gs [P, 8 + 3 d_sh] with `_mag`, and `ambiguous`."""
    T = adapter_forward(pts, gs, sh_mask, scale_act, scale_min, scale_max, opacity_exponent, dtype=dtype, mutate=mutate, _keep=True)["_T"]
    P, d_sh = len(T.ambiguous), T.d_sh
    cot = lambda a, shape: V(np.zeros(shape, dtype)) if a is None else V(np.asarray(a, np.float64).reshape(shape).astype(dtype))
    gm, G, gh, gp = cot(d_means, (P, 3)), cot(d_cov, (P, 3, 3)), cot(d_harm, (P, 3 * d_sh)), cot(d_op, (P,))
    graw, gsc, grot = cot(d_raw, (P, 11 + 3 * d_sh)), cot(d_scales, (P, 3)), cot(d_rot, (P, 4))
    raw = (lambda c: graw[:, c]) if d_raw is not None else None
    plus = lambda a, b: a if b is None else a + b
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        # ---- means: m = x k(d);  d > 1e-8: k = expm1(d) / d;  below: k = expm1(d) / 1e-8 (the clamp has no derivative, expm1 has)
        g = [plus(gm[:, c], raw(c) if raw else None) for c in range(3)]
        gx = _dot(g, T.x)
        d, em = T.d, T.em
        kp = ((em + 1.0) * d - em) / (d * d)
        if mutate == "kp0":
            kp = V(np.zeros_like(kp.v))
        dsafe = V.where(T.d.v > 0, d, 1.0, dtype)
        radial = V.where(T.far, gx * kp / dsafe, V.where(T.d.v > 0, gx * d.fn(np.exp, np.exp) / (dsafe * DIST_CLAMP), 0.0, dtype), dtype)
        d_pts = [g[c] * T.k + radial * T.x[c] for c in range(3)]
        # ---- opacity
        p, e = T.p, T.e
        dp = gp * p * (1.0 - p)
        if e > 0 and e != 1.0:
            dp = gp * (0.5 * (e * (1.0 - p).pow(e - 1.0) + (1.0 / e) * p.pow(1.0 / e - 1.0))) * p * (1.0 - p)
        d_gs = [None] * (8 + 3 * d_sh)
        d_gs[0] = plus(dp, raw(3) if raw else None)
        # ---- covariance = (R S)(R S)^T -> scales and R
        dRS = [[_dot([G[:, r, m] + G[:, m, r] for m in range(3)], [T.RS[m][c] for m in range(3)]) for c in range(3)] for r in range(3)]
        for c in range(3):
            ds = _dot([dRS[r][c] for r in range(3)], [T.R[r][c] for r in range(3)])
            if d_scales is not None:
                ds = ds + gsc[:, c]
            d_gs[1 + c] = plus(ds * T.dsdv[c], raw(4 + c) if raw else None)
        dR = [[dRS[r][c] * T.s[c] for c in range(3)] for r in range(3)]
        # ---- R(q): explicit q at fixed two_s, then two_s = 2 / (q.q + 1e-8)
        q, t = T.q, T.t
        sgn = lambda r, c: -1.0 if r == c else 1.0
        dq = []
        for a in range(4):
            acc = None
            for r in range(3):
                for c in range(3):
                    for coef, i, j in _U[r][c]:
                        for (ii, jj) in ((i, j), (j, i)):
                            if ii == a:
                                term = dR[r][c] * q[jj]
                                pos = coef * sgn(r, c) > 0
                                acc = (term if pos else -term) if acc is None else (acc + term if pos else acc - term)
            dq.append(t * acc)
        if mutate != "no_two_s":
            dt = None
            for r in range(3):
                for c in range(3):
                    term = dR[r][c] * T.u[r][c]
                    dt = (-term if r == c else term) if dt is None else (dt - term if r == c else dt + term)
            dtq = -(t * t) * dt
            dq = [dq[a] + dtq * q[a] for a in range(4)]
        if d_rot is not None:
            dq = [dq[a] + grot[:, a] for a in range(4)]
        # ---- q = qr / max(|qr|, 1e-12): the projection only where the norm is not clamped
        qdq = _dot(q, dq)
        for a in range(4):
            proj = dq[a] / T.qn if mutate == "no_proj" else (dq[a] - q[a] * qdq) / T.qn
            d_gs[4 + a] = plus(V.where(T.unclamped, proj, dq[a] / T.qn, dtype), raw(7 + a) if raw else None)
        # ---- harmonics
        for c in range(3 * d_sh):
            d_gs[8 + c] = plus(gh[:, c] * T.mask[c], raw(11 + c) if raw else None)
        out = dict(ambiguous=T.ambiguous)
        _pack(out, "d_pts", d_pts)
        _pack(out, "d_gs", d_gs)
    return out


# --------------------------------------------------------------------------------------------------------------------------------------
# LayerNorm + AdaLN modulation
# --------------------------------------------------------------------------------------------------------------------------------------
def out_rows(M, grp_in=0, grp_out=0, grp_off=0):
    m = np.arange(M)
    return m if grp_in <= 0 else (m // grp_in) * grp_out + grp_off + m % grp_in


def _ln_core(x, w, b, eps, scale, shift, mod_rows, dtype, mutate):
    x = np.asarray(x, np.float64)
    M, C = x.shape
    xv, wv, bv = V(x.astype(dtype)), V(np.asarray(w, np.float64).astype(dtype)), V(np.asarray(b, np.float64).astype(dtype))
    mean = xv.sum(1, keepdims=True) / float(C)
    xc = xv - mean
    if mutate == "var_ex2":
        var = (xv * xv).sum(1, keepdims=True) / float(C) - mean * mean
        var = V(np.maximum(var.v, 0), var.m)
    else:
        var = (xc * xc).sum(1, keepdims=True) / float(C)
    r = (var + V.lift(eps, dtype)).fn(lambda a: 1.0 / np.sqrt(a), lambda a: 0.5 / (a * np.sqrt(a)))
    xh = xc * r
    grp = np.arange(M) // (mod_rows if mod_rows > 0 else M)
    one_s = None if scale is None else 1.0 + V(np.asarray(scale, np.float64).astype(dtype))[grp]
    return xv, wv, bv, r, xh, grp, one_s


def layernorm_forward(x, w, b, eps=1e-6, scale=None, shift=None, mod_rows=0, *, dtype=np.float64, mutate=None):
    """y [M, C] = LN(x; w, b, eps) * (1 + scale[m // mod_rows]) + shift[m // mod_rows] in input-row order (out_rows() gives the row of
    the kernel's output buffer that holds row m).  -> dict(y, y_mag)."""
    with np.errstate(invalid="ignore"):
        xv, wv, bv, r, xh, grp, one_s = _ln_core(x, w, b, eps, scale, shift, mod_rows, dtype, mutate)
        y = xh * wv + bv
        if one_s is not None:
            y = y * one_s
        if shift is not None:
            y = y + V(np.asarray(shift, np.float64).astype(dtype))[grp]
    return dict(y=y.v, y_mag=y.m.astype(np.float64))


def layernorm_backward(dout, x, w, b, eps=1e-6, scale=None, mod_rows=0, dx_add=None, *, dtype=np.float64, mutate=None):
    """dout [M, C] in input-row order -> dx (+ dx_add), dw, db and, with a modulation, dscale / dshift [G, C]; each with `_mag`."""
    with np.errstate(invalid="ignore"):
        xv, wv, bv, r, xh, grp, one_s = _ln_core(x, w, b, eps, scale, None, mod_rows, dtype, mutate)
        M, C = xv.v.shape
        do = V(np.asarray(dout, np.float64).astype(dtype))
        dy = do if one_s is None else do * one_s
        g = dy * wv
        dx = g - g.sum(1, keepdims=True) / float(C)
        if mutate != "no_xhat_term":
            dx = dx - xh * ((g * xh).sum(1, keepdims=True) / float(C))
        dx = r * dx
        if dx_add is not None:
            dx = dx + V(np.asarray(dx_add, np.float64).astype(dtype))
        out = {}
        _pack(out, "dx", dx)
        _pack(out, "dw", (dy * xh).sum(0))
        _pack(out, "db", dy.sum(0))
        if scale is not None:
            G = np.asarray(scale).shape[0]
            gsum = grp if mutate != "dscale_wave8" else (np.arange(M) // 8 * 8) // mod_rows     # the group of the first of 8 rows
            pre = do * (xh * wv + bv)
            zero = V(np.zeros((C,), dtype))
            _pack(out, "dscale", V.stack([pre[gsum == k].sum(0) if (gsum == k).any() else zero for k in range(G)], 0))
            _pack(out, "dshift", V.stack([do[grp == k].sum(0) if (grp == k).any() else zero for k in range(G)], 0))
    return out


# --------------------------------------------------------------------------------------------------------------------------------------
# criterion
# --------------------------------------------------------------------------------------------------------------------------------------
HALF_ULP = {"f32": 0.0, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}
# below the normal range a result is a subnormal of its type: one step of an f32 intermediate (2^-149: the gradient through a scale of
# 1e-16 is ~1e-44), plus half a step of a 16-bit output (f16 2^-25, bf16 2^-134)
SUBNORMAL = {"f32": 2.0 ** -149, "f16": 2.0 ** -25 + 2.0 ** -149, "bf16": 2.0 ** -134 + 2.0 ** -149}


def bound(ref, name, B, out_storage="f32", extra_rel=0.0):
    """Per-element allowance: B 2^-24 mag, plus, for a 16-bit output, half an ulp of it, plus the subnormal step of the type.  An element
    of magnitude 0 has allowance 0."""
    m = ref[name + "_mag"]
    a = B * U32 * m + (HALF_ULP[out_storage] + extra_rel) * np.abs(ref[name])
    return np.where(m > 0, a + SUBNORMAL[out_storage], 0.0)


def ratio(got, ref, name, B, out_storage="f32", extra_rel=0.0, extra_abs=0.0):
    """max over the elements of |got - ref| / allowance (<= 1 passes); an element with allowance 0 must be exact (else inf); any
    non-finite value of `got` is inf."""
    got = np.asarray(got, np.float64).reshape(ref[name].shape)
    r64 = ref[name].astype(np.float64)
    lim = bound(ref, name, B, out_storage, extra_rel) + extra_abs
    if out_storage == "f16":      # a value that rounds to infinity in f16 (>= 65520) is right as that infinity
        got = np.where(np.isinf(got) & (np.sign(got) == np.sign(r64)) & (np.abs(r64) + lim >= 65520.0), r64, got)
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - r64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / lim)
    return float(q.max()) if q.size else 0.0


def units(got, ref, name):
    """max |got - ref| / (2^-24 mag): the measured ratio in the units of r32 (elements of magnitude 0 are skipped: they must be exact;
    one f32 subnormal step is taken off the error, so that results of ~1e-44 do not count as thousands of units)."""
    got = np.asarray(got, np.float64).reshape(ref[name].shape)
    m = ref[name + "_mag"]
    ok = (m > 0) & np.isfinite(got)
    err = np.maximum(np.abs(got - ref[name].astype(np.float64)) - SUBNORMAL["f32"], 0.0)
    return float((err[ok] / (U32 * m[ok])).max()) if ok.any() else 0.0


# --------------------------------------------------------------------------------------------------------------------------------------
# edge inputs
# --------------------------------------------------------------------------------------------------------------------------------------
def round_to(a, storage):
    """float64 array -> the nearest value of the storage type, as float64 (exact in f32)."""
    import torch
    dt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[storage]
    return torch.from_numpy(np.asarray(a, np.float64)).to(dt).double().numpy()


_DIRS = np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1], [0.6, -0.64, 0.48], [-0.36, 0.48, 0.8], [0.48, 0.6, -0.64]], np.float64)
_QGEN = np.array([[0.5, -0.1, 0.7, 0.5], [-0.3, 0.8, 0.1, -0.5], [0.2, 0.2, -0.9, 0.3]], np.float64)
_QGEN /= np.sqrt((_QGEN ** 2).sum(1, keepdims=True))
SCALE_TABLE = dict(softplus=[-30.0, -10.0, 0.0, 5.0, 19.5, 20.5, 25.0, 290.0, 310.0], exp=[-20.0, -3.0, -1.3, -1.1, 2.0],
                   bounded=[0.0, 5.0, -5.0, 20.0, -20.0])


def adapter_edge_inputs(scale_act, d_sh, storage, opacity_exponent, P=None, pts_ch=3, seed=0):
    """The edge table, crossed per channel group by cycling every group with its own period: pts [P, pts_ch], gs [P, 8 + 3 d_sh] as
    float64 holding values of `storage`.  P defaults to one full crossing of (scale x quaternion) and (radius x direction)."""
    radii = [0.0, 1e-4, 1e-2, 1.0, 5.0, 11.0] + ([1e-9, 1e-7] if storage == "f32" else [])
    ops_ = [0.0, 1.0, -1.0, 8.0, -8.0, 15.0, -15.0] + ([20.0, -20.0] if opacity_exponent == 1.0 or opacity_exponent <= 0 else [])
    quats = [[0, 0, 0, 1], [1, 0, 0, 0], [0, 0, 0, -1], [-1, 0, 0, 0], [0, 0, 0, 0]] + list(_QGEN) + [_QGEN[0] * 1e-6, _QGEN[1] * 1e4]
    if storage == "f32":      # norms below F.normalize's 1e-12: far below, and close enough that q = qr / 1e-12 is not small
        quats += [_QGEN[2] * 1e-20, _QGEN[0] * 4e-13]
    st = SCALE_TABLE[scale_act]
    if P is None:
        P = max(len(st) * len(quats), len(radii) * len(_DIRS)) * 3
    rng = np.random.default_rng(seed)
    i = np.arange(P)
    pts = np.zeros((P, pts_ch))
    pts[:, :3] = np.asarray(radii)[i % len(radii)][:, None] * _DIRS[(i // len(radii)) % len(_DIRS)]
    if pts_ch > 3:
        pts[:, 3:] = rng.standard_normal((P, pts_ch - 3))     # channels the kernels must ignore
    gs = np.zeros((P, 8 + 3 * d_sh))
    gs[:, 0] = np.asarray(ops_)[i % len(ops_)]
    for c in range(3):      # the three scale channels walk the table at different phases; quaternions change once per table pass
        gs[:, 1 + c] = np.asarray(st)[(i + c * (1 + i // (len(st) * len(quats)))) % len(st)]
    gs[:, 4:8] = np.asarray(quats, np.float64)[(i // len(st)) % len(quats)]
    gs[:, 8:] = rng.standard_normal((P, 3 * d_sh)) * 2.0
    return round_to(pts, storage), round_to(gs, storage)


def adapter_cotangents(gs, d_sh, scale_act, seed=1, with_raw=True, with_scales_rot=False):
    """Random cotangents of order 1 (f32 values).  The covariance cotangent is weighted so that its share of d_gs is comparable with the
    others: by 30 (scales <= 0.3) or 0.05 (bounded scales up to 15), and by the quaternion's norm (the gradient carries 1 / norm)."""
    P = gs.shape[0]
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32).astype(np.float64)
    n = np.minimum(1.0, np.maximum(np.sqrt((gs[:, 4:8] ** 2).sum(1)), QUAT_EPS))
    c = dict(d_means=f(P, 3), d_cov=(f(P, 3, 3) * ((0.05 if scale_act == "bounded" else 30.0) * n)[:, None, None]).astype(np.float32).astype(np.float64),
             d_harm=f(P, 3, d_sh), d_op=f(P), d_raw=f(P, 11 + 3 * d_sh) if with_raw else None)
    if with_scales_rot:
        c.update(d_scales=f(P, 3), d_rot=(f(P, 4) * n[:, None]).astype(np.float32).astype(np.float64))
    return c


LN_ROW_KINDS = ("mean300", "constant", "spread1e-5", "outlier1e4", "ordinary")


def layernorm_edge_inputs(M, C, G, seed=0):
    """x [M, C] cycling through LN_ROW_KINDS (row m has kind m % 5), w, b, scale / shift [G, C], dout [M, C], dx_add [M, C]; f32 values."""
    rng = np.random.default_rng(seed + 1000 * M + C)
    x = rng.standard_normal((M, C))
    for m in range(M):
        kind = LN_ROW_KINDS[m % len(LN_ROW_KINDS)]
        if kind == "mean300":
            x[m] += 300.0
        elif kind == "constant":
            x[m] = 1.7 * (1 + m)
        elif kind == "spread1e-5":
            x[m] = 0.5 + 1e-5 * x[m]
        elif kind == "outlier1e4":
            x[m, (7 * m + 1) % C] = 1e4
    f = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)
    return dict(x=f(x), w=f(1 + 0.2 * rng.standard_normal(C)), b=f(0.1 * rng.standard_normal(C)), scale=f(0.3 * rng.standard_normal((G, C))),
                shift=f(0.3 * rng.standard_normal((G, C))), dout=f(rng.standard_normal((M, C))), dx_add=f(rng.standard_normal((M, C))))
