"""Float64 reference (numpy) of the depth-smoothness loss, LossDepth of src/loss/loss_depth.py:34-60: the loss, a hand-written backward with
respect to depth, and per-output magnitudes in the manner of tests/pointwise_f64.py (its class V carries them: 2^-24 mag is the
first-order bound of the same formula in f32 with every operation rounded once -- the logs, the division by log far - log near, the
argument of exp and exp itself, every difference, the sums).  Independent of vicasplat_amd/callers.py.  The yardstick of
tests/test_depth_loss_gpu.py, pinned to the real reference (tests/golden/depth_loss.npz) and to float64 autograd of the torch backend by
tests/test_depth_loss_cpu.py.

Decisions.  The formula decides at four places: the clamp (depth against log far and log near), the sign of every weighted difference
(|.|), the channel maximum and the neighbour maximum of the colour differences.  `decisions_ok` states that every one of them is
unambiguous -- taken by a margin of >= 1e-4, or an exact tie that f32 and float64 see alike -- and `make_inputs` guarantees it by
resampling the depths that take part in an ambiguous one (colours are multiples of 1/256: their differences are exact and so are their
ties).  No element is then exempted from any comparison.

Ties at the clamp.  log far is not an f32 number, so "depth equals log far" can only mean the f32 value nearest to it: a depth that is
bit-equal to f32(log far) or f32(log near) (or, in a float64 evaluation, to the float64 logarithm itself) is a tie, and torch's
subgradient there is one half.  make_inputs plants none (the real reference evaluated in float64 does not see an f32 tie); `with_ties`
does.

`mutate=` plants one deliberate defect (MUTANTS); dtype=np.float32 runs the same formulas in f32.
"""
import numpy as np

from pointwise_f64 import U32, V

SIGMA = 4.0        # config/loss/depth.yaml has sigma_image: null; the bilateral configurations need a value
WEIGHT = 0.25      # config/loss/depth.yaml
CONFIGS = [(None, False), (None, True), (SIGMA, False), (SIGMA, True)]       # (sigma_image, use_second_derivative)
MUTANTS = ("tie_full", "abs_colour", "left_neighbour", "count_w", "dy_cx", "no_log", "sigma_sign")
# r32: max |torch f32 restatement (callers.depth_smoothness_loss(backend="torch")) - f64| / (2^-24 mag) per output over the cases of
# tests/test_depth_loss_cpu.py::test_torch_backend_matches_and_r32 and on the golden (printed there with -s: loss 0.065, d_depth 0.336),
# rounded up to two places.
# The GPU bound of an output is 4 max(r32, 1) 2^-24 mag = 4 units for both, with no other floor and no exempted element.
R32 = dict(loss=0.07, d_depth=0.34)
# What the torch restatement itself is held to on the CPU (its summation order, and with it its last bits, may change with the thread count
# and the torch build): one unit; R32 records what was measured.
F32_LIMIT = 1.0


def gpu_factor(key):
    """B of the GPU criterion |gpu - ref| <= B 2^-24 mag for output `key` ("loss", "d_depth")."""
    return 4.0 * max(R32[key], 1.0)


def tag(sigma, second):
    return f"s{int(sigma is not None)}d{2 if second else 1}"


def f32_logs(near, far):
    """(f32(log near), f32(log far)): the correctly rounded f32 logarithms, as float64 arrays."""
    return (np.log(np.asarray(near, np.float64)).astype(np.float32).astype(np.float64),
            np.log(np.asarray(far, np.float64)).astype(np.float32).astype(np.float64))


def _bc(x, shape):
    return V(np.broadcast_to(x.v, shape).copy(), np.broadcast_to(x.m, shape).copy())


def _vmax(a, b, dtype):
    return V.where(a.v >= b.v, a, b, dtype)


def _diff(x, axis):
    n = x.v.shape[axis]
    hi = [slice(None)] * x.v.ndim
    lo = list(hi)
    hi[axis], lo[axis] = slice(1, n), slice(0, n - 1)
    return x[tuple(hi)] - x[tuple(lo)]


def _diff_back(g, axis):
    """Backward of _diff: out[j] = g[j - 1] - g[j] with the missing operand at either end absent (that element is a copy: no rounding)."""
    pad_l, pad_r = [(0, 0)] * g.v.ndim, [(0, 0)] * g.v.ndim
    pad_l[axis], pad_r[axis] = (1, 0), (0, 1)
    lv, lm = np.pad(g.v, pad_l), np.pad(g.m, pad_l)
    rv, rm = np.pad(g.v, pad_r), np.pad(g.m, pad_r)
    both = np.pad(np.ones(g.v.shape, bool), pad_l) & np.pad(np.ones(g.v.shape, bool), pad_r)
    v = lv - rv
    return V(v, lm + rm + np.where(both, np.abs(v), 0.0).astype(v.dtype))


def depth_smooth(depth, near, far, image=None, sigma=None, second=False, weight=WEIGHT, up=1.0, dtype=np.float64, mutate=None):
    """depth [N, H, W], near / far [N], image [N, 3, H, W] (read when sigma is not None) -> dict: loss, d_depth [N, H, W] (of up * loss),
    each with k + "_mag"; tx, ty: the weighted differences (V) for decisions_ok."""
    assert mutate is None or mutate in MUTANTS, mutate
    dt = dtype
    depth64 = np.asarray(depth, np.float64)
    N, H, W = depth64.shape
    s = 1 if second else 0
    assert H >= 2 + s and W >= 2 + s, "an empty mean"
    col = lambda a: V(np.asarray(a, np.float64).astype(dt).reshape(N, 1, 1))
    if mutate == "no_log":
        ln, lf = col(near), col(far)
    else:
        ln, lf = col(near).fn(np.log, lambda a: 1.0 / a), col(far).fn(np.log, lambda a: 1.0 / a)
    ln32, lf32 = f32_logs(near, far)
    x = V(depth64.astype(dt))
    lnb, lfb = _bc(ln, x.v.shape), _bc(lf, x.v.shape)
    tie_hi = (depth64 == lf32.reshape(N, 1, 1)) | (x.v == lfb.v)
    tie_lo = (depth64 == ln32.reshape(N, 1, 1)) | (x.v == lnb.v)
    above = (x.v > lfb.v) | tie_hi
    m = V.where(above, lfb, x, dt)
    below = (m.v < lnb.v) | (tie_lo & ~above)
    c = V.where(below, lnb, m, dt)
    den = lf - ln
    d = (c - ln) / den
    dx, dy = _diff(d, 2), _diff(d, 1)
    if second:
        dx, dy = _diff(dx, 2), _diff(dy, 1)
    wx = wy = None
    if sigma is not None:
        im = V(np.asarray(image, np.float64).astype(dt))
        cs = []
        for axis in (3, 2):
            cd = _diff(im, axis)
            if mutate == "abs_colour":
                cd = cd.fn(np.abs, np.sign)
            cm = _vmax(_vmax(cd[:, 0], cd[:, 1], dt), cd[:, 2], dt)
            if second:
                n = cm.v.shape[axis - 1]
                hi, lo = [slice(None)] * 3, [slice(None)] * 3
                hi[axis - 1], lo[axis - 1] = slice(1, n), slice(0, n - 1)
                cm = cm[tuple(lo)] if mutate == "left_neighbour" else _vmax(cm[tuple(hi)], cm[tuple(lo)], dt)
            cs.append(cm)
        sg = V.lift(sigma, dt)
        wx, wy = [((cm if mutate == "sigma_sign" else -cm) * sg).fn(np.exp, np.exp) for cm in cs]
        if mutate == "dy_cx":        # the x weights on the y differences: rows cut, columns repeated at the right edge
            idx = np.minimum(np.arange(W), W - 2 - s)
            wy = V(wx.v[:, :H - 1 - s][:, :, idx].copy(), wx.m[:, :H - 1 - s][:, :, idx].copy())
    tx, ty = (dx, dy) if wx is None else (dx * wx, dy * wy)
    cnt_x = dt(N * H * W) if mutate == "count_w" else dt(N * H * (W - 1 - s))
    cnt_y = dt(N * H * W) if mutate == "count_w" else dt(N * (H - 1 - s) * W)
    flat = lambda t: V(t.v.reshape(-1), t.m.reshape(-1))
    mean_x, mean_y = flat(tx.fn(np.abs, np.sign)).sum() / cnt_x, flat(ty.fn(np.abs, np.sign)).sum() / cnt_y
    wgt = V.lift(weight, dt)
    loss = wgt * (mean_x + mean_y)
    # ---- backward, in torch's order: up * weight, / count, * sgn, * w, diff backward (twice), the sum of both directions, / (lf - ln), clamp
    k = V.lift(up, dt) * wgt
    gs = []
    for t, w, cnt, axis in ((tx, wx, cnt_x, 2), (ty, wy, cnt_y, 1)):
        kc = k / cnt
        g = V(np.sign(t.v) * kc.v, np.abs(np.sign(t.v)) * kc.m)
        if w is not None:
            g = g * w
        g = _diff_back(g, axis)
        if second:
            g = _diff_back(g, axis)
        gs.append(g)
    g = (gs[0] + gs[1]) / den
    half = dt(1.0 if mutate == "tie_full" else 0.5)
    f_min = np.where(tie_hi, half, np.where(above, 0.0, 1.0))
    f_max = np.where(tie_lo & ~above, half, np.where(below, 0.0, 1.0))
    f = (f_min * f_max).astype(dt)
    d_depth = V(g.v * f, g.m * f)
    return dict(loss=np.asarray(loss.v, np.float64), loss_mag=np.asarray(loss.m, np.float64), d_depth=d_depth.v.astype(np.float64),
                d_depth_mag=d_depth.m.astype(np.float64), tx=tx, ty=ty)


def _ambiguous(z, rel=1e-4):
    """bool [N, H, W]: the depths that take part in a decision which rounding could turn (see decisions_ok)."""
    depth = z["depth"].astype(np.float64)
    N, H, W = depth.shape
    bad = np.zeros(depth.shape, bool)
    for b in f32_logs(z["near"], z["far"]):
        b = b.reshape(N, 1, 1)
        bad |= (depth != b) & (np.abs(depth - b) < rel * np.abs(b))
    for sigma, second in CONFIGS:
        if H < 2 + second or W < 2 + second:
            continue
        r = depth_smooth(z["depth"], z["near"], z["far"], z["image"], sigma, second)
        for t, axis in ((r["tx"], 2), (r["ty"], 1)):
            amb = (t.v != 0) & (np.abs(t.v) < rel * t.m)
            for o in range(2 + second):         # every pixel of the term's stencil
                pad = [(0, 0)] * 3
                pad[axis] = (o, 1 + second - o)
                bad |= np.pad(amb, pad)
    return bad


def colours_ok(image, gap=1e-4):
    """Every channel maximum and every neighbour maximum of the colour differences wins by >= gap or by an exact tie."""
    im = np.asarray(image, np.float64)
    for axis in (3, 2):
        cd = np.diff(im, axis=axis)
        top = np.sort(cd, axis=1)
        g = top[:, 2] - top[:, 1]
        if ((g != 0) & (g < gap)).any():
            return False
        cm = cd.max(axis=1)
        g = np.abs(np.diff(cm, axis=axis - 1))
        if ((g != 0) & (g < gap)).any():
            return False
    return True


def decisions_ok(z, rel=1e-4):
    """True when no decision of the formula depends on rounding, for all of CONFIGS: every depth is bit-equal to f32(log far) / f32(log near)
    or >= rel relative away from them; every weighted difference is exactly 0 or >= rel of its magnitude; every colour maximum wins by
    >= 1e-4 or ties exactly."""
    return not _ambiguous(z, rel).any() and colours_ok(z["image"])


def make_inputs(N, H, W, seed, exact_logs=False):
    """Deterministic f32 inputs with decisions_ok: dict depth [N, H, W], near, far [N], image [N, 3, H, W].  Depths are uniform in [0.5, 6]
    against near in [1.5, 3] and far in [60, 100]: about a quarter lie beyond log far and a few per cent below log near.
    exact_logs: logarithms that every precision represents exactly, so that a tie at the clamp is a tie in f32 and in float64 alike --
    even views have near = 1 (log near = 0: depths in [-1.5, 4]), odd views far = 1 and near = 0.25 (log far = 0: depths in [-2.5, 3])."""
    rng = np.random.default_rng(seed)
    near, far, shift = rng.uniform(1.5, 3.0, N), rng.uniform(60.0, 100.0, N), np.zeros(N)
    if exact_logs:
        near[0::2], shift[0::2] = 1.0, -2.0
        near[1::2], far[1::2], shift[1::2] = 0.25, 1.0, -3.0
    shift = np.broadcast_to(shift.reshape(N, 1, 1), (N, H, W))
    z = dict(near=near.astype(np.float32), far=far.astype(np.float32), depth=(rng.uniform(0.5, 6.0, (N, H, W)) + shift).astype(np.float32),
             image=(rng.integers(0, 256, (N, 3, H, W)) / 256.0).astype(np.float32))
    for _ in range(100):
        bad = _ambiguous(z)
        if not bad.any():
            assert decisions_ok(z)
            return z
        z["depth"][bad] = (rng.uniform(0.5, 6.0, int(bad.sum())) + shift[bad]).astype(np.float32)
    raise RuntimeError("resampling did not remove every ambiguous decision")


def with_ties(z, hi, lo):
    """A copy of the inputs in which the depths at the index tuples `hi` / `lo` (each (n, i, j)) are bit-equal to f32(log far[n]) /
    f32(log near[n])."""
    z = {k: v.copy() for k, v in z.items()}
    ln32, lf32 = f32_logs(z["near"], z["far"])
    for n, i, j in hi:
        z["depth"][n, i, j] = np.float32(lf32[n])
    for n, i, j in lo:
        z["depth"][n, i, j] = np.float32(ln32[n])
    return z


def inputs_digest(z):
    """SHA-256 over the bytes of the input arrays, in key order."""
    import hashlib
    h = hashlib.sha256()
    for k in sorted(z):
        h.update(k.encode() + np.ascontiguousarray(z[k]).tobytes())
    return h.hexdigest()


def units(got, ref, name):
    """max |got - ref| / (2^-24 mag) over the elements of output `name` (0 where the error is 0; an element of magnitude 0 must be exact,
    else inf; a non-finite value is inf)."""
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - ref[name])
    mag = np.asarray(ref[name + "_mag"], np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(err == 0, 0.0, err / (U32 * mag))
    return float(np.max(u))
