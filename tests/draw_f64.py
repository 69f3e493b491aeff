"""A numpy restatement of the drawing semantics of include/vicasplat_draw.h -- both coverage tests, the pass structure, the reduction and
the blend -- with ONE code path that runs in float64 or in float32, and the case builders and planted defects of tests/test_draw_cpu.py,
tests/test_draw_gpu.py, tests/golden/gen_draw_golden.py and tools/bench_draw.py.

The records are the f32 pixel-space records of the header (the world -> pixel step is f32 torch on the host in both backends, restated
here as world_to_pixel, always in f32); the float64 run is the exact semantics ON those records.

Every compared quantity is a Q: its value in the working dtype and a propagated magnitude `e`, a first-order running bound of its rounding
error in units of 2^-24 (an exact input has 0; a sum adds its operands' and its own size; a product |a| e_b + |b| e_a and its own size; a
quotient (e_a + |q| e_b) / |b| and its own size; a square root e_s / (2 r) and its own size).  A comparison within FACTOR 2^-24 (e_l + e_r)
of its threshold is `unknown`; coverage is then three-valued (surely / possibly inside).  A sample is ambiguous when an unknown record
lies above its surely-covering top record: its coverage or its topmost index can change.  FACTOR = 4 max(r32, 1), r32 = this restatement's
own f32 - f64 gap of each compared difference in units of 2^-24 (e_l + e_r), at its maximum over the case list
(tests/test_draw_cpu.py::test_r32_is_measured asserts R32 is not exceeded and prints the measured values).

render() returns per pixel: `out` in the working dtype; `amb`, the number of its 64 samples (0 or 64 for an unrefined pixel, which has one)
whose coverage or topmost index can change; `unsure`, true when a pass-0 sample of its 3 x 3 neighbourhood is ambiguous, so that its
refinement decision can flip; `mag`, the propagated magnitude of out (the 64-term colour sum counts six levels of a pairwise tree); and
`spread`, the range of the values the pixel can blend: its image value and the colours of the records that possibly cover one of its
samples.  The criterion for an f32 implementation against the float64 run, on every pixel that is not unsure:
    |out - f64| <= FACTOR 2^-24 mag + (amb / 64) spread.

DEFECTS are the planted defects; every one must change a golden scene (tests/test_draw_cpu.py).
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
# bounds of the measured gaps: max over the case list of |f32 - f64| / (2^-24 (e_l + e_r)) per comparison (test_r32_is_measured)
R32 = {"par_hi": 1.0, "par_lo": 1.0, "perp": 1.0, "cap": 1.0, "inner": 1.0, "outer": 1.0}
FACTOR = 4.0 * max(max(R32.values()), 1.0)
CAPS = ("butt", "round", "square")
DEFECTS = ("par_hi_strict", "par_lo_loose", "perp_loose", "cap_loose", "inner_strict", "outer_strict", "lowest_index", "caps_on_butt",
           "no_caps_zero_length", "border_neighbour", "no_half_offset", "alpha_sum", "colour_undivided", "swap_xy")
CHUNK = 4096      # samples per evaluation: bounds the records x samples temporaries


class Q:
    """A value in the working dtype and its propagated magnitude (float64): the rounding error is about 2^-24 e."""

    def __init__(self, v, e):
        self.v, self.e = v, np.asarray(e, np.float64)

    @staticmethod
    def exact(v, dtype):
        v = np.asarray(v).astype(dtype)
        return Q(v, np.zeros(v.shape))

    def _a(self):
        return np.abs(self.v.astype(np.float64))

    def __add__(self, o):
        r = self.v + o.v
        return Q(r, self.e + o.e + np.abs(r.astype(np.float64)))

    def __sub__(self, o):
        r = self.v - o.v
        return Q(r, self.e + o.e + np.abs(r.astype(np.float64)))

    def __neg__(self):
        return Q(-self.v, self.e)

    def __mul__(self, o):
        r = self.v * o.v
        return Q(r, self._a() * o.e + o._a() * self.e + np.abs(r.astype(np.float64)))

    def __truediv__(self, o):
        r = self.v / o.v
        q = np.abs(r.astype(np.float64))
        return Q(r, (self.e + q * o.e) / o._a() + q)

    def sqrt(self):
        r = np.sqrt(self.v)
        a = np.abs(r.astype(np.float64))
        # d sqrt(s) = ds / (2 sqrt(s)); at s = 0 the error of the root is the root of the error
        e = np.where(a > 0, self.e / (2 * np.where(a > 0, a, 1.0)), np.sqrt(self.e * U) / U)
        return Q(r, e + a)


class Tri:
    """A three-valued decision: t in the working dtype, lo = true whatever the unknown comparisons give, hi = possibly true."""

    def __init__(self, t, lo, hi):
        self.t, self.lo, self.hi = t, lo, hi

    def __and__(self, o):
        return Tri(self.t & o.t, self.lo & o.lo, self.hi & o.hi)

    def __or__(self, o):
        return Tri(self.t | o.t, self.lo | o.lo, self.hi | o.hi)


def compare(name: str, l: Q, op: str, r: Q, gaps=None) -> Tri:
    d = l.v.astype(np.float64) - r.v.astype(np.float64)
    e = l.e + r.e
    if gaps is not None:
        gaps.setdefault(name, []).append((d, e))
    t = {"<": l.v < r.v, "<=": l.v <= r.v, ">": l.v > r.v, ">=": l.v >= r.v}[op]
    unknown = np.abs(d) <= FACTOR * U * e      # false for a NaN: a comparison with a NaN is surely false
    return Tri(t, t & ~unknown, t | unknown)


def _norm(x: Q, y: Q) -> Q:
    return (x * x + y * y).sqrt()


def line_coverage(rec, px, py, cap, dtype, defects=(), gaps=None) -> Tri:
    """rec [n, 8] f32, px, py [S] -> Tri of [n, S]."""
    col = lambda k: Q.exact(rec[:, k:k + 1], dtype)
    sx, sy, ex, ey, w = (col(k) for k in range(5))
    X, Y = Q.exact(px[None], dtype), Q.exact(py[None], dtype)
    half = Q.exact(0.5 * rec[:, 4:5].astype(np.float64), dtype)      # w / 2 is exact
    zero = Q.exact(np.zeros((rec.shape[0], 1)), dtype)
    extra = half if cap == "square" else zero
    with np.errstate(all="ignore"):
        dx, dy = ex - sx, ey - sy
        n = _norm(dx, dy)
        ux, uy = dx / n, dy / n
        ix, iy = X - sx, Y - sy
        par = ux * ix + uy * iy
        qx, qy = ix - par * ux, iy - par * uy
        inside = (compare("par_hi", par, "<" if "par_hi_strict" in defects else "<=", n + extra if cap == "square" else n, gaps)
                  & compare("par_lo", par, ">=" if "par_lo_loose" in defects else ">", -extra, gaps)
                  & compare("perp", _norm(qx, qy), "<=" if "perp_loose" in defects else "<", half, gaps))
        if cap == "round" or "caps_on_butt" in defects and cap == "butt":
            op = "<=" if "cap_loose" in defects else "<"
            caps = compare("cap", _norm(ix, iy), op, half, gaps) | compare("cap", _norm(X - ex, Y - ey), op, half, gaps)
            if "no_caps_zero_length" in defects:
                keep = ~((rec[:, 0:1] == rec[:, 2:3]) & (rec[:, 1:2] == rec[:, 3:4]))
                caps = Tri(caps.t & keep, caps.lo & keep, caps.hi & keep)
            inside = inside | caps
    ok = ~np.isnan(rec[:, :5]).any(axis=1)[:, None]      # a NaN in the geometry covers nothing
    return Tri(inside.t & ok, inside.lo & ok, inside.hi & ok)


def point_coverage(rec, px, py, dtype, defects=(), gaps=None) -> Tri:
    """rec [n, 7] f32 -> Tri of [n, S]."""
    col = lambda k: Q.exact(rec[:, k:k + 1], dtype)
    cx, cy, rad, inner = (col(k) for k in range(4))
    with np.errstate(all="ignore"):
        d = _norm(Q.exact(px[None], dtype) - cx, Q.exact(py[None], dtype) - cy)
        return (compare("inner", d, ">" if "inner_strict" in defects else ">=", inner, gaps)
                & compare("outer", d, "<" if "outer_strict" in defects else "<=", rad, gaps))


def world_to_pixel(xy, shape, x_range=None, y_range=None, defects=()):
    """generate_conversions' world -> pixel map in f32: (xy - lo) / (hi - lo) * (w, h)."""
    h, w = shape
    xr = np.asarray((0, w) if x_range is None else x_range, np.float32)
    yr = np.asarray((0, h) if y_range is None else y_range, np.float32)
    lo, hi = np.stack((xr, yr), axis=-1)
    xy = np.asarray(xy, np.float32)
    if "swap_xy" in defects:
        xy = xy[..., ::-1]
    return ((xy - lo) / (hi - lo) * np.asarray((w, h), np.float32)).astype(np.float32)


def sample(kind, rec, cap, px, py, dtype, defects=(), gaps=None):
    """Samples (px, py) [S] -> rgba [S, 4] in the working dtype, amb [S] bool, and the range (cmin, cmax [S, 3]) of the colours of the
    records that possibly cover each sample (+inf / -inf when none does)."""
    n, S = rec.shape[0], px.shape[0]
    colour = rec[:, -3:].astype(dtype)
    rgba, amb = np.zeros((S, 4), dtype), np.zeros(S, bool)
    cmin, cmax = np.full((S, 3), np.inf), np.full((S, 3), -np.inf)
    order = np.arange(n)[:, None]
    for a in range(0, S, CHUNK):
        sl = slice(a, min(a + CHUNK, S))
        cov = line_coverage(rec, px[sl], py[sl], cap, dtype, defects, gaps) if kind == "lines" else point_coverage(rec, px[sl], py[sl], dtype, defects, gaps)
        if "lowest_index" in defects:
            top = np.where(cov.t.any(axis=0), np.argmax(cov.t, axis=0), 0)
        else:
            top = np.max(np.where(cov.t, order, 0), axis=0)      # an argmax over zeros: record 0 under an uncovered sample
        rgba[sl, :3] = colour[top]
        rgba[sl, 3] = cov.t.any(axis=0)
        top_sure = np.max(np.where(cov.lo, order, -1), axis=0)
        amb[sl] = ((cov.hi & ~cov.lo) & (order > top_sure[None])).any(axis=0)
        for c in range(3):
            cmin[sl, c] = np.min(np.where(cov.hi, rec[:, -3 + c][:, None].astype(np.float64), np.inf), axis=0)
            cmax[sl, c] = np.max(np.where(cov.hi, rec[:, -3 + c][:, None].astype(np.float64), -np.inf), axis=0)
    return rgba, amb, cmin, cmax


def detect(rgba, defects=(), empty=None):
    """rgba [b, h, w, 4] -> [b, h, w] bool: differs from one of the up to eight neighbours inside the grid."""
    b, h, w, _ = rgba.shape
    pad = np.full((b, h + 2, w + 2, 4), np.nan, rgba.dtype)
    exists = np.zeros((b, h + 2, w + 2), bool)
    pad[:, 1:-1, 1:-1], exists[:, 1:-1, 1:-1] = rgba, True
    if "border_neighbour" in defects:      # the planted defect: an uncovered neighbour beyond the border
        pad[:, 0, :], pad[:, -1, :], pad[:, :, 0], pad[:, :, -1] = empty, empty, empty, empty
        pad[:, 1:-1, 1:-1] = rgba
        exists[:] = True
    mask = np.zeros((b, h, w), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                other = pad[:, 1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx]
                mask |= exists[:, 1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx] & (other != rgba).any(axis=-1)
    return mask


def _dilate(m):
    h, w = m.shape
    pad = np.zeros((h + 2, w + 2), bool)
    pad[1:-1, 1:-1] = m
    return np.any([pad[1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0)


def _pass(kind, rec, cap, xs, ys, scale, remaining, dtype, defects, gaps):
    """xs, ys [b, h, w] -> rgba [b, h, w, 4], ambf [b, h, w] (the ambiguous share of each cell's weight), cmin, cmax [b, h, w, 3], and the
    pass's own per-sample amb and refine mask (for the caller's `unsure`)."""
    b, h, w = xs.shape
    rgba, amb, cmin, cmax = sample(kind, rec, cap, xs.reshape(-1), ys.reshape(-1), dtype, defects, gaps)
    rgba, amb, cmin, cmax = rgba.reshape(b, h, w, 4), amb.reshape(b, h, w), cmin.reshape(b, h, w, 3), cmax.reshape(b, h, w, 3)
    ambf, mask = amb.astype(np.float64), np.zeros((b, h, w), bool)
    e_colour = np.zeros((b, h, w, 3))      # the propagated magnitude of the colour: exact where a record's colour is taken as it is
    if remaining > 0:
        empty = np.concatenate((rec[0, -3:].astype(dtype), np.zeros(1, dtype)))
        mask = detect(rgba, defects, empty)
        bi, yi, xi = np.nonzero(mask)
        if bi.size:
            k = np.arange(8, dtype=dtype)
            off = (((k if "no_half_offset" in defects else k + dtype(0.5)) / dtype(8) - dtype(0.5)) * dtype(scale)).astype(dtype)
            fx = (xs[bi, yi, xi][:, None, None] + off[None, None, :]) + np.zeros((1, 8, 1), dtype)
            fy = (ys[bi, yi, xi][:, None, None] + off[None, :, None]) + np.zeros((1, 1, 8), dtype)
            f_rgba, f_ambf, f_cmin, f_cmax, f_amb, f_mask, f_e = _pass(kind, rec, cap, fx, fy, scale / 8, remaining - 1, dtype, defects, gaps)
            # a fine cell whose own refinement can flip is ambiguous as a whole
            if remaining > 1:
                f_ambf = np.where(np.stack([_dilate(m) for m in f_amb]), 1.0, f_ambf)
            a = f_rgba[..., 3:]
            weighted = (f_rgba[..., :3] * a).reshape(-1, 64, 3)
            asum = a.reshape(-1, 64).sum(axis=1, dtype=dtype)
            wsum = weighted.sum(axis=1, dtype=dtype)
            den = asum + dtype(1e-10)
            colour = wsum if "colour_undivided" in defects else wsum / den[:, None]
            alpha = asum if "alpha_sum" in defects else asum / dtype(64)
            rgba[bi, yi, xi, :3], rgba[bi, yi, xi, 3] = colour, alpha
            ambf[bi, yi, xi] = f_ambf.reshape(-1, 64).mean(axis=1)
            cmin[bi, yi, xi] = np.minimum(cmin[bi, yi, xi], f_cmin.reshape(-1, 64, 3).min(axis=1))
            cmax[bi, yi, xi] = np.maximum(cmax[bi, yi, xi], f_cmax.reshape(-1, 64, 3).max(axis=1))
            e_sum = 6.0 * np.abs(weighted.astype(np.float64)).sum(axis=1) + (f_e * a.astype(np.float64)).reshape(-1, 64, 3).sum(axis=1)
            q = np.abs(colour.astype(np.float64))
            d = np.abs(den.astype(np.float64))[:, None]
            e_colour[bi, yi, xi] = (e_sum + q * d) / d + q
    return rgba, ambf, cmin, cmax, amb, mask, e_colour


def render(kind, image, rec, cap="round", passes=1, dtype=np.float64, defects=(), gaps=None) -> dict:
    """image [3, H, W] f32, rec [n, 8 or 7] f32 (pixel space) -> the dict described in the module's docstring."""
    image = np.asarray(image, np.float32)
    _, H, W = image.shape
    img = image.astype(dtype)
    if rec.shape[0] == 0:      # the stated deviation: an image with no records is copied through
        z = np.zeros((H, W))
        return dict(out=img.copy(), alpha=z.astype(dtype), rgba=np.zeros((4, H, W), dtype), mask=z.astype(bool), amb=z, unsure=z.astype(bool),
                    mag=np.abs(image.astype(np.float64)), spread=np.zeros((3, H, W)))
    ys, xs = np.meshgrid(np.arange(H, dtype=dtype) + dtype(0.5), np.arange(W, dtype=dtype) + dtype(0.5), indexing="ij")
    rgba, ambf, cmin, cmax, amb0, mask, e_colour = _pass(kind, rec, cap, xs[None], ys[None], 1.0, passes, dtype, defects, gaps)
    rgba, ambf, cmin, cmax, amb0, mask, e_colour = rgba[0], ambf[0], cmin[0], cmax[0], amb0[0], mask[0], e_colour[0]
    colour, alpha = np.moveaxis(rgba[..., :3], -1, 0), rgba[..., 3][None]
    one_minus = dtype(1) - alpha
    t1, t2 = img * one_minus, colour * alpha
    out = t1 + t2
    f = lambda v: np.abs(np.asarray(v, np.float64))
    e1 = f(img) * f(one_minus) + f(t1)
    e2 = f(alpha) * np.moveaxis(e_colour, -1, 0) + f(t2)
    i64 = image.astype(np.float64)
    spread = np.maximum(i64, np.moveaxis(cmax, -1, 0)) - np.minimum(i64, np.moveaxis(cmin, -1, 0))
    return dict(out=out, alpha=alpha[0], rgba=np.moveaxis(rgba, -1, 0), mask=mask, amb=64.0 * ambf, unsure=_dilate(amb0) if passes > 0 else np.zeros((H, W), bool),
                mag=e1 + e2 + f(out), spread=spread)


def check(out, ref: dict, factor=FACTOR):
    """The criterion of the module's docstring for an f32 result `out` [3, H, W] against the float64 run `ref`: -> (ok, report) with the
    shares of unsure and of ambiguous pixels, the largest error in units of its bound, and the largest error in units of 2^-24 mag."""
    err = np.abs(np.asarray(out, np.float64) - ref["out"].astype(np.float64))
    bound = factor * U * ref["mag"] + (ref["amb"] / 64.0)[None] * ref["spread"]
    sure = ~ref["unsure"][None] & np.ones_like(err, bool)
    worst = float((err[sure] / np.maximum(bound[sure], 1e-300)).max()) if sure.any() else 0.0
    clean = sure & (ref["amb"] == 0)[None]
    report = dict(unsure=float(ref["unsure"].mean()), ambiguous=float((ref["amb"] > 0).mean()), worst_over_bound=worst,
                  worst_ulp=float((err[clean] / np.maximum(U * ref["mag"][clean], 1e-300)).max()) if clean.any() else 0.0)
    return bool((err[sure] <= bound[sure]).all()), report


# ---- cases --------------------------------------------------------------------------------------------------------------------------
S16 = 1.0 / 16.0


def lattice_image(shape, seed):
    """[3, H, W] f32 with values that are multiples of 1/8 in [0, 1]."""
    return (np.random.default_rng(seed).integers(0, 9, size=(3, *shape)) / 8.0).astype(np.float32)


def lines_rec(start, end, width, colour):
    start, end = np.atleast_2d(np.asarray(start, np.float32)), np.atleast_2d(np.asarray(end, np.float32))
    n = max(len(start), len(end))
    w = np.broadcast_to(np.asarray(width, np.float32).reshape(-1, 1), (n, 1))
    c = np.broadcast_to(np.atleast_2d(np.asarray(colour, np.float32)), (n, 3))
    return np.concatenate((np.broadcast_to(start, (n, 2)), np.broadcast_to(end, (n, 2)), w, c), axis=1).astype(np.float32)


def points_rec(xy, radius, inner, colour):
    xy = np.atleast_2d(np.asarray(xy, np.float32))
    n = len(xy)
    col = lambda v, k: np.broadcast_to(np.asarray(v, np.float32).reshape(-1, k), (n, k))
    return np.concatenate((xy, col(radius, 1), col(inner, 1), np.broadcast_to(np.atleast_2d(np.asarray(colour, np.float32)), (n, 3))), axis=1).astype(np.float32)


# The golden scenes, in WORLD coordinates (here the pixel grid: no range given), on a 24 x 40 image.  All coordinates are odd multiples of
# 1/16, so that subsamples (at odd multiples of 1/16) fall exactly on the thresholds: x = 20 1/16 has par = |D| on line 0, x = 4 1/16 has
# par = 0, y = 9 1/16 has a perpendicular distance of exactly w / 2; the offsets (3, 4) and (3, 0) from a centre are at distances 5 and 3.
GOLDEN_SHAPE = (24, 40)
GOLDEN_LINES = dict(
    start=[[4 + S16, 8 + S16], [30 + S16, 3 + S16], [10 + S16, 5 + S16], [25 + S16, 15 + S16], [16 + S16, 18 + S16]],
    end=[[20 + S16, 8 + S16], [30 + S16, 19 + S16], [10 + S16, 12 + S16], [25 + S16, 15 + S16], [36 + S16, 18 + S16]],
    width=[2.0, 4.0, 2.0, 6.0, 10.0],
    color=[[1, 0, 0.5], [0, 1, 0.25], [0.25, 0.25, 1], [1, 1, 0], [0.5, 0.125, 0.75]])
GOLDEN_POINTS = dict(points=[[10 + S16, 10 + S16], [25 + S16, 12 + S16], [28 + S16, 12 + S16]], radius=[5.0, 5.0, 2.0], inner_radius=[0.0, 3.0, 0.0],
                     color=[[1, 0.5, 0], [0, 0.75, 1], [0.25, 1, 0.25]])
# an oblique scene with ranges: exercises world_to_pixel (x / y are not symmetric) and general rounding
GOLDEN_OBLIQUE = dict(shape=(32, 48), x_range=(-1.0, 2.0), y_range=(0.5, 2.5), seed=3, n=12)


def oblique_world(spec=GOLDEN_OBLIQUE):
    g = np.random.default_rng(spec["seed"])
    n = spec["n"]
    lo, hi = np.array([spec["x_range"][0], spec["y_range"][0]]), np.array([spec["x_range"][1], spec["y_range"][1]])
    return dict(start=(lo + (hi - lo) * g.uniform(-0.1, 1.1, (n, 2))).astype(np.float32), end=(lo + (hi - lo) * g.uniform(-0.1, 1.1, (n, 2))).astype(np.float32),
                width=g.uniform(0.5, 6.0, n).astype(np.float32), color=(g.integers(0, 9, (n, 3)) / 8.0).astype(np.float32))


def golden_scenes():
    """name -> (kind, image [3, H, W], world arguments, cap, shape, x_range, y_range)."""
    img = lattice_image(GOLDEN_SHAPE, 1)
    scenes = {f"lines_{cap}": ("lines", img, GOLDEN_LINES, cap, None, None) for cap in CAPS}
    scenes["points"] = ("points", img, GOLDEN_POINTS, None, None, None)
    scenes["oblique"] = ("lines", lattice_image(GOLDEN_OBLIQUE["shape"], 2), oblique_world(), "round", GOLDEN_OBLIQUE["x_range"], GOLDEN_OBLIQUE["y_range"])
    return scenes


def scene_records(kind, image, world, x_range, y_range, defects=()):
    shape = image.shape[-2:]
    if kind == "lines":
        return lines_rec(world_to_pixel(world["start"], shape, x_range, y_range, defects), world_to_pixel(world["end"], shape, x_range, y_range, defects),
                         world["width"], world["color"])
    return points_rec(world_to_pixel(world["points"], shape, x_range, y_range, defects), world["radius"], world["inner_radius"], world["color"])


def lattice_case(kind, shape, n, seed, cap="round"):
    """Axis-aligned lines (or points) with every coordinate, width and radius a multiple of 1/16 and colours multiples of 1/8: coverage,
    sums, quotient and blend are exact in f32 under any faithful evaluation -- except the quotient sum / count, exact only when the covered
    subsamples of a pixel share one colour or their count is a power of two; so the records of a lattice case do not overlap in colour:
    every record has the SAME colour per case layer, and the image supplies the variety."""
    g = np.random.default_rng(seed)
    H, W = shape
    q = lambda lo, hi, size=None: g.integers(int(lo * 16), int(hi * 16) + 1, size) / 16.0
    colour = g.integers(1, 9, 3) / 8.0
    if kind == "points":
        rad = q(0.5, max(min(H, W) / 3.0, 1.0), n)
        return points_rec(np.stack((q(-1, W + 1, n), q(-1, H + 1, n)), axis=1), rad, rad * g.integers(0, 2, n) * 0.5, colour)
    a = np.stack((q(-2, W + 2, n), q(-2, H + 2, n)), axis=1)
    b = a.copy()
    horizontal = g.integers(0, 2, n).astype(bool)
    length = q(0, max(W, H), n) * g.choice([-1.0, 1.0], n)
    b[horizontal, 0] += length[horizontal]
    b[~horizontal, 1] += length[~horizontal]
    return lines_rec(a, b, q(0.25, 5, n), colour)


def general_lines(shape, n, seed, wmin=0.5, wmax=6.0):
    """n random oblique lines across (and a little beyond) an H x W image, widths in [wmin, wmax], colours multiples of 1/8."""
    g = np.random.default_rng(seed)
    H, W = shape
    size = np.array([W, H], np.float64)
    return lines_rec(g.uniform(-0.1, 1.1, (n, 2)) * size, g.uniform(-0.1, 1.1, (n, 2)) * size, g.uniform(wmin, wmax, n), g.integers(0, 9, (n, 3)) / 8.0)


def general_rings(shape, n, seed):
    g = np.random.default_rng(seed)
    H, W = shape
    rad = g.uniform(1.0, min(H, W) / 3.0, n)
    return points_rec(g.uniform(-0.1, 1.1, (n, 2)) * np.array([W, H]), rad, rad * g.uniform(0.0, 0.9, n), g.integers(0, 9, (n, 3)) / 8.0)


def general_image(shape, seed):
    return np.random.default_rng(seed).uniform(0, 1, (3, *shape)).astype(np.float32)


# name -> (kind, shape, builder of the records, cap): the general cases of the CPU and GPU tests
GENERAL_CASES = {
    "lines_round_56x80": ("lines", (56, 80), lambda: general_lines((56, 80), 30, 11), "round"),
    "lines_butt_47x33": ("lines", (47, 33), lambda: general_lines((47, 33), 24, 12), "butt"),
    "lines_square_64x64": ("lines", (64, 64), lambda: general_lines((64, 64), 32, 13), "square"),
    "rings_64x80": ("points", (64, 80), lambda: general_rings((64, 80), 30, 14), None),
}


def cameras(n, seed):
    """n cameras on a loose arc looking inwards: (extrinsics [n, 4, 4], intrinsics [n, 3, 3], colour [n, 3], near [n], far [n]) f32."""
    g = np.random.default_rng(seed)
    E = np.tile(np.eye(4), (n, 1, 1))
    for k in range(n):
        yaw, pitch = 0.3 * k + 0.1 * g.normal(), 0.2 * g.normal()
        cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
        E[k, :3, :3] = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
        E[k, :3, 3] = [2.0 * np.sin(0.3 * k), 0.3 * g.normal(), -2.0 * np.cos(0.3 * k)]
    K = np.tile(np.array([[0.9, 0, 0.5], [0, 1.1, 0.5], [0, 0, 1.0]]), (n, 1, 1))
    K[:, 0, 0] += 0.1 * g.uniform(-1, 1, n)
    f32 = lambda a: np.asarray(a, np.float32)
    return f32(E), f32(K), f32(g.integers(0, 9, (n, 3)) / 8.0), f32(g.uniform(0.3, 0.6, n)), f32(g.uniform(1.5, 3.0, n))
