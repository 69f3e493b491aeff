"""Float64 restatement of the visualisation kernels (include/vicasplat_viz.h, csrc/viz.hip) in numpy: the depth range of vis_depth_map, the
colour-map argument x, its index, both colour maps, the frame packing of render_video_generic, the layout functions, the equal AABB and
the orthographic camera set-up of render_projections.  Shared by tests/test_viz_cpu.py, tests/test_viz_gpu.py and
tests/golden/gen_viz_golden.py.

What is exact and what is bounded.
  The four order statistics are elements of the f32 input: exact.  The ranks are torch.quantile's for an f32 input, r = f32(q) * f32(m - 1)
  rounded to f32 (rank_f32 below; a planted defect forms it in f64).  Everything after them is float64 here and f32 in the kernel and in
  the reference; each output comes with `mag`, the sum of the absolute values of the terms that are added to form it (the amplification
  1 / |far - near| included), and a bound is a multiple of 2^-24 mag:
      K = 4 max(R32, 1),   |f32 result - float64 result| <= K 2^-24 mag
  -- the project's standing bound.  R32 is the reference's own f32 error in those units, measured by tests/test_viz_cpu.py
  (test_reference_f32_gap) on log-uniform depths with 10 % zeros: range <= 0.621 (near of `wide`), x <= 0.943 (`narrow`), both asserted <= R32;
  so K = 4.
  The index min(trunc(clip(x, 0, 1) * 256), 255) is a step function of x: a pixel is compared only where the index is the same at
  x - bound and at x + bound (`band`: the pixels where it is not; half-width 256 bound in units of x * 256).  A case may lose at most
  EXCLUSION_CAP of its pixels to the band (asserted per case, so that no input hides a failure).
  Given the index, colours are a lookup (f32: bit-equal) and bytes are trunc(clip(c, 0, 1) * 255) with the f32 product (bit-equal).
"""
from __future__ import annotations

import numpy as np

EPS = 2.0 ** -24
R32 = 0.95           # the reference's own f32 result against float64, in units of 2^-24 mag: measured 0.943 (x), 0.621 (range); see above
K = 4.0 * max(R32, 1.0)
QUANTUM = 2.0 ** -149 / EPS      # the spacing of the f32 subnormals in units of 2^-24: what one rounding can cost however small its result
EXCLUSION_CAP = 0.005
MAX_RANGE_N = 16_000_000
Q_NEAR, Q_FAR = np.float32(0.01), np.float32(0.99)


# ---- range ------------------------------------------------------------------------------------------------------------------------
def rank_f32(q, m: int, in_f64: bool = False):
    """(floor, ceil, weight) of torch.quantile's rank for an f32 input of m values; the weight is r - floor(r) in the rank's precision."""
    r = np.float64(np.float32(q)) * np.float64(m - 1) if in_f64 else np.float32(q) * np.float32(m - 1)
    lo = np.floor(r)
    return int(lo), int(np.ceil(r)), float(r - lo)


def lerp(a, b, w):
    """torch.lerp, in the precision of its arguments."""
    return a + w * (b - a) if w < 0.5 else b - (b - a) * (1 - w)


def quantile(values32: np.ndarray, q, *, rank_f64: bool = False, no_lerp: bool = False):
    """(Q in float64, (a, b) f32 order statistics, mag of Q) of torch.quantile(values32, q) for a flat f32 array, NaN when one is in it."""
    s = np.sort(values32.astype(np.float32).ravel())       # NaNs last, as torch sorts them
    lo, hi, w = rank_f32(q, s.size, rank_f64)
    a, b = s[lo], s[hi]
    if np.isnan(s[-1]):
        return np.float64(np.nan), (a, b), np.float64(np.nan)
    with np.errstate(invalid="ignore", over="ignore"):
        a64, b64 = np.float64(a), np.float64(b)
        Q = a64 if no_lerp else lerp(a64, b64, np.float64(w))
        mag = abs(a64) + abs(b64) + abs(b64 - a64) + 3 * QUANTUM      # three f32 operations, each also rounded to the subnormal spacing
    return Q, (a, b), mag


def depth_range(values32: np.ndarray, *, rank_f64=False, far_positive_only=False, no_fallback=False, no_lerp=False) -> dict:
    """near, far (float64), their mags, stats = (a, b) of near then of far (f32, exact), npos.  The keyword flags plant defects."""
    v = np.asarray(values32, np.float32).ravel()
    assert 1 <= v.size <= MAX_RANGE_N
    pos = v[v > 0]
    kw = dict(rank_f64=rank_f64, no_lerp=no_lerp)
    with np.errstate(divide="ignore", invalid="ignore"):
        Qf, sf, mf = quantile(pos if far_positive_only and pos.size else v, Q_FAR, **kw)
        far = np.log(Qf)
        mag_far = abs(far) + mf / abs(Qf)
        if pos.size:
            Qn, sn, mn = quantile(pos, Q_NEAR, **kw)
            near = np.log(Qn)
            mag_near = abs(near) + mn / abs(Qn)
        elif no_fallback:
            near, sn, mag_near = np.float64(np.nan), (np.float32(0), np.float32(0)), np.float64(np.nan)
        else:
            near, sn, mag_near = np.float64(0.0), (np.float32(0), np.float32(0)), np.float64(0.0)
    return dict(near=near, far=far, mag_near=mag_near, mag_far=mag_far, stats=np.array([sn[0], sn[1], sf[0], sf[1]], np.float32),
                npos=int(pos.size))


def within(got, want, mag, k=K) -> bool:
    """The bound for one output, with the special values compared as such."""
    got, want = np.float64(got), np.float64(want)
    if np.isnan(want) or np.isinf(want):
        return bool((np.isnan(got) and np.isnan(want)) or got == want)
    return bool(abs(got - want) <= k * EPS * mag)


def units(got, want, mag) -> float:
    return float(abs(np.float64(got) - np.float64(want)) / (EPS * mag)) if mag > 0 else float(got != want)


# ---- x, index, colours ------------------------------------------------------------------------------------------------------------
def x_depth(values32: np.ndarray, near, far, *, range_err=(0.0, 0.0), no_one_minus=False):
    """(x, bound) in float64 for the kernel's x = 1 - (log v - near) / (far - near) with the range it is GIVEN (near, far: the f32 values
    the kernel reads, or a float64 range with range_err = the bounds on the kernel's own near and far).  bound = K 2^-24 mag + the range's
    share; NaN and infinite x carry bound 0 (they are compared as such)."""
    v = np.asarray(values32, np.float32).astype(np.float64)
    near, far = np.float64(near), np.float64(far)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        lv = np.log(v)
        D = far - near
        t = (lv - near) / D
        x = t if no_one_minus else 1.0 - t
        mag = 1.0 + (np.abs(lv) + abs(near)) / abs(D) + np.abs(t) * (abs(far) + abs(near)) / abs(D)
        bound = K * EPS * mag + (range_err[0] * np.abs(1.0 - t) + range_err[1] * np.abs(t)) / abs(D)
    bound = np.where(np.isfinite(x) & np.isfinite(bound), bound, 0.0)      # (an infinite range: x is 1 or NaN exactly)
    return x, bound


def x_max(values32: np.ndarray):
    v = np.asarray(values32, np.float32).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        top = np.nan if np.isnan(v).any() else v.max()
        x = v / top
    return x, np.where(np.isfinite(x), K * EPS * np.abs(x), 0.0)


def index_of(x: np.ndarray, *, scale=256.0, rounding=False) -> np.ndarray:
    """min(trunc(clip(x, 0, 1) * 256), 255) as int32, -1 for a NaN."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        y = np.clip(x, 0.0, 1.0) * scale
        i = np.minimum(np.rint(y) if rounding else np.trunc(y), 255.0)
    return np.where(np.isnan(x), -1, i).astype(np.int32)


def band(x: np.ndarray, bound: np.ndarray) -> np.ndarray:
    """True where the index is not decided at this bound on x."""
    return index_of(x - bound) != index_of(x + bound)


def lookup(idx: np.ndarray, lut32: np.ndarray) -> np.ndarray:
    """idx [..., H, W] -> f32 planes [..., 3, H, W]; (0, 0, 0) for idx = -1."""
    c = np.where((idx < 0)[..., None], np.float32(0), np.asarray(lut32, np.float32)[np.maximum(idx, 0)])
    return np.moveaxis(c, -1, -3).astype(np.float32)


def to_u8(c32: np.ndarray, *, scale=255.0, rounding=False) -> np.ndarray:
    """trunc(clip(c, 0, 1) * 255) with the product in f32; 0 for a NaN."""
    c = np.asarray(c32, np.float32)
    with np.errstate(invalid="ignore"):
        y = np.clip(np.where(np.isnan(c), np.float32(0), c), np.float32(0), np.float32(1)) * np.float32(scale)
    return (np.rint(y) if rounding else np.trunc(y)).astype(np.uint8)


def ramp_lut() -> np.ndarray:
    """lut[i] = (i, 2 i, 255 - i) / 255: the index is visible in the output."""
    i = np.arange(256, dtype=np.float32)
    return (np.stack([i, 2 * i, 255 - i], -1) / np.float32(255)).astype(np.float32)


# ---- frames, layout ---------------------------------------------------------------------------------------------------------------
def frames(rgb32: np.ndarray, idx: np.ndarray, lut32: np.ndarray, gap: int = 8, *, gap_value=255, nan_first_entry=False, **u8kw) -> np.ndarray:
    """[M, 3, 2 H + gap, W] uint8 from rgb [M, 3, H, W] f32 and the depth indices [M, H, W]."""
    M, _, H, W = rgb32.shape
    out = np.full((M, 3, 2 * H + gap, W), gap_value, np.uint8)
    out[:, :, :H] = to_u8(rgb32, **u8kw)
    out[:, :, H + gap:] = to_u8(lookup(np.maximum(idx, 0) if nan_first_entry else idx, lut32), **u8kw)
    return out


def loop_reverse(video: np.ndarray) -> np.ndarray:
    return np.concatenate([video, video[::-1][1:-1]], 0)


def cat(axis: int, images, align="start", gap=8, gap_color=1.0) -> np.ndarray:
    """images [C, H, W] f32 joined along axis 1 (vertical) or 2 (horizontal)."""
    cross = 3 - axis
    longest = max(im.shape[cross] for im in images)
    color = np.asarray(gap_color, np.float32).reshape(-1, 1, 1)
    parts = []
    for k, im in enumerate(images):
        if k and gap > 0:
            shape = [images[0].shape[0], gap, gap]
            shape[cross] = longest
            parts.append(np.ones(shape, np.float32) * color)
        shape = list(im.shape)
        shape[cross] = longest
        slack = longest - im.shape[cross]
        at = {"start": 0, "center": slack // 2, "end": slack}[align]
        canvas = np.ones(shape, np.float32) * color
        sl = [slice(None)] * 3
        sl[cross] = slice(at, at + im.shape[cross])
        canvas[tuple(sl)] = im
        parts.append(canvas)
    return np.concatenate(parts, axis)


def hcat(*images, **kw):
    return cat(2, images, **kw)


def vcat(*images, **kw):
    return cat(1, images, **kw)


def add_border(image, border=8, color=1.0):
    c, h, w = image.shape
    out = np.ones((c, h + 2 * border, w + 2 * border), np.float32) * np.asarray(color, np.float32).reshape(-1, 1, 1)
    out[:, border:h + border, border:w + border] = image
    return out


# ---- projections ------------------------------------------------------------------------------------------------------------------
def equal_aabb_with_margin(minima, maxima, margin=0.1):
    """A cube around the midpoint whose side is the largest extent OF THE WHOLE BATCH times 1 + margin."""
    minima, maxima = np.asarray(minima, np.float64), np.asarray(maxima, np.float64)
    mid = (maxima + minima) * 0.5
    span = (maxima - minima).max() * (1 + margin)
    return mid - 0.5 * span, mid + 0.5 * span


def projection_cameras(scene_min, scene_max, look_axis: int):
    """(extrinsics [b, 4, 4], width, height, near, far) of render_projections for one look axis."""
    scene_min, scene_max = np.asarray(scene_min, np.float64), np.asarray(scene_max, np.float64)
    b = scene_min.shape[0]
    right, down = (look_axis + 1) % 3, (look_axis + 2) % 3
    E = np.zeros((b, 4, 4))
    E[:, right, 0] = E[:, down, 1] = E[:, look_axis, 2] = E[:, 3, 3] = 1
    E[:, right, 3] = 0.5 * (scene_min[:, right] + scene_max[:, right])
    E[:, down, 3] = 0.5 * (scene_min[:, down] + scene_max[:, down])
    E[:, look_axis, 3] = scene_min[:, look_axis]
    ext = scene_max - scene_min
    return E, ext[:, right], ext[:, down], np.zeros(b), ext[:, look_axis]


def orthographic_setup(extrinsics, width, height, near, far, fov_degrees=0.1) -> dict:
    """The `dump` of render_cuda_orthographic: a far, narrow perspective camera standing in for an orthographic one."""
    fov_x = np.deg2rad(np.float64(fov_degrees))
    tan_x = np.tan(0.5 * fov_x)
    dist = 0.5 * np.asarray(width, np.float64) / tan_x
    tan_y = 0.5 * np.asarray(height, np.float64) / dist
    back = np.eye(4)[None].repeat(len(dist), 0)
    back[:, 2, 3] = -dist
    return dict(extrinsics=np.asarray(extrinsics, np.float64) @ back, fov_x=fov_x, fov_y=np.arctan(2 * tan_y), near=near + dist,
                far=far + dist, tan_fov_x=tan_x, tan_fov_y=tan_y)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def log_uniform(shape, lo, hi, seed, zeros=0.1) -> np.ndarray:
    """Log-uniform depths on [lo, hi] with a share of exact zeros."""
    g = np.random.default_rng(seed)
    d = np.exp(g.uniform(np.log(lo), np.log(hi), shape)).astype(np.float32)
    d[g.uniform(size=shape) < zeros] = 0
    return d


DEPTH_CASES = {"room": (0.5, 50.0), "wide": (0.01, 100.0), "narrow": (1.0, 1.5)}


# ---- the criteria both test files apply ---------------------------------------------------------------------------------------------
def range_ok(near, far, ref: dict) -> bool:
    """(near, far) against depth_range's float64 result, per element within K 2^-24 mag."""
    return within(near, ref["near"], ref["mag_near"]) and within(far, ref["far"], ref["mag_far"])


def index_ok(idx_got: np.ndarray, x: np.ndarray, bound: np.ndarray) -> bool:
    """Equal to the float64 index outside the band, and the band within the exclusion cap."""
    out = band(x, bound)
    return bool(out.mean() <= EXCLUSION_CAP and np.array_equal(np.asarray(idx_got)[~out], index_of(x)[~out]))


def rank_rounding_size(q=Q_FAR, start=1000) -> int:
    """The first m >= start at which the f32 rank of q and the float64 product have different floors."""
    m = start
    while rank_f32(q, m)[0] == rank_f32(q, m, in_f64=True)[0]:
        m += 1
    return m


def rank_rounding_case(seed=0) -> np.ndarray:
    """m = rank_rounding_size() values with a jump from about 1 to about 10^6 exactly at the f32 rank of the 0.99 quantile: the float64 rank
    sits 0.008 below it and would blend the two sides."""
    m = rank_rounding_size()
    lo = rank_f32(Q_FAR, m)[0]
    v = np.where(np.arange(m) < lo, 1.0 + np.arange(m) / m, 1e6 + np.arange(m)).astype(np.float32)
    np.random.default_rng(seed).shuffle(v)
    return v
