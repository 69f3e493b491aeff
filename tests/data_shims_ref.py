"""The yardstick of the data shims: a numpy restatement of PIL's 8-bit Lanczos reduction (Image.resize(..., Image.LANCZOS), reducing only)
and of the reference's crop and augmentation shims (src/dataset/shims/crop_shim.py, augmentation_shim.py).  uint8 in, uint8 and float32
out, with mirror, crop and intrinsics.  Written from the algorithm (include/vicasplat_data.h states it), not from the package's code: the
package's table builder is compared with `coeffs` below, and `coeffs` with the installed PIL (tests/test_data_shims_cpu.py).

Also here: the case lists of the CPU and GPU tests, the deterministic inputs of tests/golden/crop_shim.npz, and the planted defects
(`mutant=`), each of which must change at least one byte of the golden example.
"""
from __future__ import annotations

import functools
import hashlib
import math

import numpy as np

BITS = 22
HALF = 1 << (BITS - 1)

MUTANTS = ("no_half", "truncated_coeffs", "vertical_first", "no_rounding_between", "xmin_no_half", "crop_round_up", "mirror_after_crop",
           "div_256")

# (h_in, w_in) -> (h_scaled, w_scaled): the shapes of the comparison with PIL
PIL_SHAPES = (((360, 640), (256, 455)), ((720, 960), (256, 341)), ((540, 960), (256, 455)), ((45, 80), (32, 57)), ((17, 400), (17, 390)),
              ((400, 17), (390, 17)), ((50, 71), (33, 47)), ((40, 32), (40, 32)))

# name -> (N, h_in, w_in, (h_out, w_out), mirror flags): the cases of the GPU test
GPU_CASES = {
    "45x80": (5, 45, 80, (32, 32), (1, 0, 1, 1, 0)),
    "80x45": (5, 80, 45, (32, 32), (1, 0, 1, 1, 0)),
    "50x71": (2, 50, 71, (33, 31), (0, 1)),
    "17x400": (2, 17, 400, (16, 390), (1, 0)),
    "400x17": (2, 400, 17, (390, 16), (0, 1)),
    "40x32": (2, 40, 32, (32, 32), (0, 1)),
    "360x640": (3, 360, 640, (256, 256), (0, 1, 0)),
    "720x960": (1, 720, 960, (256, 256), (0,)),
}
FILLS = ("random", "extremes", "constant")


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


@functools.lru_cache(maxsize=None)
def coeffs(n_in: int, n_out: int, mutant: str | None = None):
    """(bounds [out, 2] = (xmin, n), k [out, ksize]) int32 of one axis, n_out <= n_in."""
    assert 1 <= n_out <= n_in
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = 3.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), np.int32)
    k = np.zeros((n_out, ksize), np.int32)
    inv = 1.0 / filterscale
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        n = xmax - xmin
        w = [_lanczos((x + xmin - center + 0.5) * inv) for x in range(n)]
        if mutant == "xmin_no_half":
            # the window starts where int(center - support) puts it while the taps stay those of the right window.  (Computing the taps from
            # the wrong xmin as well is no defect: the extra tap lies outside the filter's support and weighs 0.)
            xmin = max(int(center - support), 0)
        total = 0.0
        for v in w:
            total += v
        for x, v in enumerate(w):
            v = v / total if total != 0.0 else v
            if mutant == "truncated_coeffs":
                k[xx, x] = int(v * (1 << BITS))
            else:
                k[xx, x] = int(v * (1 << BITS) - 0.5) if v < 0 else int(v * (1 << BITS) + 0.5)
        bounds[xx] = (xmin, n)
    return bounds, k


def _pass(img, n_out: int, axis: int, mutant: str | None, exact: bool = False):
    """One pass along `axis` of img [h, w, c] (uint8, or float64 when the mutant keeps unrounded values): uint8, or float64 if `exact`."""
    n_in = img.shape[axis]
    if n_in == n_out:
        return img
    bounds, k = coeffs(n_in, n_out, mutant)
    src = np.moveaxis(img, axis, 0)
    out = np.empty((n_out,) + src.shape[1:], np.float64 if (exact or src.dtype == np.float64) else np.uint8)
    for xx in range(n_out):
        xmin, n = bounds[xx]
        if src.dtype == np.float64 or exact:
            acc = np.tensordot(k[xx, :n].astype(np.float64), src[xmin:xmin + n].astype(np.float64), axes=(0, 0)) / (1 << BITS)
            out[xx] = acc if exact else np.clip(np.floor(acc + 0.5), 0, 255)
        else:
            acc = np.tensordot(k[xx, :n].astype(np.int64), src[xmin:xmin + n].astype(np.int64), axes=(0, 0))
            acc = acc + (0 if mutant == "no_half" else HALF)
            assert np.abs(acc).max() < 1 << 31
            out[xx] = np.clip(acc >> BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(img: np.ndarray, h: int, w: int, mutant: str | None = None) -> np.ndarray:
    """PIL's Image.fromarray(img).resize((w, h), Image.LANCZOS) of img [h_in, w_in, 3] uint8, h <= h_in and w <= w_in: uint8 [h, w, 3]."""
    assert img.dtype == np.uint8 and img.ndim == 3
    if mutant == "vertical_first":
        return _pass(_pass(img, h, 0, mutant), w, 1, mutant)
    if mutant == "no_rounding_between":
        mid = _pass(img, w, 1, mutant, exact=True)
        out = _pass(mid, h, 0, mutant)
        return np.clip(np.floor(out.astype(np.float64) + 0.5), 0, 255).astype(np.uint8)
    return _pass(_pass(img, w, 1, mutant), h, 0, mutant)


def quantise(x: np.ndarray) -> np.ndarray:
    """The reference's (image * 255).clip(0, 255).type(uint8) of a float32 array; NaN -> 0 (the package's stated choice)."""
    s = x.astype(np.float32) * np.float32(255.0)
    s = np.where(s > 0, np.minimum(s, np.float32(255.0)), np.float32(0.0))      # a NaN fails `> 0`
    return s.astype(np.uint8)


def scaled_size(h_in, w_in, shape):
    h_out, w_out = shape
    assert h_out <= h_in and w_out <= w_in
    f = max(h_out / h_in, w_out / w_in)
    h_scaled, w_scaled = round(h_in * f), round(w_in * f)
    assert h_scaled == h_out or w_scaled == w_out
    return h_scaled, w_scaled


def crop_frame(img: np.ndarray, shape, mirror: bool = False, mutant: str | None = None):
    """One frame [h_in, w_in, 3] uint8 through the (optional) mirror, rescale and centre crop: (uint8 [h_out, w_out, 3], (row, col),
    (h_scaled, w_scaled))."""
    h_out, w_out = shape
    h_scaled, w_scaled = scaled_size(img.shape[0], img.shape[1], shape)
    up = 1 if mutant == "crop_round_up" else 0
    row, col = (h_scaled - h_out + up) // 2, (w_scaled - w_out + up) // 2
    if mirror and mutant != "mirror_after_crop":
        img = img[:, ::-1]
    out = resize(np.ascontiguousarray(img), h_scaled, w_scaled, mutant)[row:row + h_out, col:col + w_out]
    if mirror and mutant == "mirror_after_crop":
        out = out[:, ::-1]
    return np.ascontiguousarray(out), (row, col), (h_scaled, w_scaled)


def to_float(u8_hwc: np.ndarray, mutant: str | None = None) -> np.ndarray:
    """[..., h, w, 3] uint8 -> [..., 3, h, w] float32 = float32(u) / 255."""
    f = u8_hwc.astype(np.float32) / np.float32(256.0 if mutant == "div_256" else 255.0)
    return np.ascontiguousarray(np.moveaxis(f, -1, -3))


def crop_frames(frames: np.ndarray, shape, mirror=None, mutant: str | None = None):
    """frames [N, h_in, w_in, 3] uint8, mirror [N] or None -> (uint8 [N, h_out, w_out, 3], float32 [N, 3, h_out, w_out])."""
    u = np.stack([crop_frame(f, shape, bool(mirror[i]) if mirror is not None else False, mutant)[0] for i, f in enumerate(frames)])
    return u, to_float(u, mutant)


def crop_intrinsics(K: np.ndarray, h_in, w_in, shape) -> np.ndarray:
    """The reference's correction in float32: fx *= w_scaled / w_out, fy *= h_scaled / h_out."""
    h_scaled, w_scaled = scaled_size(h_in, w_in, shape)
    K = K.astype(np.float32).copy()
    K[..., 0, 0] *= np.float32(w_scaled / shape[1])
    K[..., 1, 1] *= np.float32(h_scaled / shape[0])
    return K


def reflect_extrinsics(E: np.ndarray) -> np.ndarray:
    R = np.eye(4, dtype=np.float32)
    R[0, 0] = -1
    return (R @ E.astype(np.float32) @ R).astype(np.float32)


def normalise(x: np.ndarray, mean, std) -> np.ndarray:
    m = np.asarray(mean, np.float32).reshape(3, 1, 1)
    s = np.asarray(std, np.float32).reshape(3, 1, 1)
    return ((x - m) / s).astype(np.float32)


def make_frames(n: int, h: int, w: int, fill: str, seed: int = 0) -> np.ndarray:
    """[n, h, w, 3] uint8: random bytes, a random 0 / 255 image (both clamps of the filter act), or constant 255."""
    g = np.random.default_rng([seed, n, h, w])
    if fill == "random":
        return g.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    if fill == "extremes":
        return (g.integers(0, 2, (n, h, w, 3), dtype=np.uint8) * 255).astype(np.uint8)
    assert fill == "constant"
    return np.full((n, h, w, 3), 255, np.uint8)


# ---- the deterministic example of tests/golden/crop_shim.npz ----
GOLDEN_SHAPE = (32, 32)
GOLDEN_EXAMPLES = {"wide": (45, 80, 11), "tall": (80, 45, 12)}      # name -> (h, w, seed); 2 context + 3 target views each


def golden_example(name: str) -> dict:
    """{"context": {image [2, 3, h, w] f32, intrinsics [2, 3, 3], extrinsics [2, 4, 4]}, "target": {... 3 views}} as numpy float32.  The
    images are floats that are NOT multiples of 1 / 255 and leave [0, 1] a little, so that the reference's quantisation acts."""
    h, w, seed = GOLDEN_EXAMPLES[name]
    g = np.random.default_rng(seed)
    out = {}
    for key, v in (("context", 2), ("target", 3)):
        image = g.uniform(-0.05, 1.05, (v, 3, h, w)).astype(np.float32)
        K = np.tile(np.eye(3, dtype=np.float32), (v, 1, 1))
        K[:, 0, 0] = g.uniform(0.6, 1.2, v)
        K[:, 1, 1] = g.uniform(0.6, 1.2, v)
        K[:, 0, 2] = g.uniform(0.45, 0.55, v)
        K[:, 1, 2] = g.uniform(0.45, 0.55, v)
        E = np.tile(np.eye(4, dtype=np.float32), (v, 1, 1))
        q, _ = np.linalg.qr(g.normal(size=(v, 3, 3)))
        E[:, :3, :3] = q
        E[:, :3, 3] = g.normal(size=(v, 3))
        out[key] = dict(image=image, intrinsics=K.astype(np.float32), extrinsics=E.astype(np.float32))
    return out


def example_digest(ex: dict) -> str:
    h = hashlib.sha256()
    for key in ("context", "target"):
        for name in ("image", "intrinsics", "extrinsics"):
            h.update(np.ascontiguousarray(ex[key][name]).tobytes())
    return h.hexdigest()


def shim_views(views: dict, shape, mirror: bool = False, mutant: str | None = None) -> dict:
    """The crop shim (after reflect_views when `mirror`) on numpy views: image uint8 [V, h_out, w_out, 3] and float32 [V, 3, h_out, w_out],
    intrinsics, extrinsics."""
    image = views["image"]
    v, _, h, w = image.shape
    frames = np.ascontiguousarray(np.moveaxis(quantise(image), 1, -1))
    u, f = crop_frames(frames, shape, [mirror] * v, mutant)
    return dict(image_u8=u, image=f, intrinsics=crop_intrinsics(views["intrinsics"], h, w, shape),
                extrinsics=reflect_extrinsics(views["extrinsics"]) if mirror else views["extrinsics"])
