"""The crop shim of the reference's dataset loaders (src/dataset/shims/crop_shim.py) on the HIP path: per frame, PIL's 8-bit Lanczos
reduction, a centre crop and the intrinsics' correction -- with the reference's names, arguments and assertions.  The pixels are computed by
one launch of vsp_rescale_crop (csrc/preprocess.hip, include/vicasplat_data.h) per view group, byte for byte what the reference computes on
the host through PIL; there is no CPU fallback.

What differs from the reference, all of it additions:
  * `image` may be uint8 as well as float32: [*, 3, h, w] with any strides, so that a decoder's HWC buffer is passed as a permuted view
    (`frames.permute(..., 2, 0, 1)` or `movedim(-1, -3)`) without a copy; strides that are neither packed HWC nor planar CHW get a
    `.contiguous()`.  A float image is quantised in the kernel as the reference does it (`(image * 255).clip(0, 255).type(uint8)`).
  * any leading batch dimensions, also for `rescale`.
  * `normalize=(mean, std)`: the output is `(x - mean) / std` per channel, as the reference's normalize_image gives it on the raw output.
  * a views dict may carry the key MIRROR_KEY (set by augmentation_shim.reflect_views): a uint8 flag per view.  The crop shim consumes it --
    a flagged view is mirrored left-right before the resample, as the reference's `image.flip(-1)` ahead of the crop shim does -- and
    removes the key.
Only reductions are built (h_out <= h_in, w_out <= w_in, the reference's own assertion).
"""
from __future__ import annotations

import ctypes as C
import functools
import math

import numpy as np
import torch
from torch import Tensor

from ... import _lib as L

MIRROR_KEY = "mirror"      # views[MIRROR_KEY]: uint8 [*batch], 1 = mirror this view left-right in the crop shim
PRECISION_BITS = 22        # PIL's 8-bit resample: 32 - 8 - 2
MAX_TAPS = L.VSP_MAX_TAPS  # the tap limit and the layout codes are include/vicasplat_data.h's
LAYOUT_U8_HWC, LAYOUT_U8_CHW, LAYOUT_F32_CHW = L.VSP_LAYOUT_U8_HWC, L.VSP_LAYOUT_U8_CHW, L.VSP_LAYOUT_F32_CHW


def _sinc(x: float) -> float:
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x: float) -> float:
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


def check_overflow(k: np.ndarray) -> None:
    """Raise unless every row of the fixed-point table k [out, ksize] keeps the kernel's int32 sums safe: 255 sum|k| + 2^21 < 2^31."""
    worst = int(np.abs(k.astype(np.int64)).sum(axis=1).max()) if k.size else 0
    if 255 * worst + (1 << (PRECISION_BITS - 1)) >= 1 << 31:
        raise OverflowError(f"resample table: sum|k| = {worst} = {worst / (1 << PRECISION_BITS):.3f} x 2^{PRECISION_BITS} overflows the int32 accumulator")


@functools.lru_cache(maxsize=None)
def resample_tables(in_size: int, out_size: int) -> tuple[np.ndarray, np.ndarray]:
    """(bounds [out, 2] int32 = (xmin, n), k [out, ksize] int32) of PIL's 8-bit Lanczos reduction of one axis from in_size to out_size
    samples (out_size <= in_size): precompute_coeffs and normalize_coeffs_8bpc of PIL's Resample.c restated, float64, with math.sin -- the C
    library's sin that PIL calls.  The taps past n are zero.  Cached per (in_size, out_size); the arrays are read-only."""
    if not 1 <= out_size <= in_size:
        raise ValueError(f"resample_tables: only reductions are built, got {in_size} -> {out_size}")
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 3.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    if ksize > MAX_TAPS:
        raise ValueError(f"resample_tables: {in_size} -> {out_size} needs {ksize} taps, the kernel takes at most {MAX_TAPS}")
    ss = 1.0 / filterscale
    bounds = np.zeros((out_size, 2), np.int32)
    k = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        n = xmax - xmin
        w = [_lanczos((x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(n):
            v = w[x] / ww if ww != 0.0 else w[x]
            k[xx, x] = int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5)
        bounds[xx] = (xmin, n)
    check_overflow(k)
    bounds.setflags(write=False)
    k.setflags(write=False)
    return bounds, k


_device_tables: dict = {}


def _tables_on(in_size: int, out_size: int, dev: torch.device):
    """(bounds, k, ksize) on the device, uploaded once per (in, out, device); (None, None, 0) for a pass that is skipped."""
    if in_size == out_size:
        return None, None, 0
    key = (in_size, out_size, dev)
    if key not in _device_tables:
        bounds, k = resample_tables(in_size, out_size)
        _device_tables[key] = (torch.from_numpy(bounds.copy()).to(dev), torch.from_numpy(k.copy()).to(dev), k.shape[1])
    return _device_tables[key]


def scaled_size(h_in: int, w_in: int, shape: tuple[int, int]) -> tuple[int, int]:
    """The reference's intermediate size (rescale_and_crop), with its assertions."""
    h_out, w_out = shape
    assert h_out <= h_in and w_out <= w_in
    scale_factor = max(h_out / h_in, w_out / w_in)
    h_scaled = round(h_in * scale_factor)
    w_scaled = round(w_in * scale_factor)
    assert h_scaled == h_out or w_scaled == w_out
    return h_scaled, w_scaled


def _floats3(v, name: str):
    t = [float(x) for x in (v.tolist() if isinstance(v, Tensor) else (v if isinstance(v, (tuple, list)) else (v, v, v)))]
    if len(t) != 3:
        raise ValueError(f"normalize: {name} must be one value or three, got {v!r}")
    return (C.c_float * 3)(*t)


def _frames(image: Tensor):
    """(tensor whose memory the kernel reads, layout code, batch shape, h, w) of an image [*, 3, h, w]."""
    if image.dim() < 3 or image.shape[-3] != 3:
        raise ValueError(f"the crop shim takes images [*, 3, h, w], got {tuple(image.shape)}")
    if image.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"the crop shim takes uint8 or float32 images, got {image.dtype}")
    *batch, _, h, w = image.shape
    x = image.detach().reshape(-1, 3, h, w)
    n = x.shape[0]
    sn, sc, sh, sw = x.stride()
    if x.dtype == torch.uint8 and (sc, sh, sw) == (1, 3 * w, 3) and (n <= 1 or sn == 3 * h * w):
        return x, LAYOUT_U8_HWC, batch, h, w
    if not ((sc, sh, sw) == (h * w, w, 1) and (n <= 1 or sn == 3 * h * w)):
        x = x.contiguous()
    return x, (LAYOUT_U8_CHW if x.dtype == torch.uint8 else LAYOUT_F32_CHW), batch, h, w


def _resample(image: Tensor, h_scaled: int, w_scaled: int, row: int, col: int, h_out: int, w_out: int, mirror: Tensor | None = None,
              normalize=None) -> Tensor:
    """One launch: the window (row, col, h_out, w_out) of the image reduced to h_scaled x w_scaled, float32 [*, 3, h_out, w_out]."""
    dev = L.require_device(image, mirror)
    if dev is None:
        raise RuntimeError("vicasplat_amd kernels need HIP device tensors (got a CPU tensor); there is no CPU fallback")
    x, layout, batch, h, w = _frames(image)
    n = x.shape[0]
    if mirror is not None:
        if tuple(mirror.shape) != tuple(batch):
            raise ValueError(f"the mirror flags must have the images' batch shape {tuple(batch)}, got {tuple(mirror.shape)}")
        mirror = mirror.to(torch.uint8).reshape(-1).contiguous()
    bx, kx_t, kx = _tables_on(w, w_scaled, dev)
    by, ky_t, ky = _tables_on(h, h_scaled, dev)
    mean = std = None
    if normalize is not None:
        mean, std = _floats3(normalize[0], "mean"), _floats3(normalize[1], "std")
    out = torch.empty(n, 3, h_out, w_out, dtype=torch.float32, device=dev)
    if n > 0:       # (an empty tensor has no address to hand over)
        L.call("vsp_rescale_crop", dev, L.ptr(x), layout, n, h, w, L.ptr(bx), L.ptr(kx_t), w_scaled, kx, L.ptr(by), L.ptr(ky_t), h_scaled, ky,
               row, col, h_out, w_out, L.ptr(mirror), mean, std, L.ptr(out))
    return out.reshape(*batch, 3, h_out, w_out)


def rescale(image: Tensor, shape: tuple[int, int], *, mirror: Tensor | None = None, normalize=None) -> Tensor:
    """image [*, 3, h_in, w_in] -> [*, 3, h, w] float32: the reference's rescale (uint8 round trip through PIL's LANCZOS resize, / 255)."""
    h, w = shape
    return _resample(image, h, w, 0, 0, h, w, mirror, normalize)


def _corrected_intrinsics(intrinsics: Tensor, h_in: int, w_in: int, h_out: int, w_out: int) -> Tensor:
    intrinsics = intrinsics.clone()
    intrinsics[..., 0, 0] *= w_in / w_out  # fx
    intrinsics[..., 1, 1] *= h_in / h_out  # fy
    return intrinsics


def center_crop(images: Tensor, intrinsics: Tensor, shape: tuple[int, int]) -> tuple[Tensor, Tensor]:
    """The reference's center_crop: the centre window of the images (a view) and the intrinsics corrected for it, on the images' device."""
    *_, h_in, w_in = images.shape
    h_out, w_out = shape
    row = (h_in - h_out) // 2
    col = (w_in - w_out) // 2
    images = images[..., :, row: row + h_out, col: col + w_out]
    return images, _corrected_intrinsics(intrinsics, h_in, w_in, h_out, w_out)


def rescale_and_crop(images: Tensor, intrinsics: Tensor, shape: tuple[int, int], *, mirror: Tensor | None = None,
                     normalize=None) -> tuple[Tensor, Tensor]:
    """The reference's rescale_and_crop in one launch: only the crop window of the scaled image is computed."""
    *_, h_in, w_in = images.shape
    h_out, w_out = shape
    h_scaled, w_scaled = scaled_size(h_in, w_in, shape)
    row = (h_scaled - h_out) // 2
    col = (w_scaled - w_out) // 2
    out = _resample(images, h_scaled, w_scaled, row, col, h_out, w_out, mirror, normalize)
    return out, _corrected_intrinsics(intrinsics, h_scaled, w_scaled, h_out, w_out)


def apply_crop_shim_to_views(views: dict, shape: tuple[int, int], *, normalize=None) -> dict:
    views = dict(views)
    mirror = views.pop(MIRROR_KEY, None)
    images, intrinsics = rescale_and_crop(views["image"], views["intrinsics"], shape, mirror=mirror, normalize=normalize)
    return {
        **views,
        "image": images,
        "intrinsics": intrinsics,
    }


def apply_crop_shim(example: dict, shape: tuple[int, int], *, normalize_context=None) -> dict:
    """Crop images in the example."""
    return {
        **example,
        "context": apply_crop_shim_to_views(example["context"], shape, normalize=normalize_context),
        "target": apply_crop_shim_to_views(example["target"], shape),
    }
