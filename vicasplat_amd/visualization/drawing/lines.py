"""draw_lines of the reference's src/visualization/drawing/lines.py: antialiased line segments over an image, the highest-indexed line on
top.  Arguments broadcast as the reference's do (types.py) and are given in world coordinates, mapped onto the image by x_range / y_range
(coordinate_conversion.py); that mapping is a torch expression on the handful of primitives in both backends.

backend "hip" (the default for an image on a HIP device): one launch of vsg_draw_lines (csrc/draw.hip), num_msaa_passes 0 or 1.
backend "torch" (the default for a CPU image): the reference's algorithm in torch ops (rendering.py), any number of passes.

Besides image [3, H, W] both take image [B, 3, H, W]: start, end, color, width, x_range and y_range may then each be a list of B per-image
values (or one value shared by all), and the whole batch is one launch.  Stated deviations from the reference (include/vicasplat_draw.h):
an image with no lines is returned unchanged instead of raising, and a line with a NaN in its geometry covers nothing.
"""
from __future__ import annotations

import torch
from torch import Tensor

from .coordinate_conversion import generate_conversions
from .rendering import render_over_image, topmost
from .types import sanitize_scalar, sanitize_vector

CAPS = ("butt", "round", "square")


def pick_backend(image: Tensor, backend) -> str:
    backend = backend or ("hip" if image.is_cuda else "torch")
    if backend not in ("hip", "torch"):
        raise ValueError(f"backend {backend!r} is neither 'hip' nor 'torch'")
    return backend


def per_image(value, batch: int) -> list:
    """A `list` of `batch` tensors, lists, tuples or Nones is one value per image; anything else (a number, a tensor, a tuple, a list of
    numbers) is shared by all images."""
    if isinstance(value, list) and len(value) == batch and all(isinstance(v, (Tensor, list, tuple)) or v is None for v in value):
        return list(value)
    return [value] * batch


def offsets_of(counts: list, device) -> Tensor:
    """prim_offsets [B + 1] int32 from the per-image counts (shapes: known on the host)."""
    total, offs = 0, [0]
    for c in counts:
        total += int(c)
        offs.append(total)
    return torch.tensor(offs, dtype=torch.int32, device=device)


def line_records(shape, device, start, end, color, width, x_range, y_range) -> Tensor:
    """[n, 8] f32: start x, y, end x, y (pixel space), width, r, g, b -- the record of include/vicasplat_draw.h."""
    start, end = sanitize_vector(start, 2, device), sanitize_vector(end, 2, device)
    color, width = sanitize_vector(color, 3, device), sanitize_scalar(width, device)
    (n,) = torch.broadcast_shapes((start.shape[0],), (end.shape[0],), (color.shape[0],), tuple(width.shape))
    world_to_pixel, _ = generate_conversions(shape, device, x_range, y_range)
    return torch.cat((world_to_pixel(start).expand(n, 2), world_to_pixel(end).expand(n, 2), width.expand(n)[:, None], color.expand(n, 3)), dim=1)


def line_coverage(rec: Tensor, xy: Tensor, cap: str) -> Tensor:
    """[n, samples] bool: which of the samples xy [samples, 2] each line record covers, in the reference's f32 operations."""
    start, end, width = rec[:, 0:2], rec[:, 2:4], rec[:, 4]
    delta = end - start
    length = delta.norm(dim=-1, keepdim=True)
    unit = delta / length
    rel = xy - start[:, None]
    half = 0.5 * width[:, None]
    extra = half if cap == "square" else 0
    along = torch.einsum("lc,lsc->ls", unit, rel)
    across = rel - along[..., None] * unit[:, None]
    inside = (along <= length + extra) & (along > -extra) & (across.norm(dim=-1) < half)
    if cap == "round":
        inside = inside | (rel.norm(dim=-1) < half) | ((xy - end[:, None]).norm(dim=-1) < half)
    return inside & ~rec[:, :5].isnan().any(dim=1)[:, None]      # a NaN in the geometry covers nothing


def _draw_torch(image: Tensor, rec: Tensor, cap: str, num_passes: int) -> Tensor:
    if rec.shape[0] == 0:
        return image.clone()
    return render_over_image(image, lambda xy: topmost(line_coverage(rec, xy, cap), rec[:, 5:8]), image.device, num_passes=num_passes)


def draw_lines(image: Tensor, start, end, color, width, cap: str = "round", num_msaa_passes: int = 1, x_range=None, y_range=None, *,
               backend: str | None = None) -> Tensor:
    """-> a new tensor of the image's shape, [3, H, W] or [B, 3, H, W]."""
    if cap not in CAPS:
        raise ValueError(f"cap {cap!r} is none of {CAPS}")
    backend = pick_backend(image, backend)
    batched = image.dim() == 4
    images = image if batched else image[None]
    if images.dim() != 4 or images.shape[1] != 3:
        raise ValueError(f"draw_lines takes an image [3, H, W] or [B, 3, H, W], got {tuple(image.shape)}")
    B, _, h, w = images.shape
    args = [per_image(v, B) if batched else [v] for v in (start, end, color, width, x_range, y_range)]
    recs = [line_records((h, w), images.device, *(a[b] for a in args)) for b in range(B)]
    if backend == "torch":
        out = torch.stack([_draw_torch(images[b].float(), recs[b], cap, num_msaa_passes) for b in range(B)])
    else:
        from ... import ops
        out = ops.draw_lines(images.float().contiguous(), torch.cat(recs).contiguous(), offsets_of([r.shape[0] for r in recs], images.device),
                             cap=cap, num_passes=num_msaa_passes)
    return out if batched else out[0]
