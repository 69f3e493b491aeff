"""draw_points of the reference's src/visualization/drawing/points.py: discs or rings (inner_radius <= distance <= radius, both ends
inclusive) over an image, the highest-indexed point on top.  Backends, batching and the stated deviations are those of lines.py; the HIP
path is one launch of vsg_draw_points (csrc/draw.hip)."""
from __future__ import annotations

import torch
from torch import Tensor

from .coordinate_conversion import generate_conversions
from .lines import offsets_of, per_image, pick_backend
from .rendering import render_over_image, topmost
from .types import sanitize_scalar, sanitize_vector


def point_records(shape, device, points, color, radius, inner_radius, x_range, y_range) -> Tensor:
    """[n, 7] f32: x, y (pixel space), radius, inner radius, r, g, b -- the record of include/vicasplat_draw.h."""
    points, color = sanitize_vector(points, 2, device), sanitize_vector(color, 3, device)
    radius, inner = sanitize_scalar(radius, device), sanitize_scalar(inner_radius, device)
    (n,) = torch.broadcast_shapes((points.shape[0],), (color.shape[0],), tuple(radius.shape), tuple(inner.shape))
    world_to_pixel, _ = generate_conversions(shape, device, x_range, y_range)
    return torch.cat((world_to_pixel(points).expand(n, 2), radius.expand(n)[:, None], inner.expand(n)[:, None], color.expand(n, 3)), dim=1)


def point_coverage(rec: Tensor, xy: Tensor) -> Tensor:
    """[n, samples] bool."""
    distance = (xy[None] - rec[:, None, 0:2]).norm(dim=-1)
    return (distance >= rec[:, 3:4]) & (distance <= rec[:, 2:3])


def _draw_torch(image: Tensor, rec: Tensor, num_passes: int) -> Tensor:
    if rec.shape[0] == 0:
        return image.clone()
    return render_over_image(image, lambda xy: topmost(point_coverage(rec, xy), rec[:, 4:7]), image.device, num_passes=num_passes)


def draw_points(image: Tensor, points, color=(1, 1, 1), radius=1, inner_radius=0, num_msaa_passes: int = 1, x_range=None, y_range=None, *,
                backend: str | None = None) -> Tensor:
    """-> a new tensor of the image's shape, [3, H, W] or [B, 3, H, W]."""
    backend = pick_backend(image, backend)
    batched = image.dim() == 4
    images = image if batched else image[None]
    if images.dim() != 4 or images.shape[1] != 3:
        raise ValueError(f"draw_points takes an image [3, H, W] or [B, 3, H, W], got {tuple(image.shape)}")
    B, _, h, w = images.shape
    args = [per_image(v, B) if batched else [v] for v in (points, color, radius, inner_radius, x_range, y_range)]
    recs = [point_records((h, w), images.device, *(a[b] for a in args)) for b in range(B)]
    if backend == "torch":
        out = torch.stack([_draw_torch(images[b].float(), recs[b], num_msaa_passes) for b in range(B)])
    else:
        from ... import ops
        out = ops.draw_points(images.float().contiguous(), torch.cat(recs).contiguous(), offsets_of([r.shape[0] for r in recs], images.device),
                              num_passes=num_msaa_passes)
    return out if batched else out[0]
