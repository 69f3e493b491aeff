"""The camera plot of the reference's src/visualization/drawing/cameras.py: the cameras' frustums, and their near and far planes when
given, projected onto the three axis-aligned planes and drawn as lines.  The frustum corners, the bounding box and the line lists are
host-side torch on a few dozen elements; the drawing is draw_lines, and the three projections go out as ONE launch per layer.

Layers, in the reference's order (a later one lies on top): the near rectangles, the far rectangles, the near-to-far edges (all in grey
0.25, width 2), then per camera its four origin-to-corner edges and its image rectangle in the camera's colour.

Stated deviations: text labels need a font file, so draw_label defaults to False and True raises; the plotly figure
create_plotly_cameras_visualization is not built (callers.camera_trajectory_plot stands in for it).  The intrinsics are inverted with
torch.linalg.inv_ex, which does not wait for the device.
"""
from __future__ import annotations

import torch
from torch import Tensor

from ..validation_in_3d import compute_equal_aabb_with_margin
from .lines import draw_lines
from .types import sanitize_scalar

PLANE_GREY = 0.25
LINE_WIDTH = 2


def unproject_frustum_corners(extrinsics: Tensor, intrinsics: Tensor, depth: Tensor) -> Tensor:
    """[b, 4, 3]: the image corners (0, 0), (1, 0), (1, 1), (0, 1) -- around the rectangle -- of every camera at z-depth `depth` ([b] or [1]),
    in world space: origin + depth R (K^-1 (x, y, 1) / its z)."""
    corners = torch.tensor([[0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], dtype=torch.float32, device=extrinsics.device)
    rays = torch.einsum("bij,rj->bri", torch.linalg.inv_ex(intrinsics).inverse, corners)
    rays = rays / rays[..., -1:]
    rays = torch.einsum("bij,brj->bri", extrinsics[..., :3, :3], rays)
    return extrinsics[:, None, :3, 3] + depth[:, None, None] * rays


def compute_aabb(extrinsics: Tensor, intrinsics: Tensor, near=None, far=None) -> tuple[Tensor, Tensor]:
    """(minima [3], maxima [3]) over the camera origins and, where given, the corners of the near and far planes."""
    points = [extrinsics[:, :3, 3]]
    for depth in (near, far):
        if depth is not None:
            points.append(unproject_frustum_corners(extrinsics, intrinsics, sanitize_scalar(depth, extrinsics.device)).reshape(-1, 3))
    points = torch.cat(points, dim=0)
    return points.min(dim=0).values, points.max(dim=0).values


def camera_layers(extrinsics: Tensor, intrinsics: Tensor, color: Tensor, near, far, corner_depth: Tensor) -> list:
    """The layers as (start [n, 3], end [n, 3], colour) in world space, bottom layer first."""
    def ring(c):      # each corner joined to the one before it
        return c.reshape(-1, 3), c.roll(1, 1).reshape(-1, 3)

    layers = []
    near_c = unproject_frustum_corners(extrinsics, intrinsics, near) if near is not None else None
    far_c = unproject_frustum_corners(extrinsics, intrinsics, far) if far is not None else None
    if near_c is not None:
        layers.append((*ring(near_c), PLANE_GREY))
    if far_c is not None:
        layers.append((*ring(far_c), PLANE_GREY))
    if near_c is not None and far_c is not None:
        layers.append((near_c.reshape(-1, 3), far_c.reshape(-1, 3), PLANE_GREY))
    b = extrinsics.shape[0]
    frustum = unproject_frustum_corners(extrinsics, intrinsics, corner_depth)
    origins = extrinsics[:, None, :3, 3].expand(b, 4, 3)
    start = torch.stack((origins, frustum.roll(1, 1)), dim=1)                   # [b, 2 (from the origin | around the rectangle), 4, 3]
    end = frustum[:, None].expand(b, 2, 4, 3)
    layers.append((start.reshape(-1, 3), end.reshape(-1, 3), color[:, None, None, :].expand(b, 2, 4, 3).reshape(-1, 3)))
    return layers


def draw_cameras(resolution: int, extrinsics: Tensor, intrinsics: Tensor, color: Tensor, near=None, far=None, margin: float = 0.1,
                 frustum_scale: float = 0.05, draw_label: bool = False, *, backend: str | None = None) -> Tensor:
    """-> [3 (projection along x, y, z), 3, resolution, resolution] f32.  extrinsics [b, 4, 4] camera-to-world, intrinsics [b, 3, 3]
    normalised, color [b, 3]; near, far: numbers or [b]."""
    if draw_label:
        raise NotImplementedError("draw_cameras(draw_label=True): text labels are not built (no font file); pass draw_label=False")
    device = extrinsics.device
    extrinsics, intrinsics = extrinsics.float(), intrinsics.float()
    near = None if near is None else sanitize_scalar(near, device)
    far = None if far is None else sanitize_scalar(far, device)
    lo, hi = compute_equal_aabb_with_margin(*compute_aabb(extrinsics, intrinsics, near, far), margin=margin)
    corner_depth = ((hi - lo).max() * frustum_scale)[None]
    layers = camera_layers(extrinsics, intrinsics, color.float(), near, far, corner_depth)
    # projection k looks along axis k: the image's x is axis k + 1, its y axis k + 2
    planes = [[(k + 1) % 3, (k + 2) % 3] for k in range(3)]
    x_range = [torch.stack((lo[p[0]], hi[p[0]])) for p in planes]
    y_range = [torch.stack((lo[p[1]], hi[p[1]])) for p in planes]
    image = torch.zeros((3, 3, resolution, resolution), dtype=torch.float32, device=device)
    for start, end, col in layers:
        image = draw_lines(image, [start[:, p] for p in planes], [end[:, p] for p in planes], col, LINE_WIDTH, x_range=x_range, y_range=y_range,
                           backend=backend)
    return image
