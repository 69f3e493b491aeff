"""render_projections of the reference's src/visualization/validation_in_3d.py:25-97 with compute_equal_aabb_with_margin
(src/visualization/drawing/cameras.py:272-284): the scene's Gaussians seen along the three axes through render_cuda_orthographic; and
render_cameras (:100-122): the context cameras (white) and the target cameras (red) of scene 0 as a camera plot (drawing/cameras.py).

Stated deviation: text labels need a font file that is not available, so draw_label defaults to False here (True in the reference) and
draw_label=True raises.  The three projections have one size, so the reference's padding to a common shape is the identity.
"""
from __future__ import annotations

import torch
from torch import Tensor

from ..model.decoder.cuda_splatting import render_cuda_orthographic
from ..model.types import Gaussians


def compute_equal_aabb_with_margin(minima: Tensor, maxima: Tensor, margin: float = 0.1) -> tuple[Tensor, Tensor]:
    """A cube around each box's centre whose side is the largest extent over everything given (all scenes, all axes) times 1 + margin."""
    half_side = 0.5 * ((maxima - minima).max() * (1 + margin))
    centre = (maxima + minima) * 0.5
    return centre - half_side, centre + half_side

def render_projections(gaussians: Gaussians, resolution: int, margin: float = 0.1, draw_label: bool = False, extra_label: str = "") -> Tensor:
    """-> [batch, 3 (look axis x, y, z), 3, resolution, resolution]."""
    if draw_label:
        raise NotImplementedError("render_projections(draw_label=True): text labels are not built (no font file); pass draw_label=False")
    means, covs, shs, opac = gaussians.means, gaussians.covariances, gaussians.harmonics, gaussians.opacities
    if means.ndim > 3:
        means, covs, shs, opac = means.flatten(1, 3), covs.flatten(1, 3), shs.flatten(1, 3), opac.flatten(1)
    b = means.shape[0]
    box_lo, box_hi = compute_equal_aabb_with_margin(means.min(dim=1).values, means.max(dim=1).values, margin=margin)
    side, centre = box_hi - box_lo, 0.5 * (box_lo + box_hi)
    black = means.new_zeros(b, 3, dtype=torch.float32)
    views = []
    for look in range(3):
        # camera axes (x, y, z) = world axes (look + 1, look + 2, look): a cyclic permutation matrix as the rotation; the camera sits on
        # the box's face look = box_lo, centred in the other two axes, and sees the box's whole depth from 0 to `side`
        axes = [(look + 1) % 3, (look + 2) % 3, look]
        pose = means.new_zeros(b, 4, 4, dtype=torch.float32)
        pose[:, axes, [0, 1, 2]] = 1
        pose[:, :3, 3] = centre
        pose[:, look, 3] = box_lo[:, look]
        pose[:, 3, 3] = 1
        views.append(render_cuda_orthographic(pose, side[:, axes[0]], side[:, axes[1]], torch.zeros_like(side[:, look]), side[:, look],
                                              (resolution, resolution), black, means, covs, shs, opac, fov_degrees=10.0))
    return torch.stack(views, dim=1)


def render_cameras(batch: dict, resolution: int) -> Tensor:
    """-> [3 (projection along x, y, z), 3, resolution, resolution]: draw_cameras over the context views, in white, followed by the target
    views, in red, of the batch's first scene, with their near and far planes."""
    from .drawing.cameras import draw_cameras      # (drawing.cameras imports this module for the AABB)
    ctx, tgt = batch["context"], batch["target"]
    n_ctx, n_tgt = ctx["extrinsics"].shape[1], tgt["extrinsics"].shape[1]
    color = torch.ones((n_ctx + n_tgt, 3), dtype=torch.float32, device=tgt["extrinsics"].device)
    color[n_ctx:, 1:] = 0
    both = lambda key: torch.cat((ctx[key][0], tgt[key][0]))
    return draw_cameras(resolution, both("extrinsics"), both("intrinsics"), color, both("near"), both("far"))
