"""The wobble of the reference's src/visualization/camera_trajectory/wobble.py: a camera moved on a circle in its own image plane."""
from __future__ import annotations

import torch
from torch import Tensor


@torch.no_grad()
def generate_wobble_transformation(radius: Tensor, t: Tensor, num_rotations: int = 1, scale_radius_with_t: bool = True) -> Tensor:
    """radius [*batch], t [steps] -> [*batch, steps, 4, 4]: the identity with the translation r (sin a, -cos a, 0), a = 2 pi
    num_rotations t, and r = radius t (the circle opens as a spiral) or radius."""
    tf = torch.eye(4, dtype=torch.float32, device=t.device).repeat(*radius.shape, t.shape[0], 1, 1)
    r = radius[..., None] * t if scale_radius_with_t else radius[..., None]
    angle = 2 * torch.pi * num_rotations * t
    tf[..., 0, 3] = torch.sin(angle) * r
    tf[..., 1, 3] = -torch.cos(angle) * r
    return tf


@torch.no_grad()
def generate_wobble(extrinsics: Tensor, radius: Tensor, t: Tensor) -> Tensor:
    """extrinsics [*batch, 4, 4] -> [*batch, steps, 4, 4]: each pose followed by the wobble in its camera frame."""
    return extrinsics[..., None, :, :] @ generate_wobble_transformation(radius, t)
