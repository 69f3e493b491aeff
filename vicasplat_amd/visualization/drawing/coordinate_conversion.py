"""World <-> pixel coordinates of the reference's src/visualization/drawing/coordinate_conversion.py: the ranges x_range and y_range of the
world map onto [0, w] and [0, h]; without a range the world is the pixel grid itself."""
from __future__ import annotations

import torch

from .types import sanitize_pair


def generate_conversions(shape, device, x_range=None, y_range=None):
    """-> (world_to_pixel, pixel_to_world), each on [..., 2] tensors: pixel = (world - lo) / (hi - lo) * (w, h), in that order of
    operations, and world = pixel / (w, h) * (hi - lo) + lo."""
    h, w = shape
    xr = sanitize_pair((0, w) if x_range is None else x_range, device)
    yr = sanitize_pair((0, h) if y_range is None else y_range, device)
    lo, hi = torch.stack((xr, yr), dim=-1)
    size = torch.tensor((w, h), dtype=torch.float32, device=device)

    def world_to_pixel(xy):
        return (xy - lo) / (hi - lo) * size

    def pixel_to_world(xy):
        return xy / size * (hi - lo) + lo

    return world_to_pixel, pixel_to_world
