"""Colour maps on the GPU (the reference's src/visualization/color_map.py:9-27, without its host round trip).

The reference clips x to [0, 1], copies it to the host, calls matplotlib's Colormap and copies an f32 image three times as large back.
For a listed colour map that call is a pure lookup, idx = min(trunc(x * 256), 255) into 256 colours, with (0, 0, 0) for a NaN: here the
table lives on the device (color_tables.py, data written by gen_color_tables.py from matplotlib; matplotlib is not imported at run time) and
csrc/viz.hip does the lookup.  Only `turbo` and `magma` -- the two the reference's callers use -- are built.
"""
from __future__ import annotations

import numpy as np
import torch
from torch import Tensor

from .. import _lib as L
from .. import ops

COLOR_MAPS = ("turbo", "magma")
_host: dict = {}
_device: dict = {}


def color_table(color_map: str) -> np.ndarray:
    """The [256, 3] f32 table of `turbo` or `magma` on the host."""
    if color_map not in COLOR_MAPS:
        raise NotImplementedError(f"colour map {color_map!r} is not built: only 'turbo' and 'magma' are")
    if not _host:
        from .color_tables import TABLES
        _host.update({name: np.array(TABLES[name], dtype=np.float32) for name in COLOR_MAPS})
    return _host[color_map]


def device_table(color_map: str, device) -> Tensor:
    """The table on `device`: uploaded once per device and kept."""
    table = color_table(color_map)
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (color_map, device)
    if key not in _device:
        _device[key] = torch.from_numpy(table).to(device)
    return _device[key]


def apply_color_map_to_image(image: Tensor, color_map: str = "inferno") -> Tensor:
    """image [*batch, H, W] -> [*batch, 3, H, W] f32: lut[min(trunc(clip(x, 0, 1) * 256), 255)], (0, 0, 0) for a NaN."""
    if image.dim() < 2:
        raise ValueError(f"apply_color_map_to_image takes [*batch, H, W], got {tuple(image.shape)}")
    table = device_table(color_map, image.device)
    return ops.color_map(image.detach().float().contiguous(), table, L.VSV_MODE_UNIT)


def apply_color_map(x: Tensor, color_map: str = "inferno") -> Tensor:
    """x [*batch] -> [*batch, 3] f32 (the same lookup, colours last)."""
    planes = apply_color_map_to_image(x.reshape(1, -1), color_map)      # [3, 1, n]
    return planes.reshape(3, -1).t().reshape(*x.shape, 3).contiguous()
