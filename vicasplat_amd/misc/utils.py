"""vis_depth_map, confidence_map and inverse_normalize of the reference's src/misc/utils.py:6-35, on the device.

The reference takes two torch.quantile sorts, a log, a host copy for matplotlib and a copy back; here the range is a radix selection
(ops.depth_range) and the colours one lookup kernel (ops.color_map), both on the current stream with no host copy.  A tensor of more than
16 000 000 values raises (the reference slices the first 16 000 000; that slice of the positives is not built).
"""
from __future__ import annotations

import torch
from torch import Tensor

from .. import _lib as L
from .. import ops
from ..visualization.color_map import device_table


def inverse_normalize(tensor: Tensor, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)) -> Tensor:
    """tensor [..., C, H, W] * std + mean, per channel: undoes a (x - mean) / std normalisation."""
    scale, shift = (tensor.new_tensor(v).reshape(-1, 1, 1) for v in (std, mean))
    return tensor * scale + shift

def vis_depth_map(result: Tensor) -> Tensor:
    """result [*batch, H, W] f32 depths -> [*batch, 3, H, W] f32 `turbo` colours of 1 - (log d - near) / (far - near), near and far the
    logs of the 1 % quantile of the positive depths and of the 99 % quantile of all of them."""
    value = result.detach().float().contiguous()
    return ops.color_map(value, device_table("turbo", value.device), L.VSV_MODE_DEPTH, ops.depth_range(value))


def confidence_map(result: Tensor) -> Tensor:
    """result [*batch, H, W] f32 -> [*batch, 3, H, W] f32 `magma` colours of result / max(result)."""
    value = result.detach().float().contiguous()
    return ops.color_map(value, device_table("magma", value.device), L.VSV_MODE_MAX)


def get_overlap_tag(overlap) -> str:
    """The overlap class of an evaluation-index entry (src/misc/utils.py:38-48): "small" for [0.05, 0.3], "medium" up to 0.55, "large" up to
    0.8, else "ignore" (an overlap below 0.05 falls through to "medium", as it does in the reference)."""
    if 0.05 <= overlap <= 0.3:
        overlap_tag = "small"
    elif overlap <= 0.55:
        overlap_tag = "medium"
    elif overlap <= 0.8:
        overlap_tag = "large"
    else:
        overlap_tag = "ignore"

    return overlap_tag
