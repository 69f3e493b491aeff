"""Image layout on the device: hcat, vcat, cat and add_border with the semantics of the reference's src/visualization/layout.py.

Images are f32 [C, H, W].  `cat` lines images up along one axis: each is first set into a canvas of the gap colour as long, across the
line, as the longest image (at the start, the centre -- the smaller half of the slack first -- or the end), and `gap` rows or columns of the
gap colour go between neighbours.  Plain torch: a handful of small copies per validation step, not a hot path.  A gap colour given as a
number or a list costs no device access; one given as a device tensor is read back to the host (`.tolist()`), which waits for the device.
"""
from __future__ import annotations

from typing import Iterable

import torch
from torch import Tensor

_ALIGN = {"start": "start", "center": "center", "end": "end", "top": "start", "bottom": "end", "left": "start", "right": "end"}


def _color(color, device) -> Tensor:
    if isinstance(color, Tensor):
        color = color.tolist()
    color = list(color) if isinstance(color, Iterable) else [color]
    return torch.tensor(color, dtype=torch.float32, device=device)


def _canvas(c: int, h: int, w: int, color: Tensor) -> Tensor:
    return torch.ones(c, h, w, dtype=torch.float32, device=color.device) * color[:, None, None]


def cat(main_axis: str, *images: Tensor, align: str = "center", gap: int = 8, gap_color=1) -> Tensor:
    """main_axis "horizontal" joins along the width, "vertical" along the height; align places an image across that axis."""
    main = {"horizontal": 2, "vertical": 1}[main_axis]
    cross = 3 - main
    device = images[0].device
    color = _color(gap_color, device)
    longest = max(im.shape[cross] for im in images)
    parts = []
    for k, im in enumerate(images):
        if k and gap > 0:
            shape = [images[0].shape[0], gap, gap]
            shape[cross] = longest
            parts.append(_canvas(*shape, color))
        shape = list(im.shape)
        shape[cross] = longest
        slack = longest - im.shape[cross]
        at = {"start": 0, "center": slack // 2, "end": slack}[align]
        canvas = _canvas(*shape, color)
        canvas.narrow(cross, at, im.shape[cross]).copy_(im)
        parts.append(canvas)
    return torch.cat(parts, dim=main)


def hcat(*images: Tensor, align: str = "start", gap: int = 8, gap_color=1) -> Tensor:
    return cat("horizontal", *images, align=_ALIGN[align], gap=gap, gap_color=gap_color)


def vcat(*images: Tensor, align: str = "start", gap: int = 8, gap_color=1) -> Tensor:
    return cat("vertical", *images, align=_ALIGN[align], gap=gap, gap_color=gap_color)


def add_border(image: Tensor, border: int = 8, color=1) -> Tensor:
    c, h, w = image.shape
    out = _canvas(c, h + 2 * border, w + 2 * border, _color(color, image.device))
    out[:, border:h + border, border:w + border] = image
    return out
