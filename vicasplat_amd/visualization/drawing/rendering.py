"""The sampling scheme of the reference's src/visualization/drawing/rendering.py in torch ops: the `torch` backend of draw_lines and
draw_points, on whatever device the image is on and for any number of refinement passes.  The HIP kernel (csrc/draw.hip) does the same work
for 0 or 1 passes in one launch; include/vicasplat_draw.h states the arithmetic both follow.

A colour function maps samples [n, 2] to straight-alpha RGBA [n, 4].  Pass 0 samples the pixel centres; every further pass looks for the
pixels whose RGBA differs from that of a neighbour inside the image, samples those on a `subdivision` x `subdivision` grid and replaces
them by the alpha-weighted mean colour and the mean alpha of the grid.
"""
from __future__ import annotations

import torch
from torch import Tensor

SUBDIVISION = 8
SAMPLES_PER_CALL = 1 << 16      # the colour function sees at most this many samples at once: it bounds the primitives x samples temporaries


def generate_sample_grid(shape, device) -> Tensor:
    """[h, w, 2]: the centres (x + 0.5, y + 0.5) of an h x w grid."""
    h, w = shape
    ys, xs = torch.meshgrid(torch.arange(h, device=device) + 0.5, torch.arange(w, device=device) + 0.5, indexing="ij")
    return torch.stack((xs, ys), dim=-1)


def detect_msaa_pixels(rgba: Tensor) -> Tensor:
    """rgba [b, 4, h, w] -> [b, h, w] bool: true where any channel differs from that of one of the up to eight neighbours.  A pixel at the
    border has no neighbours beyond it."""
    b, _, h, w = rgba.shape
    mask = torch.zeros((b, h, w), dtype=torch.bool, device=rgba.device)
    # each unordered pair of neighbours once, by the offset (dy, dx) from the first to the second; both ends of a differing pair are marked
    for dy, dx in ((0, 1), (1, 0), (1, 1), (1, -1)):
        rows_a, rows_b = slice(0, h - dy), slice(dy, h)
        cols_a, cols_b = (slice(0, w - 1), slice(1, w)) if dx > 0 else (slice(1, w), slice(0, w - 1)) if dx < 0 else (slice(0, w), slice(0, w))
        differs = (rgba[:, :, rows_a, cols_a] != rgba[:, :, rows_b, cols_b]).any(dim=1)
        mask[:, rows_a, cols_a] |= differs
        mask[:, rows_b, cols_b] |= differs
    return mask


def reduce_straight_alpha(rgba: Tensor) -> Tensor:
    """rgba [n, 4, s, s] -> [n, 4]: colour = sum(c a) / (sum(a) + 1e-10), alpha = mean(a)."""
    colour, alpha = rgba[:, :3], rgba[:, 3:]
    weighted = (colour * alpha).sum(dim=(2, 3))
    return torch.cat((weighted / (alpha.sum(dim=(2, 3)) + 1e-10), alpha.mean(dim=(2, 3))), dim=-1)


@torch.no_grad()
def run_msaa_pass(xy: Tensor, color_function, scale: float, subdivision: int, remaining_passes: int) -> Tensor:
    """xy [b, h, w, 2] -> RGBA [b, 4, h, w]."""
    b, h, w, _ = xy.shape
    flat = xy.reshape(-1, 2)
    rgba = torch.cat([color_function(part) for part in flat.split(SAMPLES_PER_CALL)], dim=0) if flat.shape[0] else flat.new_zeros(0, 4)
    rgba = rgba.reshape(b, h, w, 4).permute(0, 3, 1, 2).contiguous()
    if remaining_passes > 0:
        which = torch.where(detect_msaa_pixels(rgba))      # (reads the mask back: the torch backend waits for the device here)
        if which[0].numel():
            bi, yi, xi = which
            offsets = (generate_sample_grid((subdivision, subdivision), xy.device) / subdivision - 0.5) * scale
            fine = run_msaa_pass(xy[bi, yi, xi][:, None, None] + offsets, color_function, scale / subdivision, subdivision, remaining_passes - 1)
            rgba[bi, :, yi, xi] = reduce_straight_alpha(fine)
    return rgba


@torch.no_grad()
def render(shape, color_function, device, subdivision: int = SUBDIVISION, num_passes: int = 2) -> Tensor:
    """-> RGBA [4, h, w] with straight alpha."""
    return run_msaa_pass(generate_sample_grid(shape, device)[None], color_function, 1.0, subdivision, num_passes)[0]


def render_over_image(image: Tensor, color_function, device, subdivision: int = SUBDIVISION, num_passes: int = 1) -> Tensor:
    """image [3, h, w] with the rendered layer blended over it: image (1 - alpha) + colour alpha."""
    overlay = render(image.shape[-2:], color_function, device, subdivision=subdivision, num_passes=num_passes)
    colour, alpha = overlay[:3], overlay[3:]
    return image * (1 - alpha) + colour * alpha


def topmost(inside: Tensor, colour: Tensor) -> Tensor:
    """inside [n, samples] bool, colour [n, 3] -> RGBA [samples, 4]: the colour of the highest-indexed covering primitive and alpha 1; an
    uncovered sample has alpha 0 and, as an argmax over zeros gives, the colour of primitive 0."""
    order = torch.arange(inside.shape[0], device=inside.device)[:, None]
    top = (inside * order).argmax(dim=0)
    return torch.cat((colour[top], inside.any(dim=0).float()[:, None]), dim=-1)
