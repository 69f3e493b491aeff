"""The argument conventions of the reference's src/visualization/drawing/types.py: a vector, a scalar or a pair may be given as a number,
a nested list or a tensor, and comes back as an f32 tensor on the device, ready to broadcast over the primitives."""
from __future__ import annotations

import torch
from torch import Tensor


def _as_f32(value, device) -> Tensor:
    if isinstance(value, Tensor):
        return value.type(torch.float32).to(device)
    return torch.tensor(value, dtype=torch.float32, device=device)


def sanitize_vector(vector, dim: int, device) -> Tensor:
    """-> [n or 1, dim]: a number or a [.., 1] value is repeated over the `dim` components, a [dim] value becomes one row."""
    v = _as_f32(vector, device)
    while v.ndim < 2:
        v = v[None]
    if v.shape[-1] == 1:
        v = v.expand(*v.shape[:-1], dim)
    assert v.ndim == 2 and v.shape[-1] == dim, f"expected [n, {dim}], got {tuple(v.shape)}"
    return v


def sanitize_scalar(scalar, device) -> Tensor:
    """-> [n or 1]."""
    s = _as_f32(scalar, device)
    while s.ndim < 1:
        s = s[None]
    assert s.ndim == 1, f"expected [n], got {tuple(s.shape)}"
    return s


def sanitize_pair(pair, device) -> Tensor:
    """-> [2]."""
    p = _as_f32(pair, device)
    assert tuple(p.shape) == (2,), f"expected a pair, got {tuple(p.shape)}"
    return p
