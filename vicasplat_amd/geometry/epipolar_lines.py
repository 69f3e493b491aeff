"""View overlap: for ordered camera pairs (i -> j), how many rays of camera i have an epipolar segment that crosses the image of camera j.

This is `project_rays(...)["overlaps_image"]` of the reference's src/geometry/epipolar_lines.py:157-251 (near = far = None) over the rays of
`get_world_rays(sample_image_grid((h, w)), ...)`, the only thing src/evaluation/evaluation_index_generator.py asks of it, reduced to the closed
form that include/vicasplat_overlap.h writes out.  backend="hip" counts every pair of the list in one launch (vso_view_overlap_counts,
csrc/overlap.hip) on the current stream, with no host synchronisation; backend="torch" restates the same closed form in torch ops on any
device and in the dtype of the cameras (f32 or f64): the check of the kernel and the baseline of tools/bench_overlap.py.

One stated deviation from the reference: a pair whose origin o lies within 1e-6 of camera j takes o = 0 exactly in the
frame-line terms, so its count is the number of camera i's rays that point into image j.
"""
from __future__ import annotations

import torch
from torch import Tensor

from .. import _lib as L

EPS = 1e-6
EPS32 = float(torch.finfo(torch.float32).eps)
INFINITY = 1e8
_DTYPES = {torch.float32: 0, torch.float64: 5}     # the dtype codes of include/vicasplat_overlap.h
_TORCH_ELEMENTS = 1 << 21      # ray-pairs per slice of the torch backend


def _check(extrinsics: Tensor, intrinsics: Tensor, shape, pairs: Tensor):
    if extrinsics.dim() != 3 or tuple(extrinsics.shape[1:]) != (4, 4) or extrinsics.shape[0] < 1:
        raise ValueError(f"view_overlap_counts takes extrinsics [V, 4, 4] with V >= 1, got {tuple(extrinsics.shape)}")
    if tuple(intrinsics.shape) != (extrinsics.shape[0], 3, 3):
        raise ValueError(f"view_overlap_counts: expected intrinsics of shape {(extrinsics.shape[0], 3, 3)}, got {tuple(intrinsics.shape)}")
    if extrinsics.dtype not in _DTYPES or intrinsics.dtype != extrinsics.dtype:
        raise ValueError(f"view_overlap_counts takes f32 or f64 cameras of one dtype, got {extrinsics.dtype} and {intrinsics.dtype}")
    h, w = (int(s) for s in shape)
    if h < 1 or w < 1 or h * w > 1 << 30:
        raise ValueError(f"view_overlap_counts: the image shape must be at least 1 x 1 and at most 2^30 pixels, got {(h, w)}")
    if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"view_overlap_counts takes pairs [P, 2] of int32 or int64 indices, got {tuple(pairs.shape)} {pairs.dtype}")
    if pairs.device != extrinsics.device or intrinsics.device != extrinsics.device:
        raise ValueError("view_overlap_counts: extrinsics, intrinsics and pairs must live on one device")
    return h, w


def view_overlap_counts(extrinsics: Tensor, intrinsics: Tensor, shape, pairs: Tensor, *, backend: str | None = None) -> Tensor:
    """counts [P] int32: for each pair (i, j) of `pairs` [P, 2], the number of the h w pixel-centre rays of camera i whose epipolar segment
    overlaps the image of camera j.  extrinsics [V, 4, 4] camera-to-world and intrinsics [V, 3, 3] normalised, f32 or f64 of one dtype.
    A pair with an index outside [0, V) counts -1.  backend: "hip" (the default for device tensors) or "torch" (the default for CPU tensors)."""
    h, w = _check(extrinsics, intrinsics, shape, pairs)
    if backend is None:
        backend = "hip" if extrinsics.is_cuda else "torch"
    if backend == "torch":
        return _counts_torch(extrinsics.detach(), intrinsics.detach(), h, w, pairs)
    if backend != "hip":
        raise ValueError(f"view_overlap_counts: backend must be 'hip' or 'torch', got {backend!r}")
    dev = L.require_device(extrinsics, intrinsics, pairs)
    E, K = extrinsics.detach().contiguous(), intrinsics.detach().contiguous()
    prs = pairs.to(torch.int32).contiguous()
    P = prs.shape[0]
    if P > 2 ** 31 - 1:
        raise ValueError(f"view_overlap_counts: {P} pairs exceed 2^31 - 1")
    counts = torch.empty(P, dtype=torch.int32, device=dev)
    if P > 0:       # (an empty tensor has no address to hand over)
        L.call("vso_view_overlap_counts", dev, L.ptr(E), L.ptr(K), _DTYPES[E.dtype], E.shape[0], h, w, L.ptr(prs), P, L.ptr(counts))
    return counts


def overlap_from_counts(counts: Tensor, num_rays: int) -> Tensor:
    """counts / num_rays in f32, as torch computes `overlaps_image.float().mean()` where `counts` lives: the sum of ones is exact in f32 (up to
    2^24 rays); the CPU kernel divides it by the number of elements, the device kernel multiplies it by the f32 reciprocal of that number
    (checked against the own mean of torch 2.10 on both devices by tests/test_overlap_cpu.py and tests/test_overlap_gpu.py, which fail if a later
    torch computes its mean otherwise; the evaluation-index generator compares on the host and so takes the division)."""
    total = counts.to(torch.float32)
    if counts.is_cuda:
        return total * (torch.ones((), dtype=torch.float32) / num_rays).item()
    return total / num_rays


def view_overlap(extrinsics: Tensor, intrinsics: Tensor, shape, pairs: Tensor, *, backend: str | None = None) -> Tensor:
    """overlap [P] f32 = view_overlap_counts / (h w), computed as torch computes `overlaps_image.float().mean()` (overlap_from_counts).
    A pair with an index outside [0, V) gives a negative value."""
    h, w = (int(s) for s in shape)
    return overlap_from_counts(view_overlap_counts(extrinsics, intrinsics, shape, pairs, backend=backend), h * w)


# ---- the torch backend: the closed form of include/vicasplat_overlap.h in torch ops ------------------------------------------------------
def _adjugate(A: Tensor):
    """(adj(A), det(A)) of A [..., 3, 3], in the operation order of csrc/overlap.hip."""
    rows = []
    for r in range(3):
        c1, c2 = (r + 1) % 3, (r + 2) % 3
        rows.append(torch.stack([A[..., (c + 1) % 3, c1] * A[..., (c + 2) % 3, c2] - A[..., (c + 1) % 3, c2] * A[..., (c + 2) % 3, c1]
                                 for c in range(3)], -1))
    adj = torch.stack(rows, -2)
    det = (A[..., 0, 0] * adj[..., 0, 0] + A[..., 0, 1] * adj[..., 1, 0]) + A[..., 0, 2] * adj[..., 2, 0]
    return adj, det


def _matmul3(A: Tensor, B: Tensor) -> Tensor:
    """A B for [..., 3, 3] (or B [..., 3, 1]), each entry summed from the left."""
    return (A[..., :, 0, None] * B[..., None, 0, :] + A[..., :, 1, None] * B[..., None, 1, :]) + A[..., :, 2, None] * B[..., None, 2, :]


def _in_bounds(v: Tensor) -> Tensor:
    return (v >= -EPS) & (v <= 1 + EPS)


def _projects_inside(px, py, pz, K) -> Tensor:
    den = pz + EPS32
    q = [(p / den).nan_to_num(nan=0.0, posinf=INFINITY, neginf=-INFINITY) for p in (px, py, pz)]
    x = (K[0][0] * q[0] + K[0][1] * q[1]) + K[0][2] * q[2]
    y = (K[1][0] * q[0] + K[1][1] * q[1]) + K[1][2] * q[2]
    return _in_bounds(x) & _in_bounds(y)


def _crosses_line(c, o_s, o_q, o_z, d_s, d_q, d_z, f_o, c_o, den) -> Tensor:
    t = (c * o_z - o_s) / (d_s - c * d_z)
    num = f_o * (o_q * (c * d_z - d_s) + d_q * (o_s - c * o_z))
    other = c_o + num / den
    z = o_z + t * d_z
    return _in_bounds(other) & (z > -EPS) & (t > -EPS)


def _counts_torch(E: Tensor, K: Tensor, h: int, w: int, pairs: Tensor) -> Tensor:
    dev, T, V, N = E.device, E.dtype, E.shape[0], h * w
    P = pairs.shape[0]
    out = torch.empty(P, dtype=torch.int32, device=dev)
    if P == 0:
        return out
    # the grid is formed in f32, as sample_image_grid forms it, whatever the dtype of the cameras
    n = torch.arange(N, device=dev)
    x = ((n % w).to(torch.float32) + 0.5) / torch.tensor(float(w), dtype=torch.float32, device=dev)
    y = (torch.div(n, w, rounding_mode="floor").to(torch.float32) + 0.5) / torch.tensor(float(h), dtype=torch.float32, device=dev)
    x, y = x.to(T)[None], y.to(T)[None]
    step = max(1, _TORCH_ELEMENTS // N)
    for lo in range(0, P, step):
        prs = pairs[lo:lo + step].long()
        i, j = prs[:, 0], prs[:, 1]
        ok = (i >= 0) & (i < V) & (j >= 0) & (j < V)
        i, j = i.clamp(0, V - 1), j.clamp(0, V - 1)
        # ---- per pair, float64, rounded once
        E64, K64 = E.double(), K.double()
        adj, det = _adjugate(E64[j, :3, :3])
        R = (_matmul3(adj, E64[i, :3, :3]) / det[:, None, None]).to(T)
        o = (_matmul3(adj, (E64[i, :3, 3] - E64[j, :3, 3])[:, :, None])[..., 0] / det[:, None]).to(T)
        kadj, kdet = _adjugate(K64[i])
        Kinv = (kadj / kdet[:, None, None]).to(T)
        Kj64 = K64[j]
        cf = [((v - Kj64[:, a, 2]) / Kj64[:, a, a]).to(T)[:, None] for a in (0, 1) for v in (0.0, 1.0)]
        Kj = [[K[j, r, c][:, None] for c in range(3)] for r in range(2)]
        Rm = [[R[:, r, c][:, None] for c in range(3)] for r in range(3)]
        Ki = [[Kinv[:, r, c][:, None] for c in range(3)] for r in range(3)]
        # ---- the pair's own flags
        o0, o1, o2 = (o[:, k][:, None] for k in range(3))
        at_camera = ((o0 * o0 + o1 * o1) + o2 * o2).sqrt() < EPS
        origin_valid = _projects_inside(o0, o1, o2, Kj) & (o2 > -EPS) & ~(o2 < EPS)
        zero = torch.zeros_like(o0)
        ox, oy, oz = (torch.where(at_camera, zero, v) for v in (o0, o1, o2))
        # ---- per ray
        u = [(Ki[r][0] * x + Ki[r][1] * y) + Ki[r][2] for r in range(3)]
        norm = ((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]).sqrt()
        u = [v / norm for v in u]
        dx, dy, dz = ((Rm[r][0] * u[0] + Rm[r][1] * u[1]) + Rm[r][2] * u[2] for r in range(3))
        valid_inf = _projects_inside(dx, dy, dz, Kj) & (dz > -EPS)
        valid_0 = torch.where(at_camera, valid_inf, origin_valid.expand_as(valid_inf))
        den_x, den_y = dz * ox - dx * oz, dz * oy - dy * oz
        any_f = (_crosses_line(cf[0], ox, oy, oz, dx, dy, dz, Kj[1][1], Kj[1][2], den_x)
                 | _crosses_line(cf[1], ox, oy, oz, dx, dy, dz, Kj[1][1], Kj[1][2], den_x)
                 | _crosses_line(cf[2], oy, ox, oz, dy, dx, dz, Kj[0][0], Kj[0][2], den_y)
                 | _crosses_line(cf[3], oy, ox, oz, dy, dx, dz, Kj[0][0], Kj[0][2], den_y))
        overlaps = (valid_0 & valid_inf) | any_f
        counts = overlaps.sum(1, dtype=torch.int32)
        out[lo:lo + step] = torch.where(ok, counts, torch.full_like(counts, -1))
    return out
