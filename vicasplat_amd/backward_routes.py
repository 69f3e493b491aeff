"""Which kernels the backward of a linear layer or a 3x3 convolution runs (vicasplat_amd/ops.py: linear_backward, conv3x3_backward,
linear_backward_split, conv3x3_backward_split), named from Python values alone: no tensor, no GPU, no library.  Those four functions compute
their route once and dispatch on it; tests/test_backward_routes_cpu.py pins the table per shape, tests/test_backward_routes_gpu.py runs each leaf.

  class      function  part   leaves
  f16/bf16   linear    dx     nt             NT GEMM of dy on transpose16(w)
                       wgrad  tn256          vs_gemm_wgrad_tn on dy, x as they are: whole 256-tiles of dW, 16-byte aligned rows
                              tn_skinny      the same kernel for >= 2^20 rows, whatever the tile fill (HBM-bound; the transposes cost 3 passes)
                              transposed     two slice-blocked transpose16 + vs_gemm_wgrad
                       db     colsum, colsum_padded (N % 8 != 0 on the tn routes: rows read up to the next multiple of 8), on_transpose
  f16/bf16   conv      dx     conv           the forward kernel on the flipped, channel-transposed weights
                       wgrad  tn             vs_conv3x3_wgrad_tn on the NHWC tensors as they are (256 x 256 tiles >= 40 % full)
                              tn_grouped     the same entry point for Cin <= 128: 256 // Cin taps share a 256-row tile
                              transposed     two zero-bordered transpose16 + ONE tap-fused vs_gemm_wgrad
                       db     colsum, on_transpose
  split      linear    dx     pack_t         vs_gemm_split on the transposing pack of w (N % 64 == 0, scale exponent known, contiguous weight)
                              padded         on pack(w^T) from an f32 transpose, N padded to a multiple of 32
                       dgelu  epilogue       x GELU'(z) in that GEMM's epilogue (5)
                              pass           gelu_backward on dx
                       wgrad  atn256         vs_gemm_wgrad_split_atn: x as it is, dy through the transposing pack (whole 256-tiles of dW)
                              transposed     transpose_f32(dy) + transpose_pack_split(x) + vs_gemm_wgrad
                       db     on_transpose, colsum (no dw wanted)
  split      conv      dx     conv
                       wgrad  atn256         vs_conv3x3_wgrad_split_atn: x as it is, dy through the transposing pack
                              stream         vs_conv3x3_wgrad_split_stream: one pass over x and dy (Cin, Cout % 64 == 0, W % 32 == 0)
                              transposed     zero-bordered transpose_f32(x) with a halo + transpose_pack_split(dy) + ONE tap-fused vs_gemm_wgrad
                       db     on_transpose, stream (the streaming kernel's own)

`pad` is what the reduction is zero-padded to, per route: the unit of wgrad_ksplit (128 * ksplit for whole 256-tiles, else 64 * ksplit) on the
16-bit `transposed` routes and the split conv one, M rounded up to 1024 (M >= 4096) or 128 on the split linear routes, 64 * ksplit on the split
conv `atn256`; the reduction itself where the kernel reads the operands as they are.
"""
from __future__ import annotations

import functools
from typing import NamedTuple, Optional


def wgrad_ksplit(out_rows: int, out_cols: int, red: int, ntaps: int = 1, *, divide: bool = False) -> tuple[int, int]:
    """(ksplit, reduction padding unit) of a weight-gradient GEMM out[out_rows, out_cols] = sum over `red` rows: THE slice rule of every route
    (each count is a summation order of its own, so the bits of dW depend on it).  Mirrors the dispatch of vs_gemm_wgrad: whole 256x256
    output tiles run on the 8-wave kernel, one workgroup per CU (aim at ~256 workgroups, K slices of an even number of 64-wide tiles); anything
    else on 128x128 tiles, 3 per CU (~768), at least 2 slices.  divide (`red` is a padded length already): the largest such count, not below
    that floor, with red % (64 * ksplit) == 0."""
    if out_rows % 256 == 0 and out_cols % 256 == 0:
        tiles, floor, unit = (out_rows // 256) * (out_cols // 256) * ntaps, 1, 128
        ks = max(floor, min((256 + tiles // 2) // tiles, red // 512))
    else:
        tiles, floor, unit = ((out_rows + 127) // 128) * ((out_cols + 127) // 128) * ntaps, 2, 64
        ks = max(floor, min(768 // tiles, red // 512, 1024))
    while divide and ks > floor and red % (64 * ks) != 0:
        ks -= 1
    return ks, unit * ks


def wgrad_tn_skinny_ksplit(red: int) -> int:
    """K slices of vs_gemm_wgrad_tn on less than a whole 256-tile of output (`tn_skinny`: millions of rows onto one tile)."""
    return max(1, min(256, red // 512))


def round_up(n: int, unit: int) -> int:
    return (n + unit - 1) // unit * unit


def bordered_taps(W: int, align: int):
    """(shifts, halo) of a tap-fused weight gradient over zero-bordered (W + 2)-wide maps: tap (ty, tx) reads the transposed operand shifted by
    (ty - 1) * (W + 2) + (tx - 1) columns; halo = readable zero columns on either side, >= the largest |shift| + 1 and a multiple of `align`
    elements (16-byte rows: 8 for 16-bit, 4 for f32)."""
    return [(ty - 1) * (W + 2) + (tx - 1) for ty in range(3) for tx in range(3)], round_up(W + 4, align)


class BackwardRoute(NamedTuple):
    dx: Optional[str]       # None: not wanted
    dgelu: Optional[str]    # only with linear_backward_split(dgelu_z=)
    wgrad: Optional[str]
    ksplit: int             # K slices of the weight gradient (0: not a split-K launch)
    pad: int                # see the module docstring
    db: Optional[str]


@functools.lru_cache(maxsize=1024)      # a training step asks for the same ~80 routes every time: a dictionary look-up instead of the arithmetic
def linear_backward_route(cls: str, M: int, N: int, K: int, *, need_dx: bool = True, need_dw: bool = True, need_db: bool = True,
                          dy_ld: Optional[int] = None, x_ld: Optional[int] = None, aligned16: bool = True, scale_exp_known: bool = False,
                          w_contiguous: bool = True, dgelu: Optional[bool] = None) -> BackwardRoute:
    """dy [M,N], x [M,K].  cls "f16" / "bf16" (linear_backward) reads the row strides dy_ld / x_ld (default: contiguous) and whether both bases
    are 16-byte aligned; "split" (linear_backward_split) reads whether the weight's scale exponent is known and its f32 form contiguous, and
    dgelu: None without dgelu_z, True for a contiguous f32 [M,K] one, False for any other."""
    whole = N % 256 == 0 and K % 256 == 0
    lone_db, rides = "colsum" if need_db else None, "on_transpose" if need_db else None
    if cls == "split":
        dx = None if not need_dx else "pack_t" if N % 64 == 0 and scale_exp_known and w_contiguous else "padded"
        dg = None if dgelu is None or dx is None else "epilogue" if dgelu and round_up(N, 32) % 64 == 0 else "pass"
        if not need_dw:
            return BackwardRoute(dx, dg, None, 0, 0, lone_db)
        pad = round_up(M, 1024 if M >= 4096 else 128)      # (room for the K split; zero rows cost nothing exact)
        return BackwardRoute(dx, dg, "atn256" if whole else "transposed", wgrad_ksplit(N, K, pad, divide=True)[0], pad, rides)
    dx = "nt" if need_dx else None
    if not need_dw:
        return BackwardRoute(dx, None, None, 0, 0, lone_db)
    dy_ld, x_ld = N if dy_ld is None else dy_ld, K if x_ld is None else x_ld
    ks, unit = wgrad_ksplit(N, K, M)
    if (whole or M >= 1 << 20) and dy_ld % 8 == 0 and x_ld % 8 == 0 and aligned16 and dy_ld >= round_up(N, 8):
        return BackwardRoute(dx, None, "tn256" if whole else "tn_skinny", ks if whole else wgrad_tn_skinny_ksplit(M), M,
                             lone_db if N % 8 == 0 or not need_db else "colsum_padded")
    return BackwardRoute(dx, None, "transposed", ks, round_up(M, unit), rides)


@functools.lru_cache(maxsize=1024)
def conv3x3_backward_route(cls: str, N: int, H: int, W: int, Cin: int, Cout: int, *, contiguous: bool = True, need_dx: bool = True,
                           need_db: bool = True) -> BackwardRoute:
    """x [N,H,W,Cin], dy [N,H,W,Cout].  cls "f16" / "bf16" (conv3x3_backward) reads `contiguous`: x and dy both are; "split"
    (conv3x3_backward_split) asserts that they are."""
    dx, rides = "conv" if need_dx else None, "on_transpose" if need_db else None
    P, Pb = N * H * W, N * (H + 2) * (W + 2)             # pixels; pixels of the zero-bordered maps
    if cls == "split":
        if Cin % 256 == 0 and Cout % 256 == 0:
            ks = wgrad_ksplit(Cin, Cout, P, 9)[0]
            return BackwardRoute(dx, None, "atn256", ks, round_up(P, 64 * ks), rides)
        if Cin % 64 == 0 and Cout % 64 == 0 and W % 32 == 0:     # narrow layers (the pts3d head's 256 -> 128 and 128 -> 128 convolutions)
            return BackwardRoute(dx, None, "stream", 0, P, "stream" if need_db else None)
        ks, unit = wgrad_ksplit(Cin, Cout, Pb, 9)
        return BackwardRoute(dx, None, "transposed", ks, round_up(Pb, unit), rides)
    G = 256 // Cin if (Cin <= 128 and 256 % Cin == 0) else 1              # taps that share one 256-row tile (conv3x3_wgrad_tn_kernel)
    groups = (9 + G - 1) // G
    tile_rows = groups * 256 if G > 1 else 9 * round_up(Cin, 256)
    if Cin % 8 == 0 and Cout % 8 == 0 and 9 * Cin * Cout >= 0.4 * tile_rows * round_up(Cout, 256) and contiguous:
        ks, _ = wgrad_ksplit(256 if G > 1 else round_up(Cin, 256), round_up(Cout, 256), P, groups if G > 1 else 9)
        return BackwardRoute(dx, None, "tn_grouped" if G > 1 else "tn", ks, P, "colsum" if need_db else None)
    ks, unit = wgrad_ksplit(Cout, Cin, Pb, 9)
    return BackwardRoute(dx, None, "transposed", ks, round_up(Pb, unit), "on_transpose")      # (db comes with the transpose, wanted or not)
