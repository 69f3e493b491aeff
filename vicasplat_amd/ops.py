"""Python front-ends of the ViT-block HIP operators (thin ctypes wrappers over include/vicasplat_hip.h).

Every function requires HIP device tensors and raises otherwise -- there is no PyTorch/CPU fallback path.
16-bit operand dtype: torch.float16 (default; 10-bit mantissa like the TF32 the reference runs at) or torch.bfloat16.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch

from . import _lib as L
from .backward_routes import bordered_taps, conv3x3_backward_route, linear_backward_route, round_up
from .backward_routes import wgrad_ksplit  # noqa: F401  (ops.wgrad_ksplit: tools/bench_wgrad.py, tests)

_DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
# operand dtype codes of the MFMA kernels (GEMM / convolution / attention / upsample): 3 = f32, the reference-precision path --
# fp32 weights AND activations on the exact f32 MFMA (csrc/gemm_common.h, kDtF32); every "16-bit" output is then f32 too
_DTX = {torch.float32: 3, torch.float16: 1, torch.bfloat16: 2}
_OPERAND_DTYPES = (torch.float16, torch.bfloat16, torch.float32)
EPI_STORE16, EPI_GELU16, EPI_RESID32, EPI_STORE32 = 0, 1, 2, 3


class _RangeGuard:
    """Debug-mode range audit of the split operand class (csrc/range_guard.hip; VERDICT r3 "weak 3").  The split class keeps f32
    activations but multiplies their f16 (hi, lo) pairs: |x| >= 65520 becomes hi = +-inf, where the reference's fp32 / TF32 arithmetic still
    has range.  While enabled, every split-class GEMM / convolution / attention front-end below scans its activation operand
    (vs_range_check: one extra read pass, one atomic per wavefront that finds something) into one flag word per call; `report()` reads
    the table (one host synchronisation) and names the calls that saw out-of-range values.  Disabled (the default) it costs nothing."""
    LIMIT = 65520.0          # the smallest magnitude that rounds to +-inf in f16 (round to nearest even)
    SLOTS = 4096

    def __init__(self):
        self.enabled, self.flags, self.names = False, None, []

    def begin(self, device):
        self.enabled = True
        if self.flags is None or self.flags.device != torch.device(device):
            self.flags = torch.zeros(self.SLOTS, dtype=torch.int32, device=device)
        else:
            self.flags.zero_()
        self.names = []

    def end(self):
        self.enabled = False

    def check(self, what: str, t, rows=None, cols=None):
        """t: an f32 2-D view [rows, cols] (any row stride) / an N-D contiguous f32 tensor (flattened to rows of its last dimension) / a
        packed SplitWeight activation."""
        if not self.enabled or t is None:
            return
        packed = isinstance(t, SplitWeight)
        d = t.data if packed else t
        if d.dtype != (torch.int32 if packed else torch.float32) or d.numel() == 0:
            return
        if d.dim() != 2:
            d = d.reshape(-1, d.shape[-1])
        rows = d.shape[0] if rows is None else rows
        cols = d.shape[1] if cols is None else cols
        if d.stride(1) != 1 or cols % (32 if packed else 4) or d.stride(0) % 4 or d.data_ptr() % 16:
            d = d[:, :cols].contiguous() if not packed else d
            if packed:
                return
            pad = (-cols) % 4
            if pad:
                d = torch.nn.functional.pad(d, (0, pad))
                cols += pad
        slot = len(self.names)
        if slot >= self.SLOTS:
            return
        self.names.append(f"#{slot} {what} [{rows} x {cols}]{' packed' if packed else ''}")
        dev = d.device
        L.call("vs_range_check", dev, L.ptr(d), rows, cols, d.stride(0), 1 if packed else 0, self.LIMIT, L.ptr(self.flags), slot)

    def report(self) -> list:
        """[(call, flags)] of the calls whose operand left the f16 range (1 = finite |x| >= 65520, 2 = non-finite f32 input, 4 = a packed hi
        half that is +-inf / NaN).  Synchronises."""
        if self.flags is None or not self.names:
            return []
        f = self.flags[:len(self.names)].cpu().tolist()
        return [(n, v) for n, v in zip(self.names, f) if v]


RANGE_GUARD = _RangeGuard()


class range_guard:
    """`with ops.range_guard(device) as g: ...; bad = g.report()` -- audit every split-class operand inside the block (see _RangeGuard)."""

    def __init__(self, device, raise_on_overflow: bool = False):
        self.device, self.raise_on_overflow = device, raise_on_overflow

    def __enter__(self):
        RANGE_GUARD.begin(self.device)
        return RANGE_GUARD

    def __exit__(self, et, ev, tb):
        RANGE_GUARD.end()
        if et is None and self.raise_on_overflow:
            bad = RANGE_GUARD.report()
            if bad:
                raise SplitRangeError(bad)
        return False


class SplitRangeError(RuntimeError):
    def __init__(self, bad):
        self.calls = bad
        head = "; ".join(f"{n} (flags {v})" for n, v in bad[:6])
        super().__init__(f"split operand class: {len(bad)} call(s) saw activations outside the f16 range of their hi halves (|x| >= 65520 -> "
                         f"+-inf; the reference's fp32 / TF32 arithmetic has fp32 range there): {head}{' ...' if len(bad) > 6 else ''}.  "
                         'Run this input in the exact-f32 class (set_compute_dtype("f32")) or rescale the offending layer.')


def split_act(rows: int, cols: int, device) -> "SplitWeight":
    """Uninitialised [rows, cols] activation buffer in the PACKED (hi, lo) form (scale 2^0) for producers that write it directly --
    layernorm_mod(out=...), gemm(..., out=...) with the store / GELU epilogues -- and GEMMs that read it as their A operand without a
    conversion (vs_gemm_split_packed).  cols % 32 == 0; 4 bytes per element like the f32 tensor it stands for."""
    assert cols % 32 == 0
    return SplitWeight(torch.empty((rows, cols), dtype=torch.int32, device=device), 1.0, (rows, cols))


class SplitWeight:
    """A weight packed for the SPLIT operand class (dtype code 4; csrc/gemm_common.h, kDtSplit): f16 (hi, lo) pairs of w * 2^scale_exp,
    blocked by 32 k (vs_split_pack_weight).  `data` is an int32 tensor of the logical shape (4 bytes per element); the product entry
    points multiply the accumulators by `acc_scale` = 2^-scale_exp.  Activations of this class are plain f32 tensors."""
    __slots__ = ("data", "acc_scale", "shape")

    def __init__(self, data: torch.Tensor, acc_scale: float, shape):
        self.data, self.acc_scale, self.shape = data, acc_scale, tuple(shape)

    @property
    def device(self):
        return self.data.device

    def is_contiguous(self):
        return self.data.is_contiguous()

    def numel(self):
        return self.data.numel()


def split_scale_exp(w: torch.Tensor, with_nonzero: bool = False):
    """Power-of-two exponent e with max|w| 2^e in [2^13, 2^14) (one host read of the maximum); 0 for an all-zero / non-finite weight.
    with_nonzero: also return whether the exponent came from an actual finite non-zero maximum (a cache must not keep the 0 of a
    zero-initialised layer: it would pack the layer unscaled long after its weights have moved)."""
    amax = float(w.detach().abs().max())
    ok = amax != 0.0 and math.isfinite(amax)
    e = max(-24, min(24, 13 - math.frexp(amax)[1] + 1)) if ok else 0
    return (e, ok) if with_nonzero else e


def split_pack_weight(w: torch.Tensor, scale_exp: Optional[int] = None) -> SplitWeight:
    """f32 weight [N, ...] (flattened to [N, K], K % 32 == 0) -> SplitWeight.  The power-of-two scale puts max|w| just below 2^14: lo stays a
    normal f16 for every element within 2^-16 of the largest, and the products of the f16 range cannot overflow the f32 accumulator."""
    dev = L.require_device(w)
    w2 = w.detach().float().reshape(w.shape[0], -1).contiguous()
    N, K = w2.shape
    assert K % 32 == 0, f"split operands need K % 32 == 0 (K={K}): pad the reduction dimension"
    # scale_exp given: no host synchronisation (callers that pack every step cache the exponent; 0 = unscaled, the activations' convention)
    e = split_scale_exp(w2) if scale_exp is None else int(scale_exp)
    out = torch.empty((N, K), dtype=torch.int32, device=dev)
    L.call("vs_split_pack_weight", dev, L.ptr(w2), w2.stride(0), L.ptr(out), out.stride(0), N, K, e)
    return SplitWeight(out.view(w.shape[0], *w.shape[1:]) if w.dim() > 2 else out, 2.0 ** (-e), w.shape)


def layernorm_mod(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, out: torch.Tensor, *, eps: float = 1e-6,
                  scale: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None, mod_rows: int = 0,
                  grp_in: int = 0, grp_out: int = 0, grp_off: int = 0) -> torch.Tensor:
    """x f32 [M,C] -> out [*,C] (f32/f16/bf16).  scale/shift: [G,C] f32 views (row stride taken from .stride(0))."""
    odt = None
    out_obj = out
    if isinstance(out, SplitWeight):      # packed (hi, lo) output of the split class: the consumer GEMM skips its conversion
        assert out.acc_scale == 1.0
        out, odt = out.data, 3
    dev = L.require_device(x, weight, bias, out, scale, shift)
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    M, C = x.shape
    mod_ld = 0
    if scale is not None:
        assert scale.stride(-1) == 1 and (shift is None or shift.stride(0) == scale.stride(0))
        mod_ld = scale.stride(0)
    elif shift is not None:
        mod_ld = shift.stride(0)
    L.call("vs_layernorm_mod", dev, L.ptr(x), x.stride(0), L.ptr(weight), L.ptr(bias), L.ptr(scale), L.ptr(shift), mod_rows, mod_ld, L.ptr(out),
           out.stride(-2), _DT[out.dtype] if odt is None else odt, M, C, eps, grp_in, grp_out, grp_off)
    return out_obj


def linear_f32(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], relu_in: bool = False) -> torch.Tensor:
    """[..., K] f32 @ w[N, K]^T + bias in f32 (vs_linear_f32): the tiny camera-token layers (intrinsic embedding, pose / fov heads)."""
    dev = L.require_device(x, w, bias)
    x2 = x.reshape(-1, x.shape[-1]).float()
    if x2.stride(1) != 1:
        x2 = x2.contiguous()
    wf = w.detach().float()
    if wf.stride(1) != 1:
        wf = wf.contiguous()
    bf = None if bias is None else bias.detach().float().contiguous()
    out = torch.empty((x2.shape[0], wf.shape[0]), dtype=torch.float32, device=dev)
    L.call("vs_linear_f32", dev, L.ptr(x2), x2.stride(0), L.ptr(wf), wf.stride(0), L.ptr(bf), L.ptr(out), out.stride(0), x2.shape[0], wf.shape[0],
           x2.shape[1], int(relu_in))
    return out.view(*x.shape[:-1], wf.shape[0])


def silu_cast(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """silu(x) of an f32 tensor in `dtype` (one pass; the GEMM operand of the AdaLN projections)."""
    dev = L.require_device(x)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.numel() % 4 == 0
    out = torch.empty(x.shape, dtype=dtype, device=dev)
    L.call("vs_silu_cast", dev, L.ptr(x), L.ptr(out), x.numel(), _DT[dtype])
    return out


def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, epilogue: int, *,
         gate: Optional[torch.Tensor] = None, gate_rows: int = 0, grp_in: int = 0, grp_out: int = 0, grp_off: int = 0,
         M: Optional[int] = None, a_grp_in: int = 0, a_grp_out: int = 0, a_grp_off: int = 0) -> torch.Tensor:
    """out = epilogue(a[M,K] @ w[N,K]^T + bias).  a, w 16-bit; out 16-bit (epilogue 0/1) or f32 (2: in-place residual
    update with optional per-group gate [G,N]; 3: store)."""
    if isinstance(w, SplitWeight):
        return _gemm_split(a, w, bias, out, epilogue, gate=gate, gate_rows=gate_rows, grp_in=grp_in, grp_out=grp_out, grp_off=grp_off, M=M,
                           a_grp_in=a_grp_in, a_grp_out=a_grp_out, a_grp_off=a_grp_off)
    dev = L.require_device(a, w, bias, out, gate)
    assert a.dtype == w.dtype and a.dtype in _OPERAND_DTYPES
    assert a.dim() == 2 and w.dim() == 2 and a.stride(1) == 1 and w.stride(1) == 1 and a.shape[1] == w.shape[1]
    K = a.shape[1]
    M = a.shape[0] if M is None else M  # with an input row map, M counts the rows actually consumed
    N = w.shape[0]
    if epilogue in (EPI_STORE16, EPI_GELU16):
        assert out.dtype == a.dtype
    else:
        assert out.dtype == torch.float32
    gate_ld = gate.stride(0) if gate is not None else 0
    L.call("vs_gemm_bias_act", dev, L.ptr(a), L.ptr(w), L.ptr(bias), L.ptr(out), L.ptr(gate), M, N, K, a.stride(0), w.stride(0), out.stride(-2),
           epilogue, _DTX[a.dtype], grp_in, grp_out, grp_off, gate_rows, gate_ld, a_grp_in, a_grp_out, a_grp_off)
    return out


def _gemm_split(a, w: SplitWeight, bias, out, epilogue, *, gate=None, gate_rows=0, grp_in=0, grp_out=0, grp_off=0, M=None, a_grp_in=0,
                a_grp_out=0, a_grp_off=0, resid=None, pos=None, kind=None, C=0, base2d=0.0, theta1d=0.0):
    """vs_gemm_split: a f32 [M,K], w SplitWeight [N,K], every output f32 (epilogue codes of `gemm`, 4 = q|k|v + RoPE)."""
    wd = w.data
    packed = isinstance(a, SplitWeight)       # A already in the packed (hi, lo) form (scale 2^0): the kernels skip their conversion
    if packed:
        assert a.acc_scale == 1.0
        a = a.data
    out_obj = out
    if isinstance(out, SplitWeight):          # packed output (epilogues 0 / 1 / 3): the A operand of the next GEMM, written by this one's epilogue
        assert out.acc_scale == 1.0 and epilogue in (EPI_STORE16, EPI_GELU16, EPI_STORE32, 4) and out.data.dtype == torch.int32
        out, epilogue = out.data.view(torch.float32), epilogue | 16
    dev = L.require_device(a, wd, bias, out, gate, resid, pos, kind)
    assert a.dtype == (torch.int32 if packed else torch.float32) and out.dtype == torch.float32 and a.dim() == 2 and wd.dim() == 2 and a.stride(1) == 1
    assert wd.stride(1) == 1 and a.shape[1] == wd.shape[1] and (resid is None or (resid.dtype == torch.float32 and resid.stride() == out.stride()))
    M = a.shape[0] if M is None else M
    if RANGE_GUARD.enabled:
        RANGE_GUARD.check(f"gemm A x W[{wd.shape[0]}] epi {epilogue}", SplitWeight(a, 1.0, a.shape) if packed else a)
    L.call("vs_gemm_split_packed" if packed else "vs_gemm_split", dev, L.ptr(a), L.ptr(wd), w.acc_scale, L.ptr(bias), L.ptr(out), L.ptr(gate),
           L.ptr(resid), M, wd.shape[0], a.shape[1], a.stride(0), wd.stride(0), out.stride(-2), epilogue, grp_in, grp_out, grp_off, gate_rows,
           gate.stride(0) if gate is not None else 0, a_grp_in, a_grp_out, a_grp_off, L.ptr(pos), L.ptr(kind), C, base2d, theta1d)
    return out_obj


def gemm_resid(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], resid: torch.Tensor, *, gate: Optional[torch.Tensor] = None,
               gate_rows: int = 0) -> torch.Tensor:
    """resid [M,N] f32 + (1 + gate) * (a @ w^T + bias) into a NEW tensor (vs_gemm_resid): the residual update of gemm(..., EPI_RESID32)
    without touching (or cloning) the old stream."""
    if isinstance(w, SplitWeight):
        assert resid.is_contiguous() and resid.shape == (a.shape[0], w.shape[0])
        return _gemm_split(a, w, bias, torch.empty_like(resid), EPI_RESID32, gate=gate, gate_rows=gate_rows, resid=resid)
    dev = L.require_device(a, w, bias, resid, gate)
    assert a.dtype == w.dtype and a.dtype in _OPERAND_DTYPES and a.stride(1) == 1 and w.stride(1) == 1
    assert resid.dtype == torch.float32 and resid.is_contiguous() and resid.shape == (a.shape[0], w.shape[0])
    out = torch.empty_like(resid)
    L.call("vs_gemm_resid", dev, L.ptr(a), L.ptr(w), L.ptr(bias), L.ptr(resid), L.ptr(out), L.ptr(gate), a.shape[0], w.shape[0], a.shape[1],
           a.stride(0), w.stride(0), out.stride(0), _DTX[a.dtype], gate_rows, gate.stride(0) if gate is not None else 0)
    return out


def gemm_qkv_rope(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, C: int, pos: torch.Tensor,
                  kind: Optional[torch.Tensor] = None, base2d: float = 100.0, theta1d: float = 30.0, *, grp_in: int = 0,
                  grp_out: int = 0, grp_off: int = 0, M: Optional[int] = None, a_grp_in: int = 0, a_grp_out: int = 0,
                  a_grp_off: int = 0) -> torch.Tensor:
    """Packed q|k|v projection (w [N >= 2C, K]) with rope_qk(out, C // 64, C, pos, kind, ...) fused into the epilogue."""
    assert pos.dtype == torch.int32 and pos.is_contiguous() and (kind is None or (kind.dtype == torch.uint8 and kind.is_contiguous()))
    if isinstance(w, SplitWeight):
        return _gemm_split(a, w, bias, out, 4, grp_in=grp_in, grp_out=grp_out, grp_off=grp_off, M=M, a_grp_in=a_grp_in, a_grp_out=a_grp_out,
                           a_grp_off=a_grp_off, pos=pos, kind=kind, C=C, base2d=base2d, theta1d=theta1d)
    dev = L.require_device(a, w, bias, out, pos, kind)
    assert a.dtype == w.dtype == out.dtype and a.dtype in _OPERAND_DTYPES
    assert a.dim() == 2 and w.dim() == 2 and a.stride(1) == 1 and w.stride(1) == 1 and a.shape[1] == w.shape[1]
    assert pos.dtype == torch.int32 and pos.is_contiguous() and (kind is None or (kind.dtype == torch.uint8 and kind.is_contiguous()))
    M = a.shape[0] if M is None else M
    L.call("vs_gemm_qkv_rope", dev, L.ptr(a), L.ptr(w), L.ptr(bias), L.ptr(out), M, w.shape[0], a.shape[1], a.stride(0), w.stride(0), out.stride(-2),
           _DTX[a.dtype], grp_in, grp_out, grp_off, a_grp_in, a_grp_out, a_grp_off, L.ptr(pos), L.ptr(kind), C, base2d, theta1d)
    return out


def rope_qk(buf: torch.Tensor, H: int, k_col: int, pos: torch.Tensor, kind: Optional[torch.Tensor] = None,
            base2d: float = 100.0, theta1d: float = 30.0, inverse: bool = False) -> torch.Tensor:
    """In-place RoPE on q (col 0) and k (col k_col) of buf [rows, ld]; pos int32 [rows,2]; kind uint8 [rows] or None.
    inverse=True applies the inverse rotation (the backward pass of the embedding, on dq | dk)."""
    dev = L.require_device(buf, pos, kind)
    assert buf.dim() == 2 and buf.stride(1) == 1 and pos.dtype == torch.int32 and pos.is_contiguous()
    assert kind is None or (kind.dtype == torch.uint8 and kind.is_contiguous())
    L.call("vs_rope_qk_dir", dev, L.ptr(buf), buf.stride(0), buf.shape[0], H, k_col, L.ptr(pos), L.ptr(kind), base2d, theta1d,
           -1.0 if inverse else 1.0, _DT[buf.dtype])
    return buf


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, *, nbatch: int, H: int, Lq: int,
              Lk: int = 0, q_batch_rows: int, k_batch_rows: int = 0, kv_seg: Optional[torch.Tensor] = None,
              q_kvlen: Optional[torch.Tensor] = None, scale: float = 0.125, lse: Optional[torch.Tensor] = None,
              split: bool = False) -> torch.Tensor:
    """q/k/v: 2-D views [rows, ld] whose column 0 is head 0 (e.g. slices of a packed q|k|v buffer); out [rows, H*64].
    lse (optional, f32 [rows, H] contiguous) receives the log2-domain logsumexp for attention_backward.
    split=True (f32 tensors only): the split operand class -- three f16 MFMAs per product instead of the exact-f32 MFMA (dtype code 4).
    q, k, v int32 (column slices of the `.data` of a packed (hi, lo) q|k|v buffer, written by gemm_qkv_rope(..., out=split_act(...))):
    the packed-input kernel (dtype 4 + 32: LDS-DMA staging without conversion, key-split waves, XCD-aware grid)."""
    out_obj, out_packed = out, isinstance(out, SplitWeight)
    in_packed = q.dtype == torch.int32
    if in_packed:
        assert split and k.dtype == torch.int32 and v.dtype == torch.int32
    if out_packed:          # split class: O written in the packed (hi, lo) form, the A operand of the projection GEMM as it is
        assert split and out.acc_scale == 1.0
        out = out.data.view(torch.float32)
    dev = L.require_device(q, k, v, out, kv_seg, q_kvlen, lse)
    for t in (q, k, v, out):
        assert t.dim() == 2 and t.stride(1) == 1 and (t.dtype == q.dtype or (in_packed and t is out))
    assert kv_seg is None or (kv_seg.dtype == torch.int32 and kv_seg.is_contiguous())
    assert q_kvlen is None or (q_kvlen.dtype == torch.int32 and q_kvlen.is_contiguous())
    assert lse is None or (lse.dtype == torch.float32 and lse.is_contiguous() and lse.shape == (q.shape[0], H))
    assert not split or q.dtype == torch.float32 or in_packed
    if split and RANGE_GUARD.enabled:
        for nm_, t_ in (("q", q), ("k", k), ("v", v)):
            RANGE_GUARD.check(f"attention {nm_} (H {H}, Lq {Lq})", SplitWeight(t_, 1.0, t_.shape) if in_packed else t_, cols=H * 64)
    L.call("vs_attention_lse", dev, L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(out), nbatch, H, Lq, Lk, q_batch_rows, k_batch_rows, q.stride(0), k.stride(0),
           v.stride(0), out.stride(0), L.ptr(kv_seg), L.ptr(q_kvlen), scale,
           (4 + (16 if out_packed else 0) + (32 if in_packed else 0)) if split else _DTX[q.dtype], L.ptr(lse))
    return out_obj


def attention_backward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, dout: torch.Tensor, lse: torch.Tensor, *,
                       nbatch: int, H: int, Lq: int, Lk: int = 0, q_batch_rows: int, k_batch_rows: int = 0,
                       kv_seg: Optional[torch.Tensor] = None, q_kvlen: Optional[torch.Tensor] = None, max_keys: int = 0,
                       scale: float = 0.125, dq_out: Optional[torch.Tensor] = None, dk_out: Optional[torch.Tensor] = None,
                       dv_out: Optional[torch.Tensor] = None):
    """Backward of `attention` (used by autograd.AttentionFn).  Returns dq (16-bit [rows, H*64]; written into dq_out, e.g. the q
    block of a packed [rows, 3*H*64] gradient buffer, when given) and dk, dv (f32 [key rows, H*64], accumulated from zero).
    Without key segments dk_out / dv_out (16-bit [key rows, H*64] views, e.g. the k | v blocks of the same packed buffer) may be
    given: they are written directly (vs_attention_backward16: no atomics, no zero fill, no cast pass) and returned."""
    dev = L.require_device(q, k, v, out, dout, lse, kv_seg, q_kvlen)
    for t in (q, k, v, out, dout):
        assert t.dim() == 2 and t.stride(1) == 1
    Cc = H * 64
    if dq_out is None:
        dq = torch.empty((q.shape[0], Cc), dtype=q.dtype, device=dev)
    else:
        dq = dq_out
        assert dq.shape == (q.shape[0], Cc) and dq.dtype == q.dtype and dq.stride(1) == 1
    delta = torch.empty((q.shape[0], H), dtype=torch.float32, device=dev)
    if dk_out is not None:
        assert kv_seg is None and dv_out is not None, "direct dk / dv need key rows with a single owner (no key segments)"
        for t, ref in ((dk_out, k), (dv_out, v)):
            assert t.shape == (ref.shape[0], Cc) and t.dtype == q.dtype and t.stride(1) == 1
        L.call("vs_attention_backward16", dev, L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(out), L.ptr(dout), L.ptr(lse), L.ptr(delta), L.ptr(dq),
               L.ptr(dk_out), L.ptr(dv_out), nbatch, H, Lq, Lk, q_batch_rows, k_batch_rows, q.stride(0), k.stride(0), v.stride(0), out.stride(0),
               dout.stride(0), dq.stride(0), dk_out.stride(0), dv_out.stride(0), L.ptr(q_kvlen), scale, _DT[q.dtype])
        return dq, dk_out, dv_out
    dk = torch.zeros((k.shape[0], Cc), dtype=torch.float32, device=dev)
    dv = torch.zeros((v.shape[0], Cc), dtype=torch.float32, device=dev)
    L.call("vs_attention_backward", dev, L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(out), L.ptr(dout), L.ptr(lse), L.ptr(delta), L.ptr(dq), L.ptr(dk),
           L.ptr(dv), nbatch, H, Lq, Lk, q_batch_rows, k_batch_rows, q.stride(0), k.stride(0), v.stride(0), out.stride(0), dout.stride(0),
           dq.stride(0), dk.stride(0), dv.stride(0), L.ptr(kv_seg), L.ptr(q_kvlen), max_keys, scale, _DT[q.dtype])
    return dq, dk, dv


def gaussian_adapter(pts: torch.Tensor, gs: torch.Tensor, sh_mask: torch.Tensor, *, scale_act: str = "softplus",
                     scale_min: float = 0.0, scale_max: float = 0.0, opacity_exponent: float = 1.0, want_raw: bool = True):
    """pts [N,3,H,W], gs [N,8+3*d_sh,H,W] (any strides, f32/f16/bf16, same dtype) -> dict of f32 tensors shaped
    [N,H,W,...] (means, covariances, harmonics, opacities [...,1], scales, rotations, raw)."""
    dev = L.require_device(pts, gs, sh_mask)
    assert pts.dtype == gs.dtype and pts.dim() == 4 and gs.dim() == 4 and pts.shape[1] == 3
    N, Cg, H, W = gs.shape
    d_sh = (Cg - 8) // 3
    assert Cg == 8 + 3 * d_sh and sh_mask.numel() == d_sh and sh_mask.dtype == torch.float32
    # one flat pixel index must address both inputs: require (n,h,w) to be jointly contiguous in each (NCHW or NHWC)
    for t in (pts, gs):
        sn, sc, sh_, sw = t.stride()
        if not (sh_ == W * sw and sn == H * sh_):  # not pixel-linear (e.g. plain NCHW): make it channels-last
            raise RuntimeError("gaussian_adapter expects channels-last (NHWC) head outputs")
    f = dict(dtype=torch.float32, device=dev)
    npix = N * H * W
    out = dict(means=torch.empty(N, H, W, 3, **f), covariances=torch.empty(N, H, W, 3, 3, **f),
               harmonics=torch.empty(N, H, W, 3, d_sh, **f), opacities=torch.empty(N, H, W, 1, **f),
               scales=torch.empty(N, H, W, 3, **f), rotations=torch.empty(N, H, W, 4, **f),
               raw=torch.empty(N, H, W, 11 + 3 * d_sh, **f) if want_raw else None)
    act = {"bounded": 0, "exp": 1, "softplus": 2}[scale_act]
    L.call("vs_gaussian_adapter", dev, L.ptr(pts), pts.stride(3), pts.stride(1), L.ptr(gs), gs.stride(3), gs.stride(1), _DT[pts.dtype], npix, d_sh,
           L.ptr(sh_mask), act, scale_min, scale_max, opacity_exponent, L.ptr(out["means"]), L.ptr(out["covariances"]), L.ptr(out["harmonics"]),
           L.ptr(out["opacities"]), L.ptr(out["scales"]), L.ptr(out["rotations"]), L.ptr(out["raw"]))
    return out


def gaussian_adapter_backward(pts: torch.Tensor, gs: torch.Tensor, sh_mask: torch.Tensor, d_means: torch.Tensor, d_cov: torch.Tensor,
                              d_harm: torch.Tensor, d_op: torch.Tensor, d_raw: Optional[torch.Tensor] = None, *, scale_act: str = "softplus",
                              scale_min: float = 0.0, scale_max: float = 0.0, opacity_exponent: float = 1.0):
    """Backward of gaussian_adapter for dense NHWC 16-bit head outputs pts [N,H,W,pts_pix>=3], gs [N,H,W,8+3*d_sh]: f32 gradients of
    means [..,3], covariances [..,3,3], harmonics [..,3,d_sh], opacities [..] (and optionally raw [..,11+3*d_sh]) -> (d_pts, d_gs)
    in the inputs' shape and dtype, as views of buffers whose rows are padded to a multiple of 8 channels (16-byte aligned rows with
    zero padding: what the reduction-major weight-gradient kernel of the 1x1 convs in front of the adapter reads directly)."""
    dev = L.require_device(pts, gs, sh_mask, d_means, d_cov, d_harm, d_op, d_raw)
    assert pts.is_contiguous() and gs.is_contiguous() and pts.dtype == gs.dtype and pts.dtype in (torch.float16, torch.bfloat16, torch.float32)
    d_sh = (gs.shape[-1] - 8) // 3
    npix = gs.numel() // gs.shape[-1]
    f = lambda t: None if t is None else t.float().contiguous()
    d_means, d_cov, d_harm, d_op, d_raw = f(d_means), f(d_cov), f(d_harm), f(d_op), f(d_raw)
    assert d_means.numel() == npix * 3 and d_cov.numel() == npix * 9 and d_harm.numel() == npix * 3 * d_sh and d_op.numel() == npix
    assert d_raw is None or d_raw.numel() == npix * (11 + 3 * d_sh)
    pl, gl = (pts.shape[-1] + 7) // 8 * 8, (gs.shape[-1] + 7) // 8 * 8
    d_pts = torch.empty(pts.shape[:-1] + (pl,), dtype=pts.dtype, device=dev)
    d_gs = torch.empty(gs.shape[:-1] + (gl,), dtype=gs.dtype, device=dev)
    act = {"bounded": 0, "exp": 1, "softplus": 2}[scale_act]
    L.call("vs_gaussian_adapter_backward", dev, L.ptr(pts), pts.shape[-1], L.ptr(gs), _DT[pts.dtype], npix, d_sh, L.ptr(sh_mask), act, scale_min,
           scale_max, opacity_exponent, L.ptr(d_means), L.ptr(d_cov), L.ptr(d_harm), L.ptr(d_op), L.ptr(d_raw), L.ptr(d_pts), pl, L.ptr(d_gs), gl)
    return d_pts[..., :pts.shape[-1]], d_gs[..., :gs.shape[-1]]


def conv3x3_nhwc(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
                 relu_in: bool = False, relu_out: bool = False, out: Optional[torch.Tensor] = None, stride: int = 1,
                 mask_by: Optional[torch.Tensor] = None, residual2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [N,H,W,Cin] contiguous 16-bit, w [Cout,3,3,Cin] (see pack_conv3x3_weight) -> [N,Ho,Wo,Cout] (k=3, pad=1).
    mask_by [N,Ho,Wo,Cout]: the result is zeroed where mask_by <= 0 (ReLU backward fused into a data-gradient conv)."""
    if mask_by is not None:
        assert residual is None and not relu_out
        residual, relu_out = mask_by, 2
    split = isinstance(w, SplitWeight)
    xin_packed = isinstance(x, SplitWeight)     # split class: the input already in the packed (hi, lo) form (its producer wrote it; ReLU applied there)
    if xin_packed:
        assert split and not relu_in and residual2 is None
        x = x.data
    dev = L.require_device(x, w.data if split else w, bias, residual, out)
    assert x.dim() == 4 and x.is_contiguous() and w.is_contiguous() and (x.dtype in _OPERAND_DTYPES or xin_packed)
    assert (split and x.dtype == (torch.int32 if xin_packed else torch.float32)) or (not split and x.dtype == w.dtype)
    N, H, W, Cin = x.shape
    Cout = w.shape[0]
    assert tuple(w.shape) == (Cout, 3, 3, Cin)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if out is None:
        out = torch.empty((N, Ho, Wo, Cout), dtype=torch.float32 if xin_packed else x.dtype, device=dev)
    assert residual is None or (residual.shape == out.shape and residual.is_contiguous() and residual.dtype == out.dtype)
    assert residual2 is None or (split and mask_by is None and residual2.shape == out.shape and residual2.is_contiguous() and residual2.dtype == torch.float32)
    if split and RANGE_GUARD.enabled:
        RANGE_GUARD.check(f"conv3x3 {Cin}->{Cout} @{H}x{W}", SplitWeight(x.view(-1, Cin), 1.0, (N * H * W, Cin)) if xin_packed else x)
    if split and residual2 is not None:      # split class: out = conv + bias + residual + residual2 in the epilogue (no add pass)
        L.require_device(residual2)
        L.call("vs_conv3x3_split_res2_nhwc", dev, L.ptr(x), L.ptr(w.data), w.acc_scale, L.ptr(bias), L.ptr(residual), L.ptr(residual2), L.ptr(out), N,
               H, W, Cin, Cout, stride, int(relu_in), int(relu_out))
        return out
    if split:
        L.call("vs_conv3x3_split_nhwc", dev, L.ptr(x), L.ptr(w.data), w.acc_scale, L.ptr(bias), L.ptr(residual), L.ptr(out), N, H, W, Cin, Cout,
               stride, int(relu_in) | (16 if xin_packed else 0), int(relu_out))
        return out
    L.call("vs_conv3x3_nhwc", dev, L.ptr(x), L.ptr(w), L.ptr(bias), L.ptr(residual), L.ptr(out), N, H, W, Cin, Cout, stride, int(relu_in),
           int(relu_out), _DTX[x.dtype])
    return out


def conv3x3_head1x1_nhwc(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], w2: torch.Tensor, bias2: torch.Tensor, n_out: int,
                         relu_out: bool = True) -> torch.Tensor:
    """[N,H,W,Cin] 16-bit -> [N,H,W,ld2] 16-bit = conv1x1(act(conv3x3(x) + bias)) + bias2 in one kernel (vs_conv3x3_head1x1_nhwc): the
    last two layers of a DPT head.  w [Cout,3,3,Cin]; w2 [C2pad, Cout] (rows >= n_out zero) with bias2 [C2pad] for Cout = 256, or
    w2 [<= 4, 128] with bias2 [4] for Cout = 128.  The result keeps its padded channel stride (ld2 = w2 rows, or 4): slice it."""
    if isinstance(w, SplitWeight) and isinstance(w2, SplitWeight):   # split operands, MFMA form: Cout = 256, w2 packed [C2pad <= 96, 256]
        xin_packed = isinstance(x, SplitWeight)      # the input already in the packed (hi, lo) form (upsample2x_nhwc(..., packed=True))
        if xin_packed:
            x = x.data
        dev = L.require_device(x, w.data, bias, w2.data, bias2)
        N, H, W, Cin = x.shape
        c2pad = w2.shape[0]
        assert x.is_contiguous() and x.dtype == (torch.int32 if xin_packed else torch.float32) and tuple(w.shape) == (256, 3, 3, Cin) and tuple(w2.shape) == (c2pad, 256)
        assert bias2.dtype == torch.float32 and bias2.numel() == c2pad and n_out <= c2pad
        out = torch.empty((N, H, W, c2pad), dtype=torch.float32, device=dev)
        if RANGE_GUARD.enabled:
            RANGE_GUARD.check(f"fused head conv3x3 {Cin}->256 -> 1x1 @{H}x{W}", SplitWeight(x.view(-1, Cin), 1.0, (N * H * W, Cin)) if xin_packed else x)
        L.call("vs_conv3x3_head1x1_split_nhwc", dev, L.ptr(x), L.ptr(w.data), w.acc_scale, L.ptr(bias), L.ptr(w2.data), w2.acc_scale, L.ptr(bias2),
               L.ptr(out), N, H, W, Cin, n_out, c2pad, c2pad, int(relu_out) | (16 if xin_packed else 0))
        return out
    if isinstance(w, SplitWeight):   # split operands: the dot-product form (Cout = 128, n_out <= 4), f32 in / out, w2 f32 [>= n_out, 128]
        xin_packed = isinstance(x, SplitWeight)      # the input already packed (upsample2x_nhwc(..., packed=True)): no conversion in the main loop
        if xin_packed:
            x = x.data
        dev = L.require_device(x, w.data, bias, w2, bias2)
        N, H, W, Cin = x.shape
        assert x.is_contiguous() and x.dtype == (torch.int32 if xin_packed else torch.float32) and tuple(w.shape) == (128, 3, 3, Cin) and n_out <= 4
        assert w2.dtype == torch.float32 and w2.is_contiguous() and w2.shape[1] == 128 and w2.shape[0] >= n_out and bias2.numel() >= 4
        out = torch.empty((N, H, W, 4), dtype=torch.float32, device=dev)
        if RANGE_GUARD.enabled:
            RANGE_GUARD.check(f"fused head conv3x3 {Cin}->128 -> dot @{H}x{W}", SplitWeight(x.view(-1, Cin), 1.0, (N * H * W, Cin)) if xin_packed else x)
        L.call("vs_conv3x3_head_dot_split_nhwc", dev, L.ptr(x), L.ptr(w.data), w.acc_scale, L.ptr(bias), L.ptr(w2), L.ptr(bias2), L.ptr(out), N, H, W,
               Cin, n_out, 4, 0, int(relu_out) | (16 if xin_packed else 0))
        return out
    dev = L.require_device(x, w, bias, w2, bias2)
    assert x.dim() == 4 and x.is_contiguous() and w.is_contiguous() and w2.is_contiguous() and x.dtype == w.dtype == w2.dtype
    assert x.dtype in (torch.float16, torch.bfloat16) and bias2.dtype == torch.float32 and bias2.is_contiguous()
    N, H, W, Cin = x.shape
    Cout = w.shape[0]
    assert w.shape == (Cout, 3, 3, Cin) and w2.shape[1] == Cout
    if Cout == 256:
        c2pad = ld2 = w2.shape[0]
        assert bias2.numel() == c2pad
    else:
        c2pad, ld2 = n_out, 4
        assert w2.shape[0] >= n_out and bias2.numel() >= 4
    out = torch.empty((N, H, W, ld2), dtype=x.dtype, device=dev)
    L.call("vs_conv3x3_head1x1_nhwc", dev, L.ptr(x), L.ptr(w), L.ptr(bias), L.ptr(w2), L.ptr(bias2), L.ptr(out), N, H, W, Cin, Cout, n_out, c2pad,
           ld2, 0, int(relu_out), _DT[x.dtype])
    return out


def pack_conv3x3_weight(w: torch.Tensor, dtype: torch.dtype, cin_pad: int = 0) -> torch.Tensor:
    """nn.Conv2d weight [Cout,Cin,3,3] -> [Cout,3,3,Cin(+pad)] in the operand dtype (tap-major, channel-minor)."""
    wp = w.detach().permute(0, 2, 3, 1)
    if cin_pad > w.shape[1]:
        wp = torch.nn.functional.pad(wp, (0, cin_pad - w.shape[1]))
    if dtype == "split":
        return split_pack_weight(wp.float().contiguous())
    return wp.to(dtype).contiguous()


def pack_conv7x7_rgb_weight(w: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """nn.Conv2d(3, Cout, 7) weight [Cout,3,7,7] -> [Cout, 8, 32] with w[co, dy, dx*3 + c], zeros in columns 21..31 and in the eighth row
    (K = 256 for the 256x256 tile kernel; the 7-row route reads the same buffer with a row stride of 256)."""
    Cout = w.shape[0]
    assert w.shape == (Cout, 3, 7, 7)
    split = dtype == "split"
    wp = torch.zeros(Cout, 8, 32, dtype=torch.float32 if split else dtype, device=w.device)
    wp[:, :7, :21] = w.detach().permute(0, 2, 3, 1).reshape(Cout, 7, 21).to(wp.dtype)
    return split_pack_weight(wp.reshape(Cout, 256)) if split else wp.contiguous()


def pad_rgb_nhwc(frames: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """frames [N,3,H,W] -> zero-bordered NHWC 16-bit image [N, H+6, W+8, 3] (3 before, 3/5 after) for conv7x7_rgb_nhwc;
    the storage carries one padded row + 64 spare halfs behind the last pixel (the last window slices -- and the zero-weight eighth
    kernel row of the 256-tile route -- read past it)."""
    N, C, H, W = frames.shape
    assert C == 3
    Hp, Wp = H + 6, W + 8
    flat = torch.zeros(N * Hp * Wp * 3 + Wp * 3 + 64, dtype=dtype, device=frames.device)
    img = flat[:N * Hp * Wp * 3].view(N, Hp, Wp, 3)
    img[:, 3:3 + H, 3:3 + W] = frames.permute(0, 2, 3, 1)
    return img


def conv7x7_rgb_nhwc(img_padded: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], H: int, W: int,
                     up_add: Optional[torch.Tensor] = None):
    """img_padded from pad_rgb_nhwc, w from pack_conv7x7_rgb_weight -> [N,H,W,Cout] = conv2d(k=7, s=1, p=3) + bias.
    up_add (split class only; [N, H/2, W/2, Cout] f32 contiguous): the Gaussian-parameter head's fusion (dpt_gs_head.py:142-150) -- returns
    the PACKED (hi, lo) activation bilinear_x2(up_add) + relu(conv + bias) as a SplitWeight [N,H,W,Cout] (what
    upsample2x_nhwc(up_add, add=conv, relu_add=True, packed=True) returns) without writing the f32 stem map."""
    if isinstance(w, SplitWeight):     # split operands: f32 image, packed [Cout, 256] weight (pack_conv7x7_rgb_weight(w, "split"))
        dev = L.require_device(img_padded, w.data, bias, up_add)
        N, Hp, Wp, C = img_padded.shape
        Cout = w.shape[0]
        assert C == 3 and img_padded.is_contiguous() and img_padded.dtype == torch.float32 and tuple(w.shape) == (Cout, 256)
        assert img_padded.untyped_storage().nbytes() >= (img_padded.storage_offset() + img_padded.numel() + Wp * 3 + 64) * 4
        if up_add is not None:
            assert up_add.dtype == torch.float32 and up_add.is_contiguous() and tuple(up_add.shape) == (N, H // 2, W // 2, Cout) and bias is not None
            if RANGE_GUARD.enabled:
                RANGE_GUARD.check(f"stem + upsample-add: trunk {Cout} @{H // 2}x{W // 2}", up_add)
            outp = torch.empty((N, H, W, Cout), dtype=torch.int32, device=dev)
            L.call("vs_conv7x7_rgb_split_up_nhwc", dev, L.ptr(img_padded), L.ptr(w.data), w.acc_scale, L.ptr(bias), L.ptr(up_add), L.ptr(outp), N, H,
                   W, Hp, Wp, Cout)
            return SplitWeight(outp, 1.0, outp.shape)
        out = torch.empty((N, H, W, Cout), dtype=torch.float32, device=dev)
        L.call("vs_conv7x7_rgb_split_nhwc", dev, L.ptr(img_padded), L.ptr(w.data), w.acc_scale, L.ptr(bias), L.ptr(out), N, H, W, Hp, Wp, Cout)
        return out
    dev = L.require_device(img_padded, w, bias)
    N, Hp, Wp, C = img_padded.shape
    Cout = w.shape[0]
    assert C == 3 and img_padded.is_contiguous() and w.shape == (Cout, 8, 32) and w.is_contiguous() and img_padded.dtype == w.dtype
    assert img_padded.untyped_storage().nbytes() >= (img_padded.storage_offset() + img_padded.numel() + Wp * 3 + 64) * 2
    out = torch.empty((N, H, W, Cout), dtype=w.dtype, device=dev)
    L.call("vs_conv7x7_rgb_nhwc", dev, L.ptr(img_padded), L.ptr(w), L.ptr(bias), L.ptr(out), N, H, W, Hp, Wp, Cout, _DT[w.dtype])
    return out


def im2col7x7_rgb(frames: torch.Tensor, dtype: torch.dtype, ld: int = 256) -> torch.Tensor:
    """frames [N,3,H,W] f32 -> [N, H*W, ld] rows of the 7x7 / pad 3 windows in (c, ky, kx) order (columns 147.. zero), `dtype` f32 / f16 / bf16:
    F.unfold(frames.to(dtype), 7, padding=3).transpose(1, 2) padded to ld columns, in one pass (vs_im2col7x7_rgb)."""
    dev = L.require_device(frames)
    N, C, H, W = frames.shape
    assert C == 3 and frames.dtype == torch.float32 and frames.is_contiguous() and ld % 8 == 0 and ld >= 148
    out = torch.empty((N, H * W, ld), dtype=dtype, device=dev)
    L.call("vs_im2col7x7_rgb", dev, L.ptr(frames), L.ptr(out), N, H, W, ld, {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}[dtype])
    return out


def stem7x7_up_split_stream(img_padded: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, H: int, W: int, up_add: torch.Tensor, scale_exp: int):
    """conv7x7_rgb_nhwc(img_padded, pack(w), bias, H, W, up_add=up_add) of the split class as the streaming kernel (csrc/stem_stream.hip):
    w = the module's [256, 3, 7, 7] f32 parameter (packed in the kernel with 2^scale_exp), returns the packed SplitWeight [N,H,W,256]."""
    dev = L.require_device(img_padded, w, bias, up_add)
    N, Hp, Wp, C = img_padded.shape
    Cout = w.shape[0]
    assert C == 3 and img_padded.is_contiguous() and img_padded.dtype == torch.float32 and w.dtype == torch.float32 and w.is_contiguous()
    assert tuple(w.shape) == (256, 3, 7, 7) and W % 32 == 0 and H % 2 == 0 and bias.dtype == torch.float32 and bias.is_contiguous()
    assert up_add.dtype == torch.float32 and up_add.is_contiguous() and tuple(up_add.shape) == (N, H // 2, W // 2, Cout)
    if RANGE_GUARD.enabled:
        RANGE_GUARD.check(f"stem + upsample-add: trunk {Cout} @{H // 2}x{W // 2}", up_add)
    outp = torch.empty((N, H, W, Cout), dtype=torch.int32, device=dev)
    nwg = max(1, min(N * (W // 32), torch.cuda.get_device_properties(dev).multi_processor_count))
    L.call("vs_stem7x7_up_split_stream", dev, L.ptr(img_padded), L.ptr(w), int(scale_exp), L.ptr(bias), L.ptr(up_add), L.ptr(outp), N, H, W, Hp, Wp,
           Cout, nwg)
    return SplitWeight(outp, 1.0, outp.shape)


def upsample2x_nhwc(x: torch.Tensor, add: Optional[torch.Tensor] = None, relu_add: bool = False, packed: bool = False):
    """Bilinear x2, align_corners=True, on [N,H,W,C] contiguous 16-bit / f32; optional fused `+ add` / `+ relu(add)`.
    packed=True (f32 input, C % 32 == 0): the result is written in the packed (hi, lo) form of the split class and returned as a SplitWeight
    of shape [N,2H,2W,C] -- the operand of a split convolution that then skips its in-loop conversion."""
    dev = L.require_device(x, add)
    assert x.dim() == 4 and x.is_contiguous() and x.dtype in _OPERAND_DTYPES
    N, H, W, Cc = x.shape
    assert not packed or (x.dtype == torch.float32 and Cc % 32 == 0 and H >= 2 and W >= 2)
    out = torch.empty((N, 2 * H, 2 * W, Cc), dtype=torch.int32 if packed else x.dtype, device=dev)
    assert add is None or (add.shape == out.shape and add.is_contiguous() and add.dtype == x.dtype)
    L.call("vs_upsample2x_nhwc", dev, L.ptr(x), L.ptr(add), L.ptr(out), N, H, W, Cc, int(relu_add) | (16 if packed else 0), _DTX[x.dtype])
    return SplitWeight(out, 1.0, out.shape) if packed else out


# ---------------------------------------------------------------------------------------------------------------------
# Encoder backward building blocks: parity-tested against torch autograd (tests/test_ops_gpu.py), assembled into
# torch.autograd.Functions in vicasplat_amd/autograd.py.
# ---------------------------------------------------------------------------------------------------------------------
_DT3 = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def transpose16(x: torch.Tensor, pad_to: int = 1, *, colsum_out: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                border_hw: Optional[tuple] = None, relu: bool = False, slices: int = 1, halo: int = 0) -> torch.Tensor:
    """x [R,C] 16-bit (row stride any) -> [C, Rpad] with Rpad = R rounded up to `pad_to`, padding columns zero.
    colsum_out (f32 [C]) additionally receives the column sums of x (overwritten) from the same pass.
    border_hw = (H, W): x is [n*H*W, C] (NHWC pixels) and the transposed rows are the pixels of the zero-bordered
    [n, H+2, W+2] maps (R = n*(H+2)*(W+2)); relu zeroes negative inputs.  `out` [C, >= Rpad] may be a column-offset view.
    slices > 1: slice-blocked result [slices, C, Rpad/slices + 2*halo] (slice z = rows [z*SL - halo, (z+1)*SL + halo), zeros
    outside [0, R)): the operand layout of gemm_wgrad."""
    dev = L.require_device(x, colsum_out, out)
    assert x.dim() == 2 and x.stride(1) == 1 and x.dtype in (torch.float16, torch.bfloat16)
    R, Cc = x.shape
    bh = bw = 0
    if border_hw is not None:
        bh, bw = border_hw
        assert R % (bh * bw) == 0
        R = R // (bh * bw) * (bh + 2) * (bw + 2)
    Rpad = (R + pad_to - 1) // pad_to * pad_to
    if slices > 1:
        assert out is None and Rpad % slices == 0
        out = torch.empty((slices, Cc, Rpad // slices + 2 * halo), dtype=x.dtype, device=dev)
        ld_out, sstride = out.stride(1), out.stride(0)
    else:
        assert halo == 0
        if out is None:
            out = torch.empty((Cc, Rpad), dtype=x.dtype, device=dev)
        else:
            assert out.dtype == x.dtype and out.shape[0] == Cc and out.stride(1) == 1 and out.shape[1] >= Rpad
        ld_out, sstride = out.stride(0), 0
    if colsum_out is not None:
        assert colsum_out.dtype == torch.float32 and colsum_out.is_contiguous() and colsum_out.numel() == Cc
    L.call("vs_transpose16_ex", dev, L.ptr(x), x.stride(0), L.ptr(out), ld_out, R, Cc, Rpad, L.ptr(colsum_out), _DT[x.dtype], bh, bw, int(relu),
           slices, halo, sstride)
    return out


def colsum(x: torch.Tensor) -> torch.Tensor:
    """f32 column sums of x [M,N] (f32 / f16 / bf16)."""
    dev = L.require_device(x)
    assert x.dim() == 2 and x.stride(1) == 1
    out = torch.empty(x.shape[1], dtype=torch.float32, device=dev)
    L.call("vs_colsum", dev, L.ptr(x), x.stride(0), L.ptr(out), x.shape[0], x.shape[1], _DT3[x.dtype])
    return out


def gated_resid(x: torch.Tensor, y: torch.Tensor, gate: Optional[torch.Tensor] = None, gate_rows: int = 0, *, grp_in: int = 0,
                grp_out: int = 0, grp_off: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = x + (1 + gate[row // gate_rows]) * y[yrow(row)]: x f32 [M,C] contiguous, y 16-bit [rows,C] (row stride any), gate f32
    [G,C] or None; yrow(m) = (m // grp_in) * grp_out + grp_off + m % grp_in picks y's rows (identity by default)."""
    dev = L.require_device(x, y, gate, out)
    assert x.dim() == 2 and x.is_contiguous() and x.dtype == torch.float32 and y.stride(1) == 1 and y.shape[1] == x.shape[1]
    assert gate is None or (gate.is_contiguous() and gate.dtype == torch.float32 and gate.shape[1] == x.shape[1])
    if out is None:
        out = torch.empty_like(x)
    if y.dtype == torch.float32:      # f32 branch (split / f32 operand classes)
        L.call("vs_gated_resid_f32", dev, L.ptr(x), L.ptr(y), y.stride(0), L.ptr(gate), gate_rows, L.ptr(out), x.shape[0], x.shape[1], grp_in,
               grp_out, grp_off)
        return out
    L.call("vs_gated_resid", dev, L.ptr(x), L.ptr(y), y.stride(0), L.ptr(gate), gate_rows, L.ptr(out), x.shape[0], x.shape[1], grp_in, grp_out,
           grp_off, _DT[y.dtype])
    return out


def gated_resid_backward(dout: torch.Tensor, y: torch.Tensor, gate: Optional[torch.Tensor], gate_rows: int, dy: torch.Tensor, *,
                         grp_in: int = 0, grp_out: int = 0, grp_off: int = 0) -> Optional[torch.Tensor]:
    """Branch-side backward of gated_resid: writes dy[yrow(m)] = dout[m] * (1 + gate) into the given 16-bit buffer (other rows are
    left alone) and returns dgate [G,C] f32 (None without a gate)."""
    dev = L.require_device(dout, y, gate, dy)
    assert dout.dim() == 2 and dout.is_contiguous() and dout.dtype == torch.float32 and dy.stride(1) == 1 and dy.dtype == y.dtype
    dgate = None if gate is None else torch.zeros_like(gate)
    if y.dtype == torch.float32:
        L.call("vs_gated_resid_backward_f32", dev, L.ptr(dout), L.ptr(y), y.stride(0), L.ptr(gate), gate_rows, L.ptr(dy), dy.stride(0), L.ptr(dgate),
               dout.shape[0], dout.shape[1], grp_in, grp_out, grp_off)
        return dgate
    L.call("vs_gated_resid_backward", dev, L.ptr(dout), L.ptr(y), y.stride(0), L.ptr(gate), gate_rows, L.ptr(dy), dy.stride(0), L.ptr(dgate),
           dout.shape[0], dout.shape[1], grp_in, grp_out, grp_off, _DT[y.dtype])
    return dgate


def gelu16(z: torch.Tensor) -> torch.Tensor:
    """gelu_erf(z) on a contiguous f16 / bf16 tensor (numel % 8 == 0) or f32 tensor (numel % 4 == 0), in the dtype of z."""
    dev = L.require_device(z)
    assert z.is_contiguous() and z.dtype in (torch.float16, torch.bfloat16, torch.float32)
    out = torch.empty_like(z)
    if z.dtype == torch.float32:
        L.call("vs_gelu_f32", dev, L.ptr(z), L.ptr(out), z.numel())
        return out
    L.call("vs_gelu16", dev, L.ptr(z), L.ptr(out), z.numel(), _DT[z.dtype])
    return out


def gelu_backward(dy: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
    """dz = dy * gelu_erf'(z); dy, z contiguous of the same shape and dtype: f16 / bf16 (numel % 8 == 0) or f32 (numel % 4 == 0)."""
    dev = L.require_device(dy, z)
    assert dy.shape == z.shape and dy.dtype == z.dtype and dy.is_contiguous() and z.is_contiguous()
    dz = torch.empty_like(dy)
    if z.dtype == torch.float32:
        L.call("vs_gelu_backward_f32", dev, L.ptr(dy), L.ptr(z), L.ptr(dz), dy.numel())
        return dz
    L.call("vs_gelu_backward", dev, L.ptr(dy), L.ptr(z), L.ptr(dz), dy.numel(), _DT[dy.dtype])
    return dz


def layernorm_backward(dout: torch.Tensor, x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, *, scale: Optional[torch.Tensor] = None,
                       mod_rows: int = 0, eps: float = 1e-6, dx: Optional[torch.Tensor] = None, accumulate_dx: bool = False,
                       grp_in: int = 0, grp_out: int = 0, grp_off: int = 0, dx_add: Optional[torch.Tensor] = None,
                       dx16: Optional[torch.Tensor] = None):
    """Backward of layernorm_mod.  x f32 [M,C]; dout [rows,C] in the forward's output layout (f32 or 16-bit).
    Returns (dx f32 [M,C], dw [C], db [C], dscale [G,C] | None, dshift [G,C] | None).  dx_add [M,C] f32: gradient arriving through the
    residual connection, added into dx (accumulate_dx=True is dx_add = dx); dx16 [M,C] 16-bit: receives a copy of dx for the next GEMMs."""
    dev = L.require_device(dout, x, w, b, scale, dx, dx_add, dx16)
    M, Cc = x.shape
    assert x.dtype == torch.float32 and x.stride(1) == 1 and dout.stride(-1) == 1
    if dx is None:
        assert not accumulate_dx
        dx = torch.empty((M, Cc), dtype=torch.float32, device=dev)
    if accumulate_dx:
        assert dx_add is None
        dx_add = dx
    assert dx_add is None or (dx_add.dtype == torch.float32 and dx_add.stride(1) == 1 and dx_add.shape == (M, Cc))
    assert dx16 is None or (dx16.dtype in (torch.float16, torch.bfloat16) and dx16.stride(1) == 1 and dx16.shape == (M, Cc))
    dw, db = torch.zeros((2, Cc), dtype=torch.float32, device=dev).unbind(0)      # (one fill for the pair: the accumulators of f32 atomics)
    dscale = dshift = None
    mod_ld = 0
    if scale is not None:
        assert scale.dtype == torch.float32 and scale.stride(-1) == 1
        mod_ld = scale.stride(0)
        # dscale / dshift are written with the row stride of `scale`: allocate [G, mod_ld] when the rows are wider than C
        dscale, dshift = torch.zeros((2, scale.shape[0], mod_ld if mod_ld != Cc else Cc), dtype=torch.float32, device=dev).unbind(0)
    L.call("vs_layernorm_backward_ex", dev, L.ptr(dout), dout.stride(-2), _DT3[dout.dtype], L.ptr(x), x.stride(0), L.ptr(w), L.ptr(b), L.ptr(scale),
           mod_rows, mod_ld, L.ptr(dx), dx.stride(0), L.ptr(dx_add), dx_add.stride(0) if dx_add is not None else 0, L.ptr(dx16),
           dx16.stride(0) if dx16 is not None else 0, _DT[dx16.dtype] if dx16 is not None else 0, L.ptr(dw), L.ptr(db), L.ptr(dscale), L.ptr(dshift),
           M, Cc, eps, grp_in, grp_out, grp_off)
    if dscale is not None and dscale.shape[1] != Cc:
        dscale, dshift = dscale[:, :Cc], dshift[:, :Cc]
    return dx, dw, db, dscale, dshift


def linear_backward(dy: torch.Tensor, x: torch.Tensor, w: torch.Tensor, *, need_dx: bool = True, need_dw: bool = True,
                    need_db: bool = True, wT: Optional[torch.Tensor] = None):
    """Backward of y = x @ w^T + b on the NT GEMM kernels: dy [M,N], x [M,K], w [N,K] 16-bit.
    dx = dy @ w (16-bit), dw = dy^T @ x (f32, f32 accumulation over M), db = column sums of dy (f32).
    `wT` = transpose16(w, 64) can be cached by the caller (weights change once per optimiser step)."""
    M, N = dy.shape
    K = x.shape[1]
    dev = dy.device
    r = linear_backward_route("f16", M, N, K, need_dx=need_dx, need_dw=need_dw, need_db=need_db, dy_ld=dy.stride(0), x_ld=x.stride(0),
                              aligned16=dy.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0)
    dx = dw = db = None
    if r.dx == "nt":
        if wT is None:
            wT = transpose16(w, 64)                       # [K, Npad]: reduction over N
        dyp = dy if N % 64 == 0 else torch.nn.functional.pad(dy, (0, wT.shape[1] - N))
        dx = torch.empty((M, K), dtype=dy.dtype, device=dev)
        gemm(dyp, wT, None, dx, EPI_STORE16)
    # dw: a reduction over the M rows -- few output tiles, a very long K, split over workgroups (partial tiles + reduce kernel)
    if r.wgrad is not None:
        dw = torch.empty((N, K), dtype=torch.float32, device=dev)
    if r.wgrad in ("tn256", "tn_skinny"):         # the reduction-major kernel reads dY and X as they are (LDS transpose reads), no transposed copies
        gemm_wgrad_tn(dy, x, dw, r.ksplit, accumulate=False)
    elif r.wgrad == "transposed":                 # slice-blocked [ks, N, pad/ks], [ks, K, pad/ks], zero padded
        if r.db == "on_transpose":
            db = torch.empty(N, dtype=torch.float32, device=dev)
        dyT, xT = transpose16(dy, r.pad, colsum_out=db, slices=r.ksplit), transpose16(x, r.pad, slices=r.ksplit)
        gemm_wgrad(dyT, xT, dw, r.ksplit, accumulate=False)
    if r.db == "colsum":
        db = colsum(dy)
    elif r.db == "colsum_padded":                 # rows padded with zeros up to a multiple of 8 (gaussian_adapter_backward): 16-byte loads
        db = colsum(torch.as_strided(dy, (M, round_up(N, 8)), (dy.stride(0), 1)))[:N].contiguous()
    return dx, dw, db


def relu_mask_(dx: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """In place dx = x > 0 ? dx : 0 (contiguous 16-bit, same shape): backward of a ReLU applied to x."""
    dev = L.require_device(dx, x)
    assert dx.shape == x.shape and dx.dtype == x.dtype and dx.is_contiguous() and x.is_contiguous()
    L.call("vs_relu_mask16", dev, L.ptr(dx), L.ptr(x), dx.numel())
    return dx


def relu_mask(dy: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """x > 0 ? dy : 0 into a new tensor (contiguous f16 / bf16 with numel % 8 == 0 or f32 with numel % 4 == 0, same shape): ReLU backward that
    leaves the incoming gradient intact."""
    dev = L.require_device(dy, x)
    assert dy.shape == x.shape and dy.dtype == x.dtype and dy.is_contiguous() and x.is_contiguous()
    out = torch.empty_like(dy)
    if x.dtype == torch.float32:
        L.call("vs_relu_mask_f32", dev, L.ptr(dy), L.ptr(x), L.ptr(out), dy.numel())
        return out
    L.call("vs_relu_mask16_to", dev, L.ptr(dy), L.ptr(x), L.ptr(out), dy.numel())
    return out


def gemm_wgrad(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, ksplit: int, *, shifts=None, K: Optional[int] = None,
               workspace: bool = True, accumulate: bool = True) -> torch.Tensor:
    """out32[t][M,N] += a[M,K] @ (w shifted by shifts[t])[N,K]^T, K split over `ksplit` workgroups per tile (vs_gemm_wgrad).
    a, w: 2-D [rows, K] (slice s = columns [s K/ksplit, ...)) or slice-blocked 3-D [ksplit, rows, K/ksplit] as transpose16(slices=)
    writes them (w may be a column-offset view into a wider halo'd buffer; K = ksplit * slice length then).
    out is [M,N] (shifts None) or [len(shifts),M,N] contiguous.  workspace: the K slices store partial tiles that a second
    kernel sums (default); False: they meet through f32 atomics.  accumulate=False (workspace mode) overwrites out: no zero fill."""
    dev = L.require_device(a, w, out)
    assert a.dtype == w.dtype and a.stride(-1) == 1 and w.stride(-1) == 1 and out.dtype == torch.float32 and out.is_contiguous()
    assert a.dim() == w.dim()
    asl = wsl = 0
    if a.dim() == 3:
        assert a.shape[0] == ksplit and w.shape[0] == ksplit and a.shape[2] == w.shape[2]
        if ksplit == 1:
            a, w = a[0], w[0]
        else:
            asl, wsl = a.stride(0), w.stride(0)
            K = ksplit * a.shape[2] if K is None else K
    K = a.shape[-1] if K is None else K
    M, N = a.shape[-2], w.shape[-2]
    ntaps = 0 if shifts is None else len(shifts)
    assert out.shape == ((M, N) if shifts is None else (ntaps, M, N))
    sh = None if shifts is None else (ctypes.c_int32 * ntaps)(*shifts)
    ws, ws_bytes = None, 0
    if workspace:
        ws = torch.empty(max(2, ksplit) * max(1, ntaps) * M * N, dtype=torch.float32, device=dev)
        ws_bytes = ws.numel() * 4
    L.call("vs_gemm_wgrad", dev, L.ptr(a), L.ptr(w), L.ptr(out), M, N, K, a.stride(-2), w.stride(-2), N, asl, wsl, M * N, sh, ntaps, ksplit,
           _DT[a.dtype], L.ptr(ws), ws_bytes, int(accumulate))
    return out


def gemm_wgrad_tn(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, ksplit: int, *, workspace: bool = True, accumulate: bool = True):
    """out32[M,N] (+)= a^T @ w for reduction-major operands a [Kred, M], w [Kred, N] (16-bit, 16-byte aligned, row strides multiples of 8 that
    cover M / N): the weight gradient dW = dY^T X without transposed copies (vs_gemm_wgrad_tn).  Any M, N: 256 x 256 tiles, columns past the
    rows' storage read as zeros; any Kred: the last of the ksplit slices is zero-filled.  accumulate=False needs the workspace."""
    dev = L.require_device(a, w, out)
    assert a.dtype == w.dtype and a.stride(1) == 1 and w.stride(1) == 1 and a.shape[0] == w.shape[0]
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape == (a.shape[1], w.shape[1])
    M, N, Kred = a.shape[1], w.shape[1], a.shape[0]
    ws, ws_bytes = None, 0
    if workspace:
        ws = torch.empty(ksplit * M * N, dtype=torch.float32, device=dev)
        ws_bytes = ws.numel() * 4
    L.call("vs_gemm_wgrad_tn", dev, L.ptr(a), L.ptr(w), L.ptr(out), M, N, Kred, a.stride(0), w.stride(0), N, ksplit, _DT[a.dtype], L.ptr(ws),
           ws_bytes, int(accumulate))
    return out


def gemm_splitk_accumulate(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, ksplit: int, *, K: Optional[int] = None) -> torch.Tensor:
    """out32 [M,N] += a[M,K] @ w[N,K]^T with K split over `ksplit` workgroups per tile, f32 atomics (vs_gemm_splitk_accumulate)."""
    dev = L.require_device(a, w, out)
    assert a.dtype == w.dtype and a.stride(1) == 1 and w.stride(1) == 1 and out.dtype == torch.float32
    K = a.shape[1] if K is None else K
    L.call("vs_gemm_splitk_accumulate", dev, L.ptr(a), L.ptr(w), L.ptr(out), a.shape[0], w.shape[0], K, a.stride(0), w.stride(0), out.stride(0),
           ksplit, _DT[a.dtype])
    return out


def conv3x3_backward(dy: torch.Tensor, x: torch.Tensor, w: torch.Tensor, *, relu_in: bool = False, need_dx: bool = True,
                     need_db: bool = True):
    """Backward of conv3x3_nhwc(x, w, bias, relu_in=relu_in) (stride 1, pad 1) for the gradient dy of its pre-activation output.
    dy [N,H,W,Cout], x [N,H,W,Cin] (the conv input, before the fused input ReLU), w [Cout,3,3,Cin], all 16-bit NHWC.
    Returns dx [N,H,W,Cin] 16-bit, dw [Cout,3,3,Cin] f32, db [Cout] f32.
      dx: the same implicit-GEMM kernel on dy with the spatially flipped, channel-transposed weights;
      dw, db: the route conv3x3_backward_route names -- either way a tap is a shift of an operand, so no im2col buffer exists here either."""
    N, H, W, Cin = x.shape
    Cout = w.shape[0]
    dev, dt = x.device, x.dtype
    dx = None
    if need_dx:
        wd = w.flip(1, 2).permute(3, 1, 2, 0).contiguous()          # [Cin, 3, 3, Cout]
        dx = conv3x3_nhwc(dy.contiguous(), wd, None, mask_by=x if relu_in else None)   # ReLU backward in the conv epilogue
    r = conv3x3_backward_route("f16", N, H, W, Cin, Cout, contiguous=x.is_contiguous() and dy.is_contiguous(), need_dx=need_dx, need_db=need_db)
    ks, P = r.ksplit, N * H * W
    if r.wgrad in ("tn", "tn_grouped"):
        # the reduction-major kernel reads the NHWC tensors as they are (tap shift = pixel-row shift, zero page outside the image, input
        # ReLU on the fragments) -- no zero-bordered transposed copies
        dw9 = torch.empty((9, Cin, Cout), dtype=torch.float32, device=dev)
        ws = torch.empty(ks * 9 * Cin * Cout, dtype=torch.float32, device=dev)
        L.call("vs_conv3x3_wgrad_tn", dev, L.ptr(x), L.ptr(dy), L.ptr(dw9), N, H, W, Cin, Cout, int(relu_in), ks, _DT[dt], L.ptr(ws), ws.numel() * 4,
               0)
        dw = dw9.view(3, 3, Cin, Cout).permute(3, 0, 1, 2).contiguous()            # [Cout, ky, kx, Cin]
        return dx, dw, (colsum(dy.view(P, Cout)) if r.db else None)
    # transposed: dY^T [Cout, pixels] and X^T [Cin, pixels] over the zero-bordered pixel grid, produced straight from the NHWC
    # tensors by the transposing kernel (border, input ReLU and the bias gradient folded into that one pass)
    shifts, halo = bordered_taps(W, 8)
    xT = transpose16(x.view(P, Cin), r.pad, border_hw=(H, W), relu=relu_in, slices=ks, halo=halo if ks > 1 else 0)
    if ks == 1:     # whole 256-tiles of a small map that missed `tn` (a strided x or dy): one slice is a plain 2-D operand, its halo added here
        xT = torch.nn.functional.pad(xT, (halo, halo)).unsqueeze(0)
    db = torch.empty(Cout, dtype=torch.float32, device=dev)
    dyT = transpose16(dy.contiguous().view(P, Cout), r.pad, colsum_out=db, border_hw=(H, W), slices=ks)
    if ks == 1:
        dyT = dyT.unsqueeze(0)
    # all 9 taps in ONE launch (workgroup order: k-slice, tap, tile): the taps of a K slice run together, so A and the nine
    # overlapping shifted views of X^T are served from the caches instead of being streamed from HBM nine times
    dw9 = torch.empty((9, Cout, Cin), dtype=torch.float32, device=dev)
    gemm_wgrad(dyT, xT[:, :, halo:halo + r.pad // ks], dw9, ks, shifts=shifts, accumulate=False)
    dw = dw9.view(3, 3, Cout, Cin).permute(2, 0, 1, 3).contiguous()
    return dx, dw, db


def upsample2x_backward_nhwc(dout: torch.Tensor) -> torch.Tensor:
    """Backward of upsample2x_nhwc (no add): dout [N,2H,2W,C] contiguous f16 / bf16 (C % 8 == 0) or f32 (C % 4 == 0) -> din [N,H,W,C]."""
    dev = L.require_device(dout)
    assert dout.dim() == 4 and dout.is_contiguous() and dout.dtype in (torch.float16, torch.bfloat16, torch.float32)
    N, Ho, Wo, Cc = dout.shape
    din = torch.empty((N, Ho // 2, Wo // 2, Cc), dtype=dout.dtype, device=dev)
    if dout.dtype == torch.float32:
        L.call("vs_upsample2x_backward_f32_nhwc", dev, L.ptr(dout), L.ptr(din), N, Ho // 2, Wo // 2, Cc)
        return din
    L.call("vs_upsample2x_backward_nhwc", dev, L.ptr(dout), L.ptr(din), N, Ho // 2, Wo // 2, Cc, _DT[dout.dtype])
    return din


# ------------------------------------------------------------------------------------------------------------------------------
# Split-class backward (reference precision: f32 tensors, three f16 MFMAs per product; csrc/split_bwd.hip, gemm.hip, attention_bwd.hip).
# Gradients must sit in the f16 range (|g| < 65504, typical magnitude >~ 1e-2 for full precision): callers.training_step keeps its
# power-of-two loss scale for this class too.
# ------------------------------------------------------------------------------------------------------------------------------
def _border_rows(R, conv_hw, border):
    if not border:
        return R
    h, w = conv_hw
    assert R % (h * w) == 0
    return R // (h * w) * (h + 2) * (w + 2)


def transpose_f32(x: torch.Tensor, pad_to: int = 64, *, relu: bool = False, conv_hw: Optional[tuple] = None, tap: tuple = (0, 0),
                  border: bool = False, halo: int = 0, colsum: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [R,C] f32 (row stride any multiple of 4 or contiguous) -> [C, Rpad] f32, Rpad = R rounded up to pad_to (a multiple of 64), zero padded.
    conv_hw = (H, W) with tap = (dy, dx): row r reads pixel r shifted by the tap, zero outside its image.  border=True: the transposed
    rows are the pixels of the zero-bordered (H+2) x (W+2) maps; halo > 0 (a multiple of 4): the result is the middle of a zero buffer with
    `halo` readable zero columns on both sides (the operand whose shifted views the tap-fused weight gradient reads).
    colsum (f32 [C], overwritten): the column sums of x -- the bias gradient, on the pass that reads dY anyway."""
    dev = L.require_device(x)
    assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == torch.float32 and pad_to % 64 == 0 and halo % 4 == 0
    assert colsum is None or (colsum.dtype == torch.float32 and colsum.is_contiguous() and colsum.numel() == x.shape[1])
    R, Cc = x.shape
    Rb = _border_rows(R, conv_hw, border)
    Rpad = (Rb + pad_to - 1) // pad_to * pad_to
    if halo:
        buf = torch.empty((Cc, halo + Rpad + halo), dtype=torch.float32, device=dev)     # (the kernel writes all Rpad columns: only the halos need zeros)
        buf[:, :halo].zero_()
        buf[:, halo + Rpad:].zero_()
        out = buf[:, halo:halo + Rpad]
    else:
        out = torch.empty((Cc, Rpad), dtype=torch.float32, device=dev)
    h, w = conv_hw if conv_hw is not None else (0, 0)
    dy, dx = (2, 0) if border else tap
    L.call("vs_transpose_f32", dev, L.ptr(x), x.stride(0), L.ptr(out), out.stride(0), Rb, Cc, Rpad, int(relu), h, w, dy, dx, L.ptr(colsum))
    return out


def transpose_pack_split(x: torch.Tensor, pad_to: int = 64, *, relu: bool = False, conv_hw: Optional[tuple] = None, tap: tuple = (0, 0),
                         scale_exp: int = 0, border: bool = False, colsum: Optional[torch.Tensor] = None) -> SplitWeight:
    """transpose_f32 written as the packed split "weight" operand [C, Rpad] (SplitWeight, acc_scale = 2^-scale_exp)."""
    dev = L.require_device(x)
    assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == torch.float32 and pad_to % 64 == 0
    R, Cc = x.shape
    R = _border_rows(R, conv_hw, border)
    Rpad = (R + pad_to - 1) // pad_to * pad_to
    out = torch.empty((Cc, Rpad), dtype=torch.int32, device=dev)
    h, w = conv_hw if conv_hw is not None else (0, 0)
    if border:
        tap = (2, 0)
    L.call("vs_transpose_pack_split", dev, L.ptr(x), x.stride(0), L.ptr(out), out.stride(0), R, Cc, Rpad, int(relu), h, w, tap[0], tap[1], scale_exp,
           L.ptr(colsum))
    return SplitWeight(out, 2.0 ** (-scale_exp), (Cc, Rpad))


def split16(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """f32 [rows, C] (row stride any multiple of 4) -> (hi, lo) f16 [rows, C] contiguous: hi = rne16(x), lo = rne16(x - hi)."""
    dev = L.require_device(x)
    assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == torch.float32 and x.shape[1] % 8 == 0
    hi = torch.empty(x.shape, dtype=torch.float16, device=dev)
    lo = torch.empty_like(hi)
    L.call("vs_split16", dev, L.ptr(x), x.stride(0), L.ptr(hi), L.ptr(lo), hi.stride(0), x.shape[0], x.shape[1])
    return hi, lo


def gemm_wgrad_split(a: torch.Tensor, w: SplitWeight, out: torch.Tensor, ksplit: int, shifts=None) -> torch.Tensor:
    """out32 [M,N] = a [M,K] @ w [N,K]^T in the split class, the reduction cut into ksplit slices (vs_gemm_wgrad, dtype 4; partial
    tiles in a workspace + a reduce kernel).  K % (64 * ksplit) == 0.  shifts (<= 9 column offsets, in floats): out [len(shifts), M, N],
    tap t reads `a` shifted by shifts[t] columns -- `a` must be a view with that many readable (zero) columns on both sides."""
    wd = w.data
    dev = L.require_device(a, wd, out)
    assert a.dtype == torch.float32 and a.dim() == 2 and a.stride(1) == 1 and wd.dim() == 2 and wd.stride(1) == 1 and a.shape[1] == wd.shape[1]
    M, N, K = a.shape[0], wd.shape[0], a.shape[1]
    ntaps = 0 if shifts is None else len(shifts)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape == ((M, N) if shifts is None else (ntaps, M, N))
    assert K % (64 * ksplit) == 0, (K, ksplit)
    sh = None if shifts is None else (ctypes.c_int32 * ntaps)(*shifts)
    ws = torch.empty(max(2, ksplit) * max(1, ntaps) * M * N, dtype=torch.float32, device=dev)
    L.call("vs_gemm_wgrad", dev, L.ptr(a), L.ptr(wd), L.ptr(out), M, N, K, a.stride(0), wd.stride(0), N, 0, 0, M * N, sh, ntaps, ksplit, 4, L.ptr(ws),
           ws.numel() * 4, 0)
    if w.acc_scale != 1.0:
        out.mul_(w.acc_scale)
    return out


def gemm_wgrad_split_atn(a: torch.Tensor, w: SplitWeight, out: torch.Tensor, ksplit: int, *, transpose_out: bool = False) -> torch.Tensor:
    """out32 [M,N] (or [N,M] with transpose_out) = a^T @ w^T in the split class: a [Kred, M] f32 AS IT IS in memory (reduction-major), w the packed
    transposed other operand [N, Kpad] (transpose_pack_split); M, N multiples of 256, Kpad % (64 * ksplit) == 0 (vs_gemm_wgrad_split_atn)."""
    wd = w.data
    dev = L.require_device(a, wd, out)
    assert a.dtype == torch.float32 and a.dim() == 2 and a.stride(1) == 1 and wd.dim() == 2 and wd.stride(1) == 1
    Kred, M = a.shape
    N, Kpad = wd.shape
    assert Kpad >= Kred and Kpad % (64 * ksplit) == 0 and M % 256 == 0 and N % 256 == 0, (a.shape, wd.shape, ksplit)
    assert out.dtype == torch.float32 and out.stride(1) == 1 and out.shape == ((N, M) if transpose_out else (M, N))
    ws = torch.empty(ksplit * M * N, dtype=torch.float32, device=dev)
    L.call("vs_gemm_wgrad_split_atn", dev, L.ptr(a), L.ptr(wd), L.ptr(out), M, N, Kred, Kpad, a.stride(0), wd.stride(0), out.stride(0), ksplit,
           int(transpose_out), L.ptr(ws), ws.numel() * 4, 0)
    if w.acc_scale != 1.0:
        out.mul_(w.acc_scale)
    return out


def _rows16_f32(t: torch.Tensor) -> torch.Tensor:
    """t, or a contiguous copy where its f32 rows are not 16-byte aligned."""
    return t if (t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0) else t.contiguous()


def linear_backward_split(dy: torch.Tensor, x: torch.Tensor, w: torch.Tensor, *, need_dx: bool = True, need_dw: bool = True, need_db: bool = True,
                          scale_exp: Optional[int] = None, dgelu_z: Optional[torch.Tensor] = None):
    """Backward of y = x @ w^T + b in the split class: dy [M,N], x [M,K], w [N,K] all f32 -> dx [M,K], dw [N,K], db [N] f32.
    dx = vs_gemm_split(dy, pack(w^T)); dw = dy^T x over the M rows; db = column sums: each on the route linear_backward_route names.
    dgelu_z [M,K] f32 (x = gelu(z), the MLP's second linear): the returned dx is the gradient of z, dy w^T * GELU'(z), multiplied in the dX
    GEMM's epilogue (vs_gemm_split epilogue 5) instead of a separate pass over dx and z."""
    M, N = dy.shape
    K = x.shape[1]
    dev = dy.device
    assert dy.dtype == torch.float32 and x.dtype == torch.float32 and dy.stride(1) == 1 and x.stride(1) == 1
    wf = w.detach().float() if need_dx else None
    r = linear_backward_route("split", M, N, K, need_dx=need_dx, need_dw=need_dw, need_db=need_db, scale_exp_known=scale_exp is not None,
                              w_contiguous=need_dx and wf.is_contiguous(),
                              dgelu=None if dgelu_z is None else dgelu_z.shape == (M, K) and dgelu_z.is_contiguous() and dgelu_z.dtype == torch.float32)
    dx = dw = db = None
    if r.dx == "pack_t":
        dyp = _rows16_f32(dy)
        wtp = transpose_pack_split(wf, 64, scale_exp=int(scale_exp))          # pack(w^T) in one pass: no transposed f32 copy of the weight
    elif r.dx == "padded":
        if N % 32 != 0:
            wt, dyp = torch.nn.functional.pad(wf.t(), (0, (-N) % 32)), torch.nn.functional.pad(dy, (0, (-N) % 32))
        else:
            wt, dyp = wf.t(), _rows16_f32(dy)
        wtp = split_pack_weight(wt.contiguous(), scale_exp)
    if r.dx is not None:
        dx = torch.empty((M, K), dtype=torch.float32, device=dev)
        if r.dgelu == "epilogue":
            _gemm_split(dyp, wtp, None, dx, 5, resid=dgelu_z)
        else:
            _gemm_split(dyp, wtp, None, dx, EPI_STORE32)
            if r.dgelu == "pass":
                dx = gelu_backward(dx, dgelu_z.contiguous())
    if r.wgrad is not None:
        dys, xs = _rows16_f32(dy), _rows16_f32(x)
        if r.db == "on_transpose":
            db = torch.empty(N, dtype=torch.float32, device=dev)
        dw = torch.empty((N, K), dtype=torch.float32, device=dev)
    if r.wgrad == "atn256":         # dW^T [K, N] = X^T dY with X read as it is (reduction-major A operand); only dY goes through a transposing (packing) pass
        gemm_wgrad_split_atn(xs, transpose_pack_split(dys, r.pad, colsum=db), dw, r.ksplit, transpose_out=True)      # dY^T [N, pad] packed
    elif r.wgrad == "transposed":
        dyT = transpose_f32(dys, r.pad, colsum=db)      # [N, pad]
        gemm_wgrad_split(dyT, transpose_pack_split(xs, r.pad), dw, r.ksplit)      # X^T [K, pad] packed
    if r.db == "colsum":
        db = colsum(dy)
    return dx, dw, db


def head1x1_backward(dy: torch.Tensor, t: torch.Tensor, w: torch.Tensor, *, relu: bool = True, scale_exp: int = 0):
    """Backward of y = t @ w^T + b (the last 1x1 convolution of a DPT head) fused with the ReLU backward of t = relu(...), ONE pass over the
    full-resolution tensors (csrc/head_bwd.hip).  dy [P, Cout] (row stride >= Cout allowed: aligned rows of the adapter's backward), t [P, Cin]
    contiguous, both f32 (split class: three f16 MFMAs per product, w packed with 2^scale_exp) or both f16 / bf16; w [Cout, Cin] f32 ->
    dt [P, Cin] = (t > 0) * (dy @ w) in t's dtype, dw [Cout, Cin] = dy^T t and db [Cout] in f32 (per-workgroup partials summed here)."""
    dev = L.require_device(dy, t, w)
    P, Cout = dy.shape
    Cin = t.shape[1]
    assert dy.dtype == t.dtype and w.dtype == torch.float32 and dy.stride(1) == 1 and t.is_contiguous() and w.is_contiguous()
    assert t.shape[0] == P and w.shape == (Cout, Cin) and P % 32 == 0 and Cin in (128, 256) and 1 <= Cout <= 96
    split = dy.dtype == torch.float32
    ldy = dy.stride(0)
    assert Cout <= ldy <= 128 and dy.data_ptr() % 16 == 0
    rows = 96 if Cout > 16 else 16
    per_cu = 2 if (Cin == 128 and Cout <= 16) else 1        # resident workgroups per CU (101 / 206 VGPRs x 8 waves)
    nwg = max(1, min(P // 32, per_cu * torch.cuda.get_device_properties(dev).multi_processor_count))
    dt = torch.empty_like(t)
    dw_part = torch.empty((nwg, rows, Cin), dtype=torch.float32, device=dev)
    db_part = torch.empty((nwg, rows), dtype=torch.float32, device=dev)
    if split:
        L.call("vs_head1x1_backward_split", dev, L.ptr(dy), ldy, L.ptr(t), L.ptr(w), int(scale_exp), L.ptr(dt), L.ptr(dw_part), L.ptr(db_part), P, Cin,
               Cout, int(relu), nwg)
    else:
        L.call("vs_head1x1_backward16", dev, L.ptr(dy), ldy, L.ptr(t), L.ptr(w), L.ptr(dt), L.ptr(dw_part), L.ptr(db_part), P, Cin, Cout, int(relu),
               nwg, _DTX[dy.dtype])
    return dt, dw_part.sum(0)[:Cout].contiguous(), db_part.sum(0)[:Cout].contiguous()


def head1x1_backward_split(dy, t, w, *, relu: bool = True, scale_exp: int = 0):
    """head1x1_backward held to the split class: the name tests/test_split_bwd_gpu.py runs vs_head1x1_backward_split under."""
    assert dy.dtype == torch.float32
    return head1x1_backward(dy, t, w, relu=relu, scale_exp=scale_exp)


def attention_backward_split(qkv_q: torch.Tensor, qkv_k: torch.Tensor, qkv_v: torch.Tensor, out: torch.Tensor, dout: torch.Tensor, lse: torch.Tensor, *,
                             nbatch: int, H: int, Lq: int, Lk: int = 0, q_batch_rows: int, k_batch_rows: int = 0,
                             kv_seg: Optional[torch.Tensor] = None, q_kvlen: Optional[torch.Tensor] = None, max_keys: int = 0, scale: float = 0.125,
                             dq_out: Optional[torch.Tensor] = None, dk_out: Optional[torch.Tensor] = None, dv_out: Optional[torch.Tensor] = None):
    """Backward of attention(..., split=True): q / k / v f32 views [rows, H*64] (row stride any), out / dout f32.  Returns (dq, dk, dv) f32;
    dq_out / dk_out / dv_out: views to write into (e.g. the blocks of a packed [rows, 3*H*64] gradient).  With key segments dk / dv are
    accumulated with atomics (zeroed here)."""
    dev = L.require_device(qkv_q, qkv_k, qkv_v, out, dout, lse, kv_seg, q_kvlen)
    Cc = H * 64
    for t in (qkv_q, qkv_k, qkv_v, out, dout):
        assert t.dim() == 2 and t.stride(1) == 1 and t.dtype == torch.float32 and t.shape[1] == Cc
    dout = _rows16_f32(dout)
    qh, ql = split16(qkv_q)
    kh, kl = split16(qkv_k)
    vh, vl = split16(qkv_v)
    dh, dl = split16(dout)
    dq = dq_out if dq_out is not None else torch.empty((qkv_q.shape[0], Cc), dtype=torch.float32, device=dev)
    if kv_seg is None:
        dk = dk_out if dk_out is not None else torch.empty((qkv_k.shape[0], Cc), dtype=torch.float32, device=dev)
        dv = dv_out if dv_out is not None else torch.empty((qkv_v.shape[0], Cc), dtype=torch.float32, device=dev)
    else:       # (dk_out / dv_out given: accumulated where they are wanted -- zeroed here -- instead of in fresh buffers that are copied afterwards)
        dk = dk_out.zero_() if dk_out is not None else torch.zeros((qkv_k.shape[0], Cc), dtype=torch.float32, device=dev)
        dv = dv_out.zero_() if dv_out is not None else torch.zeros((qkv_v.shape[0], Cc), dtype=torch.float32, device=dev)
    for t in (dq, dk, dv):
        assert t.dtype == torch.float32 and t.stride(1) == 1
    delta = torch.empty((qkv_q.shape[0], H), dtype=torch.float32, device=dev)
    L.call("vs_attention_backward_split", dev, L.ptr(qh), L.ptr(ql), L.ptr(kh), L.ptr(kl), L.ptr(vh), L.ptr(vl), L.ptr(dh), L.ptr(dl), L.ptr(out),
           L.ptr(dout), L.ptr(lse), L.ptr(delta), L.ptr(dq), L.ptr(dk), L.ptr(dv), nbatch, H, Lq, Lk, q_batch_rows, k_batch_rows, qh.stride(0),
           kh.stride(0), vh.stride(0), dh.stride(0), out.stride(0), dout.stride(0), dq.stride(0), dk.stride(0), dv.stride(0), L.ptr(kv_seg),
           L.ptr(q_kvlen), max_keys, scale)
    return dq, dk, dv


def conv3x3_wgrad_split_stream(dy: torch.Tensor, x: torch.Tensor, *, relu_in: bool = False):
    """dw9 [9, Cin, Cout] (tap = ky * 3 + kx) and db [Cout] of a 3x3 convolution (stride 1, pad 1) from x [N,H,W,Cin] and dy [N,H,W,Cout] f32 NHWC,
    split class, one streaming pass (vs_conv3x3_wgrad_split_stream); Cin, Cout multiples of 64, W a multiple of 32."""
    dev = L.require_device(dy, x)
    N, H, W, Cin = x.shape
    Cout = dy.shape[3]
    assert dy.dtype == x.dtype == torch.float32 and dy.is_contiguous() and x.is_contiguous() and dy.shape[:3] == x.shape[:3]
    assert Cin % 64 == 0 and Cout % 64 == 0 and W % 32 == 0
    nblk = (Cin // 64) * (Cout // 64)
    items = N * (W // 32)
    workers = max(8, min(torch.cuda.get_device_properties(dev).multi_processor_count // nblk, (items + 7) // 8 * 8) // 8 * 8)
    dw_part = torch.empty((workers, 9, Cin, Cout), dtype=torch.float32, device=dev)
    db_part = torch.empty((workers, Cout), dtype=torch.float32, device=dev)
    L.call("vs_conv3x3_wgrad_split_stream", dev, L.ptr(x), L.ptr(dy), L.ptr(dw_part), L.ptr(db_part), N, H, W, Cin, Cout, int(relu_in), workers)
    return dw_part.sum(0), db_part.sum(0)


def conv3x3_backward_split(dy: torch.Tensor, x: torch.Tensor, w: torch.Tensor, *, relu_in: bool = False, need_dx: bool = True, need_db: bool = True,
                           scale_exp: Optional[int] = None):
    """Backward of conv3x3_nhwc(x, pack(w), relu_in=relu_in) (stride 1, pad 1) in the split class.  dy [N,H,W,Cout], x [N,H,W,Cin] f32 NHWC,
    w the module's [Cout,Cin,3,3] f32 parameter -> dx [N,H,W,Cin], dw [Cout,Cin,3,3], db [Cout], all f32.
      dx: the forward kernel on the spatially flipped, channel-transposed weights (ReLU backward in its epilogue);
      dw, db: the route conv3x3_backward_route names; no im2col buffer on any of them."""
    N, H, W, Cin = x.shape
    Cout = w.shape[0]
    dev = x.device
    assert dy.dtype == torch.float32 and x.dtype == torch.float32 and dy.is_contiguous() and x.is_contiguous()
    dx = None
    if need_dx:
        wd = w.detach().float().flip(2, 3).permute(1, 2, 3, 0).contiguous()          # [Cin, 3, 3, Cout]: flipped taps, channels swapped
        pad_o = (-Cout) % 32
        dyp = dy
        if pad_o:
            wd = torch.nn.functional.pad(wd, (0, pad_o))
            dyp = torch.nn.functional.pad(dy, (0, pad_o))
        wdp = split_pack_weight(wd, scale_exp)
        dx = conv3x3_nhwc(dyp, wdp, None, mask_by=x if relu_in else None)
    r = conv3x3_backward_route("split", N, H, W, Cin, Cout, need_dx=need_dx, need_db=need_db)
    P = N * H * W
    if r.wgrad == "stream":
        # one streaming pass over X and dY as they are (csrc/conv_wgrad_stream.hip) instead of two transposing passes + nine 128 x 128
        # tiles per K slice on the 4-wave kernel
        dw9, db = conv3x3_wgrad_split_stream(dy, x, relu_in=relu_in)
        return dx, dw9.view(3, 3, Cin, Cout).permute(3, 2, 0, 1).contiguous(), (db if r.db else None)
    db = torch.empty(Cout, dtype=torch.float32, device=dev) if r.db else None      # (rides on the transpose of dY)
    dw9 = torch.empty((9, Cin, Cout), dtype=torch.float32, device=dev)
    if r.wgrad == "atn256":
        # X read as it is by the reduction-major A operand (tap shift = pixel-row shift, zero page outside the image): only dY goes through a
        # transposing (packing) pass
        dyTp = transpose_pack_split(dy.view(P, Cout), r.pad, colsum=db)                                     # [Cout, pad] packed
        ws = torch.empty(r.ksplit * 9 * Cin * Cout, dtype=torch.float32, device=dev)
        L.call("vs_conv3x3_wgrad_split_atn", dev, L.ptr(x), L.ptr(dyTp.data), L.ptr(dw9), N, H, W, Cin, Cout, dyTp.data.shape[1], dyTp.data.stride(0),
               int(relu_in), r.ksplit, L.ptr(ws), ws.numel() * 4, 0)
    else:
        # transposed: ONE tap-fused launch over the zero-bordered pixel grid.  A = act(X)^T [Cin, pixels] f32 with a zero halo (the nine tap
        # shifts are column offsets of this operand: LDS-DMA reads any 4-byte aligned f32 address), W = dY^T [Cout, pixels] packed (hi, lo);
        # out[tap] = [Cin, Cout].  Two transposing passes instead of nine packed shifted images.
        shifts, halo = bordered_taps(W, 4)
        xT = transpose_f32(x.view(P, Cin), r.pad, relu=relu_in, conv_hw=(H, W), border=True, halo=halo)     # [Cin, pad] view of the haloed buffer
        dyT = transpose_pack_split(dy.view(P, Cout), r.pad, conv_hw=(H, W), border=True, colsum=db)         # [Cout, pad] packed
        gemm_wgrad_split(xT, dyT, dw9, r.ksplit, shifts=shifts)
    return dx, dw9.view(3, 3, Cin, Cout).permute(3, 2, 0, 1).contiguous(), db                               # [Cout, Cin, ky, kx]


def sustained_mfma_tflops(device, ms_target: float = 40.0) -> float:
    """TFLOP/s the chip sustains on back-to-back v_mfma_f32_16x16x32_f16 with register operands holding random data and no memory traffic
    (vs_probe_mfma_rate): the power-limited ceiling of every 16-bit MFMA kernel on this device, measured, beside the 2.5 PFLOP/s headline."""
    dev = torch.device(device)
    src = (torch.rand(1 << 19, device=dev) * 4 - 2).half()
    scratch = torch.empty(512 * 256, dtype=torch.float32, device=dev)
    fl = ctypes.c_double(0.0)
    def run(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.device(dev):
            s.record()
            L.call("vs_probe_mfma_rate", dev, L.ptr(src), L.ptr(scratch), iters, ctypes.byref(fl))
            e.record()
        e.synchronize()
        return s.elapsed_time(e), fl.value
    ms, f = run(20000)                                   # warm-up and calibration (clocks settle within a few ms)
    iters = max(20000, int(20000 * ms_target / max(ms, 1e-3)))
    ms, f = run(iters)
    return f / (ms * 1e-3) / 1e12


def _ssim_args(x: torch.Tensor, y: torch.Tensor, taps):
    """(x, y, host taps) of the SSIM kernels: f32 NCHW contiguous device tensors of one shape, taps a ctypes float array."""
    if x.shape != y.shape or x.dim() != 4:
        raise ValueError(f"SSIM kernels take two [N, C, H, W] tensors of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    dev = L.require_device(x, y)
    taps = [float(t) for t in taps]
    return dev, x.contiguous().float(), y.contiguous().float(), (ctypes.c_float * len(taps))(*taps), len(taps)


def ssim_forward(x: torch.Tensor, y: torch.Tensor, taps, cov_norm: float, c1: float, c2: float, components: bool = False,
                 unit_window: bool = False):
    """Per-plane and per-image means of the SSIM map (and, with `components`, of the brightness, contrast and structure maps) of x against
    y on the valid window positions (vs_ssim_forward).  unit_window: the taps stand for a window of total weight exactly 1 (float64 taps
    rounded to float32); otherwise their own sum counts.  Returns (per_plane [nq, N, C], per_image [nq, N]), f32, nq = 4 if components else 1.
    Asynchronous on the current stream: no host synchronisation."""
    dev, x, y, tp, ws = _ssim_args(x, y, taps)
    N, C, H, W = x.shape
    flags = (L.VS_SSIM_COMPONENTS if components else 0) | (L.VS_SSIM_UNIT_WINDOW if unit_window else 0)
    nbytes = L.call("vs_ssim_workspace_bytes", dev, N, C, H, W, ws, flags)
    nq = 4 if components else 1
    work = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    per_plane = torch.empty((nq, N, C), dtype=torch.float32, device=dev)
    per_image = torch.empty((nq, N), dtype=torch.float32, device=dev)
    L.call("vs_ssim_forward", dev, L.ptr(x), L.ptr(y), N, C, H, W, tp, ws, cov_norm, c1, c2, flags, L.ptr(work), L.ptr(per_plane), L.ptr(per_image))
    return per_plane, per_image


def ssim_backward(x: torch.Tensor, y: torch.Tensor, taps, cov_norm: float, c1: float, c2: float, g_ssim: Optional[torch.Tensor],
                  g_structure: Optional[torch.Tensor], need_dx: bool = True, need_dy: bool = True, unit_window: bool = False):
    """(dx, dy) of sum g_ssim[n, c] * ssim[n, c] + g_structure[n, c] * structure[n, c], the per-plane means of ssim_forward
    (vs_ssim_backward).  g_*: [N, C] or None (zeros); an output not asked for is None."""
    dev, x, y, tp, ws = _ssim_args(x, y, taps)
    N, C, H, W = x.shape
    gs = None if g_ssim is None else g_ssim.detach().reshape(N * C).contiguous().float()
    gt = None if g_structure is None else g_structure.detach().reshape(N * C).contiguous().float()
    dx = torch.empty_like(x) if need_dx else None
    dy = torch.empty_like(y) if need_dy else None
    if dx is None and dy is None:
        return None, None
    L.call("vs_ssim_backward", dev, L.ptr(x), L.ptr(y), N, C, H, W, tp, ws, cov_norm, c1, c2, L.VS_SSIM_UNIT_WINDOW if unit_window else 0, L.ptr(gs),
           L.ptr(gt), L.ptr(dx), L.ptr(dy))
    return dx, dy


LPIPS_TAP_CHANNELS = (64, 128, 256, 512, 512)     # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3


def lpips_scale_log2(H: int, W: int) -> int:
    """The power of two the LPIPS backward runs its data gradients at (vs_lpips_head_backward / vs_lpips_prep_backward): 2^8 over the
    image's pixel count, which cancels the spatial mean of relu1_2 and keeps the split class's f16 (hi, lo) halves of the gradients normal."""
    return max(0, (H * W - 1).bit_length()) + 8


def _ptr_array(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def lpips_prep(img: torch.Tensor, normalize: bool) -> torch.Tensor:
    """[N, 3, H, W] image -> [N, H, W, 32] f32 NHWC: optional 2x - 1, the scaling layer, channels 3..31 zero (vs_lpips_prep)."""
    dev = L.require_device(img)
    img = img.contiguous().float()
    N, _, H, W = img.shape
    out = torch.empty((N, H, W, 32), dtype=torch.float32, device=dev)
    L.call("vs_lpips_prep", dev, L.ptr(img), N, H, W, int(normalize), L.ptr(out))
    return out


def lpips_prep_backward(g32: torch.Tensor, g: torch.Tensor, normalize: bool) -> torch.Tensor:
    """conv1_1's data gradient [N, H, W, 32] (at the scale of lpips_scale_log2) -> the image gradient [N, 3, H, W] (vs_lpips_prep_backward)."""
    dev = L.require_device(g32, g)
    N, H, W, _ = g32.shape
    g = g.detach().reshape(N).contiguous().float()
    out = torch.empty((N, 3, H, W), dtype=torch.float32, device=dev)
    L.call("vs_lpips_prep_backward", dev, L.ptr(g32), L.ptr(g), N, H, W, int(normalize), lpips_scale_log2(H, W), L.ptr(out))
    return out


def lpips_maxpool(x: torch.Tensor) -> torch.Tensor:
    """2 x 2 stride-2 max-pool of an NHWC f32 tensor (vs_lpips_maxpool)."""
    dev = L.require_device(x)
    N, H, W, C = x.shape
    y = torch.empty((N, H // 2, W // 2, C), dtype=torch.float32, device=dev)
    L.call("vs_lpips_maxpool", dev, L.ptr(x), N, H, W, C, L.ptr(y))
    return y


def lpips_maxpool_backward(dy: torch.Tensor, x: torch.Tensor, g_add: Optional[torch.Tensor]) -> torch.Tensor:
    """(x > 0) * (g_add + dy routed to the first maximum of each 2 x 2 window of x) (vs_lpips_maxpool_backward)."""
    dev = L.require_device(dy, x, g_add)
    N, H, W, C = x.shape
    dx = torch.empty_like(x)
    L.call("vs_lpips_maxpool_backward", dev, L.ptr(dy), L.ptr(x), L.ptr(g_add), N, H, W, C, L.ptr(dx))
    return dx


def lpips_head_forward(taps0, taps1, lins) -> torch.Tensor:
    """Per-image LPIPS distance [N] f32 from the five taps of both images (NHWC f32) and the five lin weights (vs_lpips_head_forward)."""
    dev = L.require_device(*taps0, *taps1, *lins)
    N, H, W, _ = taps0[0].shape
    nbytes = L.call("vs_lpips_workspace_bytes", dev, N, H, W)
    work = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    out = torch.empty(N, dtype=torch.float32, device=dev)
    L.call("vs_lpips_head_forward", dev, _ptr_array(taps0), _ptr_array(taps1), _ptr_array(lins), N, H, W, L.ptr(work), L.ptr(out))
    return out


def lpips_head_backward(taps0, taps1, lins, g: torch.Tensor, need0: bool, need1: bool):
    """dL/dtap (times the tap's ReLU mask, at the scale of lpips_scale_log2) for image 0 and / or image 1: two lists of five NHWC tensors
    (None for a side not asked for) (vs_lpips_head_backward)."""
    dev = L.require_device(*taps0, *taps1, *lins, g)
    N, H, W, _ = taps0[0].shape
    g = g.detach().reshape(N).contiguous().float()
    d0 = [torch.empty_like(t) for t in taps0] if need0 else None
    d1 = [torch.empty_like(t) for t in taps1] if need1 else None
    L.call("vs_lpips_head_backward", dev, _ptr_array(taps0), _ptr_array(taps1), _ptr_array(lins), L.ptr(g), N, H, W, lpips_scale_log2(H, W),
           None if d0 is None else _ptr_array(d0), None if d1 is None else _ptr_array(d1))
    return d0, d1


# ---------------------------------------------------------------------------------------------------------------------------
# distillation point loss (csrc/distill.hip, include/vicasplat_distill.h)
# ---------------------------------------------------------------------------------------------------------------------------
def _regr3d_args(gt1, gt2, pr1, pr2, cg1, cg2, pc1, pc2):
    if pc1 is None or pc2 is None:       # the reference adds the confidence term only when both are given
        pc1 = pc2 = None
    dev = L.require_device(gt1, gt2, pr1, pr2, cg1, cg2, pc1, pc2)
    if gt1.dim() != 4 or gt1.shape[-1] != 3 or gt1.numel() == 0:
        raise ValueError(f"Regr3D takes points [B, H, W, 3], got {tuple(gt1.shape)}")
    B, H, W, _ = gt1.shape
    for t, shape in ((gt2, (B, H, W, 3)), (pr1, (B, H, W, 3)), (pr2, (B, H, W, 3)), (cg1, (B, H, W)), (cg2, (B, H, W)), (pc1, (B, H, W)), (pc2, (B, H, W))):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"Regr3D: expected a tensor of shape {shape}, got {tuple(t.shape)}")
    ts = [None if t is None else t.detach().float().contiguous() for t in (gt1, gt2, pr1, pr2, cg1, cg2, pc1, pc2)]
    return dev, ts, (B, H, W)


def regr3d_forward(gt1, gt2, pr1, pr2, cg1, cg2, pc1=None, pc2=None, normalize_pts: bool = False):
    """(loss [] f32, workspace) of the distillation point loss (vsd_regr3d_forward); the workspace goes to regr3d_backward with the same
    inputs.  Waits for the stream once: a NaN among the pseudo-GT points raises RuntimeError."""
    dev, ts, (B, H, W) = _regr3d_args(gt1, gt2, pr1, pr2, cg1, cg2, pc1, pc2)
    nbytes = L.call("vsd_regr3d_workspace_bytes", dev, B, H, W)
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    L.call("vsd_regr3d_forward", dev, *[L.ptr(t) for t in ts], B, H, W, int(bool(normalize_pts)), L.ptr(work), nbytes, L.ptr(loss))
    return loss, work


def regr3d_backward(gt1, gt2, pr1, pr2, cg1, cg2, pc1, pc2, normalize_pts: bool, grad_loss: torch.Tensor, work: torch.Tensor):
    """(d_pr_pts1, d_pr_pts2, d_pr_conf1, d_pr_conf2) of grad_loss * loss (vsd_regr3d_backward); the last two are None without both pr_conf."""
    dev, ts, (B, H, W) = _regr3d_args(gt1, gt2, pr1, pr2, cg1, cg2, pc1, pc2)
    g = grad_loss.detach().reshape(1).float().contiguous()
    d1, d2 = torch.empty(B, H, W, 3, dtype=torch.float32, device=dev), torch.empty(B, H, W, 3, dtype=torch.float32, device=dev)
    has_conf = ts[6] is not None
    c1 = torch.empty(B, H, W, dtype=torch.float32, device=dev) if has_conf else None
    c2 = torch.empty(B, H, W, dtype=torch.float32, device=dev) if has_conf else None
    L.call("vsd_regr3d_backward", dev, *[L.ptr(t) for t in ts], B, H, W, int(bool(normalize_pts)), L.ptr(g), L.ptr(work), work.numel(),
           L.ptr(d1), L.ptr(d2), L.ptr(c1), L.ptr(c2))
    return d1, d2, c1, c2


def regr3d_workspace_view(work: torch.Tensor, B: int) -> dict:
    """What the forward left in its workspace, for tests and diagnostics: thresholds [2, B, 2] (view, element, (q01, q99)), the counts of
    valid pixels per view over the batch, the factors of prediction and pseudo-GT [B]."""
    w = work.view(torch.float32)
    return dict(thresholds=w[8:8 + 4 * B].view(2, B, 2), counts=w[1:3], factor_pr=w[8 + 4 * B:8 + 5 * B], factor_gt=w[8 + 5 * B:8 + 6 * B])


# ---------------------------------------------------------------------------------------------------------------------------
# depth-smoothness loss (csrc/depth_loss.hip, include/vicasplat_loss.h)
# ---------------------------------------------------------------------------------------------------------------------------
# One workgroup of the tile kernel covers a band of rows times a chunk of columns of one view.  Twins of kBandRows / kChunkCols in
# csrc/depth_loss.hip: change them together (tests/test_depth_loss_gpu.py takes its tile-edge shapes from here).
DEPTH_SMOOTH_BAND_ROWS = 16
DEPTH_SMOOTH_CHUNK_COLS = 64


def _depth_smooth_args(depth, near, far, image, sigma_image, use_second_derivative):
    if sigma_image is None:
        image = None           # the reference reads the colours only for the bilateral weights
    elif image is None:
        raise ValueError("depth smoothness: sigma_image is given, so the target image [N, 3, H, W] is needed")
    dev = L.require_device(depth, near, far, image)
    if depth.dim() != 3 or depth.numel() == 0:
        raise ValueError(f"depth smoothness takes depth [N, H, W], got {tuple(depth.shape)}")
    N, H, W = depth.shape
    for name, t, shape in (("near", near, (N,)), ("far", far, (N,)), ("image", image, (N, 3, H, W))):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"depth smoothness: expected {name} of shape {shape}, got {tuple(t.shape)}")
    for name, t in (("depth", depth), ("near", near), ("far", far), ("image", image)):
        if t is not None and not t.is_floating_point():
            raise ValueError(f"depth smoothness: {name} must be a floating-point tensor, got {t.dtype}")
    need = 3 if use_second_derivative else 2
    if H < need or W < need:
        raise ValueError(f"depth smoothness: {H} x {W} is too small, a {'second' if use_second_derivative else 'first'} difference needs at "
                         f"least {need} rows and columns (torch returns NaN from the empty mean)")
    ts = [None if t is None else t.detach().float().contiguous() for t in (depth, near, far, image)]
    return dev, ts, (N, H, W)


def depth_smooth_forward(depth, near, far, image=None, sigma_image=None, use_second_derivative: bool = False, weight: float = 1.0,
                         need_grad: bool = True):
    """(loss [] f32, d_depth_unit [N, H, W] f32 or None) of the depth-smoothness loss (vsl_depth_smooth_forward): depth [N, H, W], near and
    far [N], image [N, 3, H, W] (read only when sigma_image is not None).  d_depth_unit is d loss / d depth for an upstream gradient of 1,
    written by the same pass (need_grad); depth_smooth_backward scales it.  No host synchronisation."""
    dev, ts, (N, H, W) = _depth_smooth_args(depth, near, far, image, sigma_image, use_second_derivative)
    nbytes = L.call("vsl_depth_smooth_workspace_bytes", dev, N, H, W)
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    unit = torch.empty((N, H, W), dtype=torch.float32, device=dev) if need_grad else None
    L.call("vsl_depth_smooth_forward", dev, *[L.ptr(t) for t in ts], N, H, W, 0.0 if sigma_image is None else float(sigma_image),
           int(bool(use_second_derivative)), float(weight), L.ptr(work), nbytes, L.ptr(loss), L.ptr(unit))
    return loss, unit


def depth_smooth_backward(d_depth_unit: torch.Tensor, grad_loss: torch.Tensor) -> torch.Tensor:
    """grad_loss * d_depth_unit (vsl_depth_smooth_backward): the gradient of the depth-smoothness loss with respect to depth [N, H, W]."""
    dev = L.require_device(d_depth_unit, grad_loss)
    if d_depth_unit.dim() != 3 or d_depth_unit.dtype != torch.float32 or not d_depth_unit.is_contiguous() or d_depth_unit.numel() == 0:
        raise ValueError(f"depth smoothness backward takes the contiguous f32 [N, H, W] image of the forward, got {tuple(d_depth_unit.shape)} "
                         f"{d_depth_unit.dtype}")
    if grad_loss.numel() != 1:
        raise ValueError(f"depth smoothness backward: the loss is a scalar, got an upstream gradient of shape {tuple(grad_loss.shape)}")
    N, H, W = d_depth_unit.shape
    g = grad_loss.detach().reshape(1).float().contiguous()
    out = torch.empty_like(d_depth_unit)
    L.call("vsl_depth_smooth_backward", dev, L.ptr(d_depth_unit), L.ptr(g), N, H, W, L.ptr(out))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the distillation teacher's tail (csrc/teacher.hip, include/vicasplat_teacher.h)
# ---------------------------------------------------------------------------------------------------------------------------
def points_conf(raw: torch.Tensor, transform: Optional[torch.Tensor] = None, *, out_pts: Optional[torch.Tensor] = None,
                out_conf: Optional[torch.Tensor] = None):
    """(pts [n, H, W, 3] f32, conf [n, H, W] f32) of the raw four-channel pts3d head output raw [n, H, W, 4] (f32 or f16, contiguous: what
    forward_pts3d_raw returns before its permute): p = xyz / max(|xyz|, 1e-8) * expm1(|xyz|), conf = 1 + exp(c), and with transform
    [n, 3, 4] (rows of (R | t), f32) pts = R p + t (vst_points_conf).  out_pts / out_conf: contiguous f32 tensors to write into.  No host
    synchronisation."""
    dev = L.require_device(raw, transform, out_pts, out_conf)
    if raw.dim() != 4 or raw.shape[-1] != 4 or raw.numel() == 0 or raw.dtype not in (torch.float32, torch.float16) or not raw.is_contiguous():
        raise ValueError(f"points_conf takes the contiguous f32 or f16 head output [n, H, W, 4], got {tuple(raw.shape)} {raw.dtype} "
                         f"(strides {raw.stride()})")
    n, H, W, _ = raw.shape
    if transform is not None:
        if tuple(transform.shape) != (n, 3, 4):
            raise ValueError(f"points_conf: expected a transform of shape {(n, 3, 4)}, got {tuple(transform.shape)}")
        transform = transform.detach().float().contiguous()
    pts = torch.empty(n, H, W, 3, dtype=torch.float32, device=dev) if out_pts is None else out_pts
    conf = torch.empty(n, H, W, dtype=torch.float32, device=dev) if out_conf is None else out_conf
    for name, t, shape in (("out_pts", pts, (n, H, W, 3)), ("out_conf", conf, (n, H, W))):
        if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"points_conf: {name} must be a contiguous f32 tensor of shape {shape}, got {tuple(t.shape)} {t.dtype}")
    L.call("vst_points_conf", dev, L.ptr(raw), int(raw.dtype == torch.float16), L.ptr(transform), n, H, W, L.ptr(pts), L.ptr(conf))
    return pts, conf


# ---------------------------------------------------------------------------------------------------------------------------
# trajectory metrics (csrc/trajectory.hip, include/vicasplat_metrics.h)
# ---------------------------------------------------------------------------------------------------------------------------
_TRAJ_DTYPES = {torch.float32: 0, torch.float64: 5}      # the dtype codes of vsm_trajectory_metrics


def trajectory_metrics(pred: torch.Tensor, gt: torch.Tensor, delta: int = 1, return_alignment: bool = False):
    """(metrics [B, 3] f64 = ate, rpe_trans, rpe_rot (degrees); valid [B] int32) of estimated against true camera-to-world poses, both
    [B, V, 4, 4], contiguous, f32 or f64 (one dtype for both), on a HIP device: Umeyama alignment with scale, then ATE and the relative pose
    errors over the pairs (i, i + delta) (vsm_trajectory_metrics; the algorithm is written out in include/vicasplat_metrics.h).  A degenerate
    scene -- fewer than two singular values above 2^-52, V < 3, delta >= V, a non-finite element -- has valid 0, metrics 0 and the identity as
    its alignment.  return_alignment: also align [B, 13] f64 = R row-major, t, c.  One launch on the current stream, no host synchronisation."""
    dev = L.require_device(pred, gt)
    if pred.dim() != 4 or tuple(pred.shape[-2:]) != (4, 4) or pred.shape[1] < 1:
        raise ValueError(f"trajectory_metrics takes poses [B, V, 4, 4] with V >= 1, got {tuple(pred.shape)}")
    if gt.shape != pred.shape:
        raise ValueError(f"trajectory_metrics: expected ground truth of shape {tuple(pred.shape)}, got {tuple(gt.shape)}")
    if pred.dtype not in _TRAJ_DTYPES or gt.dtype != pred.dtype:
        raise ValueError(f"trajectory_metrics takes f32 or f64 poses of one dtype, got {pred.dtype} and {gt.dtype}")
    if not (pred.is_contiguous() and gt.is_contiguous()):
        raise ValueError(f"trajectory_metrics takes contiguous poses, got strides {pred.stride()} and {gt.stride()}")
    if int(delta) != delta or delta < 1:
        raise ValueError(f"trajectory_metrics: delta must be a positive number of frames, got {delta!r}")
    B, V = pred.shape[:2]
    metrics = torch.empty(B, 3, dtype=torch.float64, device=dev)
    valid = torch.empty(B, dtype=torch.int32, device=dev)
    align = torch.empty(B, 13, dtype=torch.float64, device=dev) if return_alignment else None
    if B > 0:       # (an empty tensor has no address to hand over)
        L.call("vsm_trajectory_metrics", dev, L.ptr(pred.detach()), L.ptr(gt.detach()), _TRAJ_DTYPES[pred.dtype], B, V,
               min(int(delta), 2 ** 31 - 1), L.ptr(metrics), L.ptr(valid), L.ptr(align))
    return (metrics, valid, align) if return_alignment else (metrics, valid)


# ---- visualisation (include/vicasplat_viz.h, csrc/viz.hip) ---------------------------------------------------------------------------
def _viz_f32(name: str, t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{name} takes a contiguous f32 {what}, got {t.dtype} with strides {t.stride()}")
    return t.detach()


def depth_range(values: torch.Tensor, return_order_stats: bool = False):
    """range [2] f32 = (near, far) of vis_depth_map (src/misc/utils.py:13-22) for a contiguous f32 tensor of at most L.VSV_MAX_RANGE_N
    values on a HIP device: far = log(Q_0.99(all values)), near = log(Q_0.01(the values > 0)) or 0 when none is, Q = torch.quantile
    (vsv_depth_range; include/vicasplat_viz.h states the arithmetic).  return_order_stats: also [4] f32, the two order statistics of
    near, then of far.  On the current stream, no host copy, no synchronisation."""
    dev = L.require_device(values)
    v = _viz_f32("depth_range", values, "tensor")
    n = v.numel()
    if n < 1:
        raise ValueError("depth_range of an empty tensor (torch.quantile raises on one too)")
    ws = torch.empty(int(L.call("vsv_depth_range_workspace_bytes", dev, n)), dtype=torch.uint8, device=dev)
    out = torch.empty(2, dtype=torch.float32, device=dev)
    stats = torch.empty(4, dtype=torch.float32, device=dev) if return_order_stats else None
    L.call("vsv_depth_range", dev, L.ptr(v), n, L.ptr(out), L.ptr(stats), L.ptr(ws), ws.numel())
    return (out, stats) if return_order_stats else out


def color_map(value: torch.Tensor, lut: torch.Tensor, mode: int, value_range: Optional[torch.Tensor] = None,
              out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """value [..., H, W] f32 -> [..., 3, H, W] f32 or uint8 colours through lut [256, 3] f32 (vsv_color_map).  mode L.VSV_MODE_DEPTH:
    x = 1 - (log v - near) / (far - near) with value_range = (near, far) on the device; L.VSV_MODE_MAX: x = v / max(v).  The index is
    min(trunc(clip(x, 0, 1) * 256), 255); a NaN x gives 0.  On the current stream, no host copy, no synchronisation."""
    dev = L.require_device(value, lut, value_range)
    v = _viz_f32("color_map", value, "value")
    if v.dim() < 2:
        raise ValueError(f"color_map takes [..., H, W], got {tuple(v.shape)}")
    if tuple(lut.shape) != (256, 3):
        raise ValueError(f"color_map takes a table [256, 3], got {tuple(lut.shape)}")
    lut = _viz_f32("color_map", lut, "table")
    if out_dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"color_map writes f32 or uint8, got {out_dtype}")
    if mode == L.VSV_MODE_DEPTH:
        if value_range is None or value_range.numel() != 2:
            raise ValueError("color_map in the depth mode takes value_range = (near, far) on the device")
        value_range = _viz_f32("color_map", value_range, "value_range")
    H, W = v.shape[-2:]
    M = v.numel() // max(H * W, 1)
    out = torch.empty(*v.shape[:-2], 3, H, W, dtype=out_dtype, device=dev)
    nws = int(L.call("vsv_color_map_workspace_bytes", dev, mode))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev) if nws else None
    if v.numel():
        L.call("vsv_color_map", dev, L.ptr(v), M, H, W, mode, L.ptr(value_range), L.ptr(lut), L.ptr(out),
               L.VSV_OUT_U8 if out_dtype == torch.uint8 else L.VSV_OUT_F32, L.ptr(ws), nws)
    return out


def video_frames(rgb: torch.Tensor, depth: torch.Tensor, value_range: torch.Tensor, lut: torch.Tensor, gap: int = 8) -> torch.Tensor:
    """frames [M, 3, 2 H + gap, W] uint8 of render_video_generic (src/model/model_wrapper.py:805-813) in one launch: rgb [M, 3, H, W] f32
    clipped and truncated to bytes, `gap` white rows, and depth [M, H, W] f32 through the depth colour map with value_range = (near, far)
    and lut [256, 3] (vsv_video_frames).  A NaN gives 0.  On the current stream, no host copy, no synchronisation."""
    dev = L.require_device(rgb, depth, value_range, lut)
    rgb, depth = _viz_f32("video_frames", rgb, "rgb"), _viz_f32("video_frames", depth, "depth")
    value_range, lut = _viz_f32("video_frames", value_range, "value_range"), _viz_f32("video_frames", lut, "table")
    if rgb.dim() != 4 or rgb.shape[1] != 3 or depth.dim() != 3 or tuple(depth.shape) != (rgb.shape[0], rgb.shape[2], rgb.shape[3]):
        raise ValueError(f"video_frames takes rgb [M, 3, H, W] and depth [M, H, W], got {tuple(rgb.shape)} and {tuple(depth.shape)}")
    if tuple(lut.shape) != (256, 3) or value_range.numel() != 2 or int(gap) != gap or gap < 0:
        raise ValueError("video_frames takes a table [256, 3], value_range = (near, far) and a gap >= 0")
    M, _, H, W = rgb.shape
    frames = torch.empty(M, 3, 2 * H + int(gap), W, dtype=torch.uint8, device=dev)
    if frames.numel():
        L.call("vsv_video_frames", dev, L.ptr(rgb), L.ptr(depth), M, H, W, int(gap), L.ptr(value_range), L.ptr(lut), L.ptr(frames))
    return frames


# ---- vector drawing (include/vicasplat_draw.h, csrc/draw.hip) --------------------------------------------------------------------------
_DRAW_CAPS = {"butt": L.VSG_CAP_BUTT, "round": L.VSG_CAP_ROUND, "square": L.VSG_CAP_SQUARE}


def _draw(entry: str, what: str, floats: int, image: torch.Tensor, prims: torch.Tensor, prim_offsets: torch.Tensor, num_passes: int,
          out: Optional[torch.Tensor], extra: tuple) -> torch.Tensor:
    dev = L.require_device(image, prims, prim_offsets, out)
    image = _viz_f32(what, image, "image")
    prims = _viz_f32(what, prims, "record array")
    if image.dim() != 4 or image.shape[1] != 3:
        raise ValueError(f"{what} takes images [B, 3, H, W], got {tuple(image.shape)}")
    B, _, H, W = image.shape
    if prims.dim() != 2 or prims.shape[1] != floats:
        raise ValueError(f"{what} takes records [n, {floats}], got {tuple(prims.shape)}")
    if prim_offsets.dtype != torch.int32 or tuple(prim_offsets.shape) != (B + 1,) or not prim_offsets.is_contiguous():
        raise ValueError(f"{what} takes prim_offsets [B + 1 = {B + 1}] int32, got {tuple(prim_offsets.shape)} {prim_offsets.dtype}")
    if H > L.VSG_MAX_SIDE or W > L.VSG_MAX_SIDE or B > L.VSG_MAX_BATCH:
        raise ValueError(f"{what}: images of {H} x {W} in a batch of {B} exceed {L.VSG_MAX_SIDE} a side or {L.VSG_MAX_BATCH} images")
    if num_passes not in (0, 1):
        raise NotImplementedError(f"{what}: num_passes = {num_passes!r}: the HIP kernel refines once at the most (0 or 1)")
    if out is None:
        out = torch.empty_like(image)
    elif out.shape != image.shape or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"{what}: out must be a contiguous f32 tensor of shape {tuple(image.shape)}, got {tuple(out.shape)} {out.dtype}")
    if image.numel():
        L.call(entry, dev, L.ptr(image), L.ptr(out), B, H, W, L.ptr(prims) if prims.numel() else None, prims.shape[0], L.ptr(prim_offsets),
               *extra, int(num_passes))
    return out


def draw_lines(image: torch.Tensor, lines: torch.Tensor, prim_offsets: torch.Tensor, cap: str = "round", num_passes: int = 1,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One layer of antialiased lines over image [B, 3, H, W] f32 -> out of the same shape (vsg_draw_lines).  lines [n, L.VSG_LINE_FLOATS]
    f32 IN PIXEL SPACE: start x, y, end x, y, width, r, g, b; prim_offsets [B + 1] int32 on the device gives image b the records
    [off[b], off[b + 1]).  The topmost record is the highest-indexed one; cap is "butt", "round" or "square"; num_passes 0 samples the pixel
    centres, 1 also refines every pixel that differs from a neighbour on an 8 x 8 grid.  An image without records is copied.  out may be
    `image` itself.  include/vicasplat_draw.h states the arithmetic.  One launch on the current stream, no workspace, no synchronisation."""
    if cap not in _DRAW_CAPS:
        raise ValueError(f"draw_lines: cap {cap!r} is none of {sorted(_DRAW_CAPS)}")
    return _draw("vsg_draw_lines", "draw_lines", L.VSG_LINE_FLOATS, image, lines, prim_offsets, num_passes, out, (_DRAW_CAPS[cap],))


def draw_points(image: torch.Tensor, points: torch.Tensor, prim_offsets: torch.Tensor, num_passes: int = 1,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One layer of points (rings) over image [B, 3, H, W] f32 (vsg_draw_points): points [n, L.VSG_POINT_FLOATS] f32 in pixel space:
    x, y, radius, inner radius, r, g, b; a sample is covered when inner <= |p - c| <= radius.  Everything else as draw_lines."""
    return _draw("vsg_draw_points", "draw_points", L.VSG_POINT_FLOATS, image, points, prim_offsets, num_passes, out, ())
