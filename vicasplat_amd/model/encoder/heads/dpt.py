"""DPT output heads of VicaSplat: `pts3d` regression head (downstream_head1) and Gaussian-parameter head
(gaussian_param_head).  Reference: heads/dpt_block.py:79-218,264-419, heads/dpt_head.py:21-119,
heads/dpt_gs_head.py:98-206, heads/postprocess.py:10-63.  Parameter names == the reference's state_dict keys.

SURVEY.md 8(f)-1: the heads are 42 % of the forward FLOPs.  Every convolution, GEMM and bilinear x2 runs on the hand-written HIP kernels on
NHWC activations (16-bit, or f32 in the f32 / split classes).  HIP device tensors only.  The trunk is one sequence for every operand class;
the tail is a ROUTE that `pts3d_route` / `gs_route` name from Python values alone (no GPU, no library) and the forwards dispatch once:
  pts3d  split_packed_dot   upsample2x(packed) -> [conv3x3 + ReLU + 1x1 as f32 dot products] in one kernel (split class)
         fused16            upsample2x -> [conv3x3 + ReLU + 1x1] in one kernel (f16 / bf16)
         unfused            upsample2x -> conv3x3 + ReLU -> GEMM
  gs     split_stream_stem  streaming 7x7 stem that writes up2(trunk) + relu(stem) packed -> [conv3x3 + ReLU + 1x1] (split class)
         split_stem_up      the same sum from the window-GEMM stem's epilogue -> the same head kernel
         split_up_packed    stem map -> upsample2x(+ relu(stem), packed) -> the same head kernel
         fused16 / unfused  stem map -> upsample2x(+ relu(stem)) -> [conv3x3 + ReLU + 1x1] (f16 / bf16) / conv3x3 + ReLU -> GEMM
  stem map: "split7" (split-class window GEMM), "im2col_f32" (im2col + GEMM of the f32 class) or "window16" (16-bit window GEMM).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F      # F.pad / F.unfold of weight packing and the im2col stem only -- no torch convolution / interpolation anywhere
from torch import nn

from .... import ops

# Twin of `big >= 224` in conv3x3_route (csrc/routes.h): in the split class a convolution with Cout % 128 == 0 && Cout % 256 != 0 (the pts3d
# head's 256 -> 128) runs on a 256-pixel tile kernel, the only kind that reads a packed (hi, lo) input, from 224 tiles on -- so from this many
# pixels on (in whole tiles) the trunk writes its last map packed.  tests/test_routes_cpu.py holds the two together over every batch and grid.
PACKED_CONV_MIN_PIXELS = 224 * 256
# K per tap of the fused conv3x3 -> 1x1 kernels in 2-byte units: `Cin == 64 << s` in vs_conv3x3_head1x1_nhwc (16-bit channels), `2 * Cin ==
# 64 << s` in vs_conv3x3_head1x1_split_nhwc (f32 channels, two units each) -- ONE constraint: 64..512 16-bit or 32..256 f32 channels.
_FUSED_HEAD_K_UNITS = (64, 128, 256, 512)
_CLASS_OF = {torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: "f32"}


def pts3d_route(cls: str, BT: int, gh: int, gw: int, c_trunk: int, c_h0: int, c_h2: int):
    """-> (route, trunk_packed: the trunk's last bilinear pass writes the packed (hi, lo) form) for operand class "f16" / "bf16" / "f32" / "split", BT
    frames of gh x gw tokens, the channels of the trunk, head[0] and head[2].  The head's 256 * BT * gh * gw pixels always fill 256-pixel tiles."""
    # head[0] then runs on the 256 x 128 tile kernel (conv3x3_entry: a whole, even number of K tiles); otherwise the trunk writes plain f32
    trunk_packed = cls == "split" and c_h0 == 128 and c_trunk in (64, 128, 256) and -(-BT * 64 * gh * gw // 256) * 256 >= PACKED_CONV_MIN_PIXELS
    if c_h0 == 128 and cls == "split" and c_h2 == 128:
        return "split_packed_dot", trunk_packed
    return ("fused16" if c_h0 == 128 and cls in ("f16", "bf16") else "unfused"), trunk_packed     # (no other one-kernel form: conv3x3, then a GEMM)


def gs_route(cls: str, gh: int, gw: int, H: int, W: int, num_channels: int, c_trunk: int, c_stem: int, c_h0: int):
    """-> (route, stem) for H x W frames and the channels of the trunk, the 7x7 stem and head[0]; stem names the stem's kernel ("stream":
    inside `split_stream_stem`).  BT * 16gh * 16gw pixels are a multiple of 256 for every batch and grid, so BT selects nothing."""
    # the split window GEMM tiles Cout by 256: otherwise the split class takes the f32 class's im2col + GEMM, on split operands
    stem = {"split": "split7" if c_stem % 256 == 0 else "im2col_f32", "f32": "im2col_f32"}.get(cls, "window16")
    # otherwise two kernels: the fused 1x1 holds <= 96 output rows of a 256-wide 3x3, on a K it can tile; the f32 class has no such kernel
    if cls == "f32" or num_channels > 96 or c_h0 != 256 or c_trunk * (2 if cls == "split" else 1) not in _FUSED_HEAD_K_UNITS:
        return "unfused", stem
    if cls != "split":
        return "fused16", stem
    # the stem's epilogue adds the trunk pixel for pixel; otherwise the stem is a map of its own (and upsample2x_nhwc refuses a mismatched one)
    if stem != "split7" or c_trunk != c_stem or (16 * gh, 16 * gw) != (H, W):
        return "split_up_packed", stem
    # the streaming kernel walks 32-pixel column strips of a 256-channel stem; otherwise the window GEMM's epilogue forms the same sum
    return ("split_stream_stem", "stream") if W % 32 == 0 and c_stem == 256 else ("split_stem_up", stem)


def _no_torch_forward(self, *a, **k):
    raise RuntimeError(f"{type(self).__name__} is a PARAMETER CONTAINER (the reference's state_dict names): the computation runs on the HIP "
                       "kernels driven by PixelwiseTaskWithDPT -- there is no PyTorch / MIOpen forward in vicasplat_amd")


class _RCU(nn.Module):      # ResidualConvUnit_custom (dpt_block.py:79-150): parameters only
    forward = _no_torch_forward

    def __init__(self, c: int):
        super().__init__()
        self.conv1 = nn.Conv2d(c, c, 3, 1, 1, bias=True)
        self.conv2 = nn.Conv2d(c, c, 3, 1, 1, bias=True)


class _Fusion(nn.Module):   # FeatureFusionBlock_custom (dpt_block.py:153-218): parameters only
    forward = _no_torch_forward

    def __init__(self, c: int):
        super().__init__()
        self.out_conv = nn.Conv2d(c, c, 1, bias=True)
        self.resConfUnit1 = _RCU(c)
        self.resConfUnit2 = _RCU(c)


class _Scratch(nn.Module):
    def __init__(self, layer_dims, feat):
        super().__init__()
        self.layer1_rn = nn.Conv2d(layer_dims[0], feat, 3, 1, 1, bias=False)
        self.layer2_rn = nn.Conv2d(layer_dims[1], feat, 3, 1, 1, bias=False)
        self.layer3_rn = nn.Conv2d(layer_dims[2], feat, 3, 1, 1, bias=False)
        self.layer4_rn = nn.Conv2d(layer_dims[3], feat, 3, 1, 1, bias=False)
        # same tensors under a second name, as in the reference (dpt_block.py:70-75)
        self.layer_rn = nn.ModuleList([self.layer1_rn, self.layer2_rn, self.layer3_rn, self.layer4_rn])
        self.refinenet1 = _Fusion(feat)
        self.refinenet2 = _Fusion(feat)
        self.refinenet3 = _Fusion(feat)
        self.refinenet4 = _Fusion(feat)


class _DPT(nn.Module):      # DPTOutputAdapter / its GS variant (dpt_block.py:264-419, dpt_gs_head.py:98-157): parameters only
    forward = _no_torch_forward

    def __init__(self, dim_tokens, hooks, num_channels: int, head_type: str, feat: int = 256, layer_dims=(96, 192, 384, 768)):
        super().__init__()
        self.hooks, self.head_type = list(hooks), head_type
        ld = list(layer_dims)
        self.scratch = _Scratch(ld, feat)
        self.act_postprocess = nn.ModuleList([
            nn.Sequential(nn.Conv2d(dim_tokens[0], ld[0], 1), nn.ConvTranspose2d(ld[0], ld[0], 4, 4)),
            nn.Sequential(nn.Conv2d(dim_tokens[1], ld[1], 1), nn.ConvTranspose2d(ld[1], ld[1], 2, 2)),
            nn.Sequential(nn.Conv2d(dim_tokens[2], ld[2], 1)),
            nn.Sequential(nn.Conv2d(dim_tokens[3], ld[3], 1), nn.Conv2d(ld[3], ld[3], 3, 2, 1)),
        ])
        if head_type == "regression":
            self.head = nn.Sequential(nn.Conv2d(feat, feat // 2, 3, 1, 1), nn.Identity(), nn.Conv2d(feat // 2, feat // 2, 3, 1, 1),
                                      nn.ReLU(True), nn.Conv2d(feat // 2, num_channels, 1))
        else:  # gs_params
            self.head = nn.Sequential(nn.Conv2d(feat, feat, 3, padding=1, bias=False), nn.Identity(), nn.ReLU(True),
                                      nn.Dropout(0.1, False), nn.Conv2d(feat, num_channels, 1))
            self.input_merger = nn.Sequential(nn.Conv2d(3, feat, 7, 1, 3), nn.ReLU())


def _pad_to(n: int, m: int = 64) -> int:
    return (n + m - 1) // m * m


class PixelwiseTaskWithDPT(nn.Module):
    """`.dpt` holds the parameters (reference naming: <head>.dpt.<...>); the forward drives the hand-written HIP kernels.  `_trunk`, the same
    for both heads: every 3x3 convolution is the implicit-GEMM MFMA kernel behind `ops.conv3x3_nhwc`, its ReLUs / bias / residuals fused; every
    1x1 convolution and both ConvTranspose2d(k == stride) are plain GEMMs -- tokens [BT, gh*gw, C] ARE an NHWC gh x gw map; bilinear x2 is
    `ops.upsample2x_nhwc`; channel counts that are no multiple of 64 (96) are zero-padded in the packed weights.  The tail is a route of the module
    docstring: pts3d split_packed_dot / fused16 / unfused; gs split_stream_stem / split_stem_up / split_up_packed / fused16 / unfused."""

    def __init__(self, net, num_channels: int, head_type: str):
        super().__init__()
        L = net.dec_depth
        assert L > 9
        self.dpt = _DPT([net.enc_embed_dim] + [net.dec_embed_dim] * 3, [0, L * 2 // 4, L * 3 // 4, L], num_channels, head_type)
        self.head_type = head_type
        self.num_channels = num_channels
        self.compute_dtype = torch.float16
        self.split = False    # split operand class: f32 activations + ops.SplitWeight weights (VicaSplat.set_compute_dtype("split"))
        self._pk: dict = {}
        self._pk_key = None

    # ---- packed 16-bit weights (re-made when a parameter changes / moves / the compute dtype changes) ----
    def _packed(self):
        d = self.dpt
        w0 = d.scratch.layer1_rn.weight
        key = (self.compute_dtype, self.split, w0.device, sum(p._version for p in self.parameters()), id(w0))
        if key == self._pk_key:
            return self._pk
        dt = self.compute_dtype
        fin = (lambda t: ops.split_pack_weight(t)) if self.split else (lambda t: t)   # (split: pack the padded f32 GEMM weight)
        P = {}

        def lin(name, conv, n_pad=0, k_pad=0):  # 1x1 conv -> GEMM weight [N(+pad), K(+pad)], f32 bias [N(+pad)]
            w = conv.weight.detach().flatten(1)
            N, K = w.shape
            Np, Kp = max(n_pad, N), max(k_pad, K)
            wp = torch.zeros(Np, Kp, dtype=dt, device=w.device)
            wp[:N, :K] = w.to(dt)
            b = torch.zeros(Np, dtype=torch.float32, device=w.device)
            if conv.bias is not None:
                b[:N] = conv.bias.detach().float()
            P[name + ".w"], P[name + ".b"] = fin(wp), b

        def convT(name, ct, k_pad, co_pad):  # ConvTranspose2d(k == stride) -> GEMM weight [(i, j, co_pad), ci_pad]
            w = ct.weight.detach()  # [Cin, Cout, k, k]
            Cin, Cout, k, _ = w.shape
            wp = torch.zeros(k, k, co_pad, k_pad, dtype=dt, device=w.device)
            wp[:, :, :Cout, :Cin] = w.permute(2, 3, 1, 0).to(dt)
            b = torch.zeros(k, k, co_pad, dtype=torch.float32, device=w.device)
            b[:, :, :Cout] = ct.bias.detach().float()
            P[name + ".w"], P[name + ".b"] = fin(wp.reshape(k * k * co_pad, k_pad).contiguous()), b.reshape(-1).contiguous()

        def c3(name, conv, cin_pad=0):
            P[name + ".w"] = ops.pack_conv3x3_weight(conv.weight, "split" if self.split else dt, cin_pad)
            P[name + ".b"] = None if conv.bias is None else conv.bias.detach().float().contiguous()

        ap = d.act_postprocess
        c0, c1 = _pad_to(ap[0][0].out_channels), _pad_to(ap[1][0].out_channels)   # 96 -> 128; 192 stays (a multiple of 64 already)
        lin("ap0.0", ap[0][0], n_pad=c0); convT("ap0.1", ap[0][1], k_pad=c0, co_pad=c0)
        lin("ap1.0", ap[1][0], n_pad=c1); convT("ap1.1", ap[1][1], k_pad=c1, co_pad=c1)
        lin("ap2.0", ap[2][0])
        lin("ap3.0", ap[3][0]); c3("ap3.1", ap[3][1])
        for i, cp in enumerate((c0, c1, 0, 0)):
            c3(f"rn{i}", d.scratch.layer_rn[i], cp)
        for r in (1, 2, 3, 4):
            f = getattr(d.scratch, f"refinenet{r}")
            for u in ("resConfUnit1", "resConfUnit2"):
                c3(f"rf{r}.{u}.c1", getattr(f, u).conv1); c3(f"rf{r}.{u}.c2", getattr(f, u).conv2)
            lin(f"rf{r}.out", f.out_conv)
        c3("h0", d.head[0]); lin("h4", d.head[4])
        if self.head_type == "regression":
            c3("h2", d.head[2]); lin("h4f", d.head[4], n_pad=4)   # fused form: [4, 128] rows (row 3 zero), bias [4]
        else:
            lin("h4f", d.head[4], n_pad=_pad_to(self.num_channels, 16))   # fused form: channels padded to a multiple of 16
        self._pk, self._pk_key = P, key
        return P

    # Weights that one route alone reads, made on first use per weight version (`_lazy`).  Made in _packed, "stem.e" would cost every head of
    # every class a host synchronisation, and each class would pack what it never reads.
    _LAZY = {
        "h4f32.w": lambda s, P: F.pad(s.dpt.head[4].weight.detach().float().flatten(1), (0, 0, 0, 4 - s.dpt.head[4].out_channels)).contiguous(),
        "h4f32.b": lambda s, P: F.pad(s.dpt.head[4].bias.detach().float(), (0, 4 - s.dpt.head[4].out_channels)).contiguous(),   # split dot head: f32 [4, 128], [4]
        "stem.b": lambda s, P: s.dpt.input_merger[0].bias.detach().float().contiguous(),
        "stem.w": lambda s, P: ops.pack_conv7x7_rgb_weight(s.dpt.input_merger[0].weight, s.compute_dtype),     # 16-bit window GEMM
        "stem.ws7": lambda s, P: ops.pack_conv7x7_rgb_weight(s.dpt.input_merger[0].weight, "split"),            # split window GEMM
        "stem.w32": lambda s, P: s.dpt.input_merger[0].weight.detach().float().contiguous(),                     # streaming stem: packs in the kernel ...
        "stem.e": lambda s, P: ops.split_scale_exp(s._lazy(P, "stem.w32")),                                      # ... with this exponent (one host read)
        "stem.wk": lambda s, P: F.pad(s.dpt.input_merger[0].weight.detach().float().flatten(1), (0, 160 - 147)).contiguous(),   # im2col stem: (c, ky, kx) rows, K 147 -> 160
        "stem.ws": lambda s, P: ops.split_pack_weight(s._lazy(P, "stem.wk")),                                    # ... and its split-class packing
    }

    def _lazy(self, P, key):
        if key not in P:
            P[key] = self._LAZY[key](self, P)
        return P[key]

    def _stem(self, stem: str, frames: torch.Tensor, P) -> torch.Tensor:
        """The 7x7 stem (dpt_gs_head.py:112-118) as a map of its own [N,H,W,Cout], bias fused; its ReLU rides on the upsample-add that reads it."""
        N, _, H, W = frames.shape
        bias = self._lazy(P, "stem.b")
        if stem == "split7":
            return ops.conv7x7_rgb_nhwc(ops.pad_rgb_nhwc(frames, torch.float32), self._lazy(P, "stem.ws7"), bias, H, W)
        if stem == "window16":
            return ops.conv7x7_rgb_nhwc(ops.pad_rgb_nhwc(frames, self.compute_dtype), self._lazy(P, "stem.w"), bias, H, W)
        assert stem == "im2col_f32", stem
        # reference precision: im2col rows through the f32 (or split) MFMA GEMM, 8 frames at a time (65 536 x 160 floats per frame)
        wk = self._lazy(P, "stem.ws" if self.split else "stem.wk")
        out = torch.empty(N, H, W, wk.shape[0], dtype=torch.float32, device=frames.device)
        for i in range(0, N, 8):
            cols = F.pad(F.unfold(frames[i:i + 8].float(), 7, padding=3).transpose(1, 2), (0, 160 - 147)).reshape(-1, 160).contiguous()
            ops.gemm(cols, wk, bias, out[i:i + 8].view(-1, wk.shape[0]), ops.EPI_STORE16)
        return out

    @staticmethod
    def _gemm1x1(x, P, name, n_out=None):
        """x [..., K] NHWC 16-bit -> [..., N] via the GEMM kernel (1x1 convolution)."""
        w, b = P[name + ".w"], P[name + ".b"]
        lead = x.shape[:-1]
        a = x.reshape(-1, x.shape[-1])
        out = torch.empty(a.shape[0], w.shape[0], dtype=x.dtype, device=x.device)
        ops.gemm(a, w, b, out, ops.EPI_STORE16)
        return out.view(*lead, w.shape[0])

    @staticmethod
    def _rcu(x, P, name, extra=None):
        """ResidualConvUnit (dpt_block.py:79-142): x + conv2(relu(conv1(relu(x)))) (+ extra: a second residual added in the same epilogue)."""
        t = ops.conv3x3_nhwc(x, P[name + ".c1.w"], P[name + ".c1.b"], relu_in=True, relu_out=True)
        return ops.conv3x3_nhwc(t, P[name + ".c2.w"], P[name + ".c2.b"], residual=x, residual2=extra)

    def _fusion(self, P, r, x, skip=None, packed_out=False):
        if skip is not None:
            if self.split:      # x + rcu(skip): the add rides on the epilogue of the unit's last convolution
                x = self._rcu(skip, P, f"rf{r}.resConfUnit1", extra=x.contiguous())
            else:
                x = x + self._rcu(skip, P, f"rf{r}.resConfUnit1")
        # out_conv (1x1) commutes with the bilinear x2 (both linear, interpolation weights sum to 1): run it on the 4x
        # smaller map, then upsample (dpt_block.py:210-218 upsamples first)
        return ops.upsample2x_nhwc(self._gemm1x1(self._rcu(x, P, f"rf{r}.resConfUnit2"), P, f"rf{r}.out"), packed=packed_out)

    def _trunk(self, tokens, gh: int, gw: int, packed_out: bool = False):
        """tokens[hook] [BT, gh*gw, C] 16-bit -> path_1 [BT, 8gh, 8gw, 256] (dpt_head.py:35-62)."""
        P = self._packed()
        dt = self.compute_dtype
        t = [tokens[h] for h in self.dpt.hooks]
        BT = t[0].shape[0]
        maps = [x.reshape(BT, gh, gw, x.shape[-1]).to(dt).contiguous() for x in t]
        # reassemble: 1x1 (+ ConvT k=s as a GEMM followed by a depth-to-space copy)
        def convT(x, name, k):
            y = self._gemm1x1(x, P, name)                         # [BT, gh, gw, k*k*Cp]
            Cp = y.shape[-1] // (k * k)
            return y.view(BT, gh, gw, k, k, Cp).permute(0, 1, 3, 2, 4, 5).reshape(BT, gh * k, gw * k, Cp)
        l0 = convT(self._gemm1x1(maps[0], P, "ap0.0"), "ap0.1", 4)
        l1 = convT(self._gemm1x1(maps[1], P, "ap1.0"), "ap1.1", 2)
        l2 = self._gemm1x1(maps[2], P, "ap2.0")
        l3 = ops.conv3x3_nhwc(self._gemm1x1(maps[3], P, "ap3.0"), P["ap3.1.w"], P["ap3.1.b"], stride=2)
        l0, l1, l2, l3 = [ops.conv3x3_nhwc(l.contiguous(), P[f"rn{i}.w"], None) for i, l in enumerate((l0, l1, l2, l3))]
        p4 = self._fusion(P, 4, l3)[:, :l2.shape[1], :l2.shape[2]].contiguous()
        p3 = self._fusion(P, 3, p4, l2)
        p2 = self._fusion(P, 2, p3, l1)
        # packed_out (split class, pts3d head): path_1 only feeds a 3x3 convolution -- the bilinear kernel writes it packed (hi, lo)
        return self._fusion(P, 1, p2, l0, packed_out=packed_out), P

    operand_class = property(lambda self: "split" if self.split else _CLASS_OF[self.compute_dtype])      # as the route functions name it

    def forward_pts3d_raw(self, tokens, gh: int, gw: int) -> torch.Tensor:
        """-> [BT,C,H,W] view (channels-last memory, pixel stride 4) of the head output in the compute dtype, BEFORE the 'exp' post-process;
        C = 3 (xyz), or 4 with the confidence channel (predict_conf: the same fused kernels, whose fourth output column was zero padding)."""
        h, nc = self.dpt.head, self.num_channels
        route, trunk_packed = pts3d_route(self.operand_class, tokens[self.dpt.hooks[0]].shape[0], gh, gw, h[0].in_channels, h[0].out_channels, h[2].out_channels)
        x, P = self._trunk(tokens, gh, gw, packed_out=trunk_packed)
        x = ops.conv3x3_nhwc(x, P["h0.w"], P["h0.b"])
        # every arm -> [BT,H,W,4] (columns >= nc zero padding); in the one-kernel forms the 128-channel full-resolution activation never reaches HBM
        if route == "split_packed_dot":      # (hi, lo) pairs from the bilinear kernel (same bytes as f32): the head's main loop converts nothing
            y = ops.conv3x3_head1x1_nhwc(ops.upsample2x_nhwc(x, packed=True), P["h2.w"], P["h2.b"], self._lazy(P, "h4f32.w"), self._lazy(P, "h4f32.b"), nc)
        elif route == "fused16":
            y = ops.conv3x3_head1x1_nhwc(ops.upsample2x_nhwc(x), P["h2.w"], P["h2.b"], P["h4f.w"], P["h4f.b"], nc)
        else:
            assert route == "unfused", route
            y = self._gemm1x1(ops.conv3x3_nhwc(ops.upsample2x_nhwc(x), P["h2.w"], P["h2.b"], relu_out=True), P, "h4f")
        return y[..., :nc].permute(0, 3, 1, 2)

    def forward_pts3d(self, tokens, gh: int, gw: int) -> torch.Tensor:
        """-> [BT,H,W,3] f32 points; 'exp' depth mode (postprocess.py:46-56).  (distillation path only; the main
        path fuses this into the adapter kernel.)"""
        return self.postprocess_pts3d(self.forward_pts3d_raw(tokens, gh, gw))

    @staticmethod
    def postprocess_pts3d(raw: torch.Tensor) -> torch.Tensor:
        """[BT,>=3,H,W] raw head output -> [BT,H,W,3] f32 points, 'exp' depth mode: xyz / |xyz| * expm1(|xyz|) (postprocess.py:46-56)."""
        xyz = raw[:, :3].float().permute(0, 2, 3, 1)
        dist = xyz.norm(dim=-1, keepdim=True)
        return xyz / dist.clip(min=1e-8) * torch.expm1(dist)

    def forward_gs(self, tokens, frames: torch.Tensor, gh: int, gw: int) -> torch.Tensor:
        """-> [BT,C,H,W] view (channels-last memory) of the raw Gaussian parameters (dpt_gs_head.py:120-157)."""
        d, nc = self.dpt, self.num_channels
        x, P = self._trunk(tokens, gh, gw)
        H, W = frames.shape[-2], frames.shape[-1]
        route, stem = gs_route(self.operand_class, gh, gw, H, W, nc, x.shape[-1], d.input_merger[0].out_channels, d.head[0].out_channels)
        # conv3(256->256) -> ReLU -> conv1(256->nc) in one kernel (dpt_block.py:335-343; Dropout(0.1) is the identity at inference) -> [BT,H,W,96]
        fused = lambda xin: ops.conv3x3_head1x1_nhwc(xin, P["h0.w"], None, P["h4f.w"], P["h4f.b"], nc)
        if route == "split_stream_stem":     # up2(trunk) + relu(stem) leaves the stem kernel packed: no f32 stem map, no upsample-add launch
            y = fused(ops.stem7x7_up_split_stream(ops.pad_rgb_nhwc(frames, torch.float32), self._lazy(P, "stem.w32"), self._lazy(P, "stem.b"), H, W, x,
                                                  self._lazy(P, "stem.e")))
        elif route == "split_stem_up":
            y = fused(ops.conv7x7_rgb_nhwc(ops.pad_rgb_nhwc(frames, torch.float32), self._lazy(P, "stem.ws7"), self._lazy(P, "stem.b"), H, W, up_add=x))
        elif route == "split_up_packed":
            y = fused(ops.upsample2x_nhwc(x, add=self._stem(stem, frames, P), relu_add=True, packed=True))
        elif route == "fused16":
            y = fused(ops.upsample2x_nhwc(x, add=self._stem(stem, frames, P), relu_add=True))
        else:
            assert route == "unfused", route
            x = ops.upsample2x_nhwc(x, add=self._stem(stem, frames, P), relu_add=True)
            y = self._gemm1x1(ops.conv3x3_nhwc(x, P["h0.w"], None, relu_out=True), P, "h4")
        return y[..., :nc].permute(0, 3, 1, 2)
