"""The distillation teacher: the DUSt3R two-view network (src/model/distiller/dust3d_backbone.py, croco/blocks.py:94-191) -- MI355X-native.

Module tree and parameter names are the reference's (mask_token, patch_embed.proj, enc_blocks.*, enc_norm, decoder_embed, dec_blocks.* and
dec_blocks2.*, dec_norm, downstream_head1.dpt.*, downstream_head2.dpt.*), so `load_state_dict(ckpt["model"], strict=True)` accepts its
checkpoints; a checkpoint without dec_blocks2.* gets the first decoder's weights there, as in the reference.  As in backbone_vica.py the
nn.Modules only HOLD the parameters; the forward drives the HIP operators (vicasplat_amd.ops) over flat token buffers:

  * both views go through the encoder as ONE batch of 2B frames (view 1 of every scene first): the enc_blocks loop of VicaNet, on
    gh * gw tokens per frame (no intrinsic token);
  * the two decoders keep their residual streams in one f32 buffer [2, B * N, C].  A step first forms, from the PREVIOUS pair, what each
    branch needs of the other (norm_y of the other branch's stream), then updates both streams in place: no copy of a stream is kept;
  * cross-attention: norm2(x) and norm_y(y) sit in the two halves of one operand buffer, ONE q|k|v projection with the RoPE epilogue runs
    over both halves (q of the second half and k | v of the first are computed and never read: 3 of a block's 19 C x C products), and the
    attention kernel reads q from the first half and k | v of the other view through its `kv_seg` row segments -- K / V are not copied.
    Both views share one patch grid, so one position table serves the query's and the key's RoPE;
  * hooks 0 (encoder output before decoder_embed), 6, 9 and 12 (after dec_norm) feed the two four-channel pts3d DPT heads, whose raw
    channels-last output goes through ONE streaming kernel (ops.points_conf, csrc/teacher.hip) to points and confidences.

Operand classes: "split" (default, as get_encoder chooses it) and "f16".  HIP device tensors only; there is no CPU fallback.
Parity with the published DUSt3R weights is UNVERIFIED: no DUSt3R checkpoint exists where this package is built and tested; the network is
pinned against the real reference on seeded weights (tests/golden/teacher_tiny.npz).
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional

import torch
from torch import nn

from ... import ops
from ..encoder.backbone.backbone_vica import _Attention, _CrossNeighborAttention, _EncBlock, _Mlp, _PatchEmbed
from ..encoder.heads.dpt import PixelwiseTaskWithDPT


class _TeacherDecBlock(nn.Module):      # croco/blocks.py:171-191 (DecoderBlock): parameters only
    def __init__(self, dim: int, heads: int, mlp_ratio: float):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = _Attention(dim, heads)
        self.cross_attn = _CrossNeighborAttention(dim, heads)      # projq / projk / projv / proj: the same four layers
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.norm3 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = _Mlp(dim, int(dim * mlp_ratio))
        self.norm_y = nn.LayerNorm(dim, eps=1e-6)


class Dust3R(nn.Module):
    def __init__(self, img_size=(512, 512), patch_size=16, enc_embed_dim=1024, enc_depth=24, enc_num_heads=16, dec_embed_dim=768, dec_depth=12,
                 dec_num_heads=12, mlp_ratio=4.0, pos_embed="RoPE100", head_type="dpt", output_mode="pts3d",
                 depth_mode=("exp", -float("inf"), float("inf")), conf_mode=("exp", 1, float("inf")), compute_dtype="split"):
        super().__init__()
        if pos_embed != "RoPE100" or head_type != "dpt" or output_mode != "pts3d" or tuple(depth_mode) != ("exp", -float("inf"), float("inf")) \
                or tuple(conf_mode) != ("exp", 1, float("inf")) or patch_size != 16:
            raise NotImplementedError("only the configuration of the reference's get_distiller is implemented (RoPE100, DPT heads, pts3d, depth mode "
                                      "('exp', -inf, inf), confidence mode ('exp', 1, inf), 16-pixel patches)")
        if enc_embed_dim % 64 or dec_embed_dim % 64 or enc_embed_dim // enc_num_heads != 64 or dec_embed_dim // dec_num_heads != 64:
            raise NotImplementedError("the HIP attention kernel is specialised for head_dim 64")
        self.config = SimpleNamespace(img_size=tuple(img_size), patch_size=patch_size, enc_embed_dim=enc_embed_dim, enc_depth=enc_depth,
                                      enc_num_heads=enc_num_heads, dec_embed_dim=dec_embed_dim, dec_depth=dec_depth, dec_num_heads=dec_num_heads,
                                      mlp_ratio=mlp_ratio)
        self.enc_depth, self.dec_depth, self.enc_embed_dim, self.dec_embed_dim = enc_depth, dec_depth, enc_embed_dim, dec_embed_dim
        self.depth_mode, self.conf_mode = tuple(depth_mode), tuple(conf_mode)
        self.patch_embed = _PatchEmbed(patch_size, enc_embed_dim)
        self.enc_blocks = nn.ModuleList([_EncBlock(enc_embed_dim, enc_num_heads, mlp_ratio) for _ in range(enc_depth)])
        self.enc_norm = nn.LayerNorm(enc_embed_dim, eps=1e-6)
        self.mask_token = nn.Parameter(torch.zeros(1, 1, dec_embed_dim))      # CroCo's; never read by the two-view forward
        self.decoder_embed = nn.Linear(enc_embed_dim, dec_embed_dim, bias=True)
        self.dec_blocks = nn.ModuleList([_TeacherDecBlock(dec_embed_dim, dec_num_heads, mlp_ratio) for _ in range(dec_depth)])
        self.dec_norm = nn.LayerNorm(dec_embed_dim, eps=1e-6)
        self.dec_blocks2 = nn.ModuleList([_TeacherDecBlock(dec_embed_dim, dec_num_heads, mlp_ratio) for _ in range(dec_depth)])
        self.downstream_head1 = PixelwiseTaskWithDPT(self, 4, "regression")
        self.downstream_head2 = PixelwiseTaskWithDPT(self, 4, "regression")
        self._probe = None      # test hook: callable(name, tensor) on every block's output stream (enc%02d, dec%02d_1, dec%02d_2)
        self._wp: dict = {}
        self._wp_key = None
        self._tables: dict = {}
        self.set_compute_dtype(compute_dtype)
        self.requires_grad_(False)      # a frozen teacher (the reference converts its parameters to buffers)
        super().train(False)

    def train(self, mode: bool = True):
        """The teacher stays in eval mode whatever the module that holds it is switched to."""
        return super().train(False)

    def set_compute_dtype(self, dt):
        """"split" (default: f32 activations, f16 (hi, lo) operand pairs, three MFMAs per product) or "f16" / torch.float16."""
        if dt not in ("split", "f16", torch.float16):
            raise ValueError(f'Dust3R: the operand class must be "split" or "f16", got {dt!r}')
        self.split = dt == "split"
        self.compute_dtype = torch.float32 if self.split else torch.float16
        for h in (self.downstream_head1, self.downstream_head2):
            h.compute_dtype, h.split = self.compute_dtype, self.split

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """A checkpoint without the second decoder gets the first decoder's weights there (dust3d_backbone.py:54-61)."""
        sd = dict(state_dict)
        if not any(k.startswith("dec_blocks2") for k in sd):
            for k, v in state_dict.items():
                if k.startswith("dec_blocks"):
                    sd[k.replace("dec_blocks", "dec_blocks2")] = v
        return super().load_state_dict(sd, strict=strict, **kw)

    # ---- packed operand copies of the GEMM weights, re-made when a parameter changes or moves or the class changes ----
    def _weights(self):
        key = (self.split, self.patch_embed.proj.weight.device, sum(p._version for p in self.parameters()), id(self.patch_embed.proj.weight))
        if key == self._wp_key:
            return self._wp
        c = (lambda t: ops.split_pack_weight(t)) if self.split else (lambda t: t.detach().to(torch.float16).contiguous())
        W = {"patch": c(self.patch_embed.proj.weight.flatten(1)), "dec_embed": c(self.decoder_embed.weight)}
        for i, b in enumerate(self.enc_blocks):
            W[f"e{i}.qkv"], W[f"e{i}.proj"] = c(b.attn.qkv.weight), c(b.attn.proj.weight)
            W[f"e{i}.fc1"], W[f"e{i}.fc2"] = c(b.mlp.fc1.weight), c(b.mlp.fc2.weight)
        for v, blocks in enumerate((self.dec_blocks, self.dec_blocks2)):
            for i, b in enumerate(blocks):
                p, ca = f"d{v}.{i}", b.cross_attn
                W[p + ".qkv"], W[p + ".proj"] = c(b.attn.qkv.weight), c(b.attn.proj.weight)
                W[p + ".cqkv"] = c(torch.cat([ca.projq.weight, ca.projk.weight, ca.projv.weight], 0))
                W[p + ".cqkv_b"] = torch.cat([ca.projq.bias, ca.projk.bias, ca.projv.bias], 0).detach().float().contiguous()
                W[p + ".cproj"] = c(ca.proj.weight)
                W[p + ".fc1"], W[p + ".fc2"] = c(b.mlp.fc1.weight), c(b.mlp.fc2.weight)
        self._wp, self._wp_key = W, key
        return W

    def _pos_tables(self, B: int, gh: int, gw: int, dev):
        key = (B, gh, gw, str(dev))
        if key not in self._tables:
            N = gh * gw
            ys, xs = torch.meshgrid(torch.arange(gh), torch.arange(gw), indexing="ij")
            frame = torch.stack([ys, xs], -1).reshape(N, 2).int()
            # cross-attention operand buffer: rows [0, B N) hold norm2(x), rows [B N, 2 B N) norm_y(y); scene b reads the keys of its own scene
            seg = torch.tensor([[B * N + b * N, N, 0, 0] for b in range(B)], dtype=torch.int32)
            self._tables[key] = dict(pos=frame.repeat(2 * B, 1).contiguous().to(dev), seg=seg.to(dev))
        return self._tables[key]

    # ------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, context: dict, symmetrize_batch: bool = False, return_views: bool = False, normalize: bool = False, *,
                transform: Optional[torch.Tensor] = None):
        """context["image"] [B, 2 (or more: the first two are read), 3, H, W] -> (res1, res2), each {"pts3d" [B,H,W,3], "conf" [B,H,W]} in f32;
        view 2's points in view 1's frame (dust3d_backbone.py:187-226).  normalize: the images are in [0, 1] and are mapped to [-1, 1].
        return_views: also the two views, {"img": ...}.  H and W are multiples of 16 and H <= W: a portrait input raises (the reference
        transposes portrait inputs around its heads; that is not implemented).  symmetrize_batch=True belongs to estimate_pose and its
        global aligner and raises NotImplementedError.
        transform (extension; None gives the reference's outputs): [B, 3, 4] or [B, 4, 4] rigid transform per scene, applied to the points
        of BOTH views inside the tail kernel (callers.distill_targets passes the first anchor's extrinsics)."""
        if symmetrize_batch:
            raise NotImplementedError("Dust3R.forward(symmetrize_batch=True) serves estimate_pose, whose global aligner is not part of this package")
        image = context["image"]
        if not image.is_cuda:
            raise RuntimeError("Dust3R.forward needs HIP device tensors: vicasplat_amd has no CPU fallback path")
        B, _, _, H, Wd = image.shape
        cfg, dt, dev = self.config, self.compute_dtype, image.device
        p = cfg.patch_size
        if H % p or Wd % p:
            raise ValueError(f"Dust3R.forward: {H} x {Wd} is no multiple of the {p}-pixel patch")
        if H > Wd:
            raise NotImplementedError(f"Dust3R.forward: portrait input {H} x {Wd} (the reference's transpose around the heads is not implemented); "
                                      "pass landscape frames")
        if normalize:
            image = (image - 0.5) / 0.5
        view1, view2 = image[:, 0], image[:, 1]
        if transform is not None:
            if transform.dim() != 3 or transform.shape[0] != B or tuple(transform.shape[1:]) not in ((3, 4), (4, 4)):
                raise ValueError(f"Dust3R.forward: transform must be [B, 3, 4] or [B, 4, 4], got {tuple(transform.shape)}")
            transform = transform[:, :3].float().contiguous()
        gh, gw = H // p, Wd // p
        N, F2 = gh * gw, 2 * B
        R = B * N                      # rows of one view
        Ce, Cd, He, Hd = cfg.enc_embed_dim, cfg.dec_embed_dim, cfg.enc_num_heads, cfg.dec_num_heads
        W = self._weights()
        tabs = self._pos_tables(B, gh, gw, dev)
        pos = tabs["pos"]
        f32 = dict(dtype=torch.float32, device=dev)
        split = self.split
        act = (lambda r, c: ops.split_act(r, c, dev)) if split else (lambda r, c: torch.empty(r, c, dtype=dt, device=dev))
        raw = lambda t: t.data if split else t                                                      # the tensor behind an operand buffer
        rows = lambda t, a, b: ops.SplitWeight(t.data[a:b], 1.0, (b - a, t.shape[1])) if split else t[a:b]      # a row range of one, as an operand
        cols3 = lambda t, C_: (raw(t)[:, :C_], raw(t)[:, C_:2 * C_], raw(t)[:, 2 * C_:])

        # ---- patch embedding as a GEMM over im2col rows; both views as one batch, view 1 of every scene first ----
        frames = torch.cat([view1, view2], 0).float().reshape(F2, 3, gh, p, gw, p)
        cols = frames.permute(0, 2, 4, 1, 3, 5).reshape(F2 * N, 3 * p * p).to(dt)
        xe = torch.empty(F2 * N, Ce, **f32)
        ops.gemm(cols, W["patch"], self.patch_embed.proj.bias, xe, ops.EPI_STORE32)

        # ---- encoder blocks (croco/blocks.py:94-130): the loop of VicaNet.forward ----
        h, qkv, att = act(F2 * N, Ce), act(F2 * N, 3 * Ce), act(F2 * N, Ce)
        hid = act(F2 * N, int(Ce * cfg.mlp_ratio))
        for i, blk in enumerate(self.enc_blocks):
            ops.layernorm_mod(xe, blk.norm1.weight, blk.norm1.bias, h)
            ops.gemm_qkv_rope(h, W[f"e{i}.qkv"], blk.attn.qkv.bias, qkv, Ce, pos, None, 100.0, 1.0)
            ops.attention(*cols3(qkv, Ce), att, nbatch=F2, H=He, Lq=N, Lk=N, q_batch_rows=N, k_batch_rows=N, split=split)
            ops.gemm(att, W[f"e{i}.proj"], blk.attn.proj.bias, xe, ops.EPI_RESID32)
            ops.layernorm_mod(xe, blk.norm2.weight, blk.norm2.bias, h)
            ops.gemm(h, W[f"e{i}.fc1"], blk.mlp.fc1.bias, hid, ops.EPI_GELU16)
            ops.gemm(hid, W[f"e{i}.fc2"], blk.mlp.fc2.bias, xe, ops.EPI_RESID32)
            if self._probe is not None:
                self._probe(f"enc{i:02d}", xe)
        enc = torch.empty(F2 * N, Ce, dtype=dt, device=dev)
        ops.layernorm_mod(xe, self.enc_norm.weight, self.enc_norm.bias, enc)
        del h, qkv, att, hid

        # ---- the two decoders (dust3d_backbone.py:146-165, croco/blocks.py:186-191) ----
        L = cfg.dec_depth
        hooks = (L * 2 // 4, L * 3 // 4)
        tokens = [[None] * (L + 1), [None] * (L + 1)]
        for v in (0, 1):
            tokens[v][0] = enc[v * R:(v + 1) * R].view(B, N, Ce)
        xd = torch.empty(2 * R, Cd, **f32)
        ops.gemm(enc, W["dec_embed"], self.decoder_embed.bias, xd, ops.EPI_STORE32)
        x = (xd[:R], xd[R:])
        h, qkv, att = act(R, Cd), act(R, 3 * Cd), act(R, Cd)
        hid = act(R, int(Cd * cfg.mlp_ratio))
        hc = (act(2 * R, Cd), act(2 * R, Cd))        # per branch: norm2(x) | norm_y(y)
        qkvc = act(2 * R, 3 * Cd)
        pos1 = pos[:R]
        for i in range(L):
            blks = (self.dec_blocks[i], self.dec_blocks2[i])
            # both branches read the PREVIOUS pair: the other stream's norm_y leaves before either stream is updated
            for v, blk in enumerate(blks):
                ops.layernorm_mod(x[1 - v], blk.norm_y.weight, blk.norm_y.bias, rows(hc[v], R, 2 * R))
            for v, blk in enumerate(blks):
                xv, k = x[v], f"d{v}.{i}"
                ops.layernorm_mod(xv, blk.norm1.weight, blk.norm1.bias, h)
                ops.gemm_qkv_rope(h, W[k + ".qkv"], blk.attn.qkv.bias, qkv, Cd, pos1, None, 100.0, 1.0)
                ops.attention(*cols3(qkv, Cd), att, nbatch=B, H=Hd, Lq=N, Lk=N, q_batch_rows=N, k_batch_rows=N, split=split)
                ops.gemm(att, W[k + ".proj"], blk.attn.proj.bias, xv, ops.EPI_RESID32)
                # cross-attention: q from norm2(x) (rows [0, R)), k | v from norm_y(y) (rows [R, 2R)) through the row segments
                ops.layernorm_mod(xv, blk.norm2.weight, blk.norm2.bias, rows(hc[v], 0, R))
                ops.gemm_qkv_rope(hc[v], W[k + ".cqkv"], W[k + ".cqkv_b"], qkvc, Cd, pos, None, 100.0, 1.0)
                qc, kc, vc = cols3(qkvc, Cd)
                ops.attention(qc[:R], kc, vc, att, nbatch=B, H=Hd, Lq=N, q_batch_rows=N, kv_seg=tabs["seg"], split=split)
                ops.gemm(att, W[k + ".cproj"], blk.cross_attn.proj.bias, xv, ops.EPI_RESID32)
                ops.layernorm_mod(xv, blk.norm3.weight, blk.norm3.bias, h)
                ops.gemm(h, W[k + ".fc1"], blk.mlp.fc1.bias, hid, ops.EPI_GELU16)
                ops.gemm(hid, W[k + ".fc2"], blk.mlp.fc2.bias, xv, ops.EPI_RESID32)
            if self._probe is not None:
                self._probe(f"dec{i:02d}_1", x[0])
                self._probe(f"dec{i:02d}_2", x[1])
            if (i + 1) in hooks:
                for v in (0, 1):
                    tokens[v][i + 1] = x[v].view(B, N, Cd).to(dt, copy=True)      # (copy: the stream keeps changing, and dt may be f32)
        last = torch.empty(2 * R, Cd, dtype=dt, device=dev)
        ops.layernorm_mod(xd, self.dec_norm.weight, self.dec_norm.bias, last)
        for v in (0, 1):
            tokens[v][L] = last[v * R:(v + 1) * R].view(B, N, Cd)

        # ---- the two heads and the tail kernel ----
        res = []
        for v, head in enumerate((self.downstream_head1, self.downstream_head2)):
            out = head.forward_pts3d_raw(tokens[v], gh, gw).permute(0, 2, 3, 1)      # [B, H, W, 4], the kernels' own channels-last memory
            pts, conf = ops.points_conf(out if out.is_contiguous() else out.contiguous(), transform)
            res.append({"pts3d": pts, "conf": conf})
        if return_views:
            return res[0], res[1], {"img": view1}, {"img": view2}
        return res[0], res[1]
