"""The distillation teacher (DUSt3R two-view network) restated in plain PyTorch, in any dtype: the yardstick of tests/test_teacher_*.py.

Written from the architecture, not from the package: a weight dict with the reference's state_dict names goes in, torch.nn.functional does
the arithmetic.  `teacher_forward` is the network; `tail` is the post-process of the two heads (heads/postprocess.py:46-56, 73-74 with the
modes ('exp', -inf, inf) and ('exp', 1, inf)) with per-element magnitudes in the project's form: `mag` is the sum of the absolute terms
an output is formed from, through |R||p| + |t| for the transform.

`mutant=` switches ONE deliberate mistake on (test_teacher_cpu.py shows that the fixture's bound rejects each of them).  One cannot be
rejected by any input: "swap_cross_pos" hands the key's positions to the query and the query's to the key, and both views of a call share
one patch grid, so the two tables are equal and the swap changes nothing; "cross_k_no_rope" (the key side not rotated at all) is the
observable mistake next to it.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

MUTANTS = ("no_norm_y", "swap_cross_pos", "cross_k_no_rope", "dec2_is_dec1", "branch2_reads_current", "hook5", "dec_norm_one_branch")
TAIL_MUTANTS = ("exp_minus_1", "conf_no_plus_1")
F32_MAX = float(torch.finfo(torch.float32).max)


# ---------------------------------------------------------------------------------------------------------------------------
# network
# ---------------------------------------------------------------------------------------------------------------------------
def _lin(W, name, x):
    return F.linear(x, W[name + ".weight"], W.get(name + ".bias"))


def _ln(W, name, x):
    return F.layer_norm(x, (x.shape[-1],), W[name + ".weight"], W[name + ".bias"], 1e-6)


def _conv(W, name, x, stride=1, padding=0):
    return F.conv2d(x, W[name + ".weight"], W.get(name + ".bias"), stride=stride, padding=padding)


def rope2d(t: torch.Tensor, pos: torch.Tensor, base: float = 100.0) -> torch.Tensor:
    """t [B, heads, N, D], pos [N, 2] (y, x): the first half of D turns with y, the second with x, each as a rotate-half RoPE over D / 2.
    The angle table is formed in f32 whatever the dtype of t and then cast, as the reference's RoPE2D forms it -- its float64 run has
    f32-rounded angles, and a restatement that is to meet it to 1e-10 must have them too."""
    D = t.shape[-1] // 2
    inv = 1.0 / (base ** (torch.arange(0, D, 2).float() / D))

    def turn(u, p):
        ang = (p.float()[:, None] * inv[None, :]).to(u.dtype)
        ang = torch.cat([ang, ang], -1)
        u1, u2 = u[..., :D // 2], u[..., D // 2:]
        return u * ang.cos() + torch.cat([-u2, u1], -1) * ang.sin()

    return torch.cat([turn(t[..., :D], pos[:, 0]), turn(t[..., D:], pos[:, 1])], -1)


def _heads(x, h):
    B, N, C = x.shape
    return x.reshape(B, N, h, C // h).transpose(1, 2)


def _attend(q, k, v):
    a = (q @ k.transpose(-2, -1)) * q.shape[-1] ** -0.5
    o = a.softmax(-1) @ v
    return o.transpose(1, 2).reshape(o.shape[0], o.shape[2], -1)


def _self_attn(W, p, x, pos, h):
    B, N, C = x.shape
    qkv = _lin(W, p + ".qkv", x).reshape(B, N, 3, h, C // h).permute(2, 0, 3, 1, 4)
    return _lin(W, p + ".proj", _attend(rope2d(qkv[0], pos), rope2d(qkv[1], pos), qkv[2]))


def _mlp(W, p, x):
    return _lin(W, p + ".fc2", F.gelu(_lin(W, p + ".fc1", x)))


def _dec_block(W, p, x, y, xpos, ypos, h, mutant):
    x = x + _self_attn(W, p + ".attn", _ln(W, p + ".norm1", x), xpos, h)
    y_ = y if mutant == "no_norm_y" else _ln(W, p + ".norm_y", y)
    qpos, kpos = (ypos, xpos) if mutant == "swap_cross_pos" else (xpos, ypos)
    q = rope2d(_heads(_lin(W, p + ".cross_attn.projq", _ln(W, p + ".norm2", x)), h), qpos)
    k = _heads(_lin(W, p + ".cross_attn.projk", y_), h)
    k = k if mutant == "cross_k_no_rope" else rope2d(k, kpos)
    v = _heads(_lin(W, p + ".cross_attn.projv", y_), h)
    x = x + _lin(W, p + ".cross_attn.proj", _attend(q, k, v))
    return x + _mlp(W, p + ".mlp", _ln(W, p + ".norm3", x))


def _dpt_raw(W, p, toks, gh, gw):
    """hooked tokens [n, gh * gw, C] x 4 -> raw head output [n, 4, 16 gh, 16 gw]"""
    maps = [t.transpose(1, 2).reshape(t.shape[0], -1, gh, gw) for t in toks]
    ap = p + ".act_postprocess."
    l0 = F.conv_transpose2d(_conv(W, ap + "0.0", maps[0]), W[ap + "0.1.weight"], W[ap + "0.1.bias"], stride=4)
    l1 = F.conv_transpose2d(_conv(W, ap + "1.0", maps[1]), W[ap + "1.1.weight"], W[ap + "1.1.bias"], stride=2)
    l2 = _conv(W, ap + "2.0", maps[2])
    l3 = _conv(W, ap + "3.1", _conv(W, ap + "3.0", maps[3]), stride=2, padding=1)
    ls = [_conv(W, f"{p}.scratch.layer_rn.{i}", l, padding=1) for i, l in enumerate((l0, l1, l2, l3))]

    def rcu(q, x):
        return x + _conv(W, q + ".conv2", F.relu(_conv(W, q + ".conv1", F.relu(x), padding=1)), padding=1)

    def fuse(r, x, skip=None):
        q = f"{p}.scratch.refinenet{r}"
        if skip is not None:
            x = x + rcu(q + ".resConfUnit1", skip)
        x = F.interpolate(rcu(q + ".resConfUnit2", x), scale_factor=2, mode="bilinear", align_corners=True)
        return _conv(W, q + ".out_conv", x)

    x = fuse(4, ls[3])[:, :, :ls[2].shape[2], :ls[2].shape[3]]
    x = fuse(1, fuse(2, fuse(3, x, ls[2]), ls[1]), ls[0])
    x = _conv(W, p + ".head.0", x, padding=1)
    x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
    return _conv(W, p + ".head.4", F.relu(_conv(W, p + ".head.2", x, padding=1)))


def teacher_forward(W: dict, image: torch.Tensor, enc_heads: int, dec_heads: int, dtype=torch.float64, mutant: str | None = None,
                    probe=None):
    """W: the teacher's state dict; image [B, 2, 3, H, W] (already normalised) -> (res1, res2), each {"pts3d" [B, H, W, 3], "conf" [B, H, W],
    "raw" [B, H, W, 4]} in `dtype`; view 2's points in view 1's frame.  probe(name, tensor) sees every block's output (enc%02d: both views
    as one batch of 2B, view 1 first; dec%02d_1 / dec%02d_2)."""
    assert mutant is None or mutant in MUTANTS, mutant
    W = {k: v.to(dtype) for k, v in W.items()}
    B, _, _, H, Wd = image.shape
    n_enc = 1 + max(int(k.split(".")[1]) for k in W if k.startswith("enc_blocks."))
    n_dec = 1 + max(int(k.split(".")[1]) for k in W if k.startswith("dec_blocks."))
    gh, gw = H // 16, Wd // 16
    pos = torch.cartesian_prod(torch.arange(gh), torch.arange(gw))
    x = torch.cat([image[:, 0], image[:, 1]], 0).to(dtype)
    x = _conv(W, "patch_embed.proj", x, stride=16).flatten(2).transpose(1, 2)
    for i in range(n_enc):
        p = f"enc_blocks.{i}"
        x = x + _self_attn(W, p + ".attn", _ln(W, p + ".norm1", x), pos, enc_heads)
        x = x + _mlp(W, p + ".mlp", _ln(W, p + ".norm2", x))
        if probe is not None:
            probe(f"enc{i:02d}", x)
    x = _ln(W, "enc_norm", x)
    outs = [(x[:B], x[B:])]
    f = _lin(W, "decoder_embed", x)
    f1, f2 = f[:B], f[B:]
    for i in range(n_dec):
        b1, b2 = f"dec_blocks.{i}", (f"dec_blocks.{i}" if mutant == "dec2_is_dec1" else f"dec_blocks2.{i}")
        n1 = _dec_block(W, b1, f1, f2, pos, pos, dec_heads, mutant)
        n2 = _dec_block(W, b2, f2, n1 if mutant == "branch2_reads_current" else f1, pos, pos, dec_heads, mutant)
        f1, f2 = n1, n2
        if probe is not None:
            probe(f"dec{i:02d}_1", f1)
            probe(f"dec{i:02d}_2", f2)
        outs.append((f1, f2))
    outs[-1] = (_ln(W, "dec_norm", f1), f2 if mutant == "dec_norm_one_branch" else _ln(W, "dec_norm", f2))
    hooks = [0, n_dec * 2 // 4 - (1 if mutant == "hook5" else 0), n_dec * 3 // 4, n_dec]
    res = []
    for v in (0, 1):
        raw = _dpt_raw(W, f"downstream_head{v + 1}.dpt", [outs[h][v] for h in hooks], gh, gw).permute(0, 2, 3, 1)
        t = tail(raw)
        res.append(dict(pts3d=t["pts"], conf=t["conf"], raw=raw))
    return res[0], res[1]


# ---------------------------------------------------------------------------------------------------------------------------
# tail
# ---------------------------------------------------------------------------------------------------------------------------
def tail(raw: torch.Tensor, transform: torch.Tensor | None = None, mutant: str | None = None, f32_overflow: bool = False) -> dict:
    """raw [n, H, W, 4] -> pts [n, H, W, 3], conf [n, H, W] in raw's dtype, and the magnitudes mag_pts / mag_conf (same shapes):
    d = |xyz|, p = xyz / max(d, 1e-8) * expm1(d), pts = R p + t with transform [n, 3, 4], conf = 1 + exp(c).
    mag_pts = |p| without a transform, |R||p| + |t| with one; mag_conf = 1 + exp(c).
    f32_overflow (the float64 yardstick of an f32 kernel): expm1(d) is +inf from where its f32 value is, as the reference's f32 arithmetic has
    it; a zero component stays an exact zero there and a product of the transform with a zero factor is left out (0 * inf is 0)."""
    assert mutant is None or mutant in TAIL_MUTANTS, mutant
    xyz, c = raw[..., :3], raw[..., 3]
    d = xyz.norm(dim=-1, keepdim=True)
    e = (d.exp() - 1) if mutant == "exp_minus_1" else d.expm1()
    if f32_overflow:
        e = torch.where(e > F32_MAX, torch.full_like(e, math.inf), e)
    p = xyz / d.clip(min=1e-8) * e
    if f32_overflow:
        p = torch.where(xyz == 0, torch.zeros_like(p), p)
    mag = p.abs()
    if transform is not None:
        T = transform.to(raw.dtype)
        R, t = T[:, None, None, :, :3], T[:, None, None, :, 3]
        prod = R * p[..., None, :]                                   # [n, H, W, 3 (i), 3 (j)]
        aprod = R.abs() * p.abs()[..., None, :]
        if f32_overflow:
            skip = (R == 0) | (p[..., None, :] == 0)
            prod, aprod = torch.where(skip, torch.zeros_like(prod), prod), torch.where(skip, torch.zeros_like(aprod), aprod)
        p = prod.sum(-1) + t
        mag = aprod.sum(-1) + t.abs()
    conf = c.exp() if mutant == "conf_no_plus_1" else 1 + c.exp()
    return dict(pts=p, conf=conf, mag_pts=mag, mag_conf=1 + c.exp())


def tail_torch_f32(raw: torch.Tensor, transform: torch.Tensor | None = None):
    """The PyTorch passes the kernel replaces, in f32 as the package ran them: PixelwiseTaskWithDPT.postprocess_pts3d, the confidence of
    vicasplat.py and the einsum + add of distillation_loss."""
    raw = raw.float()
    xyz = raw[..., :3]
    dist = xyz.norm(dim=-1, keepdim=True)
    p = xyz / dist.clip(min=1e-8) * torch.expm1(dist)
    if transform is not None:
        T = transform.float()
        p = torch.einsum("bij,bhwj->bhwi", T[:, :, :3], p) + T[:, None, None, :, 3]
    return p, 1 + raw[..., 3].exp()


def tail_ratio(got_pts, got_conf, ref: dict) -> float:
    """max over the finite elements of |got - ref| / (2^-24 mag): the error in units of the f32 rounding of the magnitude."""
    worst = 0.0
    for got, want, mag in ((got_pts, ref["pts"], ref["mag_pts"]), (got_conf, ref["conf"], ref["mag_conf"])):
        fin = torch.isfinite(want) & torch.isfinite(mag) & (mag > 0) & torch.isfinite(got)      # (torch's f32 0 * inf is NaN where the yardstick is 0)
        if fin.any():
            worst = max(worst, float(((got.double() - want).abs()[fin] / (2.0 ** -24 * mag[fin])).max()))
    return worst


def tail_edge_input(n: int, H: int, W: int, dtype: torch.dtype, seed: int = 0) -> torch.Tensor:
    """raw [n, H, W, 4] of `dtype` (f32 or f16): seeded normal values with the edge values planted at the front of every image (as many as
    the image has pixels for): the zero vector; d = 1e-6 and 1e-3 (in f16 the components of the first are subnormals, 5.96e-7 and 7.75e-7: the 8-byte load path's conversion); d = 88 and 89
    along one axis, just below and just above ln(f32 max) = 88.72 where the f32 expm1 overflows; c in {-inf, -100, 0, 88, 89}.  Every
    component is exactly 0 or at least 1e-18 in size, so no f32 square underflows where the float64 one does not."""
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(n, H, W, 4, generator=g)
    raw[..., :3] *= 1.5
    small = (1e-6, 1e-3)
    edges = [
        ((0.0, 0.0, 0.0), 0.0),
        ((small[0] * 0.6, 0.0, -small[0] * 0.8), -math.inf),
        ((small[1] * 0.6, -small[1] * 0.8, 0.0), -100.0),
        ((0.0, 88.0, 0.0), 88.0),
        ((0.0, 0.0, -89.0), 89.0),
        ((-88.0, 0.0, 0.0), 0.0),
        ((89.0, 0.0, 0.0), -100.0),
        ((52.0, -50.0, 50.0), 89.0),           # d = 87.8: every component huge and finite
    ]
    flat = raw.view(n, H * W, 4)
    for i, (xyz, c) in enumerate(edges[:H * W]):
        flat[:, i, :3] = torch.tensor(xyz)
        flat[:, i, 3] = c
    if H * W == 1:      # a single pixel per image: the images take the edges in turn
        for b in range(n):
            xyz, c = edges[b % len(edges)]
            flat[b, 0, :3], flat[b, 0, 3] = torch.tensor(xyz), c
    raw = raw.to(dtype)
    tiny = (raw[..., :3] != 0) & (raw[..., :3].abs().float() < 1e-18)
    assert not tiny.any()
    return raw


def tail_transforms(n: int, seed: int = 0) -> torch.Tensor:
    """n different rigid transforms [n, 3, 4] f32: seeded rotations (orthonormalised), translations of a few units; the first is axis-aligned
    (a permutation with a sign: zeros in R, the case the zero-skip rule is for)."""
    g = torch.Generator().manual_seed(1000 + seed)
    q, _ = torch.linalg.qr(torch.randn(n, 3, 3, generator=g, dtype=torch.float64))
    q[0] = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    t = 3.0 * torch.randn(n, 3, 1, generator=g, dtype=torch.float64)
    return torch.cat([q, t], -1).float()


def teacher_input(b: int, h: int, w: int, seed: int) -> torch.Tensor:
    """[b, 2, 3, h, w] in [-1, 1]: a smooth pattern plus seeded noise, view 2 a phase-shifted copy of view 1's pattern (the fixture's input)."""
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    img = torch.empty(b, 2, 3, h, w)
    for s in range(b):
        for v in range(2):
            for c in range(3):
                img[s, v, c] = 0.6 * torch.sin(2 * math.pi * ((2 + s) * xs / w + (1 + c) * ys / h) + 0.7 * v + c)
    return (img + 0.3 * (torch.rand(img.shape, generator=g) - 0.5)).clamp(-1, 1)


TINY = dict(enc_depth=2, dec_depth=12, enc_embed_dim=128, dec_embed_dim=64, enc_num_heads=2, dec_num_heads=1)      # the fixture's teacher


def checksum(t: torch.Tensor) -> torch.Tensor:
    """mean, mean |.| and eight fixed elements of a block's output, in float64 (the per-block fingerprint of the fixture)."""
    f = t.detach().double().flatten()
    idx = torch.tensor([p % f.numel() for p in (0, 1, 7, 100, 1000, 5000, 20000, 50000)])
    return torch.cat([f.mean()[None], f.abs().mean()[None], f[idx]])
