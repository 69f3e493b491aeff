"""Every kernel route of the DPT heads (vicasplat_amd/model/encoder/heads/dpt.py), run once on the smallest shape that selects it.

PixelwiseTaskWithDPT on a stub backbone (64-wide tokens, dec_depth 12; the heads keep feat = 256 and layer_dims (96, 192, 384, 768), which
the routes depend on), seeded random weights and tokens.  The `ops` front-ends of the tail are wrapped with a recorder that calls through;
each case asserts that (1) the route function names the expected route for these shapes, (2) the calls after the trunk are the sequence
that route stands for, (3) the output is finite and has the documented shape.  No numeric tolerance: the committed goldens of
test_encoder_gpu / test_f32_path_gpu / test_split_path_gpu / test_e2e_gpu carry the numerics.

BT = 1 frame of 2 x 2 tokens (a 32 x 32 image) everywhere, except: the trunk-packing case needs 64 * BT * gh * gw >= 224 * 256 (4 frames of
16 x 16 tokens), and `split_stem_up` needs a width that is no multiple of 32 (3 x 3 tokens, 48 x 48).  `split_up_packed` is selected by
no shape that the stock module can run (its trunk and stem are both `feat` wide, and a frame that is not 16gh x 16gw is refused by the
upsample-add): its arm is run by handing the forward that route name, and the route function is asserted NOT to name it.
"""
from types import SimpleNamespace

import pytest
import torch

from vicasplat_amd import ops
from vicasplat_amd.model.encoder.heads import dpt

pytestmark = pytest.mark.gpu

RECORDED = ("upsample2x_nhwc", "conv3x3_nhwc", "conv3x3_head1x1_nhwc", "gemm", "conv7x7_rgb_nhwc", "stem7x7_up_split_stream")
FLAGS = ("add", "up_add", "packed", "relu_out")      # keyword arguments that tell the calls of one front-end apart
CLASSES = {"split": (torch.float32, True), "f32": (torch.float32, False), "f16": (torch.float16, False), "bf16": (torch.bfloat16, False)}

# what each route stands for: the calls that follow the trunk's last bilinear pass (pts3d: and the head's first 3x3 convolution)
PTS3D_TAIL = {
    "split_packed_dot": ["upsample2x_nhwc[packed]", "conv3x3_head1x1_nhwc"],
    "fused16": ["upsample2x_nhwc", "conv3x3_head1x1_nhwc"],
    "unfused": ["upsample2x_nhwc", "conv3x3_nhwc[relu_out]", "gemm"],
}
STEM_MAP = {"split7": "conv7x7_rgb_nhwc", "window16": "conv7x7_rgb_nhwc", "im2col_f32": "gemm"}     # (im2col: one GEMM per 8 frames)
GS_TAIL = {
    "split_stream_stem": lambda stem: ["stem7x7_up_split_stream", "conv3x3_head1x1_nhwc"],
    "split_stem_up": lambda stem: ["conv7x7_rgb_nhwc[up_add]", "conv3x3_head1x1_nhwc"],
    "split_up_packed": lambda stem: [STEM_MAP[stem], "upsample2x_nhwc[add,packed]", "conv3x3_head1x1_nhwc"],
    "fused16": lambda stem: [STEM_MAP[stem], "upsample2x_nhwc[add]", "conv3x3_head1x1_nhwc"],
    "unfused": lambda stem: [STEM_MAP[stem], "upsample2x_nhwc[add]", "conv3x3_nhwc[relu_out]", "gemm"],
}


@pytest.fixture
def calls(monkeypatch):
    log = []

    def wrap(name):
        fn = getattr(ops, name)

        def recorded(*a, **k):
            flags = [f for f in FLAGS if k.get(f) is not None and k.get(f) is not False]
            log.append(name + (f"[{','.join(flags)}]" if flags else ""))
            return fn(*a, **k)
        return recorded
    for name in RECORDED:
        monkeypatch.setattr(ops, name, wrap(name))
    return log


def make_head(cls, num_channels, head_type, BT, gh, gw):
    torch.manual_seed(0)
    net = SimpleNamespace(enc_embed_dim=64, dec_embed_dim=64, dec_depth=12)
    head = dpt.PixelwiseTaskWithDPT(net, num_channels, head_type).to("cuda").eval().requires_grad_(False)
    head.compute_dtype, head.split = CLASSES[cls]
    tokens = [torch.randn(BT, gh * gw, 64, device="cuda") for _ in range(net.dec_depth + 1)]
    frames = torch.rand(BT, 3, 16 * gh, 16 * gw, device="cuda")
    return head, tokens, frames


@pytest.mark.parametrize("cls,BT,gh,gw,route,trunk_packed", [
    ("split", 1, 2, 2, "split_packed_dot", False),
    ("split", 4, 16, 16, "split_packed_dot", True),       # the smallest batch of 16 x 16 grids past the 224-tile threshold
    ("f16", 1, 2, 2, "fused16", False),
    ("f32", 1, 2, 2, "unfused", False),
])
def test_pts3d_route_runs_its_sequence(calls, cls, BT, gh, gw, route, trunk_packed):
    head, tokens, _ = make_head(cls, 3, "regression", BT, gh, gw)
    h = head.dpt.head
    assert dpt.pts3d_route(head.operand_class, BT, gh, gw, h[0].in_channels, h[0].out_channels, h[2].out_channels) == (route, trunk_packed)
    out = head.forward_pts3d_raw(tokens, gh, gw)
    torch.cuda.synchronize()
    tail = ["upsample2x_nhwc[packed]" if trunk_packed else "upsample2x_nhwc", "conv3x3_nhwc"] + PTS3D_TAIL[route]
    assert calls[-len(tail):] == tail, calls[-len(tail) - 2:]
    assert tuple(out.shape) == (BT, 3, 16 * gh, 16 * gw) and out.dtype == head.compute_dtype
    assert bool(torch.isfinite(out).all())


def test_packed_trunk_map_gives_the_plain_map_s_bits_in_a_ragged_last_tile():
    """BT = 47 frames of 19 x 1 tokens: head[0] sees 57 152 pixels = 223.25 tiles of 256, the smallest count that conv3x3_route (csrc/routes.h)
    sends to the 256 x 128 tile kernel, so pts3d_route packs the trunk map there; the packed and the plain input must give the same bits."""
    assert dpt.pts3d_route("split", 47, 19, 1, 256, 128, 128) == ("split_packed_dot", True)
    assert dpt.pts3d_route("split", 46, 19, 1, 256, 128, 128) == ("split_packed_dot", False)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(47, 76, 4, 256, generator=g).cuda()
    w = ops.pack_conv3x3_weight((torch.randn(128, 256, 3, 3, generator=g) / 48).cuda(), "split")
    b = torch.randn(128, generator=g).cuda()
    plain = ops.conv3x3_nhwc(ops.upsample2x_nhwc(x), w, b)
    packed = ops.conv3x3_nhwc(ops.upsample2x_nhwc(x, packed=True), w, b)
    assert plain.shape[0] * plain.shape[1] * plain.shape[2] == 57152
    assert torch.equal(plain.view(torch.int32), packed.view(torch.int32))


@pytest.mark.parametrize("cls,gh,gw,route,stem,forced", [
    ("split", 2, 2, "split_stream_stem", "stream", False),
    ("split", 3, 3, "split_stem_up", "split7", False),
    ("split", 2, 2, "split_up_packed", "split7", True),
    ("f16", 2, 2, "fused16", "window16", False),
    ("f32", 2, 2, "unfused", "im2col_f32", False),
])
def test_gs_route_runs_its_sequence(calls, monkeypatch, cls, gh, gw, route, stem, forced):
    head, tokens, frames = make_head(cls, 83, "gs_params", 1, gh, gw)
    d = head.dpt
    named = dpt.gs_route(head.operand_class, gh, gw, 16 * gh, 16 * gw, 83, d.head[0].in_channels, d.input_merger[0].out_channels, d.head[0].out_channels)
    if forced:
        assert named[0] != route
        monkeypatch.setattr(dpt, "gs_route", lambda *a, **k: (route, stem))
    else:
        assert named == (route, stem)
    out = head.forward_gs(tokens, frames, gh, gw)
    torch.cuda.synchronize()
    tail = ["upsample2x_nhwc"] + GS_TAIL[route](stem)       # the trunk ends with a plain bilinear pass in every class
    assert calls[-len(tail):] == tail, calls[-len(tail) - 2:]
    assert tuple(out.shape) == (1, 83, 16 * gh, 16 * gw) and out.dtype == head.compute_dtype
    assert bool(torch.isfinite(out).all())
