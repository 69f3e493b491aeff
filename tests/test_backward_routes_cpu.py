"""The route table of the linear / 3x3-convolution backward (vicasplat_amd/backward_routes.py), no GPU and no HIP library.

  - every leaf of the table is the route of at least one case of tests/backward_route_cases.py, and every case of
    tests/test_backward_routes_gpu.py takes the route its id names;
  - over a sweep of shapes, the (ksplit, pad) of every route satisfies what the entry point it launches checks;
  - PINNED: shape -> (route, ksplit, pad) as recorded from the launches of the commit BEFORE the routes were named (its four backward
    functions run on storage-less tensors with the library calls recorded), for the shapes of the existing GPU parametrisations and for
    every linear / convolution layer of the two full-size training steps (their shapes and flags logged from one real step each).  A slice
    count is a summation order: a changed number here is a change of the bits of dW.
"""
import itertools

import pytest

import backward_route_cases as C
from vicasplat_amd.backward_routes import bordered_taps, conv3x3_backward_route, linear_backward_route, wgrad_ksplit, wgrad_tn_skinny_ksplit

LEAVES = {        # the table of vicasplat_amd/backward_routes.py
    ("16", "linear"): dict(dx={"nt"}, wgrad={"tn256", "tn_skinny", "transposed", None}, db={"colsum", "colsum_padded", "on_transpose"}),
    ("16", "conv"): dict(dx={"conv"}, wgrad={"tn", "tn_grouped", "transposed"}, db={"colsum", "on_transpose"}),
    ("split", "linear"): dict(dx={"pack_t", "padded"}, dgelu={"epilogue", "pass"}, wgrad={"atn256", "transposed", None}, db={"on_transpose", "colsum"}),
    ("split", "conv"): dict(dx={"conv"}, wgrad={"atn256", "stream", "transposed"}, db={"on_transpose", "stream"}),
}
GPU_CASES = [("16", "linear", C.LINEAR16), ("16", "conv", C.CONV16), ("split", "linear", C.LINEAR_SPLIT), ("split", "conv", C.CONV_SPLIT)]


def _route(cls, kind, case):
    return (C.linear_route if kind == "linear" else C.conv_route)(cls, case[1], case[2])


def test_every_gpu_case_takes_the_route_its_id_names_and_every_leaf_has_a_case():
    for group, kind, cases in GPU_CASES:
        seen = {part: set() for part in LEAVES[group, kind]}
        for case in cases:
            for cls in (("f16", "bf16") if group == "16" else ("split",)):
                r = _route(cls, kind, case)
                assert C.route_id(r) == case[0], (case, r)
                for part in seen:
                    seen[part].add(getattr(r, part))
        for part, leaves in LEAVES[group, kind].items():
            assert seen[part] - {None} == leaves - {None} and (None in leaves) <= (None in seen[part]), (group, kind, part, seen[part])
    # the shapes are the smallest of their kind: the 2^20-row cases sit ON the threshold of `tn_skinny`, one row less leaves the route
    assert linear_backward_route("f16", (1 << 20) - 1, 8, 64).wgrad == "transposed" and linear_backward_route("f16", 1 << 20, 8, 64).wgrad == "tn_skinny"
    # the one-slice arm of the 16-bit `transposed` convolution: whole 256-tiles always fill `tn`, so only a strided x or dy reaches it
    case = [c for c in C.CONV16 if c[2].get("strided_dy")][0]
    assert C.conv_route("f16", case[1], case[2])[2:5] == ("transposed", 1, 128) and C.conv_route("f16", case[1], {}).wgrad == "tn"


SWEEP_NK = (3, 8, 64, 83, 96, 128, 192, 256, 768, 1024, 3072, 4096)
CONV_SHAPES = [(2, 16, 16, 64, 128), (1, 37, 21, 128, 256), (3, 64, 64, 256, 256), (2, 13, 7, 256, 256), (1, 5, 100, 256, 512), (5, 8, 8, 512, 256),
               (2, 20, 12, 256, 128), (1, 9, 33, 192, 256), (2, 11, 19, 128, 128), (1, 30, 8, 128, 256), (3, 6, 6, 64, 256),      # test_ops_gpu
               (1, 8, 8, 768, 256), (2, 32, 32, 128, 128), (1, 16, 16, 256, 512), (2, 37, 21, 256, 256), (5, 7, 50, 512, 256)]    # test_split_bwd_gpu


def _check_contract(r, rows, cols, red, split):
    """What the entry point behind r.wgrad checks of (ksplit, pad); rows x cols = the shape of dW per tap, red = the unpadded reduction."""
    ks, pad = r.ksplit, r.pad
    if r.wgrad in ("tn256", "tn_skinny", "tn", "tn_grouped"):        # vs_gemm_wgrad_tn / vs_conv3x3_wgrad_tn pad the last slice themselves
        assert 1 <= ks <= 65535 and pad == red
    elif r.wgrad == "atn256":                                           # vs_gemm_wgrad_split_atn / vs_conv3x3_wgrad_split_atn
        assert ks >= 1 and pad % (64 * ks) == 0 and red <= pad
    elif r.wgrad == "transposed":                                       # vs_gemm_wgrad (launch_wgrad)
        assert red <= pad
        if split:                                                       # gemm_wgrad_split: K % (64 * ksplit); never whole 256-tiles here
            assert not (rows % 256 == 0 and cols % 256 == 0) and ks >= 2 and pad % (64 * ks) == 0
        elif rows % 256 == 0 and cols % 256 == 0:                       # 256-tiles: an even number of 64-wide K tiles per slice
            assert ks >= 1 and pad % (128 * ks) == 0
        else:                                                           # 128-tiles: at least two slices of whole 64-wide K tiles
            assert ks >= 2 and pad % (64 * ks) == 0
    else:
        assert r.wgrad in (None, "stream") and ks == 0


def test_ksplit_and_pad_satisfy_the_entry_points_over_a_sweep():
    for M in itertools.chain(range(1, 5001), (1 << 20, (1 << 20) + 1)):
        for N, K in itertools.product(SWEEP_NK, SWEEP_NK):
            for cls in ("f16", "split"):
                _check_contract(linear_backward_route(cls, M, N, K), N, K, M, cls == "split")
            if M % 97 == 0 or M >= 1 << 20:      # rows too narrow or misaligned for the reduction-major kernel: the transposed route, whatever the shape
                _check_contract(linear_backward_route("bf16", M, N, K, dy_ld=N + 1), N, K, M, False)
    for (N, H, W, Cin, Cout), cls, contiguous in itertools.product(CONV_SHAPES + [c[1] for c in C.CONV16 + C.CONV_SPLIT], ("f16", "split"), (True, False)):
        r = conv3x3_backward_route(cls, N, H, W, Cin, Cout, contiguous=contiguous)
        bordered = r.wgrad == "transposed"
        _check_contract(r, Cin, Cout, N * (H + 2) * (W + 2) if bordered else N * H * W, cls == "split")


def test_the_slice_rule_is_one_rule():
    """wgrad_ksplit is the only slice rule: `divide` only ever lowers its count, to a divisor of the padded reduction, never below the floor;
    the skinny rule is the other name."""
    for rows, cols, red, taps in [(768, 768, 640, 1), (1024, 4096, 2176, 1), (192, 64, 128, 1), (83, 256, 5120, 1), (256, 256, 17408, 1), (768, 768, 17408, 1)]:
        ks, unit = wgrad_ksplit(rows, cols, red, taps)
        kd, _ = wgrad_ksplit(rows, cols, red, taps, divide=True)
        floor = 1 if rows % 256 == 0 and cols % 256 == 0 else 2
        assert floor <= kd <= ks and (red % (64 * kd) == 0 or kd == floor) and unit == (128 if floor == 1 else 64) * ks
        assert all(red % (64 * k) != 0 for k in range(kd + 1, ks + 1))
    assert [wgrad_tn_skinny_ksplit(m) for m in (1, 1023, 1024, 1 << 20, 1 << 24)] == [1, 1, 2, 256, 256]
    shifts, halo = bordered_taps(16, 8)
    assert shifts == [-19, -18, -17, -1, 0, 1, 17, 18, 19] and halo == 24


# (class, shape, route arguments other than the defaults, route id, ksplit, pad): recorded from the commit before the routes were named
PINNED_LINEAR = [
    # test_ops_gpu.test_linear_backward_matches_autograd
    ("f16", (514, 768, 768), {}, "nt-tn256-colsum", 1, 514),
    ("f16", (16448, 1024, 1024), {}, "nt-tn256-colsum", 16, 16448),
    ("f16", (100, 192, 64), {}, "nt-transposed-on_transpose", 2, 128),
    ("f16", (257, 3072, 768), {}, "nt-tn256-colsum", 1, 257),
    # test_split_bwd_gpu.test_linear_backward_split_matches_float64
    ("split", (514, 768, 768), {}, "padded-atn256-on_transpose", 1, 640),
    ("split", (16448, 1024, 1024), {}, "padded-atn256-on_transpose", 16, 17408),
    ("split", (100, 192, 64), {}, "padded-transposed-on_transpose", 2, 128),
    ("split", (257, 3072, 768), {}, "padded-atn256-on_transpose", 1, 384),
    ("split", (300, 8, 128), {}, "padded-transposed-on_transpose", 2, 384),
    ("split", (5000, 83, 256), {}, "padded-transposed-on_transpose", 10, 5120),
    ("split", (2056, 1024, 4096), {}, "padded-atn256-on_transpose", 2, 2176),
    # ---- the 8-scene split-class training step (8 views of 256 x 256: 64 frames of 257 tokens), in the order of its backward ----
    ("split", (4194304, 256, 256), dict(need_dx=False, scale_exp_known=True), "none-atn256-on_transpose", 256, 4194304),   # Gaussian head: 7x7 stem as im2col GEMM
    ("split", (1048576, 256, 256), dict(scale_exp_known=True), "pack_t-atn256-on_transpose", 256, 1048576),      # refinenet1.out_conv (1x1 at 128 x 128), both heads
    ("split", (262144, 256, 256), dict(scale_exp_known=True), "pack_t-atn256-on_transpose", 256, 262144),        # refinenet2.out_conv (64 x 64)
    ("split", (65536, 256, 256), dict(scale_exp_known=True), "pack_t-atn256-on_transpose", 128, 65536),          # refinenet3.out_conv (32 x 32)
    ("split", (16384, 256, 256), dict(scale_exp_known=True), "pack_t-atn256-on_transpose", 32, 16384),           # refinenet4.out_conv (16 x 16)
    ("split", (16384, 768, 768), dict(scale_exp_known=True), "pack_t-atn256-on_transpose", 16, 16384),           # act_postprocess[3] 1x1 768 -> 768
    ("split", (16384, 384, 768), dict(scale_exp_known=True), "pack_t-transposed-on_transpose", 32, 16384),       # act_postprocess[2] 1x1 768 -> 384
    ("split", (16384, 768, 192), dict(scale_exp_known=True), "pack_t-transposed-on_transpose", 32, 16384),       # act_postprocess[1] ConvTranspose k2 as a GEMM
    ("split", (16384, 192, 768), dict(scale_exp_known=True), "pack_t-transposed-on_transpose", 32, 16384),       # act_postprocess[1] 1x1 768 -> 192
    ("split", (16384, 1536, 96), dict(scale_exp_known=True), "pack_t-transposed-on_transpose", 32, 16384),       # act_postprocess[0] ConvTranspose k4 as a GEMM
    ("split", (16384, 96, 1024), dict(scale_exp_known=True), "padded-transposed-on_transpose", 32, 16384),       # act_postprocess[0] 1x1 1024 -> 96
    ("split", (16448, 768, 3072), dict(scale_exp_known=True, dgelu=True), "pack_t-epilogue-atn256-on_transpose", 4, 17408),      # dec_blocks.mlp.fc2
    ("split", (16448, 3072, 768), dict(scale_exp_known=True), "pack_t-atn256-on_transpose", 4, 17408),           # dec_blocks.mlp.fc1
    ("split", (16448, 768, 768), dict(scale_exp_known=True), "pack_t-atn256-on_transpose", 17, 17408),           # dec_blocks.cross_attn.proj
    ("split", (16448, 2304, 768), dict(scale_exp_known=True), "pack_t-atn256-on_transpose", 8, 17408),           # dec_blocks.cross_attn.proj{q,k,v} stacked
    ("split", (64, 4608, 768), dict(scale_exp_known=True), "pack_t-atn256-on_transpose", 1, 128),                # dec_blocks.modulation2.proj (one row per frame)
    ("split", (16512, 768, 768), dict(scale_exp_known=True), "pack_t-atn256-on_transpose", 17, 17408),           # dec_blocks.attn.proj (258 rows per frame)
    ("split", (16512, 2304, 768), dict(scale_exp_known=True), "pack_t-atn256-on_transpose", 8, 17408),           # dec_blocks.attn.qkv
    ("split", (64, 2304, 768), dict(scale_exp_known=True), "pack_t-atn256-on_transpose", 1, 128),                # dec_blocks.modulation1.proj
    ("split", (64, 768, 3072), dict(scale_exp_known=True), "pack_t-atn256-on_transpose", 1, 128),                # dec_blocks.mlp_cam.fc2
    ("split", (64, 3072, 768), dict(scale_exp_known=True), "pack_t-atn256-on_transpose", 1, 128),                # dec_blocks.mlp_cam.fc1
    ("split", (16448, 768, 1024), dict(scale_exp_known=True), "pack_t-atn256-on_transpose", 17, 17408),          # decoder_embed
    ("split", (16448, 1024, 4096), dict(scale_exp_known=True, dgelu=True), "pack_t-epilogue-atn256-on_transpose", 4, 17408),     # enc_blocks.mlp.fc2
    ("split", (16448, 4096, 1024), dict(scale_exp_known=True), "pack_t-atn256-on_transpose", 4, 17408),          # enc_blocks.mlp.fc1
    ("split", (16448, 1024, 1024), dict(scale_exp_known=True), "pack_t-atn256-on_transpose", 16, 17408),         # enc_blocks.attn.proj
    ("split", (16448, 3072, 1024), dict(scale_exp_known=True), "pack_t-atn256-on_transpose", 4, 17408),          # enc_blocks.attn.qkv
    ("split", (64, 1024, 32), dict(need_dx=False, dy_ld=263168, scale_exp_known=True), "none-transposed-on_transpose", 2, 128),      # intrinsic_encoder (K = 9 padded to 32)
    ("split", (16384, 1024, 768), dict(need_dx=False, scale_exp_known=True), "none-atn256-on_transpose", 16, 16384),                 # patch_embed as a GEMM
    # ---- the 24-scene f16 training step (192 frames), the same layers ----
    ("f16", (12582912, 256, 256), dict(need_dx=False), "none-tn256-colsum", 256, 12582912),
    ("f16", (3145728, 256, 256), {}, "nt-tn256-colsum", 256, 3145728),
    ("f16", (786432, 256, 256), {}, "nt-tn256-colsum", 256, 786432),
    ("f16", (196608, 256, 256), {}, "nt-tn256-colsum", 256, 196608),
    ("f16", (49152, 256, 256), {}, "nt-tn256-colsum", 96, 49152),
    ("f16", (49152, 768, 768), {}, "nt-tn256-colsum", 28, 49152),
    ("f16", (49152, 384, 768), {}, "nt-transposed-on_transpose", 42, 51072),
    ("f16", (49152, 768, 192), {}, "nt-transposed-on_transpose", 64, 49152),
    ("f16", (49152, 192, 768), {}, "nt-transposed-on_transpose", 64, 49152),
    ("f16", (49152, 1536, 128), {}, "nt-transposed-on_transpose", 64, 49152),      # (K = 96 padded to 128 in this class)
    ("f16", (49152, 96, 1024), {}, "nt-transposed-on_transpose", 96, 49152),
    ("f16", (49344, 768, 3072), {}, "nt-tn256-colsum", 7, 49344),
    ("f16", (49344, 3072, 768), {}, "nt-tn256-colsum", 7, 49344),
    ("f16", (49344, 768, 768), {}, "nt-tn256-colsum", 28, 49344),
    ("f16", (49344, 2304, 768), {}, "nt-tn256-colsum", 9, 49344),
    ("split", (192, 4608, 768), dict(scale_exp_known=True), "pack_t-atn256-on_transpose", 1, 256),               # (the per-frame linears stay in the split class)
    ("f16", (49536, 768, 768), {}, "nt-tn256-colsum", 28, 49536),
    ("f16", (49536, 2304, 768), {}, "nt-tn256-colsum", 9, 49536),
    ("split", (192, 2304, 768), dict(scale_exp_known=True), "pack_t-atn256-on_transpose", 1, 256),
    ("split", (192, 768, 3072), dict(scale_exp_known=True), "pack_t-atn256-on_transpose", 1, 256),
    ("split", (192, 3072, 768), dict(scale_exp_known=True), "pack_t-atn256-on_transpose", 1, 256),
    ("f16", (49344, 768, 1024), {}, "nt-tn256-colsum", 21, 49344),
    ("f16", (49344, 1024, 4096), {}, "nt-tn256-colsum", 4, 49344),
    ("f16", (49344, 4096, 1024), {}, "nt-tn256-colsum", 4, 49344),
    ("f16", (49344, 1024, 1024), {}, "nt-tn256-colsum", 16, 49344),
    ("f16", (49344, 3072, 1024), {}, "nt-tn256-colsum", 5, 49344),
    ("split", (192, 1024, 32), dict(need_dx=False, dy_ld=263168, scale_exp_known=True), "none-transposed-on_transpose", 2, 256),
    ("f16", (49152, 1024, 768), dict(need_dx=False), "none-tn256-colsum", 21, 49152),
]
PINNED_CONV = [
    # test_ops_gpu.test_conv3x3_backward_matches_autograd
    ("f16", (2, 16, 16, 64, 128), {}, "conv-transposed-on_transpose", 2, 768),
    ("f16", (1, 37, 21, 128, 256), {}, "conv-tn_grouped-colsum", 1, 777),
    ("f16", (3, 64, 64, 256, 256), {}, "conv-tn-colsum", 24, 12288),
    ("f16", (2, 13, 7, 256, 256), {}, "conv-tn-colsum", 1, 182),
    ("f16", (1, 5, 100, 256, 512), {}, "conv-tn-colsum", 1, 500),
    ("f16", (5, 8, 8, 512, 256), {}, "conv-tn-colsum", 1, 320),
    ("f16", (2, 20, 12, 256, 128), {}, "conv-tn-colsum", 1, 480),
    ("f16", (1, 9, 33, 192, 256), {}, "conv-tn-colsum", 1, 297),
    ("f16", (2, 11, 19, 128, 128), {}, "conv-tn_grouped-colsum", 1, 418),
    ("f16", (1, 30, 8, 128, 256), {}, "conv-tn_grouped-colsum", 1, 240),
    ("f16", (3, 6, 6, 64, 256), {}, "conv-tn_grouped-colsum", 1, 108),
    # test_split_bwd_gpu.test_conv3x3_backward_split_matches_float64
    ("split", (2, 16, 16, 64, 128), {}, "conv-transposed-on_transpose", 2, 768),
    ("split", (1, 37, 21, 128, 256), {}, "conv-transposed-on_transpose", 2, 1024),
    ("split", (3, 64, 64, 256, 256), {}, "conv-atn256-on_transpose", 24, 12288),
    ("split", (1, 8, 8, 768, 256), {}, "conv-atn256-on_transpose", 1, 64),
    ("split", (2, 32, 32, 128, 128), {}, "conv-stream-stream", 0, 2048),
    ("split", (1, 16, 16, 256, 512), {}, "conv-atn256-on_transpose", 1, 256),
    ("split", (2, 37, 21, 256, 256), {}, "conv-atn256-on_transpose", 3, 1728),
    ("split", (5, 7, 50, 512, 256), {}, "conv-atn256-on_transpose", 3, 1920),
    # ---- the 8-scene split-class training step (64 frames), in the order of its backward ----
    ("split", (64, 256, 256, 256, 256), dict(need_db=False), "conv-atn256-none", 28, 4195072),       # Gaussian head: head[0] at 256 x 256 (its bias gradient comes with the fused 1x1)
    ("split", (64, 64, 64, 256, 256), {}, "conv-atn256-on_transpose", 28, 263424),                    # refinenet2 residual conv units, both heads
    ("split", (64, 32, 32, 256, 256), {}, "conv-atn256-on_transpose", 28, 66304),                     # refinenet3
    ("split", (64, 16, 16, 256, 256), {}, "conv-atn256-on_transpose", 28, 17920),                     # refinenet4's output scale
    ("split", (64, 8, 8, 256, 256), {}, "conv-atn256-on_transpose", 8, 4096),                         # refinenet4
    ("split", (64, 8, 8, 768, 256), dict(need_db=False), "conv-atn256-none", 8, 4096),                # layer4_rn (no bias)
    ("split", (64, 16, 16, 384, 256), dict(need_db=False), "conv-transposed-none", 14, 21504),        # layer3_rn
    ("split", (64, 32, 32, 192, 256), dict(need_db=False), "conv-stream-none", 0, 65536),             # layer2_rn
    ("split", (64, 64, 64, 96, 256), dict(need_db=False), "conv-transposed-none", 42, 279552),        # layer1_rn
    ("split", (64, 16, 16, 768, 768), {}, "conv-atn256-on_transpose", 3, 16512),                      # act_postprocess[3] stride-2 conv (zero-dilated gradient)
    ("split", (64, 256, 256, 128, 128), {}, "conv-stream-stream", 0, 4194304),                        # pts3d head: head[2] at 256 x 256
    ("split", (64, 128, 128, 256, 128), {}, "conv-stream-stream", 0, 1048576),                        # pts3d head: head[0] at 128 x 128
    # ---- the 24-scene f16 training step (192 frames), the same layers ----
    ("f16", (192, 256, 256, 256, 256), dict(need_db=False), "conv-tn-none", 28, 12582912),
    ("f16", (192, 64, 64, 256, 256), {}, "conv-tn-colsum", 28, 786432),
    ("f16", (192, 32, 32, 256, 256), {}, "conv-tn-colsum", 28, 196608),
    ("f16", (192, 16, 16, 256, 256), {}, "conv-tn-colsum", 28, 49152),
    ("f16", (192, 8, 8, 256, 256), {}, "conv-tn-colsum", 24, 12288),
    ("f16", (192, 8, 8, 768, 256), dict(need_db=False), "conv-tn-none", 9, 12288),
    ("f16", (192, 16, 16, 384, 256), dict(need_db=False), "conv-tn-none", 14, 49152),
    ("f16", (192, 32, 32, 192, 256), dict(need_db=False), "conv-tn-none", 28, 196608),
    ("f16", (192, 64, 64, 96, 256), dict(need_db=False), "conv-transposed-on_transpose", 42, 838656),
    ("f16", (192, 16, 16, 768, 768), {}, "conv-tn-colsum", 3, 49152),
    ("f16", (192, 256, 256, 128, 128), {}, "conv-tn_grouped-colsum", 51, 12582912),
    ("f16", (192, 128, 128, 256, 128), {}, "conv-tn-colsum", 28, 3145728),
]


@pytest.mark.parametrize("route_fn,table", [(linear_backward_route, PINNED_LINEAR), (conv3x3_backward_route, PINNED_CONV)], ids=["linear", "conv3x3"])
def test_pinned_routes(route_fn, table):
    for cls, shape, kw, rid, ksplit, pad in table:
        r = route_fn(cls, *shape, **kw)
        assert (C.route_id(r), r.ksplit, r.pad) == (rid, ksplit, pad), (cls, shape, kw, r)
        if cls == "f16":
            assert route_fn("bf16", *shape, **kw) == r
