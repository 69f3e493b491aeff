"""Route tables of the DPT heads (vicasplat_amd/model/encoder/heads/dpt.py: pts3d_route, gs_route), no GPU and no HIP library.

Every expected value below was derived by hand from the `if` chains of forward_pts3d_raw / forward_gs as they stood before the route
functions existed (commit f87e734), not from the functions under test:
  pts3d  pk = split and head[0].out == 128 and head[0].in in (64, 128, 256);  trunk packed = pk and BT * 64 * gh * gw >= 224 * 256 (= 57 344);
         split and pixels % 256 == 0 and head[0].out == 128 and head[2].out == 128 -> packed bilinear + split dot head;
         else compute dtype != f32 (the split class computes in f32) and pixels % 256 == 0 and head[0].out == 128 -> 16-bit dot head;
         else conv3x3 + GEMM.
  gs     fuse = split and num_channels <= 96 and pixels % 256 == 0 and head[0].out == 256 and trunk channels in (32, 64, 128, 256);
         split and stem Cout % 256 == 0: [fuse and trunk channels == stem Cout and (16gh, 16gw) == (H, W): W % 32 == 0 and stem Cout == 256 ->
         streaming stem, else stem with the upsample-add epilogue]; else the split window-GEMM stem as a map;
         elif f32 compute dtype (f32 class, and the split class with another stem Cout): im2col stem;  else 16-bit window GEMM;
         fuse -> packed upsample-add + split head;  else 16-bit and num_channels <= 96 and head[0].out == 256 and trunk channels in
         (64, 128, 256, 512) -> 16-bit head;  else conv3x3 + GEMM.
The head's map has BT * 16gh * 16gw = 256 * BT * gh * gw pixels, so `pixels % 256 == 0` holds for every integer grid (BT = 1, gh = 1,
gw = 3 gives 768): a case that fails it does not exist, and none is listed.
"""
import pytest

from vicasplat_amd.model.encoder.heads.dpt import PACKED_CONV_MIN_PIXELS, gs_route, pts3d_route

SHAPES = [  # (BT, gh, gw, trunk packed in the split class): 64 * BT * gh * gw against 57 344
    (24 * 8, 16, 16, True),   # 3 145 728
    (1, 16, 16, False),       # 16 384
    (4, 16, 16, True),        # 65 536
    (3, 16, 16, False),       # 49 152
    (1, 1, 3, False),         # 192; 768 upsampled pixels
]


def test_threshold_is_224_tiles_of_256_pixels():
    assert PACKED_CONV_MIN_PIXELS == 224 * 256 == 57344


@pytest.mark.parametrize("BT,gh,gw,packed", SHAPES)
def test_pts3d_routes(BT, gh, gw, packed):
    stock = dict(c_trunk=256, c_h0=128, c_h2=128)
    assert pts3d_route("split", BT, gh, gw, **stock) == ("split_packed_dot", packed)
    assert pts3d_route("f16", BT, gh, gw, **stock) == ("fused16", False)
    assert pts3d_route("bf16", BT, gh, gw, **stock) == ("fused16", False)
    assert pts3d_route("f32", BT, gh, gw, **stock) == ("unfused", False)
    for cls in ("split", "f16", "bf16", "f32"):      # head[0].out_channels != 128: two kernels in every class, and pk is false
        assert pts3d_route(cls, BT, gh, gw, c_trunk=256, c_h0=64, c_h2=64) == ("unfused", False)
    # a split head whose second convolution is not 128 wide: two kernels (f32 compute dtype); pk does not look at head[2]
    assert pts3d_route("split", BT, gh, gw, c_trunk=256, c_h0=128, c_h2=64) == ("unfused", packed)
    # a trunk width the 256 x 128 tile kernel does not take (pk false): the route stays, the trunk writes plain f32
    assert pts3d_route("split", BT, gh, gw, c_trunk=32, c_h0=128, c_h2=128) == ("split_packed_dot", False)


GS = dict(gh=16, gw=16, H=256, W=256, num_channels=83, c_trunk=256, c_stem=256, c_h0=256)


@pytest.mark.parametrize("cls,change,expected", [
    ("split", {}, ("split_stream_stem", "stream")),                                        # W = 256
    ("split", dict(gh=2, gw=2, H=32, W=32), ("split_stream_stem", "stream")),              # one 32-pixel strip
    ("split", dict(gh=3, gw=3, H=48, W=48), ("split_stem_up", "split7")),                  # W % 32 != 0
    ("split", dict(c_trunk=128), ("split_up_packed", "split7")),                           # trunk channels != stem channels
    ("split", dict(H=128, W=128), ("split_up_packed", "split7")),                          # frames that are not 16gh x 16gw
    ("split", dict(num_channels=97), ("unfused", "split7")),
    ("split", dict(c_stem=128), ("split_up_packed", "im2col_f32")),                        # stem Cout % 256 != 0: the im2col stem
    ("split", dict(c_stem=128, num_channels=97), ("unfused", "im2col_f32")),
    ("split", dict(c_h0=128), ("unfused", "split7")),
    ("split", dict(c_trunk=512, c_stem=512), ("unfused", "split7")),                       # 512 f32 channels: outside (32, 64, 128, 256)
    ("f16", {}, ("fused16", "window16")),
    ("bf16", {}, ("fused16", "window16")),
    ("f16", dict(c_trunk=512), ("fused16", "window16")),                                   # 512 16-bit channels: inside (64, 128, 256, 512)
    ("f16", dict(c_trunk=32), ("unfused", "window16")),
    ("f16", dict(num_channels=97), ("unfused", "window16")),
    ("f16", dict(gh=3, gw=3, H=48, W=48), ("fused16", "window16")),
    ("f32", {}, ("unfused", "im2col_f32")),
    ("f32", dict(num_channels=97), ("unfused", "im2col_f32")),
])
def test_gs_routes(cls, change, expected):
    assert gs_route(cls, **{**GS, **change}) == expected


def test_route_functions_need_no_library(monkeypatch):
    from vicasplat_amd import _lib

    def no_library():
        raise AssertionError("a route function loaded the HIP library")
    monkeypatch.setattr(_lib, "_load", no_library)
    monkeypatch.setattr(_lib, "_lib", None)
    assert gs_route("split", **GS)[0] == "split_stream_stem"
    assert pts3d_route("split", 4, 16, 16, 256, 128, 128) == ("split_packed_dot", True)
