"""The PNG encoder on the GPU: vse_png_encode (csrc/png.hip) and the Python surface of vicasplat_amd.misc.image_io against the restatement of
tests/png_ref.py (which tests/test_png_cpu.py pins against PIL, zlib and the host build of csrc/png_deflate.h).  Every comparison is byte
for byte; PIL decodes the GPU's own bytes to the exact pixels."""
import io

import numpy as np
import pytest
import torch

import png_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def _dev():
    return torch.device("cuda:0")


def _pil(data, shape):
    from PIL import Image
    Image.open(io.BytesIO(data)).verify()
    im = Image.open(io.BytesIO(data))
    im.load()
    return np.asarray(im).reshape(shape)


def _as_float(pixels):
    """f32 values whose quantisation is `pixels` for certain: (k + 0.5) / 255."""
    return ((pixels.astype(np.float32) + np.float32(0.5)) / np.float32(255)).astype(np.float32)


def _guarded(images: torch.Tensor, layout, shape, mode, pad):
    """The entry itself with files, lengths and workspace in the middle of sentinel-filled buffers (the files `pad` bytes in, at the bound's
    own stride): [file bytes] after the bands around all three, and every byte past a file's length, were found untouched."""
    from vicasplat_amd import _lib
    dev = _dev()
    n, h, w, c = shape
    bound = _lib.call("vse_png_bound", dev, h, w, c)
    need = _lib.call("vse_png_workspace_bytes", dev, n, h, w, c)
    assert bound == R.bound(h, w, c)
    out = torch.full((pad + n * bound + 133,), SENTINEL, dtype=torch.uint8, device=dev)
    lengths = torch.full((3 + n + 5,), -77, dtype=torch.int32, device=dev)
    work = torch.full((256 + need + 256,), SENTINEL, dtype=torch.uint8, device=dev)
    assert work.data_ptr() % 16 == 0 and out.data_ptr() % 4 == 0
    _lib.call("vse_png_encode", dev, _lib.ptr(images), layout, n, h, w, c, mode, _lib.ptr(work[256:]), need, _lib.ptr(out[pad:]), bound,
              _lib.ptr(lengths[3:]))
    out, lengths, work = out.cpu().numpy(), lengths.cpu().numpy(), work.cpu().numpy()
    assert (out[:pad] == SENTINEL).all() and (out[pad + n * bound:] == SENTINEL).all(), "bytes written outside the output"
    assert (lengths[:3] == -77).all() and (lengths[3 + n:] == -77).all(), "lengths written outside [n]"
    assert (work[:256] == SENTINEL).all() and (work[256 + need:] == SENTINEL).all(), "the workspace was overrun"
    files = []
    for i in range(n):
        size = int(lengths[3 + i])
        assert 0 < size <= bound
        row = out[pad + i * bound:pad + (i + 1) * bound]
        assert (row[size:] == SENTINEL).all(), "bytes written past the file's length"
        files.append(row[:size].tobytes())
    return files


def _differing(got: bytes, want: bytes) -> int:
    return sum(a != b for a, b in zip(got, want)) + abs(len(got) - len(want))


@pytest.mark.parametrize("name", list(R.cases()))
def test_every_case_equals_the_restatement_and_decodes_to_its_pixels(name):
    from vicasplat_amd import _lib
    from vicasplat_amd.misc import image_io
    pixels, mode = R.cases()[name]
    want = R.reference_file(name)
    h, w, c = pixels.shape
    dev = _dev()
    hwc = torch.from_numpy(pixels).to(dev)[None]
    chw = hwc.permute(0, 3, 1, 2).contiguous()
    f32 = torch.from_numpy(_as_float(pixels)).to(dev)[None].permute(0, 3, 1, 2).contiguous()
    shifted = torch.empty(f32.numel() + 1, dtype=torch.float32, device=dev)[1:]          # 4 bytes off the allocation's alignment
    shifted.copy_(f32.reshape(-1))
    assert shifted.data_ptr() % 16 == 4
    runs = {"u8 hwc, aligned out": _guarded(hwc, _lib.VSP_LAYOUT_U8_HWC, (1, h, w, c), mode, 64),
            "u8 chw, misaligned out": _guarded(chw, _lib.VSP_LAYOUT_U8_CHW, (1, h, w, c), mode, 67),
            "f32 chw, misaligned in": _guarded(shifted, _lib.VSP_LAYOUT_F32_CHW, (1, h, w, c), mode, 64),
            "f32 through encode_png_batch": image_io.encode_png_batch(f32, filter=mode),
            "u8 through encode_png_batch": image_io.encode_png_batch(hwc, filter=mode)}
    for what, (got,) in runs.items():
        differing = _differing(got, want)
        print(f"{name}, {what}: {len(got)} bytes, {differing} differing")
        assert differing == 0, (name, what)
    assert np.array_equal(_pil(runs["u8 hwc, aligned out"][0], pixels.shape), pixels)


def test_float_quantisation_at_its_edges():
    from vicasplat_amd.misc import image_io
    x = R.float_probes()
    image = torch.from_numpy(x).to(_dev()).reshape(1, 1, 1, -1)
    got, = image_io.encode_png_batch(image, filter="none")
    want = R.quantise(x).reshape(1, -1, 1)
    assert _differing(got, R.encode(want, 0)) == 0
    assert np.array_equal(_pil(got, want.shape), want)                                     # NaN -> 0, -0 -> 0, +inf -> 255, -inf -> 0 among them
    rgb = image.expand(1, 3, 1, -1).reshape(1, 3, 1, -1)
    assert np.array_equal(image_io.prep_image(rgb[0]).cpu().numpy(), np.repeat(want, 3, axis=2))


@pytest.mark.parametrize("batch", list(R.batches()))
def test_mixed_batches_equal_the_files_alone(batch):
    from vicasplat_amd import _lib
    from vicasplat_amd.misc import image_io
    pixels = R.batches()[batch]
    n, h, w, c = pixels.shape
    hwc = torch.from_numpy(pixels).to(_dev())
    want = [R.encode(p, R.ADAPTIVE) for p in pixels]
    got = image_io.encode_png_batch(hwc)
    print(f"{batch}: {[len(g) for g in got]} bytes, {sum(_differing(g, w_) for g, w_ in zip(got, want))} differing")
    assert got == want
    assert image_io.encode_png_batch(hwc) == got                                                   # two runs are bit-equal
    for i in range(n):                                                                             # a file alone equals the file in the batch
        assert image_io.encode_png_batch(hwc[i:i + 1]) == [got[i]], i
    f32 = torch.from_numpy(_as_float(pixels)).to(_dev()).permute(0, 3, 1, 2).contiguous()
    assert image_io.encode_png_batch(list(f32)) == got                                             # a list of frames, floats
    for pad in (64, 67):
        assert _guarded(hwc, _lib.VSP_LAYOUT_U8_HWC, (n, h, w, c), R.ADAPTIVE, pad) == want
    for p, g in zip(pixels, got):
        assert np.array_equal(_pil(g, p.shape), p)


def test_no_host_synchronisation_before_the_length_copy():
    from vicasplat_amd.misc import image_io
    pixels = R.batches()["23x40_rgb"]
    f32 = torch.from_numpy(_as_float(pixels)).to(_dev()).permute(0, 3, 1, 2).contiguous()
    warm = image_io.encode_png_batch(f32)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out, lengths = image_io.encode_png_device(f32)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    sizes = lengths.tolist()
    assert [out[i, :s].cpu().numpy().tobytes() for i, s in enumerate(sizes)] == warm


def test_graph_capture_and_replay_on_other_pixels():
    from vicasplat_amd.misc import image_io
    pixels = R.batches()["23x40_rgb"]
    dev = _dev()
    first = torch.from_numpy(_as_float(pixels)).to(dev).permute(0, 3, 1, 2).contiguous()
    second = first.flip(0).contiguous()
    static = first.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        image_io.encode_png_device(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lengths = image_io.encode_png_device(static)
    static.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    want = [R.encode(p, R.ADAPTIVE) for p in pixels[::-1]]
    assert [out[i, :s].cpu().numpy().tobytes() for i, s in enumerate(lengths.tolist())] == want


def test_save_image_lays_a_batch_side_by_side(tmp_path):
    from vicasplat_amd.misc import image_io
    g = torch.Generator().manual_seed(3)
    x = torch.rand(3, 3, 17, 9, generator=g) * 1.2 - 0.1
    image_io.save_image(x.to(_dev()), tmp_path / "a" / "b" / "batch.png")          # parent directories are made
    want = R.quantise(x.numpy()).transpose(1, 2, 0, 3).reshape(3, 17, 27).transpose(1, 2, 0)          # b c h w -> c h (b w) -> h w c
    assert np.array_equal(_pil((tmp_path / "a" / "b" / "batch.png").read_bytes(), (17, 27, 3)), want)
    assert np.array_equal(image_io.prep_image(x.to(_dev())).cpu().numpy(), want)
    grey = torch.rand(17, 9, generator=g)
    image_io.save_image(grey.to(_dev()), tmp_path / "grey.png")                    # one channel becomes three
    assert np.array_equal(_pil((tmp_path / "grey.png").read_bytes(), (17, 9, 3)), np.repeat(R.quantise(grey.numpy())[:, :, None], 3, axis=2))
    rgba = torch.rand(4, 5, 6, generator=g)
    image_io.save_images(rgba.to(_dev())[None], [tmp_path / "rgba.png"])
    assert np.array_equal(_pil((tmp_path / "rgba.png").read_bytes(), (5, 6, 4)), R.quantise(rgba.numpy()).transpose(1, 2, 0))


def test_save_test_outputs_on_the_tiny_encoder(tmp_path):
    import json
    import os
    from oracle import chain
    from oracle import encoder_ref as er
    from vicasplat_amd import callers
    from vicasplat_amd.misc import image_io
    from vicasplat_amd.misc.utils import vis_depth_map
    from vicasplat_amd.model.decoder import DecoderSplattingCUDACfg, get_decoder
    from vicasplat_amd.model.encoder import default_cfg, get_encoder
    d = _dev()
    shapes = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shapes_tiny.json")))
    m, _ = get_encoder(default_cfg(enc_depth=2, dec_embed_dim=192, dec_num_heads=3))
    m.load_state_dict(er.golden_weights(shapes, seed=0), strict=True)
    m = m.to(d).eval().requires_grad_(False)
    m.set_compute_dtype("split")
    B, V = 2, 2
    image, K = er.synthetic_input(B, V, 256, 0)
    E, Kt, near, far = (torch.tensor(a, dtype=torch.float32, device=d)[None].repeat(B, *[1] * np.ndim(a)) for a in chain.config1_targets(V))
    ctx = dict(image=image.to(d), intrinsics=K.to(d), extrinsics=E, near=near, far=far, index=torch.tensor([[0, 12], [7, 300]]))
    batch = dict(scene=["scene_a", "scene_b"], context=ctx,
                 target=dict(extrinsics=E, intrinsics=Kt, near=near, far=far, index=torch.tensor([[5, 6], [100, 200]])))
    decoder = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", [0.0, 0.0, 0.0], False)).to(d)
    with torch.no_grad():
        outs = m({k: v for k, v in ctx.items() if k != "index"})
        output = decoder.forward(outs["gaussians"], E, Kt, near, far, (256, 256))
    paths = callers.save_test_outputs(batch, outs, output, tmp_path)
    assert len(paths) == 8 and all(p.exists() for p in paths)
    found = sorted(str(p.relative_to(tmp_path)) for p in tmp_path.rglob("*") if p.is_file())
    assert found == sorted([f"scene_a/context/{i:0>6}.png" for i in (0, 12)] + [f"scene_b/context/{i:0>6}.png" for i in (7, 300)] +
                           [f"scene_a/color/{i:0>6}.png" for i in (5, 6)] + [f"scene_b/color/{i:0>6}.png" for i in (100, 200)] +
                           ["scene_a/transforms.json", "scene_b/transforms.json"])
    for b, scene in enumerate(batch["scene"]):
        frames = json.load(open(tmp_path / scene / "transforms.json"))
        assert [f["file_path"] for f in frames] == [f"context/{i:0>6}.png" for i in ctx["index"][b].tolist()]
        assert np.array_equal(np.asarray([f["transform_matrix"] for f in frames], np.float32), outs["gaussian_camera_extrins"][b].cpu().numpy())
        depth = vis_depth_map(output.depth[b])
        for v in range(V):
            got = _pil((tmp_path / scene / f"context/{int(ctx['index'][b, v]):0>6}.png").read_bytes(), (256, 256, 3))
            assert np.array_equal(got, image_io.prep_image(ctx["image"][b, v] * 0.5 + 0.5).cpu().numpy())
            got = _pil((tmp_path / scene / f"color/{int(batch['target']['index'][b, v]):0>6}.png").read_bytes(), (256, 520, 3))
            assert np.array_equal(got[:, :256], image_io.prep_image(output.color[b, v]).cpu().numpy()) and (got[:, 256:264] == 255).all()
            assert np.array_equal(got[:, 264:], image_io.prep_image(depth[v]).cpu().numpy())
    del outs, output, decoder, m, batch, ctx
    import gc
    gc.collect()
    torch.cuda.empty_cache()
