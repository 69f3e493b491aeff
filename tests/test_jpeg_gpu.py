"""The JPEG decoder on the GPU: vsj_decode (csrc/jpeg.hip) and the Python surface of vicasplat_amd.dataset against PIL's pixels as
tests/golden/jpeg_cases.npz holds them (written by tests/golden/gen_jpeg_cases.py; tests/test_jpeg_cpu.py pins the fixture, the yardstick
of tests/jpeg_ref.py and the host build of the decoder on the CPU).  Every comparison is byte for byte.
"""
import numpy as np
import pytest
import torch

import data_shims_ref as S
import jpeg_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def _dev():
    return torch.device("cuda:0")


def _streams(names):
    return [R.fixture()[n][0] for n in names]


def _pixels(names):
    return np.stack([R.fixture()[n][1] for n in names])


def _differing(got: torch.Tensor, want: np.ndarray) -> int:
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape, (tuple(got.shape), want.shape)
    return int((got.cpu().numpy() != want).sum())


def _guarded(datas, pad: int):
    """The entry itself with pixels, status and workspace in the middle of sentinel-filled buffers (the pixels `pad` bytes in): (pixels, status)
    as numpy, after the bands around all three were found untouched."""
    from vicasplat_amd import _lib
    from vicasplat_amd.dataset import pack_jpeg_batch
    dev = _dev()
    pk = pack_jpeg_batch(datas)
    packed = torch.from_numpy(pk.buffer).to(dev)
    count = pk.n * pk.h * pk.w * 3
    need = _lib.call("vsj_workspace_bytes", dev, pk.blocks, pk.segments)
    pix = torch.full((pad + count + 133,), SENTINEL, dtype=torch.uint8, device=dev)
    stat = torch.full((3 + pk.n + 5,), -77, dtype=torch.int32, device=dev)
    work = torch.full((256 + need + 256,), SENTINEL, dtype=torch.uint8, device=dev)
    assert work.data_ptr() % 16 == 0
    _lib.call("vsj_decode", dev, _lib.ptr(packed), packed.numel(), pk.n, pk.h, pk.w, pk.segments, pk.max_frame_segments, pk.n_quant, pk.n_huff,
              pk.blocks, _lib.ptr(work[256:]), need, _lib.ptr(pix[pad:]), _lib.ptr(stat[3:]))
    pix, stat, work = pix.cpu().numpy(), stat.cpu().numpy(), work.cpu().numpy()
    assert (pix[:pad] == SENTINEL).all() and (pix[pad + count:] == SENTINEL).all(), "pixels written outside the output"
    assert (stat[:3] == -77).all() and (stat[3 + pk.n:] == -77).all(), "status written outside [N]"
    assert (work[:256] == SENTINEL).all() and (work[256 + need:] == SENTINEL).all(), "the workspace was overrun"
    return pix[pad:pad + count].reshape(pk.n, pk.h, pk.w, 3), stat[3:3 + pk.n]


@pytest.mark.parametrize("name", list(R.CASES))
def test_every_case_alone_equals_pil(name):
    from vicasplat_amd.dataset import decode_jpeg_batch
    data, rgb = R.fixture()[name]
    got, status = decode_jpeg_batch([data], device=_dev(), return_status=True)
    differing = _differing(got, rgb[None])
    print(f"{name}: {differing} differing bytes, status {status.tolist()}")
    assert differing == 0 and status.dtype == torch.int32 and status.tolist() == [0]
    again = decode_jpeg_batch([torch.frombuffer(bytearray(data), dtype=torch.uint8)], device=_dev())      # a tensor, as the chunks hold frames
    assert torch.equal(again, got)
    # the entry between guard bands, the pixels at a 4-byte aligned and at a misaligned address (the dword and the byte stores)
    for pad in (64, 67):
        pix, stat = _guarded([data], pad)
        assert np.array_equal(pix[0], rgb) and stat.tolist() == [0], (name, pad)


@pytest.mark.parametrize("batch", list(R.BATCHES))
def test_mixed_batches_equal_pil_and_the_frames_alone(batch):
    from vicasplat_amd.dataset import decode_jpeg_batch
    names = R.BATCHES[batch]
    got, status = decode_jpeg_batch(_streams(names), device=_dev(), return_status=True)
    differing = _differing(got, _pixels(names))
    print(f"{batch}: {differing} differing bytes")
    assert differing == 0 and status.tolist() == [0] * 5
    assert torch.equal(decode_jpeg_batch(_streams(names), device=_dev()), got)          # two runs are bit-equal
    for i, n in enumerate(names):                                                       # a frame alone equals the frame inside the batch
        assert torch.equal(decode_jpeg_batch(_streams([n]), device=_dev())[0], got[i]), n
    for pad in (64, 67):
        pix, stat = _guarded(_streams(names), pad)
        assert np.array_equal(pix, _pixels(names)) and not stat.any()


def test_convert_images_is_the_decode_over_255():
    from vicasplat_amd.dataset import convert_images
    for names in list(R.BATCHES.values()) + [("13x11_gray",), ("1x1",)]:
        got = convert_images(_streams(names), device=_dev())
        want = np.moveaxis(_pixels(names), -1, 1).astype(np.float32) / np.float32(255)
        assert got.dtype == torch.float32 and got.is_contiguous() and np.array_equal(got.cpu().numpy(), want), names


@pytest.mark.parametrize("batch", list(R.BATCHES))
def test_the_crop_shim_reads_the_decoders_buffer(batch):
    """decode -> apply_crop_shim_to_views on the 45 x 80 and 80 x 45 frames -> (32, 32): the shim's yardstick applied to PIL's pixels."""
    from vicasplat_amd.dataset import apply_crop_shim_to_views, decode_jpeg_batch
    from vicasplat_amd.dataset.shims import crop_shim
    names = R.BATCHES[batch]
    frames = decode_jpeg_batch(_streams(names), device=_dev()).permute(0, 3, 1, 2)
    assert crop_shim._frames(frames)[1] == crop_shim.LAYOUT_U8_HWC and crop_shim._frames(frames)[0].data_ptr() == frames.data_ptr()      # no copy
    views = dict(image=frames, intrinsics=torch.eye(3, device=_dev()).repeat(5, 1, 1))
    got = apply_crop_shim_to_views(views, (32, 32))
    want = S.crop_frames(_pixels(names), (32, 32))[1]
    assert np.array_equal(got["image"].cpu().numpy(), want)


def test_no_host_synchronisation_without_the_check():
    from vicasplat_amd.dataset import decode_jpeg_batch
    names = R.BATCHES["80x45"]
    warm = decode_jpeg_batch(_streams(names), device=_dev())
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got, status = decode_jpeg_batch(_streams(names), device=_dev(), check=False, return_status=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(got, warm) and status.tolist() == [0] * 5


def test_graph_capture_and_replay_on_other_bytes():
    from vicasplat_amd.dataset import pack_jpeg_batch
    from vicasplat_amd.dataset.jpeg import decode_packed
    dev = _dev()
    names = R.BATCHES["80x45"]
    first, second = pack_jpeg_batch(_streams(names)), pack_jpeg_batch(_streams(names[::-1]))
    sizes = lambda p: (p.n, p.h, p.w, p.segments, p.max_frame_segments, p.n_quant, p.n_huff, p.blocks, len(p.buffer))
    assert sizes(first) == sizes(second)          # the same frames in another order: every argument of the call is the same
    static = torch.from_numpy(first.buffer).to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        decode_packed(first, dev, buffer=static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, status = decode_packed(first, dev, buffer=static)
    static.copy_(torch.from_numpy(second.buffer).to(dev))
    graph.replay()
    torch.cuda.synchronize()
    assert _differing(out, _pixels(names[::-1])) == 0 and status.tolist() == [0] * 5


def test_damaged_frames_are_flagged_and_harm_nothing_else():
    """Frame 2 is a truncated stream and frame 4 has a flipped bit, both among the streams the sanitizer build has decoded in bounds on the
    CPU (tests/test_jpeg_cpu.py): the status is non-zero exactly where the restatement flags, the other frames are PIL's pixels, and
    nothing is written outside the call's buffers."""
    from vicasplat_amd.dataset import JpegError, decode_jpeg_batch
    datas = [R.damage(R.fixture()[n][0], kind, arg) for n, kind, arg in R.DAMAGED_BATCH]
    flagged = [R.decode_coefficients(d)[1] != 0 for d in datas]
    assert flagged == [False, False, True, False, True]
    for pad in (64, 67):
        pix, stat = _guarded(datas, pad)
        print(f"pad {pad}: status {stat.tolist()}")
        assert [int(s) != 0 for s in stat] == flagged
        for i, (n, _, _) in enumerate(R.DAMAGED_BATCH):
            if not flagged[i]:
                assert np.array_equal(pix[i], R.fixture()[n][1]), n
    with pytest.raises(JpegError, match="damaged") as e:
        decode_jpeg_batch(datas, device=_dev())
    assert e.value.frames == (2, 4) and isinstance(e.value, OSError)
    got, status = decode_jpeg_batch(datas, device=_dev(), check=False, return_status=True)
    assert [s != 0 for s in status.tolist()] == flagged and np.array_equal(got.cpu().numpy()[[0, 1, 3]], pix[[0, 1, 3]])
