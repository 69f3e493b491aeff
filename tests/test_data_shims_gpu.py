"""The data shims on the GPU: vsp_rescale_crop (csrc/preprocess.hip) and the Python surface of vicasplat_amd.dataset against the numpy
restatement of tests/data_shims_ref.py -- the yardstick, itself pinned to the installed PIL and to the real reference on the CPU
(tests/test_data_shims_cpu.py) -- and against the reference's golden vectors (tests/golden/crop_shim.npz).  Every comparison is bit for bit.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import data_shims_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "crop_shim.npz")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
FORMS = ("u8_hwc", "u8_chw", "f32")
SENTINEL = -77.25
_refs: dict = {}


def _dev():
    return torch.device("cuda:0")


def _reference(case: str, fill: str):
    """(frames [N, h, w, 3] uint8, mirror flags, float32 [N, 3, h_out, w_out]) of a case, computed once."""
    if (case, fill) not in _refs:
        n, h, w, shape, mirror = R.GPU_CASES[case]
        frames = R.make_frames(n, h, w, fill, seed=7)
        _refs[case, fill] = (frames, np.array(mirror, np.uint8), R.crop_frames(frames, shape, mirror)[1])
    return _refs[case, fill]


def _as_form(frames: np.ndarray, form: str) -> torch.Tensor:
    """[N, 3, h, w] on the device in one of the three input forms."""
    t = torch.from_numpy(frames).to(_dev())
    if form == "u8_hwc":
        return t.permute(0, 3, 1, 2)          # a view of the packed buffer: no copy
    if form == "u8_chw":
        return t.permute(0, 3, 1, 2).contiguous()
    x = ((frames.astype(np.float32) + np.float32(0.5)) / np.float32(255)).astype(np.float32)      # floats that quantise back to the bytes
    assert np.array_equal(R.quantise(x), frames)
    return torch.from_numpy(np.ascontiguousarray(np.moveaxis(x, -1, 1))).to(_dev())


@pytest.mark.parametrize("case", list(R.GPU_CASES))
def test_bit_equal_to_the_restatement(case):
    from vicasplat_amd.dataset.shims import crop_shim
    n, h, w, shape, _ = R.GPU_CASES[case]
    K = torch.eye(3, device=_dev()).repeat(n, 1, 1)
    for fill in R.FILLS:
        frames, mirror, want = _reference(case, fill)
        flags = torch.from_numpy(mirror).to(_dev())
        for form in FORMS:
            x = _as_form(frames, form)
            got, K2 = crop_shim.rescale_and_crop(x, K, shape, mirror=flags)
            assert got.dtype == torch.float32 and tuple(got.shape) == (n, 3) + shape
            differing = int((got.cpu().numpy() != want).sum())
            print(f"{case} {fill} {form}: {differing} differing elements")
            assert differing == 0, (case, fill, form)
            assert np.array_equal(K2.cpu().numpy(), R.crop_intrinsics(np.tile(np.eye(3, dtype=np.float32), (n, 1, 1)), h, w, shape))
            # two runs are bit-equal; a frame alone equals the same frame inside the batch
            again, _ = crop_shim.rescale_and_crop(x, K, shape, mirror=flags)
            assert torch.equal(again, got)
            i = n - 1
            alone, _ = crop_shim.rescale_and_crop(x[i:i + 1], K[i:i + 1], shape, mirror=flags[i:i + 1])
            assert torch.equal(alone[0], got[i])
            # the normalised form: (x - mean) / std by torch on the CPU from the raw form
            normed, _ = crop_shim.rescale_and_crop(x, K, shape, mirror=flags, normalize=(MEAN, STD))
            raw = got.cpu()
            want_n = (raw - torch.tensor(MEAN).view(3, 1, 1)) / torch.tensor(STD).view(3, 1, 1)
            assert torch.equal(normed.cpu(), want_n), (case, fill, form)
        if fill == "constant":
            assert float(got.min()) == 1.0


@pytest.mark.parametrize("case", list(R.GPU_CASES))
def test_output_stays_inside_its_buffer(case):
    """The entry itself, writing into the middle of a sentinel-filled buffer, at a 16-byte aligned offset and at a misaligned one (the vector
    and the scalar stores)."""
    from vicasplat_amd import _lib
    from vicasplat_amd.dataset.shims import crop_shim
    n, h, w, shape, _ = R.GPU_CASES[case]
    frames, mirror, want = _reference(case, "random")
    dev = _dev()
    x = torch.from_numpy(frames).to(dev)
    flags = torch.from_numpy(mirror).to(dev)
    h_scaled, w_scaled = R.scaled_size(h, w, shape)
    row, col = (h_scaled - shape[0]) // 2, (w_scaled - shape[1]) // 2
    bx, kx_t, kx = crop_shim._tables_on(w, w_scaled, dev)
    by, ky_t, ky = crop_shim._tables_on(h, h_scaled, dev)
    count = n * 3 * shape[0] * shape[1]
    for pad in (64, 67):
        buf = torch.full((pad + count + 131,), SENTINEL, dtype=torch.float32, device=dev)
        out = buf[pad:pad + count]
        _lib.call("vsp_rescale_crop", dev, _lib.ptr(x), 0, n, h, w, _lib.ptr(bx), _lib.ptr(kx_t), w_scaled, kx, _lib.ptr(by), _lib.ptr(ky_t), h_scaled,
                  ky, row, col, shape[0], shape[1], _lib.ptr(flags), None, None, _lib.ptr(out))
        host = buf.cpu().numpy()
        assert (host[:pad] == np.float32(SENTINEL)).all() and (host[pad + count:] == np.float32(SENTINEL)).all(), (case, pad)
        assert np.array_equal(host[pad:pad + count].reshape(want.shape), want), (case, pad)


def test_float_quantisation_in_the_kernel():
    """Both passes skipped: the output is the quantised input / 255.  Exact u / 255, their neighbours, values outside [0, 1], NaN -> 0."""
    from vicasplat_amd.dataset.shims import crop_shim
    u = np.arange(256, dtype=np.float32) / np.float32(255)
    vals = np.concatenate([u, np.nextafter(u, np.float32(-np.inf)), np.nextafter(u, np.float32(np.inf)),
                           np.array([-1.0, -1e-3, -0.0, -1e-45, 1.0 + 1e-6, 1.5, 300.0, np.inf, -np.inf, np.nan], np.float32)])
    vals = np.resize(vals, 3 * 9 * 31).reshape(1, 3, 9, 31).astype(np.float32)
    got = crop_shim.rescale(torch.from_numpy(vals).to(_dev()), (9, 31)).cpu().numpy()
    assert np.array_equal(got, R.quantise(vals).astype(np.float32) / np.float32(255))


def _example_on_device(name: str, as_uint8: bool):
    ex = R.golden_example(name)
    out = {}
    for g in ("context", "target"):
        image = ex[g]["image"]
        if as_uint8:          # as a decoder delivers it: packed HWC, handed over as a permuted view
            image = torch.from_numpy(np.ascontiguousarray(np.moveaxis(R.quantise(image), 1, -1))).to(_dev()).permute(0, 3, 1, 2)
        else:
            image = torch.from_numpy(image).to(_dev())
        out[g] = dict(image=image, intrinsics=torch.from_numpy(ex[g]["intrinsics"]).to(_dev()), extrinsics=torch.from_numpy(ex[g]["extrinsics"]).to(_dev()))
    return out


def _assert_views(got: dict, golden, key: str):
    want = golden[key + "_image_u8"].astype(np.float32) / np.float32(255)
    assert np.array_equal(got["image"].cpu().numpy(), want), key
    assert np.array_equal(got["intrinsics"].cpu().numpy(), golden[key + "_intrinsics"]), key
    assert np.array_equal(got["extrinsics"].cpu().numpy(), golden[key + "_extrinsics"]), key
    assert "mirror" not in got


@pytest.mark.parametrize("as_uint8", (False, True), ids=("float", "uint8_hwc"))
def test_apply_crop_shim_reproduces_the_reference(as_uint8):
    from vicasplat_amd.dataset.shims import apply_crop_shim, reflect_views
    golden = np.load(GOLDEN)
    for name in R.GOLDEN_EXAMPLES:
        ex = _example_on_device(name, as_uint8)
        plain = apply_crop_shim(ex, R.GOLDEN_SHAPE)
        reflected = apply_crop_shim(dict(context=reflect_views(ex["context"]), target=reflect_views(ex["target"])), R.GOLDEN_SHAPE)
        for g in ("context", "target"):
            _assert_views(plain[g], golden, f"{name}_plain_{g}")
            _assert_views(reflected[g], golden, f"{name}_reflected_{g}")


def test_preprocess_batch_reproduces_the_reference():
    """Two scenes (the 45 x 80 example twice), a generator seeded with 0: the reference leaves scene 0 unchanged and reflects scene 1."""
    from vicasplat_amd.dataset import preprocess_batch
    golden = np.load(GOLDEN)
    assert golden["augmentation_unchanged"][:2].tolist() == [True, False]
    ex = _example_on_device("wide", True)
    batch = {g: {k: torch.stack([v, v]) for k, v in ex[g].items()} for g in ("context", "target")}
    batch["scene"] = ["a", "b"]
    out = preprocess_batch(batch, R.GOLDEN_SHAPE, augment=True, generator=torch.Generator().manual_seed(0))
    assert out["scene"] == ["a", "b"] and batch["context"]["image"].dtype == torch.uint8
    for g in ("context", "target"):
        for b, form in enumerate(("plain", "reflected")):
            _assert_views({k: v[b] for k, v in out[g].items()}, golden, f"wide_{form}_{g}")
    plain = preprocess_batch(batch, R.GOLDEN_SHAPE)
    for g in ("context", "target"):
        for b in range(2):
            _assert_views({k: v[b] for k, v in plain[g].items()}, golden, f"wide_plain_{g}")
    normed = preprocess_batch(batch, R.GOLDEN_SHAPE, normalize_context=((0.5,) * 3, (0.5,) * 3))
    assert torch.equal(normed["context"]["image"].cpu(), (plain["context"]["image"].cpu() - 0.5) / 0.5)
    assert torch.equal(normed["target"]["image"], plain["target"]["image"])


def test_no_host_synchronisation_and_graph_capture():
    from vicasplat_amd.dataset.shims import apply_crop_shim_to_views, reflect_views
    n, h, w, shape, _ = R.GPU_CASES["50x71"]
    frames, _, _ = _reference("50x71", "random")
    dev = _dev()
    x = torch.from_numpy(frames).to(dev).permute(0, 3, 1, 2)
    views = reflect_views(dict(image=x, intrinsics=torch.eye(3, device=dev).repeat(n, 1, 1), extrinsics=torch.eye(4, device=dev).repeat(n, 1, 1)))
    warm = apply_crop_shim_to_views(views, shape, normalize=(MEAN, STD))          # builds and uploads the tables
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = apply_crop_shim_to_views(views, shape, normalize=(MEAN, STD))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(got["image"], warm["image"]) and torch.equal(got["intrinsics"], warm["intrinsics"])
    # one single-branch capture, one replay on new bytes
    static = torch.from_numpy(frames).to(dev)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        apply_crop_shim_to_views(dict(views, image=static.permute(0, 3, 1, 2)), shape)
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        captured = apply_crop_shim_to_views(dict(views, image=static.permute(0, 3, 1, 2)), shape)["image"]
    other = R.make_frames(n, h, w, "random", seed=8)
    static.copy_(torch.from_numpy(other).to(dev))
    graph.replay()
    torch.cuda.synchronize()
    eager = apply_crop_shim_to_views(dict(views, image=torch.from_numpy(other).to(dev).permute(0, 3, 1, 2)), shape)["image"]
    assert torch.equal(captured, eager)
    assert np.array_equal(eager.cpu().numpy(), R.crop_frames(other, shape, [1] * n)[1])
