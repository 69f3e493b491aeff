"""The PNG encoder without a GPU: the yardstick (tests/png_ref.py, restated from the comment of include/vicasplat_png.h) against the installed
PIL and zlib on every case, the size caps, the planted defects, the binding of include/vicasplat_png.h with every refusal, the kernels' serial
code (csrc/png_deflate.h) compiled for the host under the address and undefined-behaviour sanitizers (tests/png_probe.cpp) byte for byte
against the yardstick, and the control flow of callers.save_test_outputs on stubs."""
import io
import json
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import png_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _pil_pixels(data, shape):
    from PIL import Image
    Image.open(io.BytesIO(data)).verify()
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.mode == {1: "L", 3: "RGB", 4: "RGBA"}[shape[2]]
    return np.asarray(im).reshape(shape)


def _check_file(data, pixels, mode):
    """Raises (AssertionError, zlib.error, OSError, SyntaxError, ...) unless `data` is a valid file of the stated shape that decodes to `pixels`."""
    h, w, c = pixels.shape
    parts = R.chunks(data)
    _, _, segs = R.shape(h, w, c)
    assert [k for k, _, _ in parts] == [b"IHDR"] + [b"IDAT"] * segs + [b"IEND"]
    for kind, body, crc in parts:
        assert crc == zlib.crc32(kind + body), kind
    idat = [body for kind, body, _ in parts if kind == b"IDAT"]
    assert idat[0][:2] == b"\x78\x01" and (idat[0][0] * 256 + idat[0][1]) % 31 == 0 and idat[0][0] >> 4 == 7      # deflate, a 32 KiB window
    stream, _ = R.filter_rows(pixels, mode)
    assert zlib.decompress(b"".join(idat)) == stream.tobytes()          # (zlib checks the Adler-32 itself)
    # every IDAT after the first starts a fresh deflate block on a byte boundary: the first k chunks inflate to the first k segments
    rows = R.shape(h, w, c)[1]
    for k in range(1, segs):
        d = zlib.decompressobj()
        assert d.decompress(b"".join(idat[:k])) == stream[:k * rows].tobytes() and not d.eof, k
    assert np.array_equal(_pil_pixels(data, pixels.shape), pixels)
    assert len(data) <= R.bound(h, w, c)


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.cases()))
def test_every_case_is_a_valid_file_with_the_exact_pixels(name):
    pixels, mode = R.cases()[name]
    data = R.reference_file(name)
    _check_file(data, pixels, mode)
    print(f"{name}: {pixels.shape} -> {len(data)} bytes, bound {R.bound(*pixels.shape)}")


def _plans(name):
    pixels, mode = R.cases()[name]
    stream, types = R.filter_rows(pixels, mode)
    return [R.plan_segment(seg) for seg in R.segments(stream, *pixels.shape)], types


def test_case_list_covers_what_it_must():
    cases = R.cases()
    assert {"golden_frame", "golden_small_rgb", "golden_small_grey"} <= set(cases), "tests/golden/png_frames.npz is missing"
    assert cases["golden_frame"][0].shape == (256, 256, 3) and cases["golden_small_rgb"][0].shape == (40, 64, 3)
    assert cases["golden_small_grey"][0].shape == (40, 64, 1)
    assert R.shape(256, 256, 3) == (769, 21, 13)
    assert [cases[f"256_rgb_{n}"][0].shape[0] for n in ("R-1", "R", "R+1", "2R+1")] == [20, 21, 22, 43]
    assert [R.shape(h, 256, 3)[2] for h in (20, 21, 22, 43)] == [1, 1, 2, 3]
    assert [cases[n][0].shape for n in ("1x1_c1", "1x1_c3", "1x1_c4", "1x7", "7x1")] == [(1, 1, 1), (1, 1, 3), (1, 1, 4), (1, 7, 3), (7, 1, 3)]
    # the longest row, and one byte more
    assert R.shape(*cases["long_row"][0].shape)[0] == 65535
    with pytest.raises(R.Refused):
        R.shape(2, 65535, 1)
    with pytest.raises(R.Refused):
        R.shape(65536, 1, 1)
    # the runs: with filter 0 on a grey row the stream is the pixels
    plans, _ = _plans("runs")
    toks = plans[0]["tokens"]
    got = {n: toks[toks.index((100 + k, None)) + 1:toks.index((200 + k, None))] for k, n in enumerate(R.RUNS)}      # after the run's first literal
    lit = lambda k: (100 + R.RUNS.index(k), None)
    assert got[2] == [lit(2)] and got[3] == [lit(3)] * 2 and got[4] == [(None, 3)] and got[258] == [(None, 257)] and got[259] == [(None, 258)]
    assert got[260] == [(None, 258), lit(260)] and got[261] == [(None, 258), lit(261), lit(261)] and got[262] == [(None, 258), (None, 3)]
    assert got[517] == [(None, 258), (None, 258)]
    # noise: stored; the limits bind; the degenerate and the full alphabets
    assert {p["form"] for p in _plans("noise")[0]} == {"stored"}
    fib, _ = _plans("fibonacci")
    assert sorted(f for f in fib[0]["freq"] if f) == R.fibonacci_counts() and R.fibonacci_counts()[-1] == 4181
    assert max(R.huffman_depths(fib[0]["freq"])[1]) > 15 and max(fib[0]["lengths"]) == 15 and fib[0]["form"] == "dynamic"
    assert not any(v is None for v, _ in fib[0]["tokens"])      # no match
    (cl,), _ = _plans("clen_limit")
    cfreq = [sum(1 for s, _ in cl["seq"] if s == k) for k in range(19)]
    assert max(R.huffman_depths(cfreq)[1]) > 7 and max(cl["clen"]) == 7 and cl["form"] == "dynamic"
    (al,), _ = _plans("all_symbols")
    assert all(al["freq"][s] > 0 for s in range(286)) and al["nlit"] == 286 and al["form"] == "dynamic"
    (nm,), _ = _plans("no_match")
    assert nm["dist"] == 0 and nm["form"] == "dynamic" and not any(v is None for v, _ in nm["tokens"])
    (mo,), _ = _plans("constant_grey_zero")
    assert [t for t in mo["tokens"]] == [(0, None)] + [(None, 258)] * 60 and mo["dist"] == 1 and mo["form"] == "dynamic"
    (two,), _ = _plans("two_symbols")
    assert sum(1 for f in two["freq"] if f) == 2 and [l for l in two["lengths"] if l] == [1, 1]
    # a Kraft sum of exactly 1 wherever a limit was applied
    for plan in (fib[0], cl):
        assert sum(2.0 ** -l for l in plan["lengths"] if l) == 1.0 and sum(2.0 ** -l for l in plan["clen"] if l) == 1.0
    # filters
    for mode in range(5):
        assert cases[f"fixed_filter_{mode}"][1] == mode and set(_plans(f"fixed_filter_{mode}")[1]) == {mode}
    assert set(_plans("each_filter")[1]) == {0, 1, 2, 3, 4}
    assert all(len(b) == 5 and len({x.shape for x in b}) == 1 for b in R.batches().values()) and len(R.batches()) == 2


def test_float_rule_equals_the_torch_expression():
    import torch
    x = R.float_probes()
    got = R.quantise(x)
    finite = ~np.isnan(x)
    t = torch.from_numpy(x[finite])
    want = (t.clip(min=0, max=1) * 255).type(torch.uint8).numpy()          # src/misc/image_io.py:53
    assert np.array_equal(got[finite], want)
    assert (got[~finite] == 0).all() and (~finite).any()                    # the stated deviation: a NaN gives 0
    assert R.quantise(np.float32(-0.0)) == 0 and R.quantise(np.float32(np.inf)) == 255 and R.quantise(np.float32(-np.inf)) == 0
    assert R.quantise(np.float32(1)) == 255 and R.quantise(np.float32(0.99999994)) == 254


# ---- sizes: caps, not measurements -----------------------------------------------------------------------------------------------------------
def test_noise_stays_within_the_bound_formula():
    pixels, _ = R.cases()["noise"]
    h, w, c = pixels.shape
    rb = 1 + w * c
    rows = min(max(16384 // rb, 1), h)
    segs = -(-h // rows)
    # signature, IHDR, IEND (45); zlib header and Adler-32 (6); filtered bytes; per segment chunk framing (12), a stored header (5), the sync block (5)
    bound = 45 + 6 + h * rb + segs * (12 + 5 + 5)
    assert bound == R.bound(h, w, c)
    assert len(R.reference_file("noise")) <= bound
    assert len(R.reference_file("noise")) == bound - 5          # every segment stored; the last one has no sync block


def test_constant_image_is_at_most_one_percent_of_raw():
    pixels, _ = R.cases()["constant_rgb"]
    size = len(R.reference_file("constant_rgb"))
    print(f"constant 256 x 256 RGB: {size} bytes, {100 * size / pixels.size:.3f} % of raw")
    assert size <= 0.01 * pixels.size


def test_golden_frame_is_within_one_percent_of_zlib_rle_per_segment():
    """The cap on the code construction: 69 bytes of framing + per segment zlib's own Z_RLE / level 9 raw deflate with a full flush + 12 bytes of chunk
    framing per segment, times 1.01.  Measured here: 118 207 bytes against a cap of 1.01 x 118 241 (ratio 0.9997); PIL's own file of the
    frame has 116 339 bytes (ratio 1.016, recorded, not asserted)."""
    pixels, mode = R.cases()["golden_frame"]
    stream, _ = R.filter_rows(pixels, mode)
    segs = R.segments(stream, *pixels.shape)
    total = 69
    for seg in segs:
        co = zlib.compressobj(9, zlib.DEFLATED, -15, 9, zlib.Z_RLE)
        total += len(co.compress(seg) + co.flush(zlib.Z_FULL_FLUSH)) + 12
    size = len(R.reference_file("golden_frame"))
    pil = np.load(R.GOLDEN)["pil_bytes"]
    print(f"golden frame: {size} bytes, zlib-per-segment size {total} (ratio {size / total:.4f}), PIL {int(pil[0])} (ratio {size / int(pil[0]):.4f})")
    for k, name in enumerate(("golden_frame", "golden_small_rgb", "golden_small_grey")):
        print(f"{name}: {len(R.reference_file(name))} bytes, PIL {int(pil[k])}")
    assert size <= 1.01 * total


# ---- the planted defects ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect", R.DEFECTS)
def test_every_planted_defect_is_caught(defect):
    caught = []
    for name, (pixels, mode) in R.cases().items():
        if pixels.size > 70000:
            continue          # (the small cases reach every defect)
        try:
            data = R.encode(pixels, mode, defect)
            if data == R.reference_file(name):
                continue
            _check_file(data, pixels, mode)
        except Exception as e:      # PIL or zlib raised, a CRC or a pixel differs
            caught.append((name, type(e).__name__))
    print(f"{defect}: caught on {len(caught)} cases: {caught[:5]}")
    assert caught, defect


def test_paeth_tie_between_a_and_b_cannot_be_observed():
    """Taking b before a on a tie is planted in the restatement as well, but it is the same predictor: pa == pb with a != b means
    a - c == c - b, so p == c and pc == 0 < pa -- c is taken whichever of a and b is asked first.  Proved here over all 2^24 byte triples;
    the tie order a decoder CAN see (b before c) is among R.DEFECTS."""
    a, b, c = np.meshgrid(*[np.arange(256, dtype=np.int32)] * 3, indexing="ij", sparse=True)
    assert np.array_equal(R.paeth(a, b, c), R.paeth(a, b, c, "paeth_b_before_a"))
    assert (R.paeth(a, b, c) != R.paeth(a, b, c, "paeth_c_before_b")).any()


# ---- the binding ------------------------------------------------------------------------------------------------------------------------
def test_the_png_header_parses_is_bound_and_is_documented():
    import ctypes as C
    from vicasplat_amd import _lib
    assert _lib.IO_HEADERS == (("vse_", "vicasplat_png.h"),)
    assert _lib.ALL_HEADERS == _lib.HEADERS + _lib.DATA_HEADERS + _lib.DRAW_HEADERS and _lib.BOUND_HEADERS == _lib.ALL_HEADERS + _lib.IO_HEADERS
    assert "vse_" not in dict(_lib.ALL_HEADERS) and _lib.ABI_VERSION == 10
    assert os.path.samefile(_lib.header_path("vse_"), os.path.join(ROOT, "include", "vicasplat_png.h"))
    text = open(_lib.header_path("vse_")).read()
    sigs = _lib.parse_header(text, prefix="vse_")
    i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
    assert sigs == {"vse_png_bound": (C.c_int64, [i32, i32, i32], False),
                    "vse_png_workspace_bytes": (C.c_int64, [i32, i32, i32, i32], False),
                    "vse_png_encode": (C.c_int, [vp, i32, i32, i32, i32, i32, i32, vp, i64, vp, i64, vp, vp], True)}
    L = _lib.lib()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for entry, (restype, argtypes, takes_stream) in sigs.items():
        fn = getattr(L, entry)
        assert fn.restype is restype and fn.argtypes == argtypes and _lib._entries[entry] == (fn, takes_stream)
        assert entry in doc, f"{entry} is not in INTEGRATION.md"
    consts = _lib.header_constants(_lib.header_path("vse_"), "VSE_")
    assert len(consts) == 9 and all(getattr(_lib, k) == v for k, v in consts.items())
    assert (_lib.VSE_FILTER_ADAPTIVE, _lib.VSE_SEGMENT_BYTES, _lib.VSE_MAX_ROW_BYTES) == (R.ADAPTIVE, R.SEGMENT_BYTES, 65535)
    assert "png.hip" in open(os.path.join(ROOT, "vicasplat_amd", "csrc", "Makefile")).read()


def test_bound_and_every_refusal_come_before_any_gpu_call():
    import torch
    from vicasplat_amd import _lib
    L = _lib.lib()
    was_initialised = torch.cuda.is_initialized()
    for name, (pixels, _) in R.cases().items():
        assert L.vse_png_bound(*pixels.shape) == R.bound(*pixels.shape), name
    assert L.vse_png_bound(256, 256, 3) == 51 + 256 * 769 + 22 * 13
    assert L.vse_png_bound(2, 65534, 1) > 0
    assert L.vse_png_bound(2, 65535, 1) < 0 and b"exceed 65535" in L.vs_last_error()
    assert L.vse_png_bound(65536, 1, 1) < 0 and b"exceed 65535" in L.vs_last_error()
    assert L.vse_png_bound(4, 4, 2) < 0 and b"channels" in L.vs_last_error()
    assert L.vse_png_bound(0, 4, 3) < 0 and b"at least 1" in L.vs_last_error()
    need = L.vse_png_workspace_bytes(3, 23, 40, 3)
    assert need > 3 * 23 * 121 and need % 16 == 0
    assert L.vse_png_workspace_bytes(-1, 23, 40, 3) < 0 and b"must not be negative" in L.vs_last_error()
    assert L.vse_png_workspace_bytes(1, 23, 40, 5) < 0 and b"channels" in L.vs_last_error()
    assert L.vse_png_workspace_bytes(20000, 256, 256, 3) < 0 and b"reach 2^31" in L.vs_last_error()
    p = 4096      # an aligned address that is never dereferenced: every call below returns before any HIP call
    bound = R.bound(23, 40, 3)
    ok = dict(images=p, layout=_lib.VSP_LAYOUT_F32_CHW, n=3, h=23, w=40, c=3, filter_mode=_lib.VSE_FILTER_ADAPTIVE, workspace=p,
              workspace_bytes=need, out=p + 1, out_stride=bound, lengths=p)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vse_png_encode(*a.values(), None)
    for name in ("images", "workspace", "out", "lengths"):
        assert call(**{name: None}) < 0 and b"null pointer" in L.vs_last_error(), name
    assert call(layout=3) < 0 and b"unknown layout" in L.vs_last_error()
    assert call(layout=-1) < 0 and b"unknown layout" in L.vs_last_error()
    assert call(c=2) < 0 and b"channels" in L.vs_last_error()
    assert call(filter_mode=6) < 0 and b"unknown filter mode" in L.vs_last_error()
    assert call(filter_mode=-1) < 0 and b"unknown filter mode" in L.vs_last_error()
    assert call(n=-1) < 0 and b"must not be negative" in L.vs_last_error()
    assert call(h=0) < 0 and b"at least 1" in L.vs_last_error()
    assert call(w=65535, c=1) < 0 and b"exceed 65535" in L.vs_last_error()
    assert call(workspace_bytes=need - 1) < 0 and b"vse_png_workspace_bytes" in L.vs_last_error()
    assert call(workspace=p + 8) < 0 and b"16-byte aligned" in L.vs_last_error()
    assert call(lengths=p + 2) < 0 and b"4-byte aligned" in L.vs_last_error()
    assert call(images=p + 2) < 0 and b"4-byte aligned" in L.vs_last_error()
    assert call(out_stride=bound - 1) < 0 and b"below the bound" in L.vs_last_error()
    assert call(n=20000, h=256, w=256, workspace_bytes=1 << 40, out_stride=1 << 20) < 0 and b"reach 2^31" in L.vs_last_error()
    assert call(n=0) == 0
    assert call(n=0, images=p + 1, layout=_lib.VSP_LAYOUT_U8_HWC) == 0          # bytes need no alignment
    assert torch.cuda.is_initialized() == was_initialised
    from vicasplat_amd.misc import image_io
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        image_io.encode_png_batch(torch.zeros(1, 3, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        image_io.save_image(torch.zeros(3, 4, 4), "never_written.png")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        image_io.prep_image(torch.zeros(3, 4, 4))
    assert image_io.encode_png_batch([]) == [] and not os.path.exists("never_written.png")


# ---- the kernels' serial code under the sanitizers ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    cxx = shutil.which("c++") or (rocm_clang if os.path.exists(rocm_clang) else None)
    assert cxx, "no host C++ compiler (c++ or ROCm's clang++): csrc/png_deflate.h cannot be checked"
    exe = str(tmp_path_factory.mktemp("png_probe") / "png_probe")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(HERE, "png_probe.cpp")], check=True)

    def run(jobs):
        """[file bytes, or None for a refused shape] of [(pixels [H, W, C] or a bare shape, mode)]."""
        blob = b""
        for pixels, mode in jobs:
            if isinstance(pixels, tuple):
                blob += struct.pack("<4i", *pixels, mode)
            else:
                blob += struct.pack("<4i", *pixels.shape, mode) + pixels.tobytes()
        done = subprocess.run([exe], input=blob, capture_output=True)
        assert done.returncode == 0 and not done.stderr, done.stderr.decode(errors="replace")[-4000:]      # the sanitizers report nothing
        out, at, files = done.stdout, 0, []
        for _ in jobs:
            n, = struct.unpack_from("<i", out, at)
            files.append(None if n < 0 else out[at + 4:at + 4 + n])
            at += 4 + max(n, 0)
        assert at == len(out)
        return files
    return run


def test_host_build_of_the_encoder_under_the_sanitizers(probe):
    names = list(R.cases())
    files = probe([R.cases()[n] for n in names] + [((2, 65535, 1), 0), ((65536, 1, 1), 0), ((3, 3, 2), 0)])
    assert files[-3:] == [None, None, None]
    for name, got in zip(names, files):
        want = R.reference_file(name)
        differing = sum(a != b for a, b in zip(got, want)) + abs(len(got) - len(want))
        print(f"{name}: {len(got)} bytes, {differing} differing")
        assert differing == 0, name
    # every image of the GPU tests' batches too, in every filter mode
    jobs = [(x, mode) for b in R.batches().values() for x in b for mode in (R.ADAPTIVE, 0, 3, 4)]
    for (pixels, mode), got in zip(jobs, probe(jobs)):
        assert got == R.encode(pixels, mode)


# ---- callers.save_test_outputs on stubs ---------------------------------------------------------------------------------------------------------
def test_save_test_outputs_writes_the_references_tree(tmp_path, monkeypatch):
    import types

    import torch
    from vicasplat_amd import callers
    from vicasplat_amd.misc import image_io, utils
    calls = []

    def encode(images, filter="adaptive", layout=None):
        calls.append(tuple(images.shape))
        return [R.encode(R.quantise(x.numpy()).transpose(1, 2, 0)) for x in images]
    monkeypatch.setattr(image_io, "encode_png_batch", encode)
    monkeypatch.setattr(utils, "vis_depth_map", lambda d: (d / d.max())[..., None, :, :].expand(*d.shape[:-2], 3, *d.shape[-2:]))
    g = torch.Generator().manual_seed(0)
    b, v, vt, h, w = 2, 2, 3, 6, 5
    batch = {"scene": ["abc", "def"],
             "context": {"image": torch.rand(b, v, 3, h, w, generator=g) * 2 - 1, "index": torch.tensor([[3, 17], [0, 123456]])},
             "target": {"index": torch.tensor([[4, 5, 6], [7, 8, 1000001]])}}
    model_outs = {"gaussian_camera_extrins": torch.rand(b, v, 4, 4, generator=g)}
    output = types.SimpleNamespace(color=torch.rand(b, vt, 3, h, w, generator=g), depth=torch.rand(b, vt, h, w, generator=g) + 0.5)
    paths = callers.save_test_outputs(batch, model_outs, output, tmp_path / "run")
    want = [f"{s}/context/{i:0>6}.png" for s, row in (("abc", (3, 17)), ("def", (0, 123456))) for i in row] + \
        [f"{s}/color/{i:0>6}.png" for s, row in (("abc", (4, 5, 6)), ("def", (7, 8, 1000001))) for i in row]
    assert [str(p.relative_to(tmp_path / "run")) for p in paths] == want
    found = sorted(str(p.relative_to(tmp_path / "run")) for p in (tmp_path / "run").rglob("*") if p.is_file())
    assert found == sorted(want + ["abc/transforms.json", "def/transforms.json"])
    assert calls == [(b * v, 3, h, w), (b * vt, 3, h, 2 * w + 8)]          # one encoder call per frame shape
    for k, scene in enumerate(batch["scene"]):
        names = [f"context/{i:0>6}.png" for i in batch["context"]["index"][k].tolist()]
        callers.export_transforms(model_outs["gaussian_camera_extrins"][k], tmp_path / "want.json", file_names=names)
        assert (tmp_path / "run" / scene / "transforms.json").read_text() == (tmp_path / "want.json").read_text()
        assert [f["file_path"] for f in json.loads((tmp_path / "want.json").read_text())] == names
    # the pixels: the context frame un-normalised; the target beside its depth map with a white gap of 8
    ctx = _pil_pixels((tmp_path / "run" / "def" / "context" / "123456.png").read_bytes(), (h, w, 3))
    assert np.array_equal(ctx, R.quantise((batch["context"]["image"][1, 1] * 0.5 + 0.5).numpy()).transpose(1, 2, 0))
    tgt = _pil_pixels((tmp_path / "run" / "abc" / "color" / "000005.png").read_bytes(), (h, 2 * w + 8, 3))
    depth = utils.vis_depth_map(output.depth[0])[1]
    assert np.array_equal(tgt[:, :w], R.quantise(output.color[0, 1].numpy()).transpose(1, 2, 0)) and (tgt[:, w:w + 8] == 255).all()
    assert np.array_equal(tgt[:, w + 8:], R.quantise(depth.numpy()).transpose(1, 2, 0))
    # without save_image: the context frames and the transforms only
    paths = callers.save_test_outputs(batch, model_outs, output, tmp_path / "bare", save_image=False)
    assert len(paths) == b * v and not (tmp_path / "bare" / "abc" / "color").exists() and (tmp_path / "bare" / "abc" / "transforms.json").exists()
