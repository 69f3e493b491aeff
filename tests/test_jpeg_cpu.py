"""The JPEG decoder without a GPU: the yardstick (tests/jpeg_ref.py) against the installed PIL, the planted defects, the package's host
parser against the yardstick's descriptors and tables, every refusal, the binding of include/vicasplat_jpeg.h, and the kernels' serial code
(csrc/jpeg_decode.h) compiled for the host under the address and undefined-behaviour sanitizers (tests/jpeg_probe.cpp) on clean and damaged
streams.  Every pixel comparison is byte for byte."""
import io
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpeg_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_and_fixture_equal_pil(name):
    data, rgb = R.fixture()[name]
    w, h = R.CASES[name][:2]
    fresh = R.pil_decode(data)
    assert fresh.shape == (h, w, 3) and np.array_equal(fresh, rgb), "the fixture's pixels are not this PIL's decode"
    got, status = R.decode(data)
    differing = int((got != fresh).sum())
    print(f"{name}: {differing} differing bytes")
    assert differing == 0 and status == 0
    again = R.encode(name)           # a stream this PIL writes now: the same holds for it
    got, status = R.decode(again)
    assert np.array_equal(got, R.pil_decode(again)) and status == 0


def test_case_list_covers_what_it_must():
    p = {name: R.parse(data) for name, (data, _) in R.fixture().items()}
    assert {(q["hs"], q["vs"]) for q in p.values() if q["ncomp"] == 3} == {(1, 1), (2, 1), (2, 2)} and p["13x11_gray"]["ncomp"] == 1
    assert len(p["96x48_restart"]["segs"]) == 72 and len(p["80x45_rows"]["segs"]) == 3
    assert p["80x45_optimize"]["dc"] != p["80x45_420"]["dc"]                        # optimised tables are not the default ones
    assert any(b"\xff\x00" in data[slice(*R.scan_range(data))] for data, _ in R.fixture().values())      # stuffing occurs
    for batch in R.BATCHES.values():
        assert len(batch) == 5 and len({R.CASES[n][:2] for n in batch}) == 1


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_planted_defect_changes_a_byte(mutant):
    changed = [name for name, (data, rgb) in R.fixture().items() if not np.array_equal(R.decode(data, mutant)[0], rgb)]
    print(f"{mutant}: changes {len(changed)} cases: {changed[:6]}")
    assert changed, mutant


# ---- the package's host parser ------------------------------------------------------------------------------------------------------------
def _assert_descriptors(names):
    from vicasplat_amd.dataset import pack_jpeg_batch
    datas = [R.fixture()[n][0] for n in names]
    want, got = R.descriptors(datas), pack_jpeg_batch(datas)
    assert np.array_equal(got.frames, want["frames"]), names
    assert np.array_equal(got.segs, want["segs"]), names
    assert np.array_equal(got.quant, want["quant"]) and np.array_equal(got.huff, want["huff"]), names
    assert (got.n, got.blocks, got.segments, got.n_quant, got.n_huff) == (len(names), want["blocks"], len(want["segs"]), len(want["quant"]), len(want["huff"]))
    assert got.max_frame_segments == int(want["frames"][:, 6].max()) and (got.w, got.h) == R.CASES[names[0]][:2]
    assert bytes(got.buffer[got.bytes_at:got.bytes_at + sum(map(len, datas))]) == b"".join(datas) and len(got.buffer) % 16 == 0


def test_host_parser_gives_the_restatements_descriptors():
    import torch
    for name in R.CASES:
        _assert_descriptors([name])
    for batch in R.BATCHES.values():
        _assert_descriptors(list(batch))
    # PIL's default tables are the same in every frame: stored once; a tensor is taken as a byte string is
    from vicasplat_amd.dataset import pack_jpeg_batch
    data = R.fixture()["80x45_420"][0]
    twice = pack_jpeg_batch([data, torch.frombuffer(bytearray(data), dtype=torch.uint8)])
    assert (twice.n_quant, twice.n_huff) == (2, 4) and np.array_equal(twice.frames[0, 8:17], twice.frames[1, 8:17])
    with pytest.raises(ValueError, match="share one size"):
        pack_jpeg_batch([data, R.fixture()["45x80_420"][0]])


def _segments(data):
    """[(marker, offset of its FF, offset past its segment)] up to and including SOS."""
    out, pos = [], 2
    while True:
        m, size = data[pos + 1], data[pos + 2] * 256 + data[pos + 3]
        out.append((m, pos, pos + 2 + size))
        pos += 2 + size
        if m == 0xDA:
            return out


def _without(data, marker):
    for m, a, b in _segments(data):
        if m == marker:
            return data[:a] + data[b:]
    raise AssertionError(marker)


def _poke(data, marker, offset, value):
    """The byte at `offset` inside the payload of the first `marker` segment replaced."""
    for m, a, _ in _segments(data):
        if m == marker:
            return data[:a + 4 + offset] + bytes([value]) + data[a + 5 + offset:]
    raise AssertionError(marker)


def _refusals():
    from PIL import Image
    base = R.fixture()["16x16_420"][0]
    full = R.fixture()["8x8"][0]          # 4:4:4
    img = Image.fromarray(R.make_image("noise", 16, 16, "RGB"))

    def saved(image, **kw):
        buf = io.BytesIO()
        image.save(buf, "JPEG", **kw)
        return buf.getvalue()
    sos = [a for m, a, _ in _segments(base) if m == 0xDA][0]
    sof = [a for m, a, _ in _segments(base) if m == 0xC0][0]
    cmyk, rgb = saved(img.convert("CMYK")), saved(img, keep_rgb=True)
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01"
    return {
        "progressive (PIL)": (saved(img, progressive=True), "progressive"),
        "arithmetic": (base[:sof + 1] + b"\xc9" + base[sof + 2:], "arithmetic"),
        "12-bit": (_poke(base, 0xC0, 0, 12), "12-bit precision"),
        "CMYK (PIL)": (cmyk, "Adobe APP14|4 components"),
        "4 components": (_without(cmyk, 0xEE), "4 components"),
        "keep_rgb (PIL)": (rgb, "Adobe APP14|RGB component ids"),
        "Adobe": (base[:2] + adobe + base[2:], "Adobe APP14"),
        "RGB ids": (_without(_without(rgb, 0xEE), 0xE0) if b"JFIF" in rgb[:32] else _without(rgb, 0xEE), "RGB component ids without JFIF"),
        "4:4:0": (_poke(full, 0xC0, 7, 0x12), "sampling factors 1x2"),
        "4:1:1": (_poke(full, 0xC0, 7, 0x41), "sampling factors 4x1"),
        "chroma 2x1": (_poke(full, 0xC0, 10, 0x21), "sampling factors"),
        "scan of one component": (_poke(base, 0xDA, 0, 1), "several scans"),
        "second scan": (base[:-2] + b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00\x12\x34" + b"\xff\xd9", "several scans"),
        "16-bit quantisation": (_poke(base, 0xDB, 0, 0x10), "16-bit quantisation tables"),
        "DNL in the header": (base[:sos] + b"\xff\xdc\x00\x04\x00\x10" + base[sos:], "DNL"),
        "DNL after the scan": (base[:-2] + b"\xff\xdc\x00\x04\x00\x10\xff\xd9", "DNL"),
        "no SOI": (base[2:], "missing SOI"),
        "no SOF": (_without(base, 0xC0), "missing SOF"),
        "no SOS": (base[:sos], "missing SOS"),
        "no EOI": (base[:-2], "missing EOI"),
        "height 0": (_poke(_poke(base, 0xC0, 1, 0), 0xC0, 2, 0), "dimensions of 0"),
        "width 0": (_poke(_poke(base, 0xC0, 3, 0), 0xC0, 4, 0), "dimensions of 0"),
    }


def test_every_refusal_names_its_reason_and_touches_no_gpu():
    import torch
    from vicasplat_amd.dataset import JpegError, decode_jpeg_batch, pack_jpeg_batch
    assert issubclass(JpegError, OSError)
    good = R.fixture()["16x16_420"][0]
    was_initialised = torch.cuda.is_initialized()
    for what, (data, reason) in _refusals().items():
        with pytest.raises(JpegError, match=reason) as e:
            pack_jpeg_batch([good, data])
        assert e.value.frames == (1,) and "frame 1" in str(e.value), what
        with pytest.raises(OSError, match=reason):          # the public entry refuses before it reaches for the device
            decode_jpeg_batch([data], device="cuda:0")
    assert torch.cuda.is_initialized() == was_initialised
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        decode_jpeg_batch([good], device="cpu")


# ---- the binding ------------------------------------------------------------------------------------------------------------------------
def test_the_jpeg_header_parses_is_bound_and_is_documented():
    import ctypes as C
    from vicasplat_amd import _lib
    assert _lib.DATA_HEADERS == (("vsj_", "vicasplat_jpeg.h"),) and "vsj_" not in dict(_lib.HEADERS)
    assert os.path.samefile(_lib.header_path("vsj_"), os.path.join(ROOT, "include", "vicasplat_jpeg.h"))
    text = open(_lib.header_path("vsj_")).read()
    sigs = _lib.parse_header(text, prefix="vsj_")
    i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
    assert sigs == {"vsj_workspace_bytes": (C.c_int64, [i64, i32], False),
                    "vsj_decode": (C.c_int, [vp, i64, i32, i32, i32, i32, i32, i32, i32, i64, vp, i64, vp, vp, vp], True)}
    L = _lib.lib()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for entry, (restype, argtypes, takes_stream) in sigs.items():
        fn = getattr(L, entry)
        assert fn.restype is restype and fn.argtypes == argtypes and _lib._entries[entry] == (fn, takes_stream)
        assert entry in doc, f"{entry} is not in INTEGRATION.md"
    for other, _ in _lib.HEADERS:
        assert not re.findall(r"\b%s[a-z0-9_]+\s*\(" % re.escape(other), re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    consts = _lib.header_constants(_lib.header_path("vsj_"), "VSJ_")
    assert len(consts) == 24 and all(getattr(_lib, k) == v for k, v in consts.items())
    assert (_lib.VSJ_FRAME_WORDS, _lib.VSJ_SEG_WORDS, _lib.VSJ_HUFF_BYTES, _lib.VSJ_LOOK_BITS) == (R.FRAME_WORDS, 4, R.HUFF_BYTES, R.LOOK_BITS)
    assert _lib.VSJ_HUFF_BYTES == 2 * (1 << _lib.VSJ_LOOK_BITS) + 72 + 72 + 256
    assert (_lib.VSJ_STATUS_INDEX, _lib.VSJ_STATUS_CODE, _lib.VSJ_STATUS_SHORT, _lib.VSJ_STATUS_LEFTOVER, _lib.VSJ_STATUS_MARKER) == \
        (R.INDEX, R.CODE, R.SHORT, R.LEFTOVER, R.MARKER)


def test_argument_validation_comes_before_any_gpu_call():
    from vicasplat_amd import _lib
    L = _lib.lib()
    p = 4096      # an aligned address that is never dereferenced: every call below returns before any HIP call
    need = L.vsj_workspace_bytes(10, 3)
    assert need == 10 * 192 + 16
    assert L.vsj_workspace_bytes(-1, 3) < 0 and b"negative" in L.vs_last_error()
    assert L.vsj_workspace_bytes(1, -3) < 0 and b"negative" in L.vs_last_error()
    ok = dict(packed=p, packed_bytes=1 << 20, N=1, h=8, w=8, segments=1, max_frame_segments=1, n_quant=1, n_huff=2, blocks=3, workspace=p,
              workspace_bytes=1 << 20, out=p, status=p)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vsj_decode(*a.values(), None)
    for name in ("packed", "workspace", "out", "status"):
        assert call(**{name: None}) < 0 and b"null pointer" in L.vs_last_error(), name
    for name in ("h", "w", "segments", "max_frame_segments", "n_quant", "n_huff", "blocks"):
        assert call(**{name: 0}) < 0 and b"at least 1" in L.vs_last_error(), name
    assert call(N=-1) < 0 and b"must not be negative" in L.vs_last_error()
    assert call(packed_bytes=100) < 0 and b"the packed buffer has 100" in L.vs_last_error()
    assert call(workspace_bytes=3 * 192 + 15) < 0 and b"vsj_workspace_bytes" in L.vs_last_error()
    assert call(packed=p + 4) < 0 and b"16-byte aligned" in L.vs_last_error()
    assert call(blocks=1 << 31, workspace_bytes=1 << 40) < 0 and b"2^31 - 1" in L.vs_last_error()
    assert call(N=0) == 0


# ---- the kernels' serial code under the sanitizers ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    cxx = shutil.which("c++") or (rocm_clang if os.path.exists(rocm_clang) else None)
    assert cxx, "no host C++ compiler (c++ or ROCm's clang++): csrc/jpeg_decode.h cannot be checked"
    exe = str(tmp_path_factory.mktemp("jpeg_probe") / "jpeg_probe")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(HERE, "jpeg_probe.cpp")], check=True)

    def run(streams):
        """[(status, coefficients int16 [blocks, 64], samples uint8 [blocks, 64] or None) or None for a stream the host parser refuses]."""
        from vicasplat_amd.dataset import JpegError, pack_jpeg_batch
        jobs, packs = [], []
        for data in streams:
            try:
                pk = pack_jpeg_batch([data])
            except JpegError:
                packs.append(None)
                continue
            packs.append(pk)
            jobs.append(struct.pack("<8i", pk.h, pk.w, pk.segments, pk.n_quant, pk.n_huff, pk.blocks, len(pk.buffer), len(data)) + pk.buffer.tobytes())
        done = subprocess.run([exe], input=b"".join(jobs), capture_output=True)
        assert done.returncode == 0 and not done.stderr, done.stderr.decode(errors="replace")[-4000:]      # the sanitizers report nothing
        out, at, results = done.stdout, 0, []
        for pk in packs:
            if pk is None:
                results.append(None)
                continue
            status = struct.unpack_from("<i", out, at)[0]
            coef = np.frombuffer(out, np.int16, pk.blocks * 64, at + 4).reshape(pk.blocks, 64)
            at += 4 + pk.blocks * 128
            samples = None
            if status == 0:
                samples = np.frombuffer(out, np.uint8, pk.blocks * 64, at).reshape(pk.blocks, 64)
                at += pk.blocks * 64
            results.append((status, coef, samples))
        assert at == len(out)
        return results
    return run


def _ref_blocks(data):
    """(coefficients [blocks, 64], samples [blocks, 64], status) of the restatement, blocks in the workspace's order; None if it refuses."""
    try:
        p = R.parse(data)
    except (ValueError, AssertionError, IndexError):
        return None
    planes, status = R.decode_coefficients(data, p)
    coef = np.concatenate([c.reshape(-1, 64) for c in planes])
    samples = np.concatenate([R.idct_plane(planes[c], p["quant"][c]).reshape(planes[c].shape[0], 8, planes[c].shape[1], 8)
                              .transpose(0, 2, 1, 3).reshape(-1, 64) for c in range(p["ncomp"])]) if status == 0 else None
    return coef, samples, status


def damaged_variants(name):
    """The damaged copies of a case the sanitizer program decodes: [(label, stream)]."""
    data = R.fixture()[name][0]
    a, b = R.scan_range(data)
    cuts = {0, 1, (b - a) // 3, (b - a) // 2, b - a - 1}
    stuffed = data.find(b"\xff\x00", a, b)
    if stuffed >= 0:
        cuts.add(stuffed + 1 - a)          # right after an FF
    out = [(f"truncate {c}", R.damage(data, "truncate", c)) for c in sorted(c for c in cuts if 0 <= c < b - a)]
    out += [(f"flip {seed}", R.damage(data, "flip", seed)) for seed in range(8)]
    out.append(("all FF", data[:a] + b"\xff" * (b - a) + data[b:]))
    out.append(("empty scan", data[:a] + data[b:]))
    return out


def test_host_build_of_the_decoder_under_the_sanitizers(probe):
    labels, streams = [], []
    for name in R.CASES:
        labels.append((name, "clean"))
        streams.append(R.fixture()[name][0])
        for label, data in damaged_variants(name):
            labels.append((name, label))
            streams.append(data)
    for name, kind, arg in R.DAMAGED_BATCH:          # the frames of the GPU test's damaged batch are among them
        labels.append((name, f"batch {kind} {arg}"))
        streams.append(R.damage(R.fixture()[name][0], kind, arg))
    results = probe(streams)
    flagged = refused = clean_after_damage = 0
    for (name, label), data, got in zip(labels, streams, results):
        want = _ref_blocks(data)
        if got is None or want is None:
            assert label != "clean" and not label.startswith("batch"), (name, label)
            refused += 1
            continue
        status, coef, samples = got
        assert (status != 0) == (want[2] != 0), (name, label, status, want[2])
        if label == "clean":
            assert status == 0, (name, status)
        if status == 0:
            assert np.array_equal(coef, want[0]) and np.array_equal(samples, want[1]), (name, label)
            clean_after_damage += label != "clean"
        else:
            flagged += 1
    print(f"{len(streams)} streams: {flagged} flagged, {clean_after_damage} damaged but decodable, {refused} refused by the parsers")
    assert flagged > len(R.CASES)
    batch = [_ref_blocks(R.damage(R.fixture()[n][0], k, a))[2] != 0 for n, k, a in R.DAMAGED_BATCH]
    assert batch == [False, False, True, False, True]
