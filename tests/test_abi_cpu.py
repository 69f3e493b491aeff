"""The C-ABI library builds for gfx950 without a GPU, loads, and exports every symbol include/*.h declares.
No compute calls here (CPU suite).  Also: argument validation returns an error code + message, never crashes."""
import ctypes as C
import glob
import os
import re

import pytest

from vicasplat_amd._lib import HEADERS as HEADER_TABLE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


ENTRY_COUNTS = {"vs_": 78, "vsd_": 3, "vsl_": 3, "vst_": 1, "vsm_": 1, "vsp_": 1, "vsv_": 5, "vso_": 1}     # pinned: 93 entries in all


def _header_text(prefix="vs_"):
    from vicasplat_amd import _lib
    return open(_lib.header_path(prefix)).read()


def _entry_like_names(prefix, text):
    """Names carrying `prefix` and followed by `(` in a header's text, /* */ comments stripped."""
    return set(re.findall(r"\b(%s[a-z0-9_]+)\s*\(" % re.escape(prefix), re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


def _declared_symbols():
    from vicasplat_amd import _lib
    syms = set()
    for prefix, _ in _lib.HEADERS:
        syms |= _entry_like_names(prefix, _header_text(prefix))
    return syms


def test_library_exports_every_declared_symbol():
    from vicasplat_amd import _lib
    so = _lib.build()
    assert os.path.exists(so)
    L = C.CDLL(so)
    syms = _declared_symbols()
    assert len(syms) == sum(ENTRY_COUNTS.values()) == 93
    assert {"vs_raster_forward", "vs_raster_backward", "vs_rope2d", "vs_gemm_bias_act", "vs_attention", "vs_layernorm_mod",
            "vs_rope_qk", "vs_gaussian_adapter", "vs_last_error", "vs_abi_version"} <= syms
    missing = [s for s in sorted(syms) if not hasattr(L, s)]
    assert not missing, missing
    assert _lib.lib().vs_abi_version() == _lib.ABI_VERSION
    # the documented version is the library's (INTEGRATION.md said 7 while the library said 6)
    doc = open(os.path.join(os.path.dirname(__file__), '..', 'INTEGRATION.md')).read()
    assert f'(ABI {_lib.ABI_VERSION})' in doc


def test_argument_validation_reports_errors():
    from vicasplat_amd import _lib
    L = _lib.lib()
    rc = L.vs_rope2d(None, None, 1, 1, 1, 64, 64, 64, 100.0, 1.0, 0, None)
    assert rc < 0 and b"null" in L.vs_last_error()
    rc = L.vs_gemm_bias_act(C.c_void_p(16), C.c_void_p(16), None, C.c_void_p(16), None, 4, 4, 30, 32, 32, 4, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, None)
    assert rc < 0 and b"multiple of 64" in L.vs_last_error()
    rc = L.vs_raster_forward(None, None, _lib.AllocFn(lambda a, b, c: 0), None, None)
    assert rc < 0


def test_product_package_never_imports_the_oracle():
    """oracle/ is test infrastructure: nothing under vicasplat_amd/ may import it."""
    bad = []
    for f in glob.glob(os.path.join(ROOT, "vicasplat_amd", "**", "*.py"), recursive=True):
        src = open(f).read()
        if re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M):
            bad.append(f)
    assert not bad, bad


def test_python_constants_mirror_the_header_enums():
    """The ctypes side indexes VsRasterOut.buffers and sets VsRasterIn.flags by number: the numbers are the header's.  So are the tap limit
    and the layout codes of the data header, and the launch geometry, limits, modes and output types of the viz and overlap headers."""
    from vicasplat_amd import _lib
    from vicasplat_amd.dataset.shims import crop_shim
    hdr = _header_text()
    enums = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(VS_(?:BUF|RASTER)_[A-Z_0-9]+)\s*=\s*(\d+)", hdr)}
    assert enums["VS_BUF_COUNT"] == 13 and enums["VS_BUF_CHECKPOINT"] == 12
    for name, val in enums.items():
        assert hasattr(_lib, name), name
        assert getattr(_lib, name) == val, (name, getattr(_lib, name), val)
    for name in ("VS_BUF_GEOM", "VS_BUF_CHECKPOINT", "VS_BUF_COUNT", "VS_RASTER_SAVE_FOR_BACKWARD", "VS_RASTER_SH_RGB_MAJOR", "VS_RASTER_COV_3X3"):
        assert hasattr(_lib, name) and name in enums, name
    assert C.sizeof(_lib.VsRasterOut) == 6 * 8 + enums["VS_BUF_COUNT"] * 8
    assert [getattr(_lib, "VS_BUF_" + n) for n in ("GEOM", "RECT", "CLAMPED", "TILE_RANGES", "TILE_CURSOR", "KEYS", "POINT_LIST", "SORT_SCRATCH",
                                                  "FINAL_T", "N_CONTRIB", "MISC", "DEPTH", "CHECKPOINT", "COUNT")] == list(range(14))
    assert (_lib.VS_RASTER_COUNT_TOUCHED, _lib.VS_RASTER_SAVE_FOR_BACKWARD, _lib.VS_RASTER_SH_RGB_MAJOR, _lib.VS_RASTER_COV_3X3) == (1, 2, 4, 8)
    assert (_lib.VS_SSIM_COMPONENTS, _lib.VS_SSIM_UNIT_WINDOW) == (1, 2)
    assert (_lib.VSP_MAX_TAPS, _lib.VSP_LAYOUT_U8_HWC, _lib.VSP_LAYOUT_U8_CHW, _lib.VSP_LAYOUT_F32_CHW) == (128, 0, 1, 2)
    assert (crop_shim.MAX_TAPS, crop_shim.LAYOUT_U8_HWC, crop_shim.LAYOUT_U8_CHW, crop_shim.LAYOUT_F32_CHW) == (128, 0, 1, 2)
    assert (_lib.VSV_THREADS, _lib.VSV_VEC, _lib.VSV_MAX_RANGE_N) == (256, 4, 16000000) and _lib.VSV_MAX_BLOCKS >= 1
    assert (_lib.VSV_MODE_DEPTH, _lib.VSV_MODE_MAX, _lib.VSV_MODE_UNIT, _lib.VSV_OUT_F32, _lib.VSV_OUT_U8) == (0, 1, 2, 0, 1)
    assert (_lib.VSO_THREADS, _lib.VSO_CHUNK) == (256, 2048)
    # the names a header gives and the names the module publishes are the same sets: 20 + 4 + 9 + 2
    per_header = {p: _lib.header_constants(_lib.header_path(p), p.upper()) for p, _ in _lib.HEADERS}
    assert {p: len(c) for p, c in per_header.items()} == {"vs_": 20, "vsd_": 0, "vsl_": 0, "vst_": 0, "vsm_": 0, "vsp_": 4, "vsv_": 9, "vso_": 2}
    for consts in per_header.values():
        for name, val in consts.items():
            assert getattr(_lib, name) == val, name


def test_every_prototype_of_the_header_is_bound_with_its_argument_list():
    """The ctypes signatures are read from the headers: every declared entry of every header has restype and argtypes on the loaded library, as many
    arguments as the prototype has parameters -- and nothing is left to ctypes' default conversion."""
    from vicasplat_amd import _lib
    L = _lib.lib()
    for prefix, _ in _lib.HEADERS:
        txt = re.sub(r"/\*.*?\*/", "", _header_text(prefix), flags=re.S)
        protos = {m.group(1): m.group(2) for m in re.finditer(r"\b(%s[a-z0-9_]+)\s*\(([^()]*)\)\s*;" % re.escape(prefix), txt)}
        assert set(protos) == _entry_like_names(prefix, txt) and len(protos) == ENTRY_COUNTS[prefix], prefix
        if prefix == "vs_":
            assert len(protos) == 78
        for name, params in protos.items():
            fn = getattr(L, name)
            n = 0 if params.strip() == "void" else params.count(",") + 1
            assert fn.argtypes is not None and len(fn.argtypes) == n, (name, fn.argtypes, n)
            assert fn.restype in (C.c_int, C.c_int64, C.c_char_p), (name, fn.restype)
    i32, i64, f32, vp = C.c_int32, C.c_int64, C.c_float, C.c_void_p
    # int vs_rope2d(void *tokens, const int64_t *pos, int32_t B, int32_t N, int32_t H, int32_t D, int64_t sB, int64_t sN, float base, float fwd,
    #               int32_t dtype, vs_stream_t stream) -- as INTEGRATION.md prints it
    assert L.vs_rope2d.restype is C.c_int
    assert L.vs_rope2d.argtypes == [vp, vp, i32, i32, i32, i32, i64, i64, f32, f32, i32, vp]
    # ... int32_t ldo, int64_t a_slice_stride, int64_t w_slice_stride, int64_t tap_out_stride, ..., void *workspace, int64_t workspace_bytes, ...
    assert L.vs_gemm_wgrad.restype is C.c_int
    assert L.vs_gemm_wgrad.argtypes == [vp, vp, vp, i32, i32, i32, i32, i32, i32, i64, i64, i64, vp, i32, i32, i32, vp, i64, i32, vp]
    assert L.vs_ssim_workspace_bytes.restype is C.c_int64 and L.vs_ssim_workspace_bytes.argtypes == [i32] * 6
    assert L.vs_raster_backward.argtypes == [C.POINTER(_lib.VsRasterIn), C.POINTER(_lib.VsRasterOut), C.POINTER(_lib.VsRasterGrads),
                                             _lib.AllocFn, vp, vp]


@pytest.mark.parametrize("prefix,name", HEADER_TABLE, ids=[n for _, n in HEADER_TABLE])
def test_each_public_header_parses_is_bound_and_is_documented(prefix, name):
    """What holds for every public header, asserted once: it parses with its own prefix into the pinned number of entries, each entry is bound
    on the loaded library as the parser read it and is named in INTEGRATION.md, and no other header's prefix gets into it."""
    from vicasplat_amd import _lib
    assert dict(_lib.HEADERS)[prefix] == name and os.path.samefile(_lib.header_path(prefix), os.path.join(ROOT, "include", name))
    text = _header_text(prefix)
    sigs = _lib.parse_header(text, prefix=prefix)
    assert len(sigs) == ENTRY_COUNTS[prefix] and all(n.startswith(prefix) for n in sigs), (name, len(sigs))
    assert set(sigs) == _entry_like_names(prefix, text), name
    L = _lib.lib()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for entry, (restype, argtypes, takes_stream) in sigs.items():
        fn = getattr(L, entry)
        assert fn.restype is restype and fn.argtypes == argtypes, (name, entry)
        assert _lib._entries[entry][0] is fn and _lib._entries[entry][1] == takes_stream, (name, entry)
        assert entry in doc, f"{name}: {entry} is not in INTEGRATION.md"
    for other, _ in _lib.HEADERS:
        if other != prefix:
            # no name of this header can be taken for an entry of another one, in code or in a // comment
            assert not _entry_like_names(other, text), (name, other)
            with pytest.raises(ValueError, match=re.escape(name) + ".*" + other + "x"):      # a prototype with a foreign prefix does not parse
                _lib.parse_header(f"int {other}x(int32_t n);", prefix=prefix)
    with pytest.raises(ValueError, match=re.escape(name) + ".*unsigned short n"):          # nor does a type outside the vocabulary
        _lib.parse_header(f"int {prefix}bad(unsigned short n);", prefix=prefix)
    assert L.vs_abi_version() == _lib.ABI_VERSION == 10


def test_header_parser_refuses_what_it_does_not_know():
    """An unknown type or an unparsable prototype is an error that quotes the prototype, never a silently defaulted argument."""
    from vicasplat_amd import _lib
    ok = _lib.parse_header("/* c */ int vs_x(const float *a, int64_t n, vs_stream_t stream);\nint64_t vs_y(int32_t n);")
    assert ok["vs_x"] == (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p], True) and ok["vs_y"] == (C.c_int64, [C.c_int32], False)
    with pytest.raises(ValueError, match=r"unsigned short n.*vs_bad"):
        _lib.parse_header("int vs_bad(const float *a, unsigned short n, vs_stream_t stream);")
    with pytest.raises(ValueError, match="vs_bad"):
        _lib.parse_header("struct Foo vs_bad(int32_t n);")
    with pytest.raises(ValueError, match="vs_bad"):
        _lib.parse_header("int vs_bad(int32_t n;")


def test_struct_mirrors_follow_the_header_field_by_field():
    """VsRasterIn / VsRasterOut / VsRasterGrads are hand-written ctypes mirrors: same field names in the same order as the header."""
    from vicasplat_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S)
    for name in ("VsRasterIn", "VsRasterOut", "VsRasterGrads"):
        body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), txt, flags=re.S).group(1)
        fields = []
        for decl in body.split(";"):
            if decl.strip():
                first, *more = decl.split(",")       # `int32_t width, height`: one declaration, two fields
                fields += [re.search(r"(\w+)\s*(?:\[\w+\])?\s*$", d).group(1) for d in [first] + more]
        assert fields == [f[0] for f in getattr(_lib, name)._fields_], (name, fields)
    assert len(_lib.VsRasterIn._fields_) == 20 and len(_lib.VsRasterGrads._fields_) == 9


def test_head_tail_refuses_an_input_that_is_not_a_relu_output():
    """the fused tail of a DPT head masks its input gradient by t > 0 and tells the producer to skip its ReLU backward -- only
    valid behind Conv3x3Fn(..., relu_out=True).  The producer is identified by its autograd node; anything else must not take the route."""
    import pytest
    import torch
    from vicasplat_amd import autograd as A
    t = torch.randn(32, 256, requires_grad=True) * 2.0          # produced by a multiplication, not by the ReLU convolution
    w = torch.randn(83, 256)
    assert not A.head_tail_ok(t, w)
    with pytest.raises(ValueError, match="relu_out=True"):
        A.head_tail(t, w, None, A.SPLIT)
    leaf = torch.randn(32, 256)                                   # outside any graph: no consumer of dt, shapes decide
    assert A.head_tail_ok(leaf, w)
