"""ctypes binding of libvicasplat_hip.so (the C ABI declared in the public headers of include/, listed once in HEADERS, DATA_HEADERS, DRAW_HEADERS and IO_HEADERS).

The product path has NO CPU fallback: if the shared library is missing or a tensor is not on a HIP device the
call raises.  PyTorch is used only for device memory (caching allocator) and streams.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# Every public header of include/, as (prefix of its entries, file name), in the order the headers were added: the one statement of the list.
# The signatures (parse_header), the integer constants (header_constants) and build()'s staleness check all read it.
HEADERS = (
    ("vs_", "vicasplat_hip.h"),          # the kernels of the model and the rasterizer; vs_abi_version, vs_last_error
    ("vsd_", "vicasplat_distill.h"),     # csrc/distill.hip
    ("vsl_", "vicasplat_loss.h"),        # csrc/depth_loss.hip
    ("vst_", "vicasplat_teacher.h"),     # csrc/teacher.hip
    ("vsm_", "vicasplat_metrics.h"),     # csrc/trajectory.hip
    ("vsp_", "vicasplat_data.h"),        # csrc/preprocess.hip
    ("vsv_", "vicasplat_viz.h"),         # csrc/viz.hip
    ("vso_", "vicasplat_overlap.h"),     # csrc/overlap.hip
)
# The headers added beside that family without a change of the ABI version: the same library, parser and binding; HEADERS and its pinned
# entry counts stay as they are.
DATA_HEADERS = (
    ("vsj_", "vicasplat_jpeg.h"),        # csrc/jpeg.hip, csrc/jpeg_decode.h
)
# The presentation layer's header, added the same way (a table of its own: DATA_HEADERS is the data path's and stays as it is).
DRAW_HEADERS = (
    ("vsg_", "vicasplat_draw.h"),        # csrc/draw.hip
)
ALL_HEADERS = HEADERS + DATA_HEADERS + DRAW_HEADERS
# The file-output header, added the same way once more; ALL_HEADERS is pinned as the three tables above, so the binding runs over BOUND_HEADERS.
IO_HEADERS = (
    ("vse_", "vicasplat_png.h"),         # csrc/png.hip, csrc/png_deflate.h
)
BOUND_HEADERS = ALL_HEADERS + IO_HEADERS


def header_path(prefix: str) -> str:
    """The path of the public header whose entries carry `prefix`."""
    return os.path.join(_HERE, "..", "include", dict(BOUND_HEADERS)[prefix])


_SO = os.environ.get("VICASPLAT_HIP_LIB") or os.path.join(_HERE, "libvicasplat_hip.so")   # (override: A/B runs of two builds)
_lock = threading.Lock()
ABI_VERSION = 10    # == vs_abi_version() of csrc/api.hip; INTEGRATION.md lists the entries of every version
_lib = None
_entries: dict = {}    # name -> (bound function, takes the stream as its last argument), filled by _load() from the header


def header_constants(path: str, prefix: str) -> dict:
    """{name: value} of the integer constants of a public header whose names carry `prefix`, its `#define NAME <int>` lines and its enum
    members written `NAME = <int>`: the header states them once."""
    with open(path) as f:
        text = f.read()
    name = re.escape(prefix) + r"\w+"
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define (%s) (-?\d+)\s*$" % name, text, flags=re.M)}
    for body in re.findall(r"\benum\b[^{;]*\{([^}]*)\}", re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)):
        consts.update((m.group(1), int(m.group(2))) for m in re.finditer(r"\b(%s)\s*=\s*(-?\d+)\s*(?:,|$)" % name, body))
    return consts


# every integer constant of every public header, under the header's own name: VS_BUF_*, VS_RASTER_*, VS_SSIM_*, VSP_*, VSV_*, VSO_*, VSJ_*, VSG_*, VSE_*
for _prefix, _ in BOUND_HEADERS:
    globals().update(header_constants(header_path(_prefix), _prefix.upper()))

AllocFn = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_int32, C.c_size_t)


class VsRasterIn(C.Structure):
    _fields_ = [
        ("num_cameras", C.c_int32), ("num_scenes", C.c_int32), ("P", C.c_int32), ("sh_degree", C.c_int32),
        ("sh_coeffs", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("flags", C.c_int32),
        ("means3D", C.c_void_p), ("cov3D", C.c_void_p), ("shs", C.c_void_p), ("colors_precomp", C.c_void_p),
        ("opacities", C.c_void_p), ("cam_scene", C.c_void_p), ("viewmatrix", C.c_void_p), ("projmatrix", C.c_void_p),
        ("campos", C.c_void_p), ("tanfov", C.c_void_p), ("background", C.c_void_p), ("capacity", C.c_int64),
    ]


class VsRasterOut(C.Structure):
    _fields_ = [
        ("color", C.c_void_p), ("depth", C.c_void_p), ("opacity", C.c_void_p), ("radii", C.c_void_p),
        ("n_touched", C.c_void_p), ("num_rendered", C.c_int64), ("buffers", C.c_void_p * VS_BUF_COUNT),
    ]


class VsRasterGrads(C.Structure):
    _fields_ = [
        ("dL_dcolor", C.c_void_p), ("dL_ddepth", C.c_void_p), ("dL_dmeans3D", C.c_void_p), ("dL_dcov3D", C.c_void_p),
        ("dL_dshs", C.c_void_p), ("dL_dcolors_precomp", C.c_void_p), ("dL_dopacities", C.c_void_p),
        ("dL_dmeans2D", C.c_void_p), ("dL_dtau", C.c_void_p),
    ]


def build(force: bool = False) -> str:
    """Compile every HIP source for gfx950 (cross-compiles without a GPU)."""
    src_dir = os.path.join(_HERE, "csrc")
    newest = max(os.path.getmtime(os.path.join(src_dir, f)) for f in os.listdir(src_dir)
                 if f.endswith((".hip", ".h", "Makefile")))
    newest = max(newest, *(os.path.getmtime(header_path(prefix)) for prefix, _ in BOUND_HEADERS))
    if force or not os.path.exists(_SO) or os.path.getmtime(_SO) < newest:
        subprocess.check_call(["make", "-C", src_dir, "-j8"], stdout=subprocess.DEVNULL)
    return _SO


_C_TYPES = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
            "vs_stream_t": C.c_void_p, "VsAllocFn": AllocFn}
_C_RETURNS = {"int": C.c_int, "int64_t": C.c_int64, "const char *": C.c_char_p}
_STRUCTS = {"VsRasterIn": VsRasterIn, "VsRasterOut": VsRasterOut, "VsRasterGrads": VsRasterGrads}


def parse_header(text: str, prefix: str = "vs_") -> dict:
    """{name: (restype, [argtypes], takes_stream)} of every prototype in the text of the header whose entries carry `prefix` (HEADERS).  The
    header is the one place where a signature is written down; a prototype without the prefix, or a type outside the small vocabulary
    below, raises with the prototype's text (ctypes' default conversion would truncate or shift the arguments silently)."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*|^\s*#[^\n]*", "", text, flags=re.S | re.M)
    text = re.sub(r'extern\s+"C"\s*\{|\b(?:typedef\s+struct|enum)\b[^{;]*\{[^}]*\}[^;]*;|\btypedef\b[^;{]*;', "", text)
    header = dict(BOUND_HEADERS).get(prefix, f"header of the {prefix} entries")
    sigs = {}
    for proto in (" ".join(p.split()) for p in text.split(";")):
        if proto in ("", "}"):
            continue
        m = re.fullmatch(r"(.+?)\b(%s\w+) ?\((.*)\)" % re.escape(prefix), proto)
        ret = m and m.group(1).strip()
        if not m or ret not in _C_RETURNS:
            raise ValueError(f"{header}: cannot parse the prototype `{proto}`")
        params = [] if m.group(3).strip() == "void" else [p.strip() for p in m.group(3).split(",")]
        argtypes = []
        for p in params:
            base = re.sub(r"\bconst\b|\w+$", "", p).replace(" ", "")      # the type without qualifiers and without the parameter's name
            if base.endswith("*"):
                argtypes.append(C.POINTER(_STRUCTS[base[:-1]]) if base[:-1] in _STRUCTS else C.c_void_p)
            elif base in _C_TYPES:
                argtypes.append(_C_TYPES[base])
            else:
                raise ValueError(f"{header}: unknown type `{p}` in the prototype `{proto}`")
        sigs[m.group(2)] = (_C_RETURNS[ret], argtypes, bool(params) and params[-1].startswith("vs_stream_t "))
    return sigs


def lib() -> C.CDLL:
    """The loaded C-ABI library (see _load)."""
    return _lib if _lib is not None else _load()


def _load() -> C.CDLL:
    """Load the C-ABI library and bind every entry point to the signature the header declares; raise loudly when it is absent (no silent
    fallback)."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(_SO):
                raise RuntimeError(
                    f"{_SO} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                    "(vicasplat_amd has no CPU / PyTorch fallback path)")
            L = C.CDLL(_SO)
            if L.vs_abi_version() != ABI_VERSION:     # the ctypes mirrors of the structs above are for exactly this layout
                raise RuntimeError(f"{_SO} has ABI version {L.vs_abi_version()}, this package needs {ABI_VERSION}: rebuild it (python -c 'import __graft_entry__ as g; g.build()')")
            sigs = {}
            for prefix, _ in BOUND_HEADERS:
                with open(header_path(prefix)) as f:
                    sigs.update(parse_header(f.read(), prefix=prefix))
            for name, (restype, argtypes, takes_stream) in sigs.items():
                fn = getattr(L, name)
                fn.restype, fn.argtypes = restype, argtypes
                _entries[name] = (fn, takes_stream)
            _lib = L
    return _lib


def call(name: str, dev: torch.device, *args):
    """Run the entry point `name` on `dev`: on the device's current stream (passed as the last argument where the header declares a
    vs_stream_t there), raising with the entry's own name and the library's message on a negative return.  Returns the entry's value."""
    if _lib is None:
        _load()
    fn, takes_stream = _entries[name]
    with torch.cuda.device(dev):
        rc = fn(*args, torch.cuda.current_stream(dev).cuda_stream) if takes_stream else fn(*args)
    return rc if rc >= 0 else check(rc, name)


def check(rc: int, what: str) -> int:
    if rc < 0:
        raise RuntimeError(f"{what}: {lib().vs_last_error().decode()}")
    return rc


def require_device(*tensors: torch.Tensor) -> torch.device:
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("vicasplat_amd kernels need HIP device tensors (got a CPU tensor); there is no CPU fallback")
        dev = dev or t.device
        if t.device != dev:
            raise RuntimeError("all tensors must live on the same device")
    return dev


def stream_ptr(device: torch.device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t) -> C.c_void_p:
    return C.c_void_p(None) if t is None else C.c_void_p(t.data_ptr())


class TorchAllocator:
    """VsAllocFn backed by the PyTorch caching allocator; keeps the tensors alive, indexed by tag."""

    def __init__(self, device: torch.device):
        self.device = device
        self.tensors: dict[int, torch.Tensor] = {}
        self.fn = AllocFn(self._alloc)

    def _alloc(self, _ctx, tag, nbytes):
        t = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        self.tensors[int(tag)] = t
        return t.data_ptr()
