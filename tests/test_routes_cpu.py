"""The forward route functions of vicasplat_amd/csrc/routes.h (gemm_plan, conv3x3_route), compiled for the host and run without a GPU.

tests/route_probe.cpp is built once per session with the host compiler; the tests then hold the header to its three restatements:
  * tests/gemm_f64.py plan(), which names the routes of the GPU GEMM tests (there may be no compiler where those run): string for string
    over a grid of every class, epilogue, packing and M at every tile edge; and under VS_DETERMINISTIC no plan splits K;
  * the halo column of tests/test_conv_halo_gpu.py CASES and a table of pinned convolution shapes, one at least per route kind;
  * PACKED_CONV_MIN_PIXELS of model/encoder/heads/dpt.py: the trunk writes its last map packed exactly where the head's first convolution
    reads a packed input (the 256 x 128 tile kernel), and never where the library would refuse one.
"""
import os
import shutil
import subprocess

import pytest

import gemm_f64
from test_conv_halo_gpu import CASES as HALO_CASES
from vicasplat_amd.model.encoder.heads.dpt import pts3d_route

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="session")
def probe(tmp_path_factory):
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    cxx = shutil.which("c++") or (rocm_clang if os.path.exists(rocm_clang) else None)
    assert cxx, "no host C++ compiler (c++ or ROCm's clang++): routes.h cannot be checked"
    exe = str(tmp_path_factory.mktemp("route_probe") / "route_probe")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-O1", "-o", exe, os.path.join(HERE, "route_probe.cpp")], check=True)

    def ask(queries):
        out = subprocess.run([exe], input="".join(q + "\n" for q in queries), capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(queries)
        return out
    return ask


# ---- GEMM ----------------------------------------------------------------------------------------------------------------------------
NS = (16, 64, 128, 192, 256, 768, 1024, 3072, 4096)
KS = (32, 64, 96, 128, 512, 1024, 4096)


def _ms():
    ms = set(range(1, 1101)) | {2056, 16684} | {c.M for c in gemm_f64.CASES}
    for k in range(1, 70000 // 256 + 1):
        ms |= {256 * k - 1, 256 * k, 256 * k + 1}
    return sorted(ms)


def _variants(cls):
    """(epi, resid, a_packed, out_packed) the entries of a class accept: vs_gemm_bias_act 0..3, vs_gemm_resid (2 with resid), vs_gemm_qkv_rope
    (4); the split class adds epilogue 5 (z in resid), a packed A (epilogues 0..4) and a packed output (epilogues 0 / 1 / 3 / 4, N % 64 == 0)."""
    base = [(0, False), (1, False), (2, False), (2, True), (3, False), (4, False)]
    if cls != "split":
        return [(e, r, False, False) for e, r in base]
    v = [(e, r, ap, False) for e, r in base for ap in (False, True)] + [(5, True, False, False)]
    return v + [(e, False, ap, True) for e in (0, 1, 3, 4) for ap in (False, True)]


def _grid():
    for cls in gemm_f64.CLASSES:
        for K in KS:
            if K % (32 if cls in ("f32x", "split") else 64):      # gemm_entry: K % 32 == 0 for f32 rows, K % 64 == 0 in 2-byte units
                continue
            for N in NS:
                for epi, resid, ap, op in _variants(cls):
                    if op and N % 64:
                        continue
                    yield cls, N, K, epi, resid, ap, op


def test_gemm_plan_equals_the_python_plan_over_the_grid(probe):
    ms, total = _ms(), 0
    for cls, N, K, epi, resid, ap, op in _grid():
        got = probe(["g %s %d %d %d %d %d %d %d 0" % (cls, M, N, K, epi, resid, ap, op) for M in ms])
        want = [gemm_f64.plan(cls, M, N, K, epi, resid, ap, op) for M in ms]
        if got != want:
            i = next(i for i in range(len(ms)) if got[i] != want[i])
            raise AssertionError(("routes.h", got[i], "plan()", want[i], cls, ms[i], N, K, epi, resid, ap, op))
        total += len(ms)
    print(f"gemm_plan == plan() on {total} combinations ({len(ms)} row counts)")
    assert total > 1_000_000


def test_deterministic_plans_never_split_k(probe):
    ms, split_somewhere = _ms(), 0
    for cls, N, K, epi, resid, ap, op in _grid():
        if epi != 2 or resid:
            continue          # (test_gemm_plan_...: only epilogue 2 with the residual in `out` splits K at all)
        q = "g %s %%d %d %d %d %d %d %d %%d" % (cls, N, K, epi, resid, ap, op)
        assert all(gemm_f64.plan_ksplit(p) == 1 for p in probe([q % (M, 1) for M in ms])), (cls, N, K, ap, op)
        split_somewhere += any(gemm_f64.plan_ksplit(p) > 1 for p in probe([q % (M, 0) for M in ms]))
    assert split_somewhere > 0


# ---- 3x3 convolution -----------------------------------------------------------------------------------------------------------------
# (dtype, images, H, W of the output, Cin, Cout, stride, packed input) -> the route, worked out by hand from the thresholds: 256 x 256 tiles
# from 150 (split) / 224 (other classes) tiles of 256 pixels and an even number of 64-unit K-tiles; 256 x 128 tiles (split, Cout 128) from 224;
# the 4-wave kernel below: MI = 8 from 512 (split) / 256 tiles of 256 x 128, MI = 2 (split) up to 192 tiles of 128 x 128, MI = 4 otherwise
PINS = [
    ((4, 192, 64, 64, 256, 256, 1, 0), "halo256 kpt=8 grid=3072"),         # the bench step's trunk convolutions
    ((4, 192, 8, 8, 256, 256, 1, 0), "wave4 mi=2 grid=384"),               # ... its 8 x 8 maps: 48 tiles of 256 x 256
    ((4, 8, 16, 16, 256, 256, 1, 0), "wave4 mi=2 grid=64"),                # one 8-view scene: 2 048 pixels
    ((4, 150, 16, 16, 256, 256, 1, 0), "halo256 kpt=8 grid=150"),          # the 150-tile threshold ...
    ((4, 149, 16, 16, 256, 256, 1, 0), "wave4 mi=4 grid=596"),
    ((4, 600, 8, 8, 256, 256, 1, 0), "tile256 kpt=8 grid=150"),            # ... on maps the halo body does not take
    ((4, 596, 8, 8, 256, 256, 1, 0), "wave4 mi=4 grid=596"),
    ((4, 150, 16, 16, 256, 256, 1, 1), "tile256 kpt=8 grid=150"),          # a packed input: never the halo body
    ((4, 150, 16, 16, 192, 256, 1, 0), "halo256 kpt=6 grid=150"),          # six K-tiles per tap: no power of two
    ((4, 150, 16, 16, 96, 256, 1, 0), "wave4 mi=4 grid=600"),              # 27 K-tiles: odd
    ((4, 150, 16, 16, 768, 768, 2, 0), "tile256 kpt=24 grid=450"),         # stride 2
    ((4, 300, 16, 16, 96, 256, 1, 1), "packed_not_taken"),                 # packed and no power of two: the refusal
    ((4, 224, 16, 16, 256, 128, 1, 0), "tile256x128 kpt=8 grid=224"),      # the 224-tile threshold of the 128-wide head convolution ...
    ((4, 224, 16, 16, 256, 128, 1, 1), "tile256x128 kpt=8 grid=224"),
    ((4, 223, 16, 16, 256, 128, 1, 0), "wave4 mi=4 grid=446"),
    ((4, 223, 16, 16, 256, 128, 1, 1), "packed_not_taken"),                # ... below which a packed input is refused
    ((4, 256, 16, 16, 32, 256, 1, 0), "wave4 mi=8 grid=512"),              # 9 K-tiles (odd): 512 tiles of 256 x 128
    ((1, 224, 16, 16, 256, 256, 1, 0), "tile256 kpt=4 grid=224"),          # the 224-tile threshold of the other classes
    ((2, 223, 16, 16, 256, 256, 1, 0), "wave4 mi=8 grid=446"),
    ((1, 127, 16, 16, 64, 256, 1, 0), "wave4 mi=4 grid=508"),              # one K-tile per tap (odd): 254 tiles of 256 x 128
    ((2, 128, 16, 16, 64, 256, 1, 0), "wave4 mi=8 grid=256"),
    ((3, 224, 16, 16, 128, 256, 1, 0), "tile256 kpt=4 grid=224"),
    ((3, 223, 16, 16, 128, 256, 1, 0), "wave4 mi=4 grid=892"),             # the f32 class has one 4-wave tile height
]
KINDS = ("halo256", "tile256", "tile256x128", "wave4 mi=2", "wave4 mi=4", "wave4 mi=8", "packed_not_taken")


def _conv(probe, shapes):
    return probe(["c %d %d %d %d %d %d %d %d" % s for s in shapes])


def test_pinned_conv_shapes_take_their_route(probe):
    got = _conv(probe, [s for s, _ in PINS])
    assert got == [r for _, r in PINS], [(s, g, r) for (s, r), g in zip(PINS, got) if g != r]
    for kind in KINDS:
        assert any(g == kind or g.startswith(kind + " ") for g in got), kind


def test_halo_cases_state_their_route(probe):
    got = _conv(probe, [(4, N, H, W, Cin, 256, 1, 0) for _, N, H, W, Cin, _ in HALO_CASES])
    for (case, *_, halo), g in zip(HALO_CASES, got):
        assert g.startswith("halo256 ") == halo, (case, g)


def test_trunk_writes_packed_exactly_where_the_head_convolution_reads_it(probe):
    """pts3d_route's trunk_packed against the route of head[0]: split class, BT * 64 gh gw pixels, c_trunk -> 128 channels, packed input."""
    shapes = [(BT, gh, gw, c) for BT in range(1, 65) for gh in range(1, 25) for gw in range(1, 25) for c in (32, 64, 96, 128, 256)]
    keys = sorted({(BT * gh * gw, c) for BT, gh, gw, c in shapes})
    route = dict(zip(keys, _conv(probe, [(4, n, 8, 8, c, 128, 1, 1) for n, c in keys])))
    packed = 0
    for BT, gh, gw, c in shapes:
        r, trunk_packed = route[BT * gh * gw, c], pts3d_route("split", BT, gh, gw, c, 128, 128)[1]
        assert trunk_packed == r.startswith("tile256x128 "), (BT, gh, gw, c, r)
        assert not (trunk_packed and r == "packed_not_taken")
        packed += trunk_packed
    assert 0 < packed < len(shapes)
