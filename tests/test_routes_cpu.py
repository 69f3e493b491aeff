"""The route functions of vicasplat_amd/csrc/routes.h (gemm_plan, conv3x3_route, attention_route, attention_bwd_route, xcd_remap), compiled
for the host and run without a GPU.

tests/route_probe.cpp is built once per session with the host compiler; the tests then hold the header to its restatements:
  * tests/gemm_f64.py plan(), which names the routes of the GPU GEMM tests (there may be no compiler where those run): string for string
    over a grid of every class, epilogue, packing and M at every tile edge; and under VS_DETERMINISTIC no plan splits K;
  * the halo column of tests/test_conv_halo_gpu.py CASES and a table of pinned convolution shapes, one at least per route kind;
  * PACKED_CONV_MIN_PIXELS of model/encoder/heads/dpt.py: the trunk writes its last map packed exactly where the head's first convolution
    reads a packed input (the 256 x 128 tile kernel), and never where the library would refuse one;
  * the ids of tests/attention_route_cases.py: every GPU attention case reaches the route its id names, every route is reached, and a table
    of pinned shapes sits on both sides of every attention threshold;
  * xcd_remap is a permutation of [0, n) that hands every XCD one contiguous range of logical ids, for every grid size tried.
"""
import os
import shutil
import subprocess

import pytest

import gemm_f64
from attention_route_cases import CASES as ATTN_CASES, PERMUTE_CASES
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


# ---- attention -----------------------------------------------------------------------------------------------------------------------
ATTN_ROUTE_OF_PREFIX = {"res": "res", "k1": "tile64", "k2": "tile128", "split1": "split64", "split2": "split128", "sp": "sp"}
ATTN_KINDS = ("res", "tile64", "tile128", "f32", "split64", "split128", "sp")


def _attn_query(cls, kw):
    """What make_case hands the ABI for these keywords: Lk = Lq when none is given; with key segments Lk = 0 and the lengths in kv_seg."""
    seg, masked = kw.get("seg") is not None, kw.get("mask", "none") != "none"
    Lk = 0 if seg else kw.get("Lk", kw["Lq"])
    return "a %s %d %d %d %d %d %d" % (cls, kw["nbatch"], kw["H"], kw["Lq"], Lk, seg, masked)


def _attn_expected(cid, cls, kw):
    prefix = cid.split("-")[0]
    if prefix in ATTN_ROUTE_OF_PREFIX:
        return ATTN_ROUTE_OF_PREFIX[prefix]
    assert prefix in ("sweep", "fam"), cid
    if cls in ("f16", "bf16"):
        plain = kw.get("seg") is None and kw.get("mask", "none") == "none"
        return "res" if plain and kw.get("Lk", kw["Lq"]) <= 320 and kw["Lq"] <= 384 else "tile64"
    return {"f32x": "f32", "split": "split64", "sp": "sp"}[cls]


def test_every_gpu_attention_case_reaches_the_route_its_id_names(probe):
    cases = [(cid, cls, kw) for cid, classes, kw in ATTN_CASES for cls in classes] + list(PERMUTE_CASES)
    got = [g.split()[0] for g in probe([_attn_query(cls, kw) for _, cls, kw in cases])]
    want = [_attn_expected(cid, cls, kw) for cid, cls, kw in cases]
    assert got == want, [(c[0], c[1], g, w) for c, g, w in zip(cases, got, want) if g != w]
    assert set(got) == set(ATTN_KINDS), set(ATTN_KINDS) - set(got)


# (class, nbatch, H, Lq, Lk, has_seg, has_len) -> the route, worked out by hand from the thresholds: resident up to 320 keys and 384 queries
# without mask or segments; 128-query tiles from 512 workgroups of them and Lk_eff > 1024 (16-bit) / > 256 (split), Lk_eff = 2 Lk with segments
ATTN_PINS = [
    (("f16", 2, 3, 384, 320, 0, 0), "res grid=1x3x2 block=512"),
    (("f16", 2, 3, 384, 321, 0, 0), "tile64 grid=6x3x2"),
    (("f16", 2, 3, 385, 320, 0, 0), "tile64 grid=7x3x2"),
    (("f16", 2, 3, 384, 320, 0, 1), "tile64 grid=6x3x2"),
    (("f16", 4, 16, 1024, 1025, 0, 0), "tile128 grid=8x16x4"),          # exactly 512 workgroups
    (("f16", 4, 16, 1024, 1024, 0, 0), "tile64 grid=16x16x4"),
    (("f16", 3, 16, 1032, 1032, 0, 0), "tile64 grid=17x16x3"),          # 432 workgroups of 128 queries
    (("split", 11, 16, 257, 257, 0, 0), "split128 grid=3x16x11"),       # 528
    (("split", 11, 16, 257, 256, 0, 0), "split64 grid=5x16x11"),
    (("split", 10, 16, 257, 257, 0, 0), "split64 grid=5x16x10"),        # 480
    (("split", 11, 16, 257, 129, 1, 0), "split128 grid=3x16x11"),       # Lk_eff = 258
    (("split", 11, 16, 257, 0, 1, 0), "split64 grid=5x16x11"),          # what every caller passes with segments
]


def test_pinned_attention_shapes_take_their_route(probe):
    got = probe(["a %s %d %d %d %d %d %d" % s for s, _ in ATTN_PINS])
    assert got == [r for _, r in ATTN_PINS], [(s, g, r) for (s, r), g in zip(ATTN_PINS, got) if g != r]
    lqs = (1, 95, 96, 97, 1032)
    assert probe(["a sp 2 2 %d %d 0 0" % (L, L) for L in lqs]) == ["sp grid=%d" % n for n in (4, 4, 4, 8, 44)]


def test_backward_grids(probe):
    """keys = max_keys under segments, Lk otherwise; dq in 128-query tiles; dk|dv in 128-key (16-bit) / 64-key (split) tiles."""
    q = ["b 16 257 257 0 0", "b 16 257 0 1 514", "b split 257 257 0 0", "b split 129 0 1 65", "b 16 128 128 0 0", "b split 128 64 0 0"]
    assert probe(q) == ["keys=257 dq=3 dkv=3", "keys=514 dq=3 dkv=5", "keys=257 dq=3 dkv=5", "keys=65 dq=2 dkv=2", "keys=128 dq=1 dkv=1",
                        "keys=64 dq=1 dkv=1"]


def test_xcd_remap_is_a_permutation_with_one_range_per_xcd(probe):
    """Otherwise two workgroups would compute one tile and one tile would never be computed, or the tiles of one XCD would not be neighbours."""
    ns = set(range(1, 4097)) | {256 * k + d for k in range(1, 65) for d in (-1, 0, 1)}
    # grids of the 8-scene bench step: 96-query tiles x 16 heads x 192 frames; 256-pixel conv tiles of 192 maps of 64 x 64; 2^20 rows / 256
    ns |= {3 * 16 * 192, 3 * 12 * 192, 22 * 16 * 24, 3072, 12288, 4096 * 3, 65535, 1 << 20}
    ns = sorted(ns)
    got = probe(["x %d" % n for n in ns])
    assert got == ["ok"] * len(ns), [(n, g) for n, g in zip(ns, got) if g != "ok"][:5]
