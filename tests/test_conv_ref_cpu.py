"""The case table and the float64 reference of tests/conv_f64.py, checked without a GPU:

  * routes: every 3x3 convolution case's hand-written route is the answer of csrc/routes.h (tests/route_probe.cpp, built as in
    test_routes_cpu.py); every route kind and every tile height of the 4-wave kernel is reached in every class that can reach it; every case
    reaches exactly the store paths of conv_epilogue it claims, by a restatement of the epilogue's conditions, and every path is reached in
    every class; the fused heads' routes follow conv_f64.head_route and cover every width, both dot kernels and the packed forms;
  * reference: conv_f64 against torch.nn.functional.conv2d / interpolate in float64 (1e-12 of the output scale) on every distinct shape of
    the table, both strides; the mask and residual2 arms and the heads' rounding points against direct formulas;
  * lattice: every lattice case's worst-case partial sum stays below its exactness limit;
  * buffers: the NaN guards and sentinels lie where build says, the batch alternates the distinct images, odd N included;
  * bounds: conv_f64.bound returns the constants of the tests it cites.
"""
import inspect
import math

import pytest
import torch
import torch.nn.functional as F

import conv_f64 as C
from conv_f64 import CASES, build, conv_f64
from test_routes_cpu import probe          # noqa: F401  (the session fixture that compiles tests/route_probe.cpp)

CONV = [c for c in CASES if c.entry == "conv3x3"]
HEADS = [c for c in CASES if c.entry in ("head1x1", "head_dot")]
UPS = [c for c in CASES if c.entry == "upsample2x"]


# ---- routes --------------------------------------------------------------------------------------------------------------------------
def test_every_conv_case_states_the_route_of_routes_h(probe):
    got = probe([C.probe_query(c) for c in CONV])
    wrong = [(c.id, c.route, g) for c, g in zip(CONV, got) if g != c.route]
    assert not wrong, wrong
    N, H, W, Cin, Cout = C.REFUSED_PACKED
    assert probe(["c 4 %d %d %d %d %d 1 1" % (N, H, W, Cin, Cout)]) == ["packed_not_taken"]
    # the packed-input identities compare with the f32-input run of the SAME kernel family
    for c in CONV:
        if c.packed:
            assert probe([C.probe_query(c, packed=False)]) == [c.route], c.id


def _kind(route):
    p = route.split()
    return p[0] + " " + p[1] if p[0] == "wave4" else p[0]


# what conv3x3_route can return per class: the f32 class has one 4-wave tile height (routes.h:147), the 16-bit classes two (148), the
# split class three (155-157) and the halo / 256 x 128 bodies (143, 151)
REACHABLE = {"f16": {"tile256", "wave4 mi=4", "wave4 mi=8"}, "bf16": {"tile256", "wave4 mi=4", "wave4 mi=8"}, "f32x": {"tile256", "wave4 mi=4"},
             "split": {"halo256", "tile256", "tile256x128", "wave4 mi=2", "wave4 mi=4", "wave4 mi=8"}}


def test_every_route_kind_and_tile_height_is_reached_in_every_class():
    for cls in C.CLASSES:
        assert {_kind(c.route) for c in CONV if c.cls == cls} == REACHABLE[cls], cls
        for stride in (1, 2):
            assert {_kind(c.route).split()[0] for c in CONV if c.cls == cls and c.stride == stride} >= {"tile256", "wave4"}, (cls, stride)
    assert {_kind(c.route).split()[0] for c in CONV if c.packed} == {"tile256", "tile256x128"}


def wave_path(cls, MI, Cout, M, mw0, nbase, out_al, res_al, res2_al, istep=16):
    """The store path one wave of conv_epilogue<cls, MI> takes (conv.hip:64-224), or None when it stores nothing.  *_al: the pointer's address
    modulo 16, None for a null pointer."""
    if mw0 >= M or nbase >= Cout:
        return None                                              # every row is skipped at conv.hip:158, every column at 170 / 212
    if cls in ("f16", "bf16"):
        vec_ok = Cout % 4 == 0 and nbase + 64 <= Cout and out_al % 8 == 0 and (res_al is None or res_al % 8 == 0)        # conv.hip:64-65
        if MI % 2 == 0 and vec_ok and Cout % 8 == 0 and out_al % 16 == 0 and mw0 + 16 * MI <= M:                         # conv.hip:69-70
            return "pair16"
        return "u2" if vec_ok else "scalar"                      # conv.hip:190 / 209
    if Cout % 4 == 0 and nbase + 64 <= Cout and mw0 + (MI - 1) * istep + 16 <= M and \
            (out_al | (res_al or 0) | (res2_al or 0)) % 16 == 0:                                                        # conv.hip:119-120
        return "f32x4"
    return "f32_tail4" if Cout % 4 == 0 else "scalar"            # conv.hip:180: a guarded float4 store per 4 columns, else single floats


def case_paths(c):
    """Every path some wave of some epilogue of the case takes: the tile geometry of the case's route (conv.hip:469-482 and 514, 626-638 and
    667, 751-765 and 894, 551-559 and 587)."""
    esz = 2 if c.cls in ("f16", "bf16") else 4
    Ho, Wo = C.out_hw(c)
    M = c.N * Ho * Wo
    p = c.route.split()
    if p[0] == "wave4":
        MI = int(p[1][3:])
        BM, BN, rows, ncol = 32 * MI, 128, 16 * MI, 2
    elif p[0] == "tile256x128":
        MI, BM, BN, rows, ncol = 4, 256, 128, 64, 2
    else:
        MI, BM, BN, rows, ncol = 8, 256, 256, 128, 4
    if p[0] == "halo256":
        waves = [((n * Ho + y0 + wr * 8) * Wo + x0, wc * 64, Wo) for n in range(c.N) for y0 in range(0, Ho, 16) for x0 in range(0, Wo, 16)
                 for wr in (0, 1) for wc in range(4)]
    else:
        waves = [(m0 + wr * rows, n0 + wc * 64, 16) for m0 in range(0, M, BM) for n0 in range(0, c.Cout, BN) for wr in range(BM // rows)
                 for wc in range(ncol)]
    assert len(waves) * 64 == int(p[-1].split("=")[1]) * (256 if p[0] == "wave4" else 512)          # the route's grid, in lanes
    found = set()
    for epi in c.epis:
        res = "res" in epi or epi == "mask"
        al = ((c.out_off * esz) % 16, (c.res_off * esz) % 16 if res else None, 0 if "res2" in epi else None)
        found |= {wave_path(c.cls, MI, c.Cout, M, mw0, nbase, *al, istep) for mw0, nbase, istep in waves}
    return found - {None}


@pytest.mark.parametrize("cls", C.CLASSES)
def test_every_case_reaches_the_epilogue_paths_it_claims(cls):
    reached = {}
    for c in (c for c in CONV if c.cls == cls):
        assert case_paths(c) == set(c.paths), (c.id, c.paths)
        for p in c.paths:
            reached.setdefault(p, set()).add(_kind(c.route).split()[0])
    want = {"pair16", "u2", "scalar"} if cls in ("f16", "bf16") else {"f32x4", "f32_tail4", "scalar"}
    assert set(reached) == want
    # the vector path and its fall-backs on the 4-wave kernel and on a tile route alike; Cout % 4 != 0 is a 4-wave shape (the tiles need Cout % 128 == 0)
    for p in want - {"scalar"}:
        assert {"wave4", "tile256"} <= reached[p], (cls, p, reached[p])
    # misaligned pointers: out by one element and by 8 bytes, residual likewise, on both
    for kind in ("wave4", "tile256"):
        offs = {(bool(c.out_off), bool(c.res_off), ((c.out_off or c.res_off) * (2 if cls in ("f16", "bf16") else 4)) % 8 == 0)
                for c in CONV if c.cls == cls and _kind(c.route).split()[0] == kind and (c.out_off or c.res_off)}
        assert offs == {(True, False, False), (True, False, True), (False, True, False), (False, True, True)}, (cls, kind)


def test_epilogues_on_every_route_and_class():
    for cls in C.CLASSES:
        for kind in REACHABLE[cls]:
            epis = set().union(*(c.epis for c in CONV if c.cls == cls and _kind(c.route) == kind and not c.packed))
            assert epis == set(C.EPIS) - (set() if cls == "split" else {"bias+res+res2"}), (cls, kind)
    for c in CONV:
        if c.packed:
            assert set(c.epis) == set(C.EPIS) - {"relu_in", "bias+res+res2"}          # ops.conv3x3_nhwc: a packed input carries its ReLU, no residual2


def test_small_shapes_of_the_4_wave_kernel():
    for cls in C.CLASSES:
        small = [c for c in CONV if c.cls == cls and c.route.startswith("wave4") and C.pixels(c) <= 129]
        assert {C.pixels(c) for c in small} >= {1, 15, 63, 64, 65, 129}
        assert {c.Cout for c in small} >= {64, 83, 128, 192, 320}
        assert {(c.H, c.W) for c in small} >= {(1, 1), (1, 15), (21, 1), (5, 7)}
        assert min(c.Cin for c in small) == (16 if cls == "f32x" else 32) and any(c.Cin == 96 for c in small)
        assert {(c.H % 2, c.W % 2) for c in small if c.stride == 2} == {(0, 0), (1, 1)}


def test_head_cases_follow_the_entry_points_rule():
    for c in HEADS:
        assert c.route == C.head_route(c.cls, c.entry, c.Cin, c.c2pad, c.packed), c.id
        assert C.pixels(c) % 256 == 0                                                    # one 256-pixel tile reaches them
    for cls in ("f16", "bf16", "split"):
        mine = [c for c in HEADS if c.cls == cls]
        assert {c.c2pad for c in mine if c.entry == "head1x1" and not c.packed} == {16, 32, 48, 64, 80, 96}
        assert all(c.n_out == c.c2pad - 13 for c in mine if c.entry == "head1x1")
        assert {(c.N, c.H, c.W) for c in mine if c.entry == "head1x1"} == set(C.HEAD_SHAPES)
        dots = {(c.route, c.n_out) for c in mine if c.entry == "head_dot"}
        routes = {"dot wave4 mi=8"} if cls != "split" else {"dot wave4 mi=8", "dot tile128", "dot tile128 packed"}
        assert dots == {(r, n) for r in routes for n in (1, 2, 3, 4)}
    assert {c.c2pad for c in HEADS if c.entry == "head1x1" and c.packed} == {16, 32, 48, 64, 80, 96}
    assert {c.Cin for c in HEADS if c.route == "dot wave4 mi=8" and c.cls == "split"} == {32, 96}
    assert math.prod(C.REFUSED_HEAD) % 256 != 0


def test_upsample_cases_cover_their_arms():
    for cls in ("f16", "bf16", "f32x"):
        mine = [c for c in UPS if c.cls == cls]
        assert {(c.H, c.W) for c in mine} >= {(h, w) for h in (1, 2, 3, 17) for w in (1, 2, 3, 17)}
        assert {c.Cin for c in mine} == ({4, 36, 64} if cls == "f32x" else {8, 40, 256})
        assert {c.N for c in mine} >= {1, 2, 3, 17}
        # vs_upsample2x_nhwc (conv.hip:1330, 1337, 1345): rows = N H (N 2 H in the H < 2 || W < 2 f32 kernel), grid.y = min(rows, 32768)
        big = [c for c in mine if c.route == "up z=2"]
        for c in big:
            rows = c.N * (2 * c.H if cls == "f32x" and (c.H < 2 or c.W < 2) else c.H)
            assert rows >= 32768 and (c.H < 2 or c.N * c.H >= 32768) and c.W == 2 and cdiv(rows, min(rows, 32768)) == 2
        assert {c.H >= 2 for c in big} == ({True, False} if cls == "f32x" else {True})
    for N, H, W, Cc in C.UPSAMPLE_PACKED:
        assert Cc % 32 == 0 and H >= 2 and W >= 2


def cdiv(a, b):
    return -(-a // b)


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _distinct(cases, key):
    seen = {}
    for c in cases:
        seen.setdefault(key(c), c)
    return list(seen.values())


def test_conv_f64_equals_conv2d_in_float64_on_every_shape():
    shapes = _distinct(CONV + HEADS, lambda c: (c.H, c.W, c.Cin, c.Cout, c.stride))
    assert {c.stride for c in shapes} == {1, 2}
    for case in shapes:
        c = build(case, "real")
        xn, w = c.x.double().permute(0, 3, 1, 2), c.w.double()
        for relu_in in (False, True):
            ref = F.conv2d(xn.clamp_min(0) if relu_in else xn, w, None, stride=c.stride, padding=1).permute(0, 2, 3, 1)
            got = C._conv_cached(c, relu_in)
            assert got.shape == ref.shape and _rel(got, ref) <= 1e-12, (case.id, relu_in)
        if case.entry != "conv3x3":
            continue
        conv, b, r1, r2 = C._conv_cached(c, False), c.bias.double(), c.r1.double(), c.r2.double()
        relu_conv = C._conv_cached(c, True)
        direct = {"none": conv, "bias": conv + b, "bias+res": conv + b + r1, "mask": conv * (r1 > 0), "relu_in": relu_conv,
                  "relu_out": F.relu(conv), "bias+res+res2": conv + b + r1 + r2}
        for epi in C.EPIS:
            assert _rel(conv_f64(c, epi), direct[epi]) <= 1e-12, (case.id, epi)
        m = conv_f64(c, "mask")
        assert bool((m[r1 <= 0] == 0).all()) and torch.equal(m[r1 > 0], conv[r1 > 0])


def test_head_f64_states_the_rounding_points():
    for case in _distinct(HEADS, lambda c: (c.cls, c.entry, c.Cin, c.H)):
        for family in ("lattice", "real"):
            c = build(case, family)
            conv = F.conv2d(c.x.double().permute(0, 3, 1, 2), c.w.double(), None, padding=1).permute(0, 2, 3, 1)
            for relu_out in (False, True):
                for with_bias in (False, True):
                    h = conv + c.bias.double() if with_bias else conv
                    if c.cls != "split":
                        h = (F.relu(h.to(c.dt)) if relu_out else h.to(c.dt)).double()          # round, then ReLU: the MFMA form's order
                    elif relu_out:
                        h = F.relu(h)
                    ref = F.linear(h, c.w2.double(), c.bias2.double())
                    got = conv_f64(c, (relu_out, with_bias))
                    assert _rel(got, ref) <= 1e-12, (case.id, family, relu_out, with_bias)
                    assert bool((got[..., c.n_out:] == 0).all())


def test_upsample_f64_equals_interpolate_in_float64():
    for case in _distinct(UPS, lambda c: (c.H, c.W, c.Cin, c.cls)):
        c = build(case, "real")
        xn = c.x.double().permute(0, 3, 1, 2)
        up = F.interpolate(xn, scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
        add = c.add.double()
        for mode, ref in (("none", up), ("add", up + add), ("relu_add", up + F.relu(add))):
            got = conv_f64(c, mode)
            assert got.shape == ref.shape and _rel(got, ref) <= 1e-12, (case.id, mode)
        if c.H == 1 and c.W == 1:
            assert torch.equal(conv_f64(c, "none"), c.x.double().expand(-1, 2, 2, -1))


# ---- lattice -------------------------------------------------------------------------------------------------------------------------
def test_every_lattice_case_is_exact_by_its_worst_case_bound():
    n = 0
    for case in CASES:
        if "lattice" not in case.families:
            continue
        for what, units, limit in C.lattice_units(case):
            assert units < limit, (case.id, what, units, limit)
        n += 1
    assert n >= len(CONV) + len(HEADS)
    # the bound's premises: the generated values stay in their ranges and are exact in bf16
    for case in (CONV[0], HEADS[0], next(c for c in UPS if "lattice" in c.families)):
        c = build(case, "lattice")
        L = C.LAT["head" if case in HEADS else "conv3x3"]
        pairs = [(c.x, L["x"])] + ([(c.add, L["r"])] if case in UPS else [(c.w, L["w"]), (c.bias, L["b"])])
        pairs += [(c.r1, L["r"]), (c.r2, L["r"])] if case in CONV else []
        pairs += [(c.w2, L["w2"]), (c.bias2, L["b2"])] if case in HEADS else []
        for t, (a, s) in pairs:
            v = t.double() * 2.0 ** s
            assert torch.equal(v, v.round()) and float(v.abs().max()) <= a and torch.equal(t.to(torch.bfloat16).double(), t.double())


# ---- buffers -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["wave4mi4-f16-m105_5x7", "wave4mi4-f32x-out+1", "wave4mi2-split-res+8B", "tile256-split-15x17", "wave4mi4-bf16-res+1"])
def test_build_leaves_guards_and_sentinels_where_it_says(cid):
    case = next(c for c in CONV if c.id == cid)
    for family in ("lattice", "real"):
        c = build(case, family)
        it = C.INT_OF[c.dt]
        Ho, Wo = C.out_hw(case)
        nx, g = case.N * case.H * case.W * case.Cin, 2 * case.W * case.Cin
        assert c.x_at == g and c.xbuf.numel() == nx + 2 * g and (g * c.xbuf.element_size()) % 16 == 0
        assert bool((c.xbuf[:g] == C.NAN_BITS[c.dt]).all()) and bool((c.xbuf[g + nx:] == C.NAN_BITS[c.dt]).all())
        assert bool(torch.isnan(c.xbuf[:g].view(c.dt)).all())
        xb = C.view_of(c.xbuf, c.x_at, (case.N, case.H, case.W, case.Cin), c.dt)
        for i in range(case.N):                           # image i is distinct[i % 2]: the last one of an odd batch is distinct[0]
            assert torch.equal(xb[i].view(it), c.x[i % 2].view(it))
        assert not torch.equal(c.x[0], c.x[1]) and bool(torch.isfinite(xb.float()).all())
        assert bool((c.out0 == c.sentinel).all()) and bool(torch.isnan(c.out0[:4].view(c.dt)).all())
        n_out = case.N * Ho * Wo * case.Cout
        lead = c.out_at - case.out_off
        assert lead >= 2 * Wo * case.Cout and (lead * c.out0.element_size()) % 16 == 0 and c.out0.numel() == c.out_at + n_out + lead
        assert c.r_at == 16 + case.res_off
        rb = C.view_of(c.rbuf, c.r_at, (case.N, Ho, Wo, case.Cout), c.dt)
        assert torch.equal(rb[case.N - 1].view(it), c.r1[(case.N - 1) % 2].view(it))
        outside = torch.ones_like(c.rbuf, dtype=torch.bool)
        outside[c.r_at:c.r_at + n_out] = False
        assert bool((c.rbuf[outside] == C.NAN_BITS[c.dt]).all())
        assert torch.equal(build(case, family).xbuf, c.xbuf)       # seeded
    assert any(c.N % 2 == 1 and c.N > 1 for c in CONV)


# ---- the bounds are the existing tests' ----------------------------------------------------------------------------------------------
def test_bounds_are_the_constants_of_the_tests_they_cite():
    import test_f32_path_gpu
    import test_ops_gpu
    from test_split_path_gpu import TOL
    src = inspect.getsource
    assert "rtol = %s if dt == torch.float16 else %s" % ("3e-3", "2e-2") in src(test_ops_gpu.test_conv3x3_nhwc_implicit_gemm)
    assert (C.bound("f16", "conv3x3"), C.bound("bf16", "conv3x3")) == (3e-3, 2e-2)
    assert "tol = 2e-3 if dt == torch.float16 else 1.6e-2" in src(test_ops_gpu.test_upsample2x_nhwc)
    assert (C.bound("f16", "upsample2x"), C.bound("bf16", "upsample2x")) == (2e-3, 1.6e-2)
    head = src(test_ops_gpu.test_conv3x3_head1x1_fused_matches_the_two_layer_path)
    assert "tol = (2e-3 if dt == torch.float16 else 1.6e-2)" in head and "<= 4 * tol" in head
    for entry in ("head1x1", "head_dot"):
        assert (C.bound("f16", entry), C.bound("bf16", entry), C.bound("split", entry)) == (4 * 2e-3, 4 * 1.6e-2, TOL)
    assert "_rel(y, ref) <= 4e-6" in src(test_f32_path_gpu.test_conv3x3_f32) and "<= 4e-6" in src(test_f32_path_gpu.test_upsample2x_f32)
    assert C.bound("f32x", "conv3x3") == C.bound("f32x", "upsample2x") == 4e-6
    assert C.bound("split", "conv3x3") == TOL == 6e-6
