"""Float64 restatement of the forward convolution entry points of csrc/conv.hip (vs_conv3x3_nhwc, vs_conv3x3_split_nhwc,
vs_conv3x3_split_res2_nhwc, vs_conv3x3_head1x1_nhwc, vs_conv3x3_head1x1_split_nhwc, vs_conv3x3_head_dot_split_nhwc, vs_upsample2x_nhwc), the
guarded input generator and the case table shared by tests/test_conv_ref_cpu.py and tests/test_conv_routes_gpu.py.

  * `CASES`     -- one record per call shape.  A 3x3 convolution states its route by hand, as the string tests/route_probe.cpp prints for
    csrc/routes.h conv3x3_route ("tile256 kpt=2 grid=151", "wave4 mi=4 grid=1", ...), and the store paths of conv_epilogue it reaches
    (`paths`); tests/test_conv_ref_cpu.py holds both to the header / to a restatement of the epilogue's conditions.  The fused heads have
    no function in routes.h: `head_route` restates their entry points' rule.
  * `build`     -- one seeded input set on the CPU.  D = 2 distinct images, image i of the batch is distinct[i % 2] (neighbours differ, so a
    tap that leaked over an image seam reads other values); the input lies in a larger allocation with NaN bit patterns for two image rows
    before the first and after the last image; the output allocation is pre-filled with a NaN payload no kernel produces, and `out` /
    `residual` can start at an element offset that breaks their 16-, 8- or 4-byte alignment (only `in` and `w` must be 16-byte aligned).
  * `conv_f64`  -- the reference, float64 on the stored values (the 16-bit or f32 tensors as uploaded), for the distinct images only:
    nine explicit shifted taps over the zero-padded input, then the epilogue in the order of conv_epilogue (conv.hip:47-224):
    + bias, + residual or the mask (out = conv if mask_by > 0 else 0), + residual2, ReLU.  The heads add the hidden map's roundings, see
    `head_f64`; the upsampling is bilinear x2 with align_corners=True, `+ add` or `+ relu(add)`.
  * `bound`     -- max |err| / max |ref| per operator and class: only numbers the suite already holds (test_ops_gpu, test_f32_path_gpu,
    test_split_path_gpu.TOL); test_conv_ref_cpu.py compares them with those files.

Two families.  "lattice": small integers times powers of two (the ranges of test_conv_halo_gpu._inputs; narrower for the fused heads, whose
second stage multiplies the first's sums): every operand is exact in bf16, every product and partial sum exact in f32 -- `lattice_units`
is the worst-case bound, asserted below 2^24 units on the CPU -- so the result must equal the float64 result rounded once to the output
type, bit for bit, in any summation order.  "real": Gaussian inputs scaled as in the existing tests.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch

CLASSES = ("f16", "bf16", "f32x", "split")
STORAGE = {"f16": torch.float16, "bf16": torch.bfloat16, "f32x": torch.float32, "split": torch.float32}
DTYPE_CODE = {"f16": 1, "bf16": 2, "f32x": 3, "split": 4}          # the ABI's dtype, as route_probe takes it
INT_OF = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32}
NAN_BITS = {torch.float16: 0x7E00, torch.bfloat16: 0x7FC0, torch.float32: 0x7FC00000}       # the guards around the input / residual
SENTINEL = {torch.float16: 0x7D5A, torch.bfloat16: 0x7FAA, torch.float32: 0x7F8A5A5A}       # NaN payloads no kernel produces
D = 2
EPIS = ("none", "bias", "bias+res", "mask", "relu_in", "relu_out", "bias+res+res2")       # the last: split class only
UP_MODES = ("none", "add", "relu_add")
# lattice ranges: integers in [-a, a] times 2^-s.  conv3x3: test_conv_halo_gpu._inputs; heads: narrower, the bound covers both stages
LAT = {"conv3x3": dict(x=(8, 3), w=(8, 6), b=(64, 4), r=(64, 4)),
       "head": dict(x=(2, 3), w=(2, 6), b=(100, 4), w2=(2, 6), b2=(4, 4))}
# (the heads' bias reaches 6.25: hidden values above 4 have more bits than f16 keeps, above 0.5 more than bf16 keeps, so the lattice family sees
# the hidden map's rounding to the 16-bit type, conv.hip:278 / 708, and the bound below still holds: 9 Cin 4 + 3200 < 2^13 units for Cin <= 128)


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------------------------------
# bounds: max |err| / max |ref| -- the constants of the existing tests, nothing measured here
# ------------------------------------------------------------------------------------------------------------------------------------
def bound(cls, entry):
    """3x3 conv: test_ops_gpu.test_conv3x3_nhwc_implicit_gemm (3e-3 / 2e-2), test_f32_path_gpu.test_conv3x3_f32 (4e-6), test_split_path_gpu.TOL.
    Fused heads: 4 x the tolerance of test_ops_gpu.test_conv3x3_head1x1_fused_matches_the_two_layer_path against the unrounded reference (2e-3 / 1.6e-2), TOL.
    Upsample: test_ops_gpu.test_upsample2x_nhwc (2e-3 / 1.6e-2), test_f32_path_gpu.test_upsample2x_f32 (4e-6).
    The mask, residual2 and alignment variants add no arithmetic: their operator's bound."""
    op = "head" if entry in ("head1x1", "head_dot") else entry
    table = {"conv3x3": {"f16": 3e-3, "bf16": 2e-2, "f32x": 4e-6, "split": 6e-6},
             "head": {"f16": 4 * 2e-3, "bf16": 4 * 1.6e-2, "split": 6e-6},
             "upsample2x": {"f16": 2e-3, "bf16": 1.6e-2, "f32x": 4e-6}}
    return table[op][cls]


# ------------------------------------------------------------------------------------------------------------------------------------
# the fused heads' route: no function in routes.h, the entry points' rule restated
# ------------------------------------------------------------------------------------------------------------------------------------
def head_route(cls, entry, Cin, c2pad, packed=False):
    """conv.hip:1240-1256 (vs_conv3x3_head1x1_nhwc: Cout = 256 -> conv3x3_256_kernel<., false, NF = C2pad / 16> by with_head_nf, conv.hip:1124-1133;
    otherwise the 4-wave kernel conv3x3_kernel<., 8, true>), conv.hip:1276-1284 (vs_conv3x3_head_dot_split_nhwc: the 256 x 128 tile kernel when
    2 Cin is 64 << s and 9 * 2 Cin / 64 is even, the 4-wave kernel with MI = 8 otherwise; a packed input needs the tile kernel),
    conv.hip:1308-1313 (vs_conv3x3_head1x1_split_nhwc: conv3x3_256_kernel<split, false, NF, packed>)."""
    if entry == "head1x1":
        return "mfma256 nf=%d%s" % (c2pad // 16, " packed" if packed else "")
    if cls != "split":
        return "dot wave4 mi=8"
    c2 = 2 * Cin
    tile128 = c2 in (64, 128, 256, 512) and (9 * c2 // 64) % 2 == 0
    assert tile128 or not packed
    return "dot tile128" + (" packed" if packed else "") if tile128 else "dot wave4 mi=8"


# ------------------------------------------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------------------------------------------
def _rec(**kw):
    base = dict(stride=1, packed=False, out_off=0, res_off=0, paths=(), families=("lattice", "real"), epis=None, Cout=0, c2pad=0, n_out=0)
    base.update(kw)
    c = SimpleNamespace(**base)
    if c.entry == "conv3x3" and c.epis is None:
        c.epis = tuple(e for e in EPIS if (e != "bias+res+res2" or (c.cls == "split" and not c.packed)) and not (c.packed and e == "relu_in"))
    return c


def _conv_cases():
    out = []
    for cls in CLASSES:
        sp, b16 = cls == "split", cls in ("f16", "bf16")
        V = "pair16" if b16 else "f32x4"          # a full wave tile of an aligned call
        R = "u2" if b16 else "f32_tail4"          # its ragged rows
        O1 = "scalar" if b16 else "f32_tail4"     # out / residual off by one element
        e8 = 4 if b16 else 2                      # elements in 8 bytes

        def add(tag, N, H, W, Cin, Cout, route, paths, **kw):
            kind = route.split()[0] + (route.split()[1].replace("=", "") if route.startswith("wave4") else "")
            out.append(_rec(id=f"{kind}-{cls}-{tag}", cls=cls, entry="conv3x3", N=N, H=H, W=W, Cin=Cin, Cout=Cout, route=route, paths=tuple(paths), **kw))

        # ---- 256 x 256 tiles.  15 x 17 = 255 pixels: every tile straddles an image seam, the last one is ragged
        ct, nt = (128 if b16 else 64), (151 if sp else 225)        # Cin2 = 128: two K-tiles per tap; 150 (split) / 224 tiles
        add("15x17", nt, 15, 17, ct, 256, f"tile256 kpt=2 grid={nt}", (V, R))
        add("s2_31x32", 150 if sp else 224, 31, 32, ct, 256, f"tile256 kpt=2 grid={150 if sp else 224}", (V,), stride=2)
        if cls in ("bf16", "split"):
            add("s2_32x31", 150 if sp else 224, 32, 31, ct, 256, f"tile256 kpt=2 grid={150 if sp else 224}", (V,), stride=2)
        add("cout512", 76 if sp else 113, 15, 17, ct, 512, f"tile256 kpt=2 grid={152 if sp else 226}", (V, R))
        add("out+1", nt, 15, 17, ct, 256, f"tile256 kpt=2 grid={nt}", (O1,), out_off=1, epis=("none", "bias+res"))
        add("out+8B", nt, 15, 17, ct, 256, f"tile256 kpt=2 grid={nt}", (R,), out_off=e8, epis=("none", "bias+res"))
        add("res+1", nt, 15, 17, ct, 256, f"tile256 kpt=2 grid={nt}", (O1,), res_off=1, epis=("bias+res", "mask"))
        add("res+8B", nt, 15, 17, ct, 256, f"tile256 kpt=2 grid={nt}", (V, R) if b16 else (R,), res_off=e8, epis=("bias+res", "mask"))
        if sp:
            add("kpt6", 151, 15, 17, 192, 256, "tile256 kpt=6 grid=151", (V, R))
            add("packed", 151, 15, 17, 64, 256, "tile256 kpt=2 grid=151", (V, R), packed=True)
            add("16x16", 150, 16, 16, 64, 256, "halo256 kpt=2 grid=150", (V,))
            # ---- 256 x 128 tiles (split only)
            add("cout128", 225, 15, 17, 64, 128, "tile256x128 kpt=2 grid=225", (V, R))
            add("cout384", 75, 15, 17, 64, 384, "tile256x128 kpt=2 grid=225", (V, R))
            add("packed", 225, 15, 17, 64, 128, "tile256x128 kpt=2 grid=225", (V, R), packed=True)
        # ---- the 4-wave kernel: rows >= M, M < 16, 1 x 1, 1 x W, H x 1 maps, tiles over several images, Cout off the column tile
        cs = 16 if cls == "f32x" else 32
        r = lambda other, split: split if sp else other
        add("m1_1x1", 1, 1, 1, cs, 64, "wave4 mi=4 grid=1", (R,))
        add("m15_1x15", 1, 1, 15, cs, 83, "wave4 mi=4 grid=1", ("scalar",))
        add("m63_21x1", 3, 21, 1, cs, 128, "wave4 mi=4 grid=1", (R,))
        add("m64_8x8", 1, 8, 8, cs, 192, "wave4 mi=4 grid=2", (V,))
        add("m65_5x13", 1, 5, 13, cs, 320, r("wave4 mi=4 grid=3", "wave4 mi=2 grid=6"), (V, R))
        add("m129_1x43", 3, 1, 43, cs, 83, r("wave4 mi=4 grid=2", "wave4 mi=2 grid=3"), ("scalar",))
        add("m105_5x7", 3, 5, 7, cs, 64, r("wave4 mi=4 grid=1", "wave4 mi=2 grid=2"), (V, R))
        add("s2_10x14", 3, 10, 14, cs, 128, r("wave4 mi=4 grid=1", "wave4 mi=2 grid=2"), (V, R), stride=2)
        add("s2_9x13", 3, 9, 13, cs, 128, r("wave4 mi=4 grid=1", "wave4 mi=2 grid=2"), (V, R), stride=2)
        add("cin96", 3, 1, 43, 96, 128, r("wave4 mi=4 grid=2", "wave4 mi=2 grid=3"), (V, R))
        add("out+1", 2, 8, 8, cs, 128, r("wave4 mi=4 grid=1", "wave4 mi=2 grid=2"), (O1,), out_off=1, epis=("none", "bias+res"))
        add("out+8B", 2, 8, 8, cs, 128, r("wave4 mi=4 grid=1", "wave4 mi=2 grid=2"), (R,), out_off=e8, epis=("none", "bias+res"))
        add("res+1", 2, 8, 8, cs, 128, r("wave4 mi=4 grid=1", "wave4 mi=2 grid=2"), (O1,), res_off=1, epis=("bias+res", "mask"))
        add("res+8B", 2, 8, 8, cs, 128, r("wave4 mi=4 grid=1", "wave4 mi=2 grid=2"), (V,) if b16 else (R,), res_off=e8, epis=("bias+res", "mask"))
        if b16:
            add("pin", 128, 16, 16, 64, 256, "wave4 mi=8 grid=256", (V,))         # test_routes_cpu.PINS
        if sp:
            add("pin", 256, 16, 16, 32, 256, "wave4 mi=8 grid=512", (V,))         # test_routes_cpu.PINS
            add("scene", 8, 16, 16, 32, 256, "wave4 mi=2 grid=64", (V,))          # one 8-view scene's 16 x 16 maps
            add("m38144", 149, 16, 16, 32, 256, "wave4 mi=4 grid=596", (V,))      # MI = 4 above 64 rows: under the tile threshold, over 192 tiles
    return out


HEAD_SHAPES = ((1, 16, 16), (4, 8, 8), (256, 1, 1))      # one map; seams inside the 256-pixel tile; nothing but seams


def _head_cases():
    out = []
    for cls in ("f16", "bf16", "split"):
        sp = cls == "split"
        for packed in ((False, True) if sp else (False,)):
            tag = "-packed" if packed else ""
            for i, c2pad in enumerate((16, 32, 48, 64, 80, 96)):           # every width with_head_nf instantiates
                N, H, W = HEAD_SHAPES[i % 3]
                Cin = 64 if sp else 128
                out.append(_rec(id=f"head1x1-{cls}{tag}-c2pad{c2pad}-{N}x{H}x{W}", cls=cls, entry="head1x1", N=N, H=H, W=W, Cin=Cin, Cout=256,
                                c2pad=c2pad, n_out=c2pad - 13, packed=packed, route=head_route(cls, "head1x1", Cin, c2pad, packed)))
        dots = [(32, False), (96, False)] if not sp else [(64, False), (32, False), (96, False), (64, True)]
        for j, (Cin, packed) in enumerate(dots):
            for n_out in (1, 2, 3, 4):
                N, H, W = HEAD_SHAPES[(n_out + j) % 3]
                out.append(_rec(id=f"head_dot-{cls}{'-packed' if packed else ''}-cin{Cin}-n{n_out}-{N}x{H}x{W}", cls=cls, entry="head_dot", N=N, H=H,
                                W=W, Cin=Cin, Cout=128, c2pad=4, n_out=n_out, packed=packed, route=head_route(cls, "head_dot", Cin, 4, packed)))
    return out


def _upsample_cases():
    out = []
    sizes = (1, 2, 3, 17)
    for cls in ("f16", "bf16", "f32x"):
        chans = (4, 36, 64) if cls == "f32x" else (8, 40, 256)
        k = 0
        for H in sizes:
            for W in sizes:
                N, C = (1, 2, 3, 17)[(k + k // 4) % 4], chans[(k // 3 + k) % 3]
                k += 1
                fam = ("lattice", "real") if H == W == 1 else ("real",)        # a copy along an axis of size 1: exact only at 1 x 1
                out.append(_rec(id=f"upsample2x-{cls}-{N}x{H}x{W}x{C}", cls=cls, entry="upsample2x", N=N, H=H, W=W, Cin=C, families=fam, route="up"))
        # rows of the launch (N * H; N * 2 H for the H < 2 || W < 2 f32 kernel) beyond the 32768 of grid.y: gridDim.z = 2
        C = 4 if cls == "f32x" else 8
        out.append(_rec(id=f"upsample2x-{cls}-16385x2x2x{C}", cls=cls, entry="upsample2x", N=16385, H=2, W=2, Cin=C, families=("real",), route="up z=2"))
        if cls == "f32x":
            out.append(_rec(id="upsample2x-f32x-16385x1x2x4", cls=cls, entry="upsample2x", N=16385, H=1, W=2, Cin=4, families=("real",), route="up z=2"))
    return out


# packed output of the f32 upsampling against the packing of the plain result (C % 32 == 0, H, W >= 2)
UPSAMPLE_PACKED = ((1, 2, 2, 32), (2, 3, 17, 64), (3, 17, 2, 96))
# VS_CHECK returns before any launch: a packed input where the route is the 4-wave kernel; a fused head whose N*H*W is no multiple of 256
REFUSED_PACKED = (1, 8, 8, 64, 128)          # N, H, W, Cin, Cout: "packed_not_taken"
REFUSED_HEAD = (1, 15, 17)                   # N, H, W

CASES = _conv_cases() + _head_cases() + _upsample_cases()
assert len({c.id for c in CASES}) == len(CASES)


def out_hw(c):
    return (c.H - 1) // c.stride + 1, (c.W - 1) // c.stride + 1


def pixels(c):
    Ho, Wo = out_hw(c)
    return c.N * Ho * Wo


def probe_query(c, packed=None):
    """The line tests/route_probe.cpp answers for a 3x3 convolution case (H, W of the OUTPUT)."""
    Ho, Wo = out_hw(c)
    return "c %d %d %d %d %d %d %d %d" % (DTYPE_CODE[c.cls], c.N, Ho, Wo, c.Cin, c.Cout, c.stride, int(c.packed if packed is None else packed))


# ------------------------------------------------------------------------------------------------------------------------------------
# lattice: the worst-case magnitude of any partial sum, in units of the smallest product
# ------------------------------------------------------------------------------------------------------------------------------------
def lattice_units(c):
    """-> list of (what, worst-case |partial sum| in units, limit).  Exact in f32 (24-bit significand) when every entry is below its limit.
    conv3x3: products are multiples of 2^-9, |sum| <= 9 Cin max|x| max|w|; bias, residual, residual2 are multiples of 2^-4 = 32 units.
    heads: stage 1 as above; the hidden value h (a multiple of 2^-9, 16-bit rounding keeps that and at most doubles the magnitude bound to the
    next power of two) times w2 (multiples of 2^-6) is a multiple of 2^-15: |sum| <= Cout P1 max|w2| plus bias2 (2^11 units each); the split
    MFMA form carries h as an f16 (hi, lo) pair: 22 bits."""
    if c.entry == "conv3x3":
        L = LAT["conv3x3"]
        s = 9 * c.Cin * L["x"][0] * L["w"][0] + 32 * L["b"][0] + 2 * 32 * L["r"][0]
        return [("conv + bias + residual + residual2", s, 2 ** 24)]
    if c.entry in ("head1x1", "head_dot"):
        L = LAT["head"]
        s1 = 9 * c.Cin * L["x"][0] * L["w"][0] + 32 * L["b"][0]
        p1 = 2 ** math.ceil(math.log2(s1 + 1))
        s2 = c.Cout * p1 * L["w2"][0] + 2 ** 11 * L["b2"][0]
        return [("hidden", s1, 2 ** 24), ("hidden as an f16 (hi, lo) pair", p1, 2 ** 22), ("1x1 product + bias2", s2, 2 ** 24)]
    return [("x + add", 2 * LAT["conv3x3"]["x"][0] + LAT["conv3x3"]["r"][0], 2 ** 8)]       # units of 2^-4: exact in bf16's 8 bits


# ------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------------
def _seed(c, family):
    return (sum(ord(ch) * (i + 1) for i, ch in enumerate(c.id)) * 2 + (family == "real")) % (2 ** 31)


def _lat(shape, g, rng):
    a, s = rng
    return torch.randint(-a, a + 1, shape, generator=g).float() * 2.0 ** -s


def guarded(data, lead, off, tail, fill_bits):
    """`data` inside a larger flat allocation of its integer twin type: [lead | off | data | tail] elements, everything but the data filled with
    the bit pattern.  -> (buffer, first element of the data)."""
    it = INT_OF[data.dtype]
    buf = torch.full((lead + off + data.numel() + tail,), fill_bits, dtype=it)
    buf[lead + off:lead + off + data.numel()] = data.reshape(-1).view(it)
    return buf, lead + off


def view_of(buf, start, shape, dtype):
    return buf[start:start + math.prod(shape)].view(dtype).view(shape)


def _up16(n):
    return cdiv(n, 16) * 16


def build(case, family):
    """The case's tensors on the CPU (see the module docstring).  Fields: the distinct images `x`, `r1`, `r2`, `add` [D, ...] as stored, `w`
    ([Cout, Cin, 3, 3] f32 holding the stored values), `bias`, `w2`, `bias2`; `idx` [N] = i % D; the flat guarded buffers `xbuf`, `rbuf`,
    `out0` with the first element of their tensors `x_at`, `r_at`, `out_at`."""
    g = torch.Generator().manual_seed(_seed(case, family))
    dt = STORAGE[case.cls]
    c = SimpleNamespace(**vars(case))
    c.family, c.dt, c.sentinel = family, dt, SENTINEL[dt]
    c.idx = torch.arange(case.N) % D
    lat = family == "lattice"
    N, H, W, Cin, Cout = case.N, case.H, case.W, case.Cin, case.Cout
    Ho, Wo = out_hw(case)
    if case.entry == "upsample2x":
        L = LAT["conv3x3"]
        x = _lat((D, H, W, Cin), g, L["x"]) if lat else torch.randn(D, H, W, Cin, generator=g)
        add = _lat((D, 2 * H, 2 * W, Cin), g, L["r"]) if lat else torch.randn(D, 2 * H, 2 * W, Cin, generator=g)
        c.x, c.add = x.to(dt), add.to(dt)
        c.xbuf, c.x_at = guarded(c.x[c.idx], 2 * W * Cin, 0, 2 * W * Cin, NAN_BITS[dt])
        return c
    if case.entry == "conv3x3":
        L = LAT["conv3x3"]
        if lat:
            x, w, b = _lat((D, H, W, Cin), g, L["x"]), _lat((Cout, Cin, 3, 3), g, L["w"]), _lat((Cout,), g, L["b"])
            r1, r2 = _lat((D, Ho, Wo, Cout), g, L["r"]), _lat((D, Ho, Wo, Cout), g, L["r"])
        else:
            x, w, b = torch.randn(D, H, W, Cin, generator=g), torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin), torch.randn(Cout, generator=g)
            r1, r2 = torch.randn(D, Ho, Wo, Cout, generator=g), torch.randn(D, Ho, Wo, Cout, generator=g)
        c.x, c.w, c.bias, c.r1, c.r2 = x.to(dt), (w if dt == torch.float32 else w.to(dt).float()), b, r1.to(dt), r2.to(dt)
        c.rbuf, c.r_at = guarded(c.r1[c.idx], 16, case.res_off, 16, NAN_BITS[dt])
        og = _up16(2 * Wo * Cout)                                   # two output rows, rounded up so that the tensor stays 16-byte aligned
        n_out = N * Ho * Wo * Cout
        c.out0 = torch.full((og + case.out_off + n_out + og,), c.sentinel, dtype=INT_OF[dt])
        c.out_at, c.out_shape = og + case.out_off, (N, Ho, Wo, Cout)
    else:
        L = LAT["head"]
        rows2 = case.c2pad
        if lat:
            x, w, b = _lat((D, H, W, Cin), g, L["x"]), _lat((Cout, Cin, 3, 3), g, L["w"]), _lat((Cout,), g, L["b"])
            w2, b2 = _lat((rows2, Cout), g, L["w2"]), _lat((rows2,), g, L["b2"])
        else:           # test_ops_gpu.test_conv3x3_head1x1_fused_matches_the_two_layer_path
            x, w, b = torch.randn(D, H, W, Cin, generator=g), torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin), torch.randn(Cout, generator=g) * 0.1
            w2, b2 = torch.randn(rows2, Cout, generator=g) / math.sqrt(Cout), torch.randn(rows2, generator=g)
        w2[case.n_out:] = 0
        b2[case.n_out:] = 0
        w2dt = torch.float32 if case.cls == "split" else dt
        c.x, c.w, c.bias, c.w2, c.bias2 = x.to(dt), (w if dt == torch.float32 else w.to(dt).float()), b, w2.to(w2dt), b2
    c.xbuf, c.x_at = guarded(c.x[c.idx], 2 * W * Cin, 0, 2 * W * Cin, NAN_BITS[dt])
    return c


def to_device(c, dev):
    d = SimpleNamespace(**vars(c))
    for k, v in vars(c).items():
        if torch.is_tensor(v):
            setattr(d, k, v.to(dev))
    return d


# ------------------------------------------------------------------------------------------------------------------------------------
# the float64 references (distinct images only)
# ------------------------------------------------------------------------------------------------------------------------------------
def conv3x3_taps_f64(x, w, stride=1):
    """x [D, H, W, Cin], w [Cout, Cin, 3, 3] float64 -> [D, Ho, Wo, Cout]: k = 3, pad = 1.  Output pixel (y, x) has its centre tap at input
    (y s, x s); tap (ky, kx) reads input (y s + ky - 1, x s + kx - 1), i.e. (y s + ky, x s + kx) of the image with a zero border of one."""
    assert x.dtype == w.dtype == torch.float64
    Dn, H, W, Cin = x.shape
    Cout = w.shape[0]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    xp = torch.zeros(Dn, H + 2, W + 2, Cin, dtype=torch.float64)
    xp[:, 1:H + 1, 1:W + 1] = x
    out = torch.zeros(Dn * Ho * Wo, Cout, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            patch = xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride]
            out += patch.reshape(-1, Cin) @ w[:, :, ky, kx].t()
    return out.view(Dn, Ho, Wo, Cout)


def _conv_cached(c, relu_in):
    cache = c.__dict__.setdefault("_conv", {})
    if relu_in not in cache:
        x = c.x.cpu().double()
        cache[relu_in] = conv3x3_taps_f64(x.clamp_min(0) if relu_in else x, c.w.cpu().double(), c.stride)
    return cache[relu_in]


def epilogue_f64(conv, epi, bias=None, r1=None, r2=None):
    """conv_epilogue's order (conv.hip:56-63 bias, 84-93 / 136-140 residual or mask, 141-144 residual2, 94-97 / 145-148 ReLU)."""
    ref = conv
    if "bias" in epi:
        ref = ref + bias.double()
    if "res" in epi:
        ref = ref + r1.double()
    if epi == "mask":
        ref = torch.where(r1.double() > 0, ref, torch.zeros_like(ref))
    if "res2" in epi:
        ref = ref + r2.double()
    if epi == "relu_out":
        ref = ref.clamp_min(0)
    return ref + 0.0            # (-0 -> +0: an f32 sum that starts from +0 never ends at -0)


def head_f64(c, relu_out, with_bias):
    """The fused heads on the built case.  Rounding points of the kernels, all applied here:
      16-bit MFMA form: the hidden value acc + bias is rounded to the 16-bit type BEFORE its ReLU when it is staged for the second GEMM
        (conv.hip:277-280; max(round(x), 0) == round(max(x, 0)));
      16-bit dot form: ReLU, then the rounding to the 16-bit type (conv.hip:706-708);
      split MFMA form: the hidden value is carried as an f16 (hi, lo) pair (conv.hip:376-385), 22 bits: no rounding the class bound would see,
        and none at all on lattice values (lattice_units); split dot form: f32 throughout (conv.hip:676, 708 is compiled out).
    Then the 1x1 product and bias2 (conv.hip:313-318 / 423 / 727-728); columns >= n_out have zero weights and zero bias2."""
    conv = _conv_cached(c, False)
    h = conv + c.bias.cpu().double() if with_bias else conv
    if relu_out:
        h = h.clamp_min(0)
    if c.cls != "split":
        h = h.to(c.dt).double()
    return h @ c.w2.cpu().double().t() + c.bias2.cpu().double() + 0.0


def _axis_f64(n_in):
    """align_corners=True, scale 2: source position of output i is i (n_in - 1) / (2 n_in - 1) -> (i0, i1, weight of i1)."""
    n_out = 2 * n_in
    src = torch.arange(n_out, dtype=torch.float64) * ((n_in - 1) / (n_out - 1))
    i0 = src.floor().long().clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    return i0, i1, src - i0.double()


def upsample_f64(c, mode):
    x = c.x.cpu().double()
    y0, y1, ly = _axis_f64(c.H)
    x0, x1, lx = _axis_f64(c.W)
    rows = x[:, y0] * (1 - ly)[None, :, None, None] + x[:, y1] * ly[None, :, None, None]
    up = rows[:, :, x0] * (1 - lx)[None, None, :, None] + rows[:, :, x1] * lx[None, None, :, None]
    if mode == "add":
        up = up + c.add.cpu().double()
    if mode == "relu_add":
        up = up + c.add.cpu().double().clamp_min(0)
    return up + 0.0


def conv_f64(c, epi):
    """The float64 reference of a built case for one epilogue: a name of EPIS (conv3x3), (relu_out, with_bias) (heads), a name of UP_MODES.
    -> [D, Ho, Wo, channels] for the distinct images; image i of the batch is [i % D]."""
    if c.entry == "conv3x3":
        return epilogue_f64(_conv_cached(c, epi == "relu_in"), epi, c.bias.cpu(), c.r1.cpu(), c.r2.cpu())
    if c.entry == "upsample2x":
        return upsample_f64(c, epi)
    return head_f64(c, *epi)
