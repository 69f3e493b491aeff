"""The visualisation kernels (csrc/viz.hip, include/vicasplat_viz.h) on the GPU, through the binding, against the float64 restatement of
tests/viz_f64.py, and the callers built on them end to end.

Criteria (viz_f64): (near, far) per element within K 2^-24 mag of float64, K = 4 max(R32, 1) = 4; the four order statistics bit-equal
(the entry's order_stats output); the index equal outside the band of its step function, the band at most 0.5 % of a case's pixels; f32
colours bit-equal to lut[idx]; bytes bit-equal to trunc(clip(lut[idx], 0, 1) * 255); the rgb half of a frame bit-equal to torch's
expression.  Every output sits between sentinel-filled guard bands and the workspace is NaN-filled on entry.

Measured on an MI355X (`-s` prints them), in units of 2^-24 mag against the 4 allowed: near <= 1.37, far <= 1.41 over every size, base offset and
value edge here (16 000 000 values: 0.04 / 0.86); no index differs outside the band in any case.

Sizes come from the launch geometry the binding exports: VSV_VEC values per lane, VSV_THREADS * VSV_VEC per workgroup and round,
VSV_MAX_BLOCKS workgroups in the grid's first round -- one fewer than, exactly, and one more than each.
"""
import numpy as np
import pytest
import torch

import viz_f64 as V

pytestmark = pytest.mark.gpu
GUARD = 64      # elements on either side of every output; 256 bytes of f32 keep the alignment of the base
SENTINEL = {torch.float32: -7.25, torch.uint8: 0xA5}


def _dev():
    return torch.device("cuda:0")


def _L():
    from vicasplat_amd import _lib
    _lib.lib()
    return _lib


def _guarded(numel, dtype):
    whole = torch.full((numel + 2 * GUARD,), SENTINEL[dtype], dtype=dtype, device=_dev())
    return whole, whole[GUARD:GUARD + numel]


def _intact(whole, numel):
    s = SENTINEL[whole.dtype]
    return bool((whole[:GUARD] == s).all() and (whole[GUARD + numel:] == s).all())


def _on_device(a: np.ndarray, offset: int = 0) -> torch.Tensor:
    """A contiguous f32 device copy whose base pointer sits `offset` elements past a 256-byte boundary."""
    buf = torch.empty(a.size + offset, dtype=torch.float32, device=_dev())
    view = buf[offset:]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32).ravel()))
    assert view.data_ptr() % 16 == (4 * offset) % 16
    return view


def run_range(values: torch.Tensor):
    """vsv_depth_range through the binding: (range [2], order_stats [4]) as numpy, guards and workspace checked."""
    L = _L()
    n = values.numel()
    need = int(L.call("vsv_depth_range_workspace_bytes", _dev(), n))
    ws_whole = torch.full((need // 4 + 2 * GUARD,), float("nan"), dtype=torch.float32, device=_dev())
    ws = ws_whole[GUARD:GUARD + need // 4]
    rw, r = _guarded(2, torch.float32)
    sw, s = _guarded(4, torch.float32)
    L.call("vsv_depth_range", _dev(), L.ptr(values), n, L.ptr(r), L.ptr(s), L.ptr(ws), need)
    torch.cuda.synchronize()
    assert _intact(rw, 2) and _intact(sw, 4) and bool(ws_whole[:GUARD].isnan().all()) and bool(ws_whole[GUARD + need // 4:].isnan().all())
    return r.cpu().numpy().copy(), s.cpu().numpy().copy()


def run_color_map(values: torch.Tensor, shape, mode, rng, lut: torch.Tensor, u8: bool, out_offset: int = 0):
    """vsv_color_map through the binding on `values` seen as [M, H, W] = shape: the [M, 3, H, W] output as numpy, guards checked."""
    L = _L()
    M, H, W = shape
    dtype = torch.uint8 if u8 else torch.float32
    whole, out = _guarded(3 * M * H * W + out_offset, dtype)
    out = out[out_offset:]
    need = int(L.call("vsv_color_map_workspace_bytes", _dev(), mode))
    ws_whole = torch.full((need // 4 + 2 * GUARD,), float("nan"), dtype=torch.float32, device=_dev())
    ws = ws_whole[GUARD:GUARD + need // 4]
    L.call("vsv_color_map", _dev(), L.ptr(values), M, H, W, mode, L.ptr(rng), L.ptr(lut), L.ptr(out), L.VSV_OUT_U8 if u8 else L.VSV_OUT_F32,
           L.ptr(ws) if need else None, need)
    torch.cuda.synchronize()
    assert bool((whole[:GUARD + out_offset] == SENTINEL[dtype]).all()) and bool((whole[GUARD + out_offset + 3 * M * H * W:] == SENTINEL[dtype]).all())
    assert bool(ws_whole[:GUARD].isnan().all()) and bool(ws_whole[GUARD + need // 4:].isnan().all())
    return out.cpu().numpy().reshape(M, 3, H, W).copy()


def ramp_index(colors: np.ndarray) -> np.ndarray:
    """The index behind f32 colours of the ramp table [M, 3, H, W]: lut[i] = (i, 2 i, 255 - i) / 255, and (0, 0, 0) is a NaN's colour."""
    i = np.rint(colors[:, 0].astype(np.float64) * 255).astype(np.int32)
    return np.where((colors == 0).all(1), -1, i)


def same_bits(a, b) -> bool:
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def check_range(data: np.ndarray, offset: int = 0):
    ref = V.depth_range(data)
    got, stats = run_range(_on_device(data, offset))
    print(f"n={data.size} offset={offset}: near {V.units(got[0], ref['near'], ref['mag_near']) if np.isfinite(ref['near']) and ref['mag_near'] else 0:.3f} "
          f"far {V.units(got[1], ref['far'], ref['mag_far']) if np.isfinite(ref['far']) else 0:.3f} units")
    assert same_bits(stats, ref["stats"]), (stats, ref["stats"])
    assert V.range_ok(got[0], got[1], ref), (got, ref)
    return got, ref


def check_colors(data: np.ndarray, shape, rng_f32: np.ndarray):
    """Depth mode with the ramp table and the range GIVEN: index outside the band, f32 colours and bytes bit-equal given the index."""
    lut = V.ramp_lut()
    d, r, t = _on_device(data), torch.tensor(rng_f32, device=_dev()), torch.tensor(lut, device=_dev())
    L = _L()
    col = run_color_map(d, shape, L.VSV_MODE_DEPTH, r, t, u8=False)
    idx = ramp_index(col)
    x, bound = V.x_depth(data.reshape(shape), rng_f32[0], rng_f32[1])
    assert V.index_ok(idx, x, bound), (float(V.band(x, bound).mean()), int((idx != V.index_of(x)).sum()))
    assert same_bits(col, V.lookup(idx, lut))
    assert np.array_equal(run_color_map(d, shape, L.VSV_MODE_DEPTH, r, t, u8=True), V.to_u8(V.lookup(idx, lut)))
    return idx


def check_colors_within_bound(data: np.ndarray, shape, rng_f32: np.ndarray):
    """The form of the index criterion that excludes no pixel, for a range so narrow that the band is every pixel: the kernel's index lies
    between the indices of x - bound and x + bound (x falls with the index's argument, so these bracket it); colours and bytes bit-equal
    given the index; guard bands intact (run_color_map)."""
    lut = V.ramp_lut()
    d, r, t = _on_device(data), torch.tensor(rng_f32, device=_dev()), torch.tensor(lut, device=_dev())
    L = _L()
    col = run_color_map(d, shape, L.VSV_MODE_DEPTH, r, t, u8=False)
    idx = ramp_index(col)
    x, bound = V.x_depth(data.reshape(shape), rng_f32[0], rng_f32[1])
    lo, hi = V.index_of(x - bound), V.index_of(x + bound)
    assert ((lo <= idx) & (idx <= hi)).all(), int(((idx < lo) | (idx > hi)).sum())
    assert len(np.unique(idx)) > 32        # the narrow range spreads the 256 distinct values over the table: the check is not vacuous
    assert same_bits(col, V.lookup(idx, lut))
    assert np.array_equal(run_color_map(d, shape, L.VSV_MODE_DEPTH, r, t, u8=True), V.to_u8(V.lookup(idx, lut)))


def _data(n, seed, zeros=0.1, negatives=0.02):
    g = np.random.default_rng(seed)
    v = g.lognormal(1.0, 1.5, n).astype(np.float32)
    v[g.uniform(size=n) < zeros] = 0
    v[g.uniform(size=n) < negatives] *= -1
    return v


# ---- sizes and guards ---------------------------------------------------------------------------------------------------------------------
def _sizes():
    L = _L()
    share = L.VSV_THREADS * L.VSV_VEC
    edges = (L.VSV_VEC, share, share * L.VSV_MAX_BLOCKS)
    return [1, 2, 3] + [e + k for e in edges for k in (-1, 0, 1)]


def test_range_sizes_from_the_launch_geometry():
    sizes = _sizes()
    assert sizes[:6] == [1, 2, 3, 3, 4, 5] and sizes[-1] == _L().VSV_THREADS * _L().VSV_VEC * _L().VSV_MAX_BLOCKS + 1
    for n in sizes:
        check_range(_data(n, seed=n % 1000))


@pytest.mark.parametrize("offset", (1, 2, 3))
def test_range_misaligned_base(offset):
    for n in (1, 2, 5, 2051):
        check_range(_data(n, seed=offset), offset)


def test_largest_size_and_refusal():
    L = _L()
    n = L.VSV_MAX_RANGE_N
    g = np.random.default_rng(5)
    data = np.exp(g.uniform(-3, 4, n).astype(np.float32))
    data[::11] = 0
    check_range(data)
    with pytest.raises(RuntimeError, match="exceeds 16000000"):
        L.call("vsv_depth_range", _dev(), L.ptr(torch.empty(4, device=_dev())), n + 1, L.ptr(torch.empty(2, device=_dev())), None,
               L.ptr(torch.empty(8192, device=_dev())), 32768)


# ---- value edges ---------------------------------------------------------------------------------------------------------------------------
def _edge_cases():
    g = np.random.default_rng(9)
    shape = (2, 31, 33)       # H W is no multiple of 4: the single-element path of the colour kernel; 2046 values
    n = int(np.prod(shape))
    low_bits = (np.float32(3.0).view(np.uint32) + g.integers(0, 256, n).astype(np.uint32)).view(np.float32)
    one_digit = g.uniform(1.0, 1.99, n).astype(np.float32)
    one_positive = np.zeros(n, np.float32)
    one_positive[777] = 2.5
    with_nan = _data(n, 3)
    with_nan[100] = np.nan
    with_inf = _data(n, 4, zeros=0, negatives=0)
    with_inf[g.choice(n, n // 50, replace=False)] = np.inf       # 2 %: both statistics of far are +inf, and inf - inf is NaN
    few_inf = _data(n, 6, zeros=0, negatives=0)
    few_inf[5] = np.inf                                          # the largest value only: far stays finite
    negatives = -_data(n, 7, zeros=0.05, negatives=0)
    negatives[g.choice(n, 40, replace=False)] = g.uniform(0.5, 2.0, 40).astype(np.float32)
    subnormal = np.exp2(g.uniform(0, 23, n)).astype(np.uint32).view(np.float32)      # log-uniform over the whole subnormal range
    return shape, dict(low_bits=low_bits, one_digit=one_digit, one_positive=one_positive, nan=with_nan, inf=with_inf, few_inf=few_inf,
                       negatives=negatives, subnormal=subnormal, zeros=np.zeros(n, np.float32))


@pytest.mark.parametrize("name", ("low_bits", "one_digit", "one_positive", "nan", "inf", "few_inf", "negatives", "subnormal", "zeros"))
def test_value_edges(name):
    shape, cases = _edge_cases()
    data = cases[name]
    got, ref = check_range(data)
    if name in ("nan", "inf"):
        assert np.isnan(got[1]) and np.isfinite(got[0])
    if name == "zeros":
        assert got[0] == 0 and got[1] == -np.inf and ref["npos"] == 0
    # low_bits: far - near is 2e-5 and x is amplified by 1 / (far - near): float64 alone decides no index (the band is every pixel), so
    # its values are mapped with a range that is given, (log 1, log 10), under the criterion of every other case, and with its own range
    # under the form of that criterion that excludes no pixel (check_colors_within_bound)
    idx = check_colors(data, shape, np.log(np.array([1.0, 10.0], np.float32)) if name == "low_bits" else got)
    if name == "low_bits":
        check_colors_within_bound(data, shape, got)
    if name in ("nan", "inf", "zeros"):
        assert (idx == -1).all()
    if name == "one_positive":
        assert got[1] == -np.inf and idx.ravel()[777] == 255 and (np.delete(idx.ravel(), 777) == -1).all()


def test_constant_map():
    """far == near: (log v - near) / 0 is 0 / 0, every colour the NaN's (0, 0, 0).  near and far are the same f32 log of the same quantile,
    and log v is that log again, so the numerator is exactly 0."""
    data = np.full(2048, 3.7, np.float32)
    got, ref = check_range(data)
    assert got[0] == got[1]
    L = _L()
    lut = torch.tensor(V.ramp_lut(), device=_dev())
    col = run_color_map(_on_device(data), (2, 32, 32), L.VSV_MODE_DEPTH, torch.tensor(got, device=_dev()), lut, u8=False)
    assert not col.any()


def test_rank_rounding():
    """The jump sits exactly at the f32 rank of the 0.99 quantile; a rank formed in float64 would blend both sides of it."""
    data = V.rank_rounding_case()
    got, ref = check_range(data)
    assert not V.range_ok(got[0], np.float32(V.depth_range(data, rank_f64=True)["far"]), ref)


# ---- colour map: paths, modes, tables ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ((1, 32, 32), (3, 17, 33), (2, 24, 34), (5, 1, 4)))
def test_color_map_paths(shape):
    lo, hi = V.DEPTH_CASES["room"]
    data = V.log_uniform(shape, lo, hi, seed=sum(shape)).ravel()
    rng, _ = check_range(data)
    check_colors(data, shape, rng)


def test_color_map_misaligned_pointers():
    """A value or an output that is not 16-byte aligned goes through the single-element path: same result."""
    L = _L()
    shape = (2, 8, 8)
    data = V.log_uniform(shape, 0.5, 50.0, seed=1).ravel()
    rng = np.array([np.log(0.5), np.log(50.0)], np.float32)
    lut, r = torch.tensor(V.ramp_lut(), device=_dev()), torch.tensor(rng, device=_dev())
    want = run_color_map(_on_device(data), shape, L.VSV_MODE_DEPTH, r, lut, u8=False)
    assert same_bits(run_color_map(_on_device(data, 1), shape, L.VSV_MODE_DEPTH, r, lut, u8=False), want)
    assert same_bits(run_color_map(_on_device(data), shape, L.VSV_MODE_DEPTH, r, lut, u8=False, out_offset=1), want)
    want8 = run_color_map(_on_device(data), shape, L.VSV_MODE_DEPTH, r, lut, u8=True)
    assert np.array_equal(run_color_map(_on_device(data), shape, L.VSV_MODE_DEPTH, r, lut, u8=True, out_offset=3), want8)
    assert np.array_equal(want8, V.to_u8(want))


@pytest.mark.parametrize("shape", ((2, 32, 32), (1, 17, 33)))
def test_max_and_unit_modes(shape):
    L = _L()
    g = np.random.default_rng(2)
    conf = (1 + g.exponential(2.0, shape)).astype(np.float32)
    conf[0, 3, 3] = -1.0
    lutn = V.ramp_lut()
    lut = torch.tensor(lutn, device=_dev())
    col = run_color_map(_on_device(conf), shape, L.VSV_MODE_MAX, None, lut, u8=False)
    idx = ramp_index(col)
    x, bound = V.x_max(conf)
    assert V.index_ok(idx, x, bound) and idx.max() == 255 and idx[0, 3, 3] == 0 and same_bits(col, V.lookup(idx, lutn))
    conf[0, 5, 5] = np.nan          # torch.max propagates it: every x is NaN
    assert not run_color_map(_on_device(conf), shape, L.VSV_MODE_MAX, None, lut, u8=True).any()
    xs = g.uniform(-0.1, 1.1, shape).astype(np.float32)
    xs[0, 0, :4] = (0.0, 1.0, np.nan, 255.0 / 256.0)
    col = run_color_map(_on_device(xs), shape, L.VSV_MODE_UNIT, None, lut, u8=False)
    assert np.array_equal(ramp_index(col), V.index_of(xs)) and ramp_index(col)[0, 0, :4].tolist() == [0, 255, -1, 255]      # x * 256 is exact


def test_apply_color_map_colours_last():
    """apply_color_map ([*batch] -> [*batch, 3]) and apply_color_map_to_image ([*batch, H, W] -> [*batch, 3, H, W]) against lut[idx]."""
    from vicasplat_amd.visualization import color_map
    g = np.random.default_rng(3)
    xs = g.uniform(-0.1, 1.1, (2, 5, 7)).astype(np.float32)
    xs[1, 2, 3] = np.nan
    lut = color_map.color_table("magma")
    want = V.lookup(V.index_of(xs), lut)                      # [2, 3, 5, 7]; x * 256 is exact in f32
    x = torch.tensor(xs, device=_dev())
    image = color_map.apply_color_map_to_image(x, "magma")
    assert image.shape == (2, 3, 5, 7) and same_bits(image.cpu().numpy(), want)
    last = color_map.apply_color_map(x, "magma")
    assert last.shape == (2, 5, 7, 3) and last.is_contiguous() and same_bits(last.cpu().numpy(), np.moveaxis(want, 1, -1))
    assert not last[1, 2, 3].any() and same_bits(color_map.apply_color_map(x[0, 0], "magma").cpu().numpy(), np.moveaxis(want, 1, -1)[0, 0])


# ---- frames --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", ((17, 33), (32, 32)))
@pytest.mark.parametrize("gap", (8, 0))
def test_video_frames(H, W, gap):
    L = _L()
    M = 3
    g = np.random.default_rng(H + gap)
    rgb = g.uniform(-0.2, 1.2, (M, 3, H, W)).astype(np.float32)
    rgb[1, 2, 4, 5] = np.nan
    depth = V.log_uniform((M, H, W), 0.5, 50.0, seed=W + gap)
    depth[2, 1, 1] = -1.0
    rng, _ = check_range(depth.ravel())
    lutn = V.ramp_lut()
    lut, r = torch.tensor(lutn, device=_dev()), torch.tensor(rng, device=_dev())
    d_rgb, d_depth = _on_device(rgb).reshape(M, 3, H, W), _on_device(depth)
    idx = ramp_index(run_color_map(d_depth, (M, H, W), L.VSV_MODE_DEPTH, r, lut, u8=False))
    x, bound = V.x_depth(depth, rng[0], rng[1])
    assert V.index_ok(idx, x, bound) and idx[2, 1, 1] == -1
    Hf = 2 * H + gap
    whole, out = _guarded(M * 3 * Hf * W, torch.uint8)
    L.call("vsv_video_frames", _dev(), L.ptr(d_rgb), L.ptr(d_depth), M, H, W, gap, L.ptr(r), L.ptr(lut), L.ptr(out))
    torch.cuda.synchronize()
    assert _intact(whole, M * 3 * Hf * W)
    frames = out.cpu().numpy().reshape(M, 3, Hf, W)
    assert np.array_equal(frames, V.frames(rgb, idx, lutn, gap))
    expr = (d_rgb.clip(min=0, max=1) * 255).type(torch.uint8).cpu().numpy()        # torch's own expression on the device
    ok = ~np.isnan(rgb)
    assert np.array_equal(frames[:, :, :H][ok], expr[ok]) and frames[1, 2, 4, 5] == 0 and (frames[:, :, H:H + gap] == 255).all()
    assert frames[2, :, H + gap + 1, 1].tolist() == [0, 0, 0]


# ---- reproducibility and stream behaviour -------------------------------------------------------------------------------------------------------
def _pipeline(depth, rgb, lut):
    from vicasplat_amd import _lib as L, ops
    rng, stats = ops.depth_range(depth, return_order_stats=True)
    return (rng, stats, ops.color_map(depth, lut, L.VSV_MODE_DEPTH, rng), ops.color_map(depth, lut, L.VSV_MODE_MAX, out_dtype=torch.uint8),
            ops.video_frames(rgb, depth, rng, lut, 8))


def test_reproducible_sync_free_and_capturable():
    from vicasplat_amd.visualization.color_map import device_table
    g = torch.Generator(device="cpu").manual_seed(0)
    depth = torch.tensor(V.log_uniform((12, 96, 128), 0.5, 50.0, seed=8), device=_dev())
    rgb = torch.rand(12, 3, 96, 128, generator=g).to(_dev())
    lut = device_table("turbo", _dev())
    first = _pipeline(depth, rgb, lut)            # (also loads the library and the table before the detector is armed)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = _pipeline(depth, rgb, lut)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert torch.equal(a.view(torch.uint8) if a.dtype == torch.uint8 else a.view(torch.int32), b.view(torch.uint8) if b.dtype == torch.uint8 else b.view(torch.int32))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _pipeline(depth, rgb, lut)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _pipeline(depth, rgb, lut)
    other = torch.tensor(V.log_uniform((12, 96, 128), 0.01, 100.0, seed=9), device=_dev())
    eager = _pipeline(other, rgb, lut)
    depth.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(captured, eager):
        assert torch.equal(a, b) or (a.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32)))
    assert not torch.equal(eager[0], first[0])


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
def test_vis_depth_map_and_confidence_map_against_golden():
    import os
    from vicasplat_amd.misc import utils
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "viz.npz"))
    d = G["depth_room"]
    ref = V.depth_range(d)
    err = (V.K * V.EPS * ref["mag_near"], V.K * V.EPS * ref["mag_far"])
    x, bound = V.x_depth(d, ref["near"], ref["far"], range_err=err)
    out = V.band(x, bound)
    got = utils.vis_depth_map(torch.tensor(d, device=_dev())).cpu().numpy()
    assert got.shape == G["vis_room"].shape and out.mean() <= V.EXCLUSION_CAP
    keep = np.broadcast_to(~out[:, None], got.shape)
    assert same_bits(got[keep], G["vis_room"][keep])
    x, bound = V.x_max(G["conf"])
    out = V.band(x, bound)
    got = utils.confidence_map(torch.tensor(G["conf"], device=_dev())).cpu().numpy()
    keep = np.broadcast_to(~out[:, None], got.shape)
    assert out.mean() <= V.EXCLUSION_CAP and same_bits(got[keep], G["vis_conf"][keep])
    assert torch.equal(utils.inverse_normalize(torch.full((3, 2, 2), -1.0, device=_dev())), torch.zeros(3, 2, 2, device=_dev()))


def test_render_projections_against_the_oracle():
    """A few isotropic Gaussians seen along the three axes, against the C oracle rasterizer given the restatement's cameras; the colour
    tolerance of tests/test_raster_gpu.py (2e-5, a share of 2e-4 of the values may flip an alpha threshold, none by 2e-2).  Measured:
    max |d colour| 9.5e-7 / 7.8e-7 / 4.2e-7 along x / y / z."""
    from oracle import raster_ref as rr
    from vicasplat_amd.model.types import Gaussians
    from vicasplat_amd.visualization.validation_in_3d import render_projections
    g = np.random.default_rng(0)
    P, res = 12, 64
    means = g.uniform(-1, 1, (1, P, 3)).astype(np.float32)
    sigma = g.uniform(0.05, 0.25, P).astype(np.float32)
    cov = (sigma[:, None, None] ** 2 * np.eye(3, dtype=np.float32))[None]
    sh = g.uniform(0.2, 2.0, (1, P, 3, 1)).astype(np.float32)
    opac = g.uniform(0.3, 0.95, (1, P)).astype(np.float32)
    T = lambda a: torch.tensor(a, device=_dev())
    got = render_projections(Gaussians(T(means), T(cov), T(sh), T(opac)), res).cpu().numpy()
    assert got.shape == (1, 3, 3, res, res)
    lo, hi = V.equal_aabb_with_margin(means.min(1), means.max(1))
    for axis in range(3):
        E, w, h, near, far = V.projection_cameras(lo, hi, axis)
        s = V.orthographic_setup(E, w, h, near, far, fov_degrees=10.0)
        PT = np.transpose(rr.get_projection_matrix(s["near"].astype(np.float32), s["far"].astype(np.float32), np.full(1, s["fov_x"], np.float32),
                                                   s["fov_y"].astype(np.float32)), (0, 2, 1)).astype(np.float32)
        view = np.transpose(np.linalg.inv(s["extrinsics"]), (0, 2, 1)).astype(np.float32)
        full = np.matmul(view.astype(np.float64), PT.astype(np.float64)).astype(np.float32)
        cam = rr.Camera(np.ascontiguousarray(view[0].reshape(16)), np.ascontiguousarray(full[0].reshape(16)), np.ascontiguousarray(PT[0].reshape(16)),
                        np.ascontiguousarray(s["extrinsics"][0, :3, 3].astype(np.float32)), float(s["tan_fov_x"]), float(s["tan_fov_y"][0]))
        o = rr.rasterize_forward(cam, res, res, np.zeros(3, np.float32), means[0], rr.cov6(cov[0]), np.ascontiguousarray(np.transpose(sh[0], (0, 2, 1))),
                                 opac[0], sh_degree=0)
        diff = np.abs(got[0, axis] - o["color"])
        print(f"axis {axis}: max |d colour| {diff.max():.2e}, lit {float((o['color'] > 0).mean()):.2f}")
        assert (o["color"] > 0).mean() > 0.02 and (diff > 2e-5).mean() <= 2e-4 and diff.max() < 2e-2


def test_validation_step_and_video_on_the_tiny_encoder():
    import json
    import os
    from oracle import chain
    from oracle import encoder_ref as er
    from vicasplat_amd import callers
    from vicasplat_amd.model.decoder import DecoderSplattingCUDACfg, get_decoder
    from vicasplat_amd.model.encoder import default_cfg, get_encoder
    d = _dev()
    shapes = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shapes_tiny.json")))
    m, _ = get_encoder(default_cfg(enc_depth=2, dec_embed_dim=192, dec_num_heads=3))
    m.load_state_dict(er.golden_weights(shapes, seed=0), strict=True)
    m = m.to(d).eval().requires_grad_(False)
    m.set_compute_dtype("split")
    image, K = er.synthetic_input(1, 2, 256, 0)
    E, Kt, near, far = (torch.tensor(a, dtype=torch.float32, device=d)[None] for a in chain.config1_targets(2))
    ctx = dict(image=image.to(d), intrinsics=K.to(d), extrinsics=E, near=near, far=far)
    tgt = dict(image=torch.rand(1, 2, 3, 256, 256, device=d), extrinsics=E, intrinsics=Kt, near=near, far=far)
    batch = dict(context=ctx, target=tgt)
    dec = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", [0.0, 0.0, 0.0], False)).to(d)
    with torch.no_grad():
        outs = m(ctx, compute_viewspace_depth=True)
    encoder = lambda c, **kw: outs           # one encoder pass: the pieces below are compared bit for bit
    out = callers.validation_step(encoder, dec, batch)
    assert list(out) == ["psnr", "ssim", "comparison", "projections", "video"] and all(v.is_cuda for v in out.values())
    assert out["comparison"].shape == (3, 2 * 256 + 8, 5 * 256 + 4 * 8) and out["projections"].shape == (3, 256, 3 * 256 + 2 * 8)
    assert out["video"].dtype == torch.uint8 and out["video"].shape == (58, 3, 2 * 256 + 8, 256)
    assert bool(torch.isfinite(out["comparison"]).all()) and 0 <= float(out["comparison"].min()) and float(out["comparison"].max()) <= 1
    # the video against its pieces: the same trajectory rendered here, packed by the frame kernel, looped by hand
    F = 30
    t = torch.linspace(0, 1, F, device=d)
    t = (torch.cos(torch.pi * (t + 1)) + 1) / 2
    Ev = callers.interpolate_extrinsics(E[:1, 0], E[:1, -1], t)
    Kv = callers.interpolate_intrinsics(K.to(d)[:1, 0].float(), K.to(d)[:1, -1].float(), t)
    with torch.no_grad():
        o = dec.forward(outs["gaussians"], Ev, Kv, near[:, :1].expand(-1, F), far[:, :1].expand(-1, F), (256, 256), "depth")
    frames = callers.depth_video_frames(o.color[0], o.depth[0])
    assert torch.equal(out["video"][:F], frames) and torch.equal(out["video"][F:], frames.flip(0)[1:-1])
    assert torch.equal(frames[:, :, :256], (o.color[0].clip(min=0, max=1) * 255).type(torch.uint8)) and bool((frames[:, :, 256:264] == 255).all())
    # the comparison's last column is vis_depth_map of the rendered target depth; its first the context images
    from vicasplat_amd.misc import utils
    assert torch.equal(out["comparison"][:, :256, :256], utils.inverse_normalize(ctx["image"][0, 0]))
    to = dec.forward(outs["gaussians"], E, Kt, near, far, (256, 256), "depth")
    assert torch.equal(out["comparison"][:, :256, -256:], utils.vis_depth_map(to.depth[0])[0])
