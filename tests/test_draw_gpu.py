"""The vector-drawing kernels (csrc/draw.hip, include/vicasplat_draw.h) on the GPU, through the binding, against the float64 restatement
of tests/draw_f64.py, and the callers built on them end to end.

Lattice cases (axis-aligned records, every coordinate, width and radius a multiple of 1/16, colours and image values multiples of 1/8,
one colour per case so that the quotient sum / count is exact too -- or several colours with num_passes = 0, where there is no quotient):
every element equals the float64 run rounded to f32; samples fall exactly on the thresholds.  General cases: draw_f64.check -- a pixel that
is not `unsure` satisfies |out - f64| <= FACTOR 2^-24 mag + (amb / 64) spread; at most 2 % of a case's pixels are unsure and at most 10 % have
amb > 0 (tests/test_draw_cpu.py asserts the same of the f32 run of the restatement on every case).  Every output sits between sentinel-
filled guard bands, on an aligned and on a misaligned base.

Shapes straddle the tile (VSG_TILE_H x VSG_TILE_W), record counts the scan chunk (VSG_SCAN_CHUNK); a list repeated 64 times forces several
LDS rounds (VSG_LIST_CAP) with the result of the plain list.

Measured on an MI355X (`-s` prints them): every lattice case 0 differing bits; general cases: the largest error on unambiguous pixels 0.37 to
0.44 of 2^-24 mag (bound 4), at most 0.39 % of a case's pixels ambiguous and 0.2 % unsure, the largest error 0.11 of its bound; the 20-camera plot
per layer and projection at most 0.13 of 2^-24 mag, 0.02 % ambiguous; draw_cameras against the reference's golden: 0 elements differ.
"""
import numpy as np
import pytest
import torch

import draw_f64 as D

pytestmark = pytest.mark.gpu
GUARD = 64
SENTINEL = -7.25


def _dev():
    return torch.device("cuda:0")


def _L():
    from vicasplat_amd import _lib
    _lib.lib()
    return _lib


def _t(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=_dev())


def _offsets(recs):
    return _t(np.concatenate(([0], np.cumsum([len(r) for r in recs]))), torch.int32)


def run(kind, images, recs, cap="round", passes=1, misalign=0, inplace=False):
    """images [B, 3, H, W] f32, recs: one record array per image -> out [B, 3, H, W] as numpy, through ops.draw_lines / ops.draw_points
    into a guarded output whose base sits `misalign` elements past a 256-byte boundary."""
    from vicasplat_amd import ops
    images = np.asarray(images, np.float32)
    n = images.size
    whole = torch.full((n + 2 * GUARD + misalign,), SENTINEL, dtype=torch.float32, device=_dev())
    out = whole[GUARD + misalign:GUARD + misalign + n].view(images.shape)
    if inplace:
        out.copy_(_t(images))
    src = out if inplace else _t(images)
    floats = 8 if kind == "lines" else 7
    rec = _t(np.concatenate([np.asarray(r, np.float32).reshape(-1, floats) for r in recs]))
    if kind == "lines":
        res = ops.draw_lines(src, rec, _offsets(recs), cap=cap, num_passes=passes, out=out)
    else:
        res = ops.draw_points(src, rec, _offsets(recs), num_passes=passes, out=out)
    torch.cuda.synchronize()
    assert res.data_ptr() == out.data_ptr()
    assert bool((whole[:GUARD + misalign] == SENTINEL).all()) and bool((whole[GUARD + misalign + n:] == SENTINEL).all()), "guard band written"
    return out.cpu().numpy().copy()


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


_REF = {}


def reference(key, kind, image, rec, cap, passes):
    if key not in _REF:
        _REF[key] = D.render(kind, image, rec, cap, passes, np.float64)
    return _REF[key]


def tile_shapes():
    L = _L()
    th, tw = L.VSG_TILE_H, L.VSG_TILE_W
    return [(1, 1), (1, 7), (7, 1), (th, tw), (th + 1, tw), (th, tw + 1), (th - 1, tw), (th, tw - 1), (33, 47)]


# ---- lattice cases: bit for bit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,cap", [("lines", "butt"), ("lines", "round"), ("lines", "square"), ("points", None)])
def test_lattice_shapes_equal_float64(kind, cap):
    for k, shape in enumerate(tile_shapes()):
        image = D.lattice_image(shape, 20 + k)
        rec = D.lattice_case(kind, shape, 6, 30 + k, cap)
        ref = reference(("lat", kind, cap, shape), kind, image, rec, cap, 1)
        want = ref["out"].astype(np.float32)
        a = run(kind, image[None], [rec], cap, 1)[0]
        b = run(kind, image[None], [rec], cap, 1, misalign=1)[0]
        assert same_bits(a, want), (kind, cap, shape, float(np.abs(a - want).max()))
        assert same_bits(a, b), (kind, cap, shape)


def test_lattice_record_counts_straddle_the_scan_chunk():
    L = _L()
    shape = (L.VSG_TILE_H + 1, L.VSG_TILE_W + 1)
    chunk = L.VSG_SCAN_CHUNK
    for n in (1, chunk - 1, chunk, chunk + 1, 2 * chunk + 88):
        image = D.lattice_image(shape, n)
        one = D.lattice_case("lines", shape, n, 100 + n, "butt")           # one colour: exact with the refinement
        ref = reference(("count", n), "lines", image, one, "butt", 1)
        assert same_bits(run("lines", image[None], [one], "butt", 1)[0], ref["out"].astype(np.float32)), n
        many = one.copy()                                                     # a colour per record: exact without it, and the order shows
        many[:, 5:8] = np.random.default_rng(n).integers(0, 9, (n, 3)) / 8.0
        ref0 = reference(("count0", n), "lines", image, many, "butt", 0)
        assert same_bits(run("lines", image[None], [many], "butt", 0)[0], ref0["out"].astype(np.float32)), n
        pts = D.lattice_case("points", shape, n, 200 + n)
        refp = reference(("countp", n), "points", image, pts, None, 1)
        assert same_bits(run("points", image[None], [pts], None, 1)[0], refp["out"].astype(np.float32)), n


def test_whole_image_cover_refines_nothing():
    shape = (19, 37)
    image = D.lattice_image(shape, 3)
    rec = D.lines_rec([[-10.0, 9.0]], [[60.0, 9.0]], 100.0, [[0.25, 0.5, 0.75]])
    for passes in (0, 1):
        out = run("lines", image[None], [rec], "butt", passes)[0]
        assert same_bits(out, np.broadcast_to(np.array([0.25, 0.5, 0.75], np.float32)[:, None, None], out.shape))
    ref = reference("cover", "lines", image, rec, "butt", 1)
    assert not ref["mask"].any() and same_bits(out, ref["out"].astype(np.float32))


def test_edge_records():
    """A zero-length line under each cap, a NaN record among valid ones, an infinite width: the float64 run, bit for bit."""
    shape = (17, 23)
    image = D.lattice_image(shape, 4)
    s = D.S16
    for cap in D.CAPS:
        rec = D.lines_rec([[8 + s, 8 + s], [3 + s, 12 + s]], [[8 + s, 8 + s], [19 + s, 12 + s]], [6.0, 2.0], [[1, 0.5, 0.25]])
        ref = reference(("zero", cap), "lines", image, rec, cap, 1)
        out = run("lines", image[None], [rec], cap, 1)[0]
        assert same_bits(out, ref["out"].astype(np.float32)), cap
        covered = ref["alpha"][5:11, 5:12].max() > 0
        assert covered == (cap == "round"), cap
    nan = np.float32("nan")
    valid = D.lines_rec([[3 + s, 5 + s]], [[19 + s, 5 + s]], 3.0, [[0.5, 0.5, 1]])
    for column in range(5):
        bad = D.lines_rec([[2 + s, 9 + s]], [[20 + s, 9 + s]], 4.0, [[0.5, 0.5, 1]])
        bad[0, column] = nan
        rec = np.concatenate((valid, bad, valid + np.array([0, 6, 0, 6, 0, 0, 0, 0], np.float32)))
        ref = reference(("nan", column), "lines", image, rec, "round", 1)
        assert same_bits(run("lines", image[None], [rec], "round", 1)[0], ref["out"].astype(np.float32)), column
        assert same_bits(ref["out"].astype(np.float32), D.render("lines", image, rec[[0, 2]], "round", 1)["out"].astype(np.float32))
    for column in range(4):
        bad = D.points_rec([[9 + s, 9 + s]], 4.0, 1.0, [[0.5, 0.5, 1]])
        bad[0, column] = nan
        rec = np.concatenate((D.points_rec([[5 + s, 5 + s]], 3.0, 0.0, [[0.5, 0.5, 1]]), bad))
        assert same_bits(run("points", image[None], [rec], None, 1)[0], D.render("points", image, rec, None, 1)["out"].astype(np.float32))
    inf = D.lines_rec([[4 + s, 8 + s]], [[15 + s, 8 + s]], np.float32("inf"), [[1, 0.25, 0]])
    for cap in ("butt", "round"):
        ref = D.render("lines", image, inf, cap, 1)
        assert ref["alpha"].max() == 1 and same_bits(run("lines", image[None], [inf], cap, 1)[0], ref["out"].astype(np.float32)), cap


# ---- general cases -------------------------------------------------------------------------------------------------------------------
def _check_general(name, out, ref):
    ok, report = D.check(out, ref)
    print(f"\n  {name}: " + "  ".join(f"{k} {v:.3g}" for k, v in report.items()))
    assert report["unsure"] <= 0.02 and report["ambiguous"] <= 0.10, (name, report)
    assert ok, (name, report)


@pytest.mark.parametrize("name", list(D.GENERAL_CASES))
def test_general_cases_against_float64(name):
    kind, shape, build, cap = D.GENERAL_CASES[name]
    image, rec = D.general_image(shape, 5), build()
    ref = reference(("gen", name), kind, image, rec, cap, 1)
    out = run(kind, image[None], [rec], cap, 1)[0]
    _check_general(name, out, ref)
    assert same_bits(out, run(kind, image[None], [rec], cap, 1, misalign=3)[0])           # two runs, two bases
    assert same_bits(out, run(kind, image[None], [rec], cap, 1, inplace=True)[0])         # out == image
    ref0 = reference(("gen0", name), kind, image, rec, cap, 0)
    _check_general(name + " (no refinement)", run(kind, image[None], [rec], cap, 0)[0], ref0)
    # every record 64 times in a row: the same picture from a list that needs several LDS rounds
    L = _L()
    many = np.repeat(rec, 64, axis=0)
    assert len(many) > L.VSG_LIST_CAP
    assert same_bits(out, run(kind, image[None], [many], cap, 1)[0]), "a list processed in several rounds changed the result"


def test_batch_is_the_images_alone():
    """B = 3 with one empty list: each image as it is alone, the empty one copied through."""
    kind, shape, build, cap = D.GENERAL_CASES["lines_butt_47x33"]
    images = np.stack([D.general_image(shape, 6 + k) for k in range(3)])
    images[1, 0, 0, 0] = -0.0
    recs = [build(), np.zeros((0, 8), np.float32), D.general_lines(shape, 9, 77)]
    out = run(kind, images, recs, cap, 1)
    assert same_bits(out[1], images[1])
    for b in (0, 2):
        assert same_bits(out[b], run(kind, images[b:b + 1], [recs[b]], cap, 1)[0]), b
    pts = [D.general_rings(shape, 5, 1), D.general_rings(shape, 7, 2), np.zeros((0, 7), np.float32)]
    outp = run("points", images, pts, None, 1)
    assert same_bits(outp[2], images[2]) and same_bits(outp[0], run("points", images[:1], pts[:1], None, 1)[0])


def test_no_synchronisation_and_graph_replay():
    from vicasplat_amd import ops
    kind, shape, build, cap = D.GENERAL_CASES["lines_round_56x80"]
    image, rec = _t(D.general_image(shape, 5)[None]), _t(build())
    off = _offsets([rec])
    out = torch.empty_like(image)
    first = ops.draw_lines(image, rec, off, cap=cap, out=out).clone()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ops.draw_lines(image, rec, off, cap=cap, out=out)
        ops.draw_points(image, rec[:, :7].contiguous(), off, out=out)
        ops.draw_lines(image, rec, off, cap=cap, out=out)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), first.view(torch.int32))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.draw_lines(image, rec, off, cap=cap, out=out)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.draw_lines(image, rec, off, cap=cap, out=out)
    other_image, other_rec = _t(D.general_image(shape, 9)[None]), _t(D.general_lines(shape, len(rec), 99))
    eager = ops.draw_lines(other_image, other_rec, off, cap=cap)
    image.copy_(other_image)
    rec.copy_(other_rec)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), eager.view(torch.int32))


# ---- the camera plot and the validation step ----------------------------------------------------------------------------------------
def _camera_layers_check(R, E, K, colour, near, far, name):
    """draw_cameras on the HIP backend, layer by layer: every launch against the float64 run on that launch's own input; returns the final
    picture, the summed bound and the pixels left out."""
    from vicasplat_amd import ops
    from vicasplat_amd.visualization.drawing import cameras as C
    from vicasplat_amd.visualization.drawing.lines import line_records
    from vicasplat_amd.visualization.validation_in_3d import compute_equal_aabb_with_margin
    E, K, colour, near, far = (_t(v) for v in (E, K, colour, near, far))
    lo, hi = compute_equal_aabb_with_margin(*C.compute_aabb(E, K, near, far), margin=0.1)
    layers = C.camera_layers(E, K, colour, near, far, ((hi - lo).max() * 0.05)[None])
    planes = [[(k + 1) % 3, (k + 2) % 3] for k in range(3)]
    image = torch.zeros(3, 3, R, R, device=_dev())
    bound, left_out = np.zeros((3, 3, R, R)), np.zeros((3, R, R), bool)
    for i, (start, end, col) in enumerate(layers):
        recs = [line_records((R, R), _dev(), start[:, p], end[:, p], col, 2, torch.stack((lo[p[0]], hi[p[0]])), torch.stack((lo[p[1]], hi[p[1]])))
                for p in planes]
        before = image.cpu().numpy()
        image = ops.draw_lines(image, torch.cat(recs), _offsets(recs), cap="round", num_passes=1)
        after = image.cpu().numpy()
        for b in range(3):
            ref = D.render("lines", before[b], recs[b].cpu().numpy(), "round", 1)
            _check_general(f"{name} layer {i} projection {b}", after[b], ref)
            bound[b] += D.FACTOR * D.U * ref["mag"] + (ref["amb"] / 64.0)[None] * ref["spread"]
            left_out[b] |= ref["unsure"]
    whole = C.draw_cameras(R, E, K, colour, near, far)
    assert whole.is_cuda and same_bits(whole.cpu().numpy(), image.cpu().numpy()), "draw_cameras is not its layers in order"
    return image.cpu().numpy(), bound, left_out


def test_draw_cameras_20_cameras():
    E, K, colour, near, far = D.cameras(20, 8)
    _camera_layers_check(64, E, K, colour, near, far, "20 cameras")


def test_draw_cameras_against_the_reference_golden():
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "draw.npz"))
    out, bound, left_out = _camera_layers_check(32, z["cam_E"], z["cam_K"], z["cam_color"], z["cam_near"], z["cam_far"], "golden cameras")
    # the reference's own f32 run and this one each lie within the layers' bounds of float64; a later layer passes an earlier error on at most once
    err = np.abs(out.astype(np.float64) - z["cam_planes"])
    keep = ~left_out[:, None] & np.ones_like(err, bool)
    print(f"\n  against the reference: max |d| {err[keep].max():.3g} over {keep.mean():.3f} of the elements, {int((err[keep] > 0).sum())} differ")
    assert left_out.mean() <= 0.02 and (err[keep] <= 2 * bound[keep]).all()
    from vicasplat_amd.visualization.drawing import draw_cameras
    plain = draw_cameras(32, _t(z["cam_E"]), _t(z["cam_K"]), _t(z["cam_color"])).cpu().numpy()
    assert (np.abs(plain - z["cam_plain"]) > 1e-6).mean() <= 0.02


def test_validation_step_with_cameras_and_the_exaggerated_video():
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
    batch = dict(context=ctx, target=dict(image=torch.rand(1, 2, 3, 256, 256, device=d), extrinsics=E, intrinsics=Kt, near=near, far=far))
    decoder = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", [0.0, 0.0, 0.0], False)).to(d)
    with torch.no_grad():
        outs = m(ctx, compute_viewspace_depth=True)
    encoder = lambda c, **kw: outs           # one encoder pass: the two calls below are compared bit for bit
    base = callers.validation_step(encoder, decoder, batch)
    out = callers.validation_step(encoder, decoder, batch, cameras=True, extended_visualization=True)
    torch.cuda.synchronize()
    h, w = batch["context"]["image"].shape[-2:]
    assert tuple(out["cameras"].shape) == (3, 256, 3 * 256 + 2 * 8) and tuple(out["camera_traj"].shape) == (3, 256, 3 * 256)
    assert out["video_exaggerated"].dtype == torch.uint8 and tuple(out["video_exaggerated"].shape) == (300, 3, 2 * h + 8, w)
    assert set(out) == set(base) | {"cameras", "camera_traj", "video_exaggerated"}
    for k, v in base.items():
        assert torch.equal(v, out[k]), k
    assert float(out["cameras"].max()) == 1.0 and float(out["camera_traj"].max()) == 1.0 and bool(torch.isfinite(out["cameras"]).all())
    # the 300-view render leaves about 1.2 GB behind in reference cycles (the model and the decoder's buffers): collect them here, so that no
    # later test that reads the allocator's statistics sees them freed in the middle of its own measurement
    del out, base, outs, encoder, decoder, m, batch, ctx
    import gc
    gc.collect()
    torch.cuda.empty_cache()
