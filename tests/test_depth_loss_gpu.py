"""The HIP depth-smoothness loss (csrc/depth_loss.hip behind callers.LossDepth) against the float64 reference of tests/depth_loss_f64.py.
-m gpu.

Shapes: 24 x 20 (rows of 16-byte multiples: the vector path, two row bands), 17 x 13 (odd: the generic path), 2 x 2 and 3 x 3 (the smallest
legal ones; the second derivative is refused on 2 x 2), 17 x 65 (one row more than the kernel's row band, one column more than its column
chunk, generic path) and 20 x 68 (the same crossing on the vector path); N = 1, 3; the four configurations of depth_loss_f64.CONFIGS.
Inputs come from depth_loss_f64.make_inputs, every decision of which is unambiguous (asserted): no element is exempted from any
comparison.

Criterion: every element of loss and d_depth within 4 max(r32, 1) 2^-24 mag = 4 units of the reference (depth_loss_f64.R32, no other
floor).  Measured on an MI355X, max |gpu - ref| / (2^-24 mag) (`-s` prints it per case), beside the torch-f32 ratio r32 of
tests/test_depth_loss_cpu.py:

    output    r32    bound   gpu
    loss      0.07   4.00    0.10
    d_depth   0.34   4.00    0.39

One training step of the tiny encoder with LossDepth(sigma_image 4, second derivative) at 64 x 64, two target views: loss_depth of the HIP
backend 0.003 units from float64 on the depth it rendered, the torch backend 0.000.
"""
import types

import numpy as np
import pytest
import torch

import depth_loss_f64 as D

pytestmark = pytest.mark.gpu

NAMES = ("loss", "d_depth")


def _dev():
    return torch.device("cuda:0")


def _edge_shapes():
    from vicasplat_amd import ops
    band, chunk = ops.DEPTH_SMOOTH_BAND_ROWS, ops.DEPTH_SMOOTH_CHUNK_COLS
    assert (band + 1) % 4 and (chunk + 1) % 4 and (chunk + 4) % 4 == 0
    return [(band + 1, chunk + 1), (band + 4, chunk + 4)]


SHAPES = [(24, 20), (17, 13), (2, 2), (3, 3), (17, 65), (20, 68)]


def _run(z, sigma, second, backend="hip", up=None, misalign=False):
    """loss and d_depth of callers.depth_smoothness_loss on the device -> dict of float64 numpy arrays."""
    from vicasplat_amd import callers
    t = {k: torch.tensor(v, device=_dev()) for k, v in z.items()}
    if misalign:           # the same values four bytes past a 16-byte boundary
        for k in ("depth", "image"):
            buf = torch.empty(t[k].numel() + 1, device=_dev())
            buf[1:] = t[k].reshape(-1)
            t[k] = buf[1:].view(t[k].shape)
            assert t[k].data_ptr() % 16 == 4 and t[k].is_contiguous()
    depth = t["depth"].requires_grad_(True)
    loss = callers.depth_smoothness_loss(depth, t["near"], t["far"], t["image"], D.WEIGHT, sigma, second, backend=backend)
    (g,) = torch.autograd.grad(loss if up is None else loss * up, depth)
    return dict(loss=loss.detach().double().cpu().numpy(), d_depth=g.double().cpu().numpy())


def _ref(z, sigma, second, **kw):
    return D.depth_smooth(z["depth"], z["near"], z["far"], z["image"], sigma, second, **kw)


def _check(got, ref, tag, worst):
    for k in NAMES:
        u = D.units(got[k], ref, k)
        worst[k] = max(worst.get(k, 0.0), u)
        assert np.isfinite(got[k]).all(), (tag, k)
        assert u <= D.gpu_factor(k), (tag, k, u)


def test_shapes_cross_the_tile_edges():
    assert _edge_shapes() == SHAPES[4:]


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_depth_smooth_matches_float64(H, W, N):
    z = D.make_inputs(N, H, W, 100 + H + N)
    assert D.decisions_ok(z)
    worst = {}
    for sigma, second in D.CONFIGS:
        if min(H, W) < 2 + second:
            with pytest.raises(ValueError, match="too small"):
                _run(z, sigma, second)
            continue
        _check(_run(z, sigma, second), _ref(z, sigma, second), (sigma, second), worst)
    print(f"depth_smooth N={N} {H}x{W}", {k: round(v, 3) for k, v in worst.items()})


def test_the_entry_refuses_the_second_derivative_on_two_rows():
    """The C entry's own check (ops raises ValueError before it): a negative return with a message, through the loaded library."""
    import ctypes as C
    from vicasplat_amd import _lib
    L, p = _lib.lib(), C.c_void_p(16)
    assert L.vsl_depth_smooth_forward(p, p, p, None, 1, 2, 2, 0.0, 1, 0.25, p, 64, p, p, None) < 0 and b"too small" in L.vs_last_error()


@pytest.mark.parametrize("exact_logs", [False, True])
def test_ties_at_the_clamp_pass_half(exact_logs):
    """Depths bit-equal to f32(log far) and f32(log near): half the gradient the same neighbourhood passes when the clamp is not met (the
    reference with the tie's factor at 1 is exactly twice the reference there), and the bound holds at them as everywhere."""
    z = D.make_inputs(2, 17, 13, 41, exact_logs=exact_logs)
    hi, lo = [(1, 2, 3), (1, 2, 4), (1, 16, 12), (0, 9, 9)], [(0, 4, 4), (0, 0, 0), (0, 5, 4), (1, 8, 2)]
    z = D.with_ties(z, hi, lo)
    assert D.decisions_ok(z)
    tied = np.zeros(z["depth"].shape, bool)
    for idx in hi + lo:
        tied[idx] = True
    worst = {}
    for sigma, second in D.CONFIGS:
        ref, full, got = _ref(z, sigma, second), _ref(z, sigma, second, mutate="tie_full"), _run(z, sigma, second)
        assert np.array_equal(full["d_depth"][tied], 2 * ref["d_depth"][tied]) and (ref["d_depth"][tied] != 0).sum() >= 6
        _check(got, ref, (sigma, second), worst)
        nz = tied & (ref["d_depth"] != 0)       # 4 units of the half are far from the whole: the factor is one half, not 1 and not 0
        assert (np.abs(got["d_depth"][nz] - ref["d_depth"][nz]) < 0.01 * np.abs(ref["d_depth"][nz])).all()
    print(f"ties exact_logs={exact_logs}", {k: round(v, 3) for k, v in worst.items()})


def test_a_view_beyond_far_has_an_exactly_zero_gradient():
    z = D.make_inputs(3, 17, 20, 42)
    z["depth"][1] = (7.0 + z["depth"][1]).astype(np.float32)
    assert D.decisions_ok(z)
    for sigma, second in D.CONFIGS:
        ref, got = _ref(z, sigma, second), _run(z, sigma, second)
        _check(got, ref, (sigma, second), {})
        assert (got["d_depth"][1] == 0.0).all() and (ref["d_depth"][1] == 0.0).all() and (got["d_depth"][0] != 0.0).any()


def test_equal_unclamped_neighbours_have_a_finite_zero_subgradient():
    z = D.make_inputs(1, 17, 13, 43)
    z["depth"][0, 5, 5:8] = 2.0          # inside (log near, log far): three equal neighbours along W ...
    z["depth"][0, 9:12, 3] = 2.5         # ... and along H: first and second differences that are exactly 0
    ln, lf = D.f32_logs(z["near"], z["far"])
    assert D.decisions_ok(z) and ln[0] < 2.0 and 2.5 < lf[0]
    for sigma, second in D.CONFIGS:
        ref, got = _ref(z, sigma, second), _run(z, sigma, second)
        assert ref["tx"].v[0, 5, 5] == 0 and ref["ty"].v[0, 9, 3] == 0 and (second or (ref["tx"].v[0, 5, 6] == 0 and ref["ty"].v[0, 10, 3] == 0))
        _check(got, ref, (sigma, second), {})


def test_one_nan_depth_makes_the_loss_nan_and_nothing_else():
    z = D.make_inputs(2, 17, 13, 44)
    bad = dict(z, depth=z["depth"].copy())
    bad["depth"][1, 3, 4] = np.nan
    for sigma, second in D.CONFIGS:
        for backend in ("hip", "torch"):
            assert np.isnan(_run(bad, sigma, second, backend)["loss"]), (sigma, second, backend)
    _check(_run(z, D.SIGMA, True), _ref(z, D.SIGMA, True), "after", {})          # the library is usable afterwards


def test_upstream_factor():
    z = D.make_inputs(3, 24, 20, 45)
    for sigma, second in D.CONFIGS:
        a, c = _run(z, sigma, second), _run(z, sigma, second, up=4.0)          # a power of two: exact
        assert np.array_equal(c["d_depth"], 4.0 * a["d_depth"])
        _check(_run(z, sigma, second, up=-3.5), _ref(z, sigma, second, up=-3.5), (sigma, second), {})


@pytest.mark.parametrize("H,W", [(17, 65), (20, 68)])
def test_two_runs_are_bit_identical(H, W):
    z = D.make_inputs(3, H, W, 46)
    for sigma, second in D.CONFIGS:
        a, b = _run(z, sigma, second), _run(z, sigma, second)
        for k in NAMES:
            assert np.array_equal(a[k], b[k]), (sigma, second, k)


def test_misaligned_rows_take_the_generic_path_to_the_same_bits():
    """W % 4 == 0 but the tensors start four bytes past a 16-byte boundary: no 16-byte load is possible, the entry takes the generic path,
    and both paths form every value in the same order."""
    z = D.make_inputs(3, 20, 68, 47)
    for sigma, second in D.CONFIGS:
        a, b = _run(z, sigma, second), _run(z, sigma, second, misalign=True)
        for k in NAMES:
            assert np.array_equal(a[k], b[k]), (sigma, second, k)


def test_forward_and_backward_do_not_synchronise():
    from vicasplat_amd import callers
    z = D.make_inputs(2, 24, 20, 48)
    t = {k: torch.tensor(v, device=_dev()) for k, v in z.items()}
    depth = t["depth"].requires_grad_(True)
    callers.depth_smoothness_loss(depth, t["near"], t["far"], t["image"], D.WEIGHT, D.SIGMA, True).backward()        # warm: loads the library
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        callers.depth_smoothness_loss(depth, t["near"], t["far"], t["image"], D.WEIGHT, D.SIGMA, True).backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.isfinite(depth.grad).all()


def test_bad_inputs_raise():
    from vicasplat_amd import ops
    z = D.make_inputs(2, 5, 8, 49)
    t = {k: torch.tensor(v, device=_dev()) for k, v in z.items()}
    with pytest.raises(ValueError, match=r"depth \[N, H, W\]"):
        ops.depth_smooth_forward(t["depth"][0], t["near"], t["far"])
    with pytest.raises(ValueError, match="near of shape"):
        ops.depth_smooth_forward(t["depth"], t["near"][:1], t["far"])
    with pytest.raises(ValueError, match="image of shape"):
        ops.depth_smooth_forward(t["depth"], t["near"], t["far"], t["image"][:, :2], 1.0)
    with pytest.raises(ValueError, match="image .* is needed"):
        ops.depth_smooth_forward(t["depth"], t["near"], t["far"], None, 1.0)
    with pytest.raises(ValueError, match="floating-point"):
        ops.depth_smooth_forward(t["depth"].int(), t["near"], t["far"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.depth_smooth_forward(t["depth"], t["near"].cpu(), t["far"])
    with pytest.raises(ValueError, match="scalar"):
        ops.depth_smooth_backward(t["depth"], torch.ones(2, device=_dev()))
    loss, unit = ops.depth_smooth_forward(t["depth"], t["near"], t["far"], need_grad=False)
    assert unit is None and bool(torch.isfinite(loss))


# ---- the full path: tiny encoder -> HIP rasterizer -> LossDepth -> dL_ddepth -> encoder, one step per backend from the same state ----
def test_training_step_with_loss_depth_on_the_tiny_encoder():
    import bench
    from oracle import encoder_ref as er
    from test_train_gpu import _tiny_model
    from vicasplat_amd import callers
    from vicasplat_amd.model.decoder import DecoderSplattingCUDACfg, get_decoder
    d = _dev()
    B, Vn, Vt, S = 1, 2, 2, 64
    img, K = er.synthetic_input(B, Vn, S, 3)
    tE, tK, tn, tf = bench.target_cameras(B, Vt, d)
    target = torch.rand(B, Vt, 3, S, S, generator=torch.Generator().manual_seed(0)).to(d)
    res, seen = {}, {}
    for backend in ("hip", "torch"):
        m, _ = _tiny_model("split")
        dec = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", [0.0, 0.0, 0.0], False)).to(d)
        batch = dict(context=dict(image=img.to(d), intrinsics=K.to(d)), target=dict(image=target, extrinsics=tE, intrinsics=tK, near=tn, far=tf))
        opt, _ = callers.configure_optimizer(m, lr=4e-5, backbone_lr_multiplier=0.25)
        loss_fn = callers.LossDepth(D.WEIGHT, D.SIGMA, True, backend=backend)

        def depth(render, batch, out, loss_fn=loss_fn, backend=backend):
            seen[backend] = render.depth.detach().float().cpu().numpy()
            return loss_fn(render, batch, out)

        res[backend] = callers.training_step(m, dec, batch, opt, compute_dtype="split", extra_losses=[depth])
    for backend, r in res.items():
        assert "loss_depth" in r and float(r["loss_depth"]) > 0
        assert not r["skipped"] and bool(torch.isfinite(r["grad_norm"]))
        ref = D.depth_smooth(seen[backend].reshape(B * Vt, S, S), tn.cpu().numpy().reshape(-1), tf.cpu().numpy().reshape(-1),
                             target.cpu().numpy().reshape(B * Vt, 3, S, S), D.SIGMA, True)
        lim = D.gpu_factor("loss") * D.U32 * float(ref["loss_mag"])
        print(f"training step, {backend}: loss_depth {float(r['loss_depth']):.8f}, "
              f"{abs(float(r['loss_depth']) - float(ref['loss'])) / (D.U32 * float(ref['loss_mag'])):.3f} units from float64; grad_norm {float(r['grad_norm']):.4f}")
        assert abs(float(r["loss_depth"]) - float(ref["loss"])) <= lim, backend
    if np.array_equal(seen["hip"], seen["torch"]):
        assert abs(float(res["hip"]["loss_depth"]) - float(res["torch"]["loss_depth"])) <= 2 * lim
    # the depth term moved the step: without it the gradient norm is another
    m, _ = _tiny_model("split")
    dec = get_decoder(DecoderSplattingCUDACfg("splatting_cuda", [0.0, 0.0, 0.0], False)).to(d)
    batch = dict(context=dict(image=img.to(d), intrinsics=K.to(d)), target=dict(image=target, extrinsics=tE, intrinsics=tK, near=tn, far=tf))
    opt, _ = callers.configure_optimizer(m, lr=4e-5, backbone_lr_multiplier=0.25)
    base = callers.training_step(m, dec, batch, opt, compute_dtype="split")
    assert abs(float(base["grad_norm"]) - float(res["hip"]["grad_norm"])) > 1e-3 * float(base["grad_norm"])
