"""LPIPS-VGG without a GPU: the float64 restatement of tests/lpips_f64.py against callers.LossLpips (the torch backend), its analytic head
gradient against torch autograd, the two conventions of csrc/lpips.hip (zero-norm pixels, max-pool ties), and the C-ABI argument validation
of the vs_lpips_* entries."""
import ctypes as C

import pytest
import torch

import lpips_f64 as R
from vicasplat_amd import callers


def _pair(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 3, h, w, generator=g, dtype=torch.float64), torch.rand(n, 3, h, w, generator=g, dtype=torch.float64)


def test_restatement_matches_loss_lpips_in_float64():
    sd = R.fake_state_dict(0)
    a, b = _pair(2, 32, 48, 1)
    loss = callers.LossLpips(sd, weight=1.0)
    for name in [n for n, _ in loss.named_buffers()]:
        setattr(loss, name, getattr(loss, name).double())
    want = loss.distance(a, b)                                   # LossLpips always applies 2x - 1: normalize=True
    got = R.value(sd, a, b, normalize=True)
    torch.testing.assert_close(got, want, rtol=0, atol=1e-12)
    assert float(got.min()) > 0
    taps = R.features(sd, a, True)
    assert [t.shape[1] for t in taps] == [64, 128, 256, 512, 512] and [t.shape[-1] for t in taps] == [48, 24, 12, 6, 3]
    assert all(float((t > 0).double().mean()) > 0.2 for t in taps)          # the positive biases keep the ReLUs alive
    # normalize=False is the same network on x itself
    torch.testing.assert_close(R.value(sd, 2 * a - 1, 2 * b - 1, normalize=False), got, rtol=0, atol=1e-12)


def test_analytic_head_gradient_matches_autograd():
    g = torch.Generator().manual_seed(3)
    shapes = [(2, c, 8 >> s, 6 >> s) for s, c in enumerate((8, 16, 16, 32, 32))]
    f0 = [torch.rand(s, generator=g, dtype=torch.float64).requires_grad_() for s in shapes]
    f1 = [torch.rand(s, generator=g, dtype=torch.float64).requires_grad_() for s in shapes]
    lin = [torch.rand(1, s[1], 1, 1, generator=g, dtype=torch.float64) for s in shapes]
    up = torch.tensor([0.7, -1.3], dtype=torch.float64)
    (R.head(f0, f1, lin) * up).sum().backward()
    d0, d1 = R.head_grad([t.detach() for t in f0], [t.detach() for t in f1], lin, up)
    for s in range(5):
        torch.testing.assert_close(d0[s], f0[s].grad, rtol=0, atol=1e-12)
        torch.testing.assert_close(d1[s], f1[s].grad, rtol=0, atol=1e-12)


def test_zero_norm_convention_autograd_nan_restatement_finite():
    """A pixel whose channel vector is all zero: torch autograd of normalize_tensor gives NaN (sqrt backward 0 / 0), the restatement (and
    the kernels) the finite limit I / (r + eps); after the ReLU mask (f > 0) nothing of it is left."""
    g = torch.Generator().manual_seed(4)
    f0 = torch.rand(1, 8, 2, 2, generator=g, dtype=torch.float64)
    f0[0, :, 1, 0] = 0
    f1 = torch.rand(1, 8, 2, 2, generator=g, dtype=torch.float64)
    lin = [torch.rand(1, 8, 1, 1, generator=g, dtype=torch.float64)]
    x = f0.clone().requires_grad_()
    R.head([x], [f1], lin).sum().backward()
    assert torch.isnan(x.grad[0, :, 1, 0]).all() and torch.isfinite(x.grad[0, :, 0, 0]).all()
    d0, _ = R.head_grad([f0], [f1], lin, torch.ones(1, dtype=torch.float64))
    assert torch.isfinite(d0[0]).all()
    u = 2 * lin[0].view(-1) * (0 - f1[0, :, 1, 0] / (f1[0, :, 1, 0].norm() + R.EPS)) / 4
    torch.testing.assert_close(d0[0][0, :, 1, 0], u / R.EPS, rtol=1e-12, atol=0)       # the limit: u / (0 + eps)
    ok = torch.ones(2, 2, dtype=torch.bool)
    ok[1, 0] = False
    torch.testing.assert_close(d0[0][0][:, ok], x.grad[0][:, ok], rtol=0, atol=1e-12)


def test_max_pool_ties_go_to_the_first_maximum():
    """torch's max_pool2d picks the first maximum of a window in row-major order; the restatement (and vs_lpips_maxpool_backward) do too,
    at zero and at positive values."""
    x = torch.tensor([[[[2.0, 2.0, 0.0, 1.0],
                        [2.0, 1.0, 1.0, 1.0],
                        [0.0, 0.5, 0.0, 0.0],
                        [0.5, 0.5, 0.0, 0.0]]]], dtype=torch.float64)
    _, idx = torch.nn.functional.max_pool2d(x, 2, 2, return_indices=True)
    best, arg = R.pool_first_max(x)
    torch.testing.assert_close(best, torch.nn.functional.max_pool2d(x, 2, 2))
    assert arg[0, 0].tolist() == [[0, 1], [1, 0]]                    # window order (0,0) (0,1) (1,0) (1,1)
    flat = torch.tensor([[0, 3], [9, 10]])                            # torch's flat indices of the same choices
    assert idx[0, 0].tolist() == flat.tolist()
    dy = torch.tensor([[[[1.0, 2.0], [3.0, 4.0]]]], dtype=torch.float64)
    xr = x.clone().requires_grad_()
    torch.nn.functional.max_pool2d(xr, 2, 2).backward(dy)
    want = torch.where(x > 0, xr.grad, torch.zeros_like(x))           # the ReLU mask of the tap below the pool
    torch.testing.assert_close(R.pool_backward(dy, x), want, rtol=0, atol=0)


def test_lpips_argument_validation_reports_errors():
    from vicasplat_amd import _lib
    L = _lib.lib()
    p = C.c_void_p(256)
    arr = lambda *v: (C.c_void_p * 5)(*v)
    five = arr(*([256] * 5))
    assert L.vs_lpips_workspace_bytes(1, 24, 32) < 0 and b"multiples of 16" in L.vs_last_error()
    assert L.vs_lpips_workspace_bytes(2, 256, 256) == 4 * 2 * (512 + 128 + 32 + 8 + 2)
    assert L.vs_lpips_prep(None, 1, 16, 16, 1, p, None) < 0 and b"null" in L.vs_last_error()
    assert L.vs_lpips_prep(p, 1, 20, 16, 1, p, None) < 0 and b"multiples of 16" in L.vs_last_error()
    assert L.vs_lpips_prep(p, 0, 16, 16, 1, p, None) < 0 and b"positive" in L.vs_last_error()
    assert L.vs_lpips_prep(p, 1, 16, 16, 1, C.c_void_p(260), None) < 0 and b"aligned" in L.vs_last_error()
    assert L.vs_lpips_prep_backward(p, None, 1, 16, 16, 1, 16, p, None) < 0 and b"null" in L.vs_last_error()
    assert L.vs_lpips_prep_backward(p, p, 1, 16, 16, 1, -1, p, None) < 0 and b"scale_log2" in L.vs_last_error()
    assert L.vs_lpips_maxpool(None, 1, 16, 16, 64, p, None) < 0 and b"null" in L.vs_last_error()
    assert L.vs_lpips_maxpool(p, 1, 15, 16, 64, p, None) < 0 and b"even" in L.vs_last_error()
    assert L.vs_lpips_maxpool(p, 1, 16, 16, 63, p, None) < 0 and b"multiple of 4" in L.vs_last_error()
    assert L.vs_lpips_maxpool_backward(p, None, None, 1, 16, 16, 64, p, None) < 0 and b"null" in L.vs_last_error()
    assert L.vs_lpips_maxpool_backward(p, p, None, 1, 16, 16, 64, None, None) < 0 and b"dx" in L.vs_last_error()
    assert L.vs_lpips_head_forward(None, five, five, 1, 16, 16, p, p, None) < 0 and b"null tap array" in L.vs_last_error()
    assert L.vs_lpips_head_forward(five, arr(256, 256, None, 256, 256), five, 1, 16, 16, p, p, None) < 0
    assert b"tap 3" in L.vs_last_error()
    assert L.vs_lpips_head_forward(five, five, arr(256, 256, 256, 260, 256), 1, 16, 16, p, p, None) < 0
    assert b"alignment" in L.vs_last_error()
    assert L.vs_lpips_head_forward(five, five, five, 1, 16, 16, None, p, None) < 0 and b"workspace" in L.vs_last_error()
    assert L.vs_lpips_head_forward(five, five, five, 1, 16, 8, p, p, None) < 0 and b"multiples of 16" in L.vs_last_error()
    assert L.vs_lpips_head_backward(five, five, five, None, 1, 16, 16, 16, five, None, None) < 0 and b"null g" in L.vs_last_error()
    assert L.vs_lpips_head_backward(five, five, five, p, 1, 16, 16, 16, None, None, None) < 0 and b"d0 and d1" in L.vs_last_error()
    assert L.vs_lpips_head_backward(five, five, five, p, 1, 16, 16, 16, arr(256, 256, 256, 256, None), None, None) < 0
    assert b"d0[4]" in L.vs_last_error()
    assert L.vs_lpips_head_backward(five, five, five, p, 1, 16, 16, 99, five, five, None) < 0 and b"scale_log2" in L.vs_last_error()


def test_loss_lpips_backend_choice_leaves_the_default_alone():
    sd = R.fake_state_dict(0)
    assert callers.LossLpips(sd).backend == "torch"
    with pytest.raises(ValueError, match="backend"):
        callers.LossLpips(sd, backend="cuda")
    if not torch.cuda.is_available():
        with pytest.raises(ValueError, match="HIP device"):
            callers.LpipsVgg(sd)
