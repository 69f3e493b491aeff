"""SSIM without a GPU: the float64 restatements of tests/ssim_f64.py against the fixtures recorded from scikit-image and from the
reference's SSIM loss (tests/golden/gen_ssim_golden.py), and the C-ABI argument validation of vs_ssim_forward / vs_ssim_backward."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import ssim_f64 as S

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _f(u8):
    return u8.astype(np.float32) / np.float32(255.0)


def _metric_cases(z):
    return sorted(k[:-5] for k in z.files if k.endswith("_ssim"))


def test_metric_restatement_matches_scikit_image_fixture():
    z = np.load(os.path.join(G, "ssim_metric.npz"))
    cases = _metric_cases(z)
    assert {"random_48x48", "smooth_64x80", "near_37x53", "flat_40x40", "batch2_32x44"} <= set(cases)
    for k in cases:
        x, y = _f(z[k + "_x"]), _f(z[k + "_y"])
        got = np.array([S.ssim_metric_f64(a, b) for a, b in zip(x, y)])
        np.testing.assert_allclose(got, z[k + "_ssim"], rtol=0, atol=1e-12, err_msg=k)


def test_metric_filter_matches_scipy_gaussian_filter():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(0)
    img = rng.random((23, 31))
    ref = ndimage.gaussian_filter(img, sigma=1.5, truncate=3.5, mode="reflect")
    np.testing.assert_allclose(S.gaussian_filter_reflect(img), ref, rtol=0, atol=1e-14)


def test_metric_restatement_rejects_small_images():
    with pytest.raises(ValueError):
        S.ssim_metric_f64(np.zeros((3, 10, 20)), np.zeros((3, 10, 20)))


@pytest.mark.parametrize("pair", ["rand", "near", "anti"])
def test_loss_restatement_matches_reference_fixture(pair):
    z = np.load(os.path.join(G, "ssim_loss.npz"))
    X = torch.tensor(_f(z[pair + "_x"]), dtype=torch.float64, requires_grad=True)
    Y = torch.tensor(_f(z[pair + "_y"]), dtype=torch.float64, requires_grad=True)
    avg = S.ssim_loss_f64(X, Y, data_range=1.0, size_average=True, retrun_seprate=True)
    img = S.ssim_loss_f64(X, Y, data_range=1.0, size_average=False, retrun_seprate=True)
    plain = S.ssim_loss_f64(X, Y, data_range=1.0, size_average=False)
    nn = S.ssim_loss_f64(X, Y, data_range=1.0, size_average=False, nonnegative_ssim=True)[0]
    close = lambda a, b: np.testing.assert_allclose(a, b, rtol=0, atol=1e-10)
    close(torch.stack(avg).detach().numpy(), z[pair + "_avg"])
    close(torch.stack(img).detach().numpy(), z[pair + "_img"])
    close(torch.stack(plain).detach().numpy(), z[pair + "_plain_img"])
    close(nn.detach().numpy(), z[pair + "_nn_img"])
    if pair + "_gx_ssim" not in z.files:
        return
    gx, gy = torch.autograd.grad(avg[0], (X, Y), retain_graph=True)
    close(gx.numpy(), z[pair + "_gx_ssim"])
    close(gy.numpy(), z[pair + "_gy_ssim"])
    gx, gy = torch.autograd.grad(avg[3], (X, Y))
    close(gx.numpy(), z[pair + "_gx_struct"])
    close(gy.numpy(), z[pair + "_gy_struct"])


def test_loss_fixture_exercises_the_clamps():
    """The near-identical pair has clamped (zero-gradient) and unclamped structure pixels; the anti pair a negative SSIM for relu."""
    z = np.load(os.path.join(G, "ssim_loss.npz"))
    g = z["near_gy_struct"]
    assert 0.1 < (g == 0).mean() < 0.9
    assert (z["anti_img"][0] < 0).all() and (z["anti_nn_img"] == 0).all()


def test_ssim_argument_validation_reports_errors():
    from vicasplat_amd import _lib
    L = _lib.lib()
    taps = (C.c_float * 11)(*([1.0 / 11] * 11))
    p = C.c_void_p(16)
    rc = L.vs_ssim_forward(None, None, 1, 3, 64, 64, taps, 11, 1.0, 1e-4, 9e-4, 0, p, p, None, None)
    assert rc < 0 and b"null" in L.vs_last_error()
    rc = L.vs_ssim_forward(p, p, 1, 3, 8, 8, taps, 11, 1.0, 1e-4, 9e-4, 0, p, p, None, None)
    assert rc < 0 and b"8 x 8" in L.vs_last_error()
    rc = L.vs_ssim_forward(p, p, 1, 3, 64, 64, taps, 10, 1.0, 1e-4, 9e-4, 0, p, p, None, None)
    assert rc < 0 and b"odd" in L.vs_last_error()
    rc = L.vs_ssim_forward(p, p, 1, 3, 64, 64, taps, 13, 1.0, 1e-4, 9e-4, 0, p, p, None, None)
    assert rc < 0 and b"at most 11" in L.vs_last_error()
    rc = L.vs_ssim_forward(p, p, 1, 3, 64, 64, taps, 11, 1.0, 1e-4, 9e-4, 0, None, p, None, None)
    assert rc < 0 and b"workspace" in L.vs_last_error()
    rc = L.vs_ssim_backward(None, p, 1, 3, 64, 64, taps, 11, 1.0, 1e-4, 9e-4, 0, None, None, p, p, None)
    assert rc < 0 and b"null" in L.vs_last_error()
    rc = L.vs_ssim_backward(p, p, 1, 3, 8, 8, taps, 11, 1.0, 1e-4, 9e-4, 0, None, None, p, p, None)
    assert rc < 0 and b"smaller" in L.vs_last_error()
    rc = L.vs_ssim_backward(p, p, 1, 3, 64, 64, taps, 4, 1.0, 1e-4, 9e-4, 0, None, None, p, p, None)
    assert rc < 0 and b"odd" in L.vs_last_error()
    rc = L.vs_ssim_backward(p, p, 1, 3, 64, 64, taps, 11, 1.0, 1e-4, 9e-4, 0, None, None, None, None, None)
    assert rc < 0 and b"dx and dy" in L.vs_last_error()
    assert L.vs_ssim_workspace_bytes(1, 3, 8, 8, 11, 0) < 0
    assert L.vs_ssim_workspace_bytes(2, 3, 256, 256, 11, 1) == 4 * 2 * 3 * 64 * 4    # 246 x 246 map: 8 x 8 tiles of 32 x 32


def test_ssim_front_ends_refuse_bad_shapes_before_any_launch():
    from vicasplat_amd import callers
    x = torch.zeros(1, 3, 10, 40)
    with pytest.raises(ValueError):
        callers.compute_ssim(x, x)
    with pytest.raises(ValueError):
        callers.ssim(x, x, data_range=1.0)
    with pytest.raises(ValueError):
        callers.ssim(torch.zeros(1, 3, 2, 16, 16), torch.zeros(1, 3, 2, 16, 16))
    with pytest.raises(ValueError, match="odd"):
        callers.ssim(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16), win_size=10)
