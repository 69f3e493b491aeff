"""Every leaf of the backward's route table (vicasplat_amd/backward_routes.py) run once, at the smallest shape that reaches it
(tests/backward_route_cases.py; tests/test_backward_routes_cpu.py proves the shapes reach their leaves without a GPU).

Each case asserts that (1) the route function, fed from the very tensors of the call, names the case's route, (2) the library entry points of
that route are the ones launched, (3) dx, dw and db match float64 on the same (rounded) inputs within the bounds of the existing tests of the
function and class: test_ops_gpu.test_linear_backward_matches_autograd / test_conv3x3_backward_matches_autograd for the 16-bit classes,
TOL of test_split_bwd_gpu for the split class.  Inputs are seeded: `linear_case` / `conv_case` build them.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import backward_route_cases as C
from vicasplat_amd import _lib, ops

pytestmark = pytest.mark.gpu
TOL = 1e-5                                                                  # test_split_bwd_gpu.TOL
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16, "split": torch.float32}
# the entry point that stands for a leaf; of the weight-gradient ones exactly one may be launched
ENTRY = {"nt": "vs_gemm_bias_act", "pack_t": "vs_transpose_pack_split", "padded": "vs_split_pack_weight", "pass": "vs_gelu_backward_f32",
         "tn256": "vs_gemm_wgrad_tn", "tn_skinny": "vs_gemm_wgrad_tn", "tn": "vs_conv3x3_wgrad_tn", "tn_grouped": "vs_conv3x3_wgrad_tn",
         "transposed": "vs_gemm_wgrad", "stream": "vs_conv3x3_wgrad_split_stream", "colsum": "vs_colsum", "colsum_padded": "vs_colsum"}
ATN256 = {"linear": "vs_gemm_wgrad_split_atn", "conv": "vs_conv3x3_wgrad_split_atn"}
WGRAD_ENTRIES = {"vs_gemm_wgrad_tn", "vs_conv3x3_wgrad_tn", "vs_gemm_wgrad", "vs_conv3x3_wgrad_split_stream", *ATN256.values()}


def _rel(a, b):
    return float((a.double() - b).abs().max() / (b.abs().max() + 1e-300))


def _err(a, b):
    return float((a.double() - b).abs().max())


@pytest.fixture
def launched(monkeypatch):
    """Names (and epilogue of vs_gemm_split) of the library entry points a call goes through; the calls run."""
    log, real = [], _lib.call

    def call(name, dev, *args):
        log.append(name + (f"[{args[13]}]" if name == "vs_gemm_split" else ""))
        return real(name, dev, *args)
    monkeypatch.setattr(_lib, "call", call)
    return log


def check_launches(log, route, kind):
    want = {part: ATN256[kind] if leaf == "atn256" else ENTRY.get(leaf) for part, leaf in route._asdict().items() if isinstance(leaf, str)}
    assert all(entry in log for entry in want.values() if entry), (want, log)
    assert [n for n in log if n in WGRAD_ENTRIES] == ([want["wgrad"]] if route.wgrad else []), log
    assert ("vs_gemm_split[5]" in log) == (route.dgelu == "epilogue"), log


def linear_case(case, cls):
    """-> (dy, x, w, keyword arguments) of the case on the GPU, seeded."""
    _, (M, N, K), opt = case
    dt, d = DTYPES[cls], torch.device("cuda:0")
    g = torch.Generator(device=d).manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g, device=d).to(dt)
    w = (torch.randn(N, K, generator=g, device=d) / math.sqrt(K)).to(dt)
    dy = (torch.randn(M, N, generator=g, device=d) * (1.0 if cls == "split" else 0.5)).to(dt)
    if opt.get("padded_dy"):      # the rows of the Gaussian adapter's backward: N values, zeros up to 8
        buf = torch.zeros(M, 8, dtype=dt, device=d)
        buf[:, :N] = dy
        dy = buf[:, :N]
    kw = dict(need_dw=opt.get("need_dw", True))
    if opt.get("scale_exp"):
        kw["scale_exp"] = ops.split_scale_exp(w)
    if opt.get("dgelu"):
        kw["dgelu_z"] = torch.randn(M, K, generator=g, device=d) * 2
    return dy, x, w, kw


def conv_case(case, cls):
    """-> (dy, x, w [Cout,Cin,3,3] f32) of the case on the GPU, seeded."""
    _, (N, H, W, Cin, Cout), opt = case
    dt, d = DTYPES[cls], torch.device("cuda:0")
    g = torch.Generator(device=d).manual_seed(N * H + Cin)
    x = torch.randn(N, H, W, Cin, generator=g, device=d).to(dt)
    w = torch.randn(Cout, Cin, 3, 3, generator=g, device=d) / math.sqrt(9 * Cin)
    dy = (torch.randn(N, H, W, Cout, generator=g, device=d) * (1.0 if cls == "split" else 0.5)).to(dt)
    if opt.get("strided_dy"):
        dy = dy.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    return dy, x, w


def linear_reference(dy, x, w, dgelu_z=None):
    dy, x, w = dy.double(), x.double(), w.double()
    dx = dy @ w
    if dgelu_z is not None:
        z = dgelu_z.double().requires_grad_()
        F.gelu(z).sum().backward()
        dx = dx * z.grad
    return dx, dy.t() @ x, dy.sum(0)


def conv_reference(dy, x, w, relu_in):
    """w [Cout,Cin,3,3]; -> dx NHWC, dw [Cout,Cin,3,3], db, float64."""
    xr = x.double().permute(0, 3, 1, 2).clone().requires_grad_()
    wr = w.double().clone().requires_grad_()
    br = torch.zeros(w.shape[0], dtype=torch.float64, device=x.device, requires_grad=True)
    y = F.conv2d(F.relu(xr) if relu_in else xr, wr, br, padding=1)
    (y * dy.double().permute(0, 3, 1, 2)).sum().backward()
    return xr.grad.permute(0, 2, 3, 1), wr.grad, br.grad


def _with_classes(cases):      # bf16 beside f16, except on the 2^20-row cases (the route does not read the class)
    return [pytest.param(c, cls, id=f"{C.pytest_id(c)}-{cls}") for c in cases for cls in (("f16",) if c[1][0] >= 1 << 20 else ("f16", "bf16"))]


@pytest.mark.parametrize("case,cls", _with_classes(C.LINEAR16))
def test_linear_backward_leaf(launched, case, cls):
    dy, x, w, kw = linear_case(case, cls)
    M, N = dy.shape
    route = ops.linear_backward_route(cls, M, N, x.shape[1], dy_ld=dy.stride(0), x_ld=x.stride(0),
                                      aligned16=dy.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0, **kw)
    assert C.route_id(route) == case[0] == C.route_id(C.linear_route(cls, case[1], case[2]))
    del launched[:]
    dx, dw, db = ops.linear_backward(dy, x, w, **kw)
    check_launches(launched, route, "linear")
    rx, rw, rb = linear_reference(dy, x, w)
    rt = 3e-3 if cls == "f16" else 1.6e-2
    errs = dict(dx=_err(dx, rx) / float(rx.abs().max()), db=_err(db, rb), db_bound=1e-4 * float(rb.abs().max()) + 1e-3)
    if route.wgrad is None:
        assert dw is None
    else:
        errs.update(dw=_err(dw, rw), dw_bound=2e-3 * float(rw.abs().max()) + 1e-4)       # f32 accumulation of exact 16-bit products
    print(C.pytest_id(case), cls, route, {k: f"{v:.2e}" for k, v in errs.items()})
    assert errs["dx"] <= rt and errs["db"] <= errs["db_bound"] and errs.get("dw", 0.0) <= errs.get("dw_bound", 0.0), errs


@pytest.mark.parametrize("case,cls", _with_classes(C.CONV16))
def test_conv3x3_backward_leaf(launched, case, cls):
    dy, x, w = conv_case(case, cls)
    wp = ops.pack_conv3x3_weight(w, DTYPES[cls])                                              # [Cout,3,3,Cin] 16-bit
    route = ops.conv3x3_backward_route(cls, *x.shape, dy.shape[3], contiguous=x.is_contiguous() and dy.is_contiguous())
    assert C.route_id(route) == case[0] == C.route_id(C.conv_route(cls, case[1], case[2]))
    assert (route.wgrad == "transposed" and route.ksplit == 1) == bool(case[2].get("strided_dy"))      # the one-slice arm is that case's and no other's
    del launched[:]
    dx, dw, db = ops.conv3x3_backward(dy, x, wp, relu_in=True)
    check_launches(launched, route, "conv")
    rx, rw, rb = conv_reference(dy, x, wp.permute(0, 3, 1, 2), True)
    rt = 4e-3 if cls == "f16" else 2.5e-2
    errs = dict(dx=_err(dx, rx) / float(rx.abs().max()), dw=_err(dw, rw.permute(0, 2, 3, 1)), dw_bound=3e-3 * float(rw.abs().max()) + 1e-3,
                db=_err(db, rb), db_bound=1e-3 * float(rb.abs().max()) + 1e-2)
    print(C.pytest_id(case), cls, route, {k: f"{v:.2e}" for k, v in errs.items()})
    assert errs["dx"] <= rt and errs["dw"] <= errs["dw_bound"] and errs["db"] <= errs["db_bound"], errs


@pytest.mark.parametrize("case", C.LINEAR_SPLIT, ids=C.pytest_id)
def test_linear_backward_split_leaf(launched, case):
    dy, x, w, kw = linear_case(case, "split")
    M, N = dy.shape
    z = kw.get("dgelu_z")
    route = ops.linear_backward_route("split", M, N, x.shape[1], need_dw=kw["need_dw"], scale_exp_known="scale_exp" in kw, w_contiguous=w.is_contiguous(),
                                      dgelu=None if z is None else z.is_contiguous())
    assert C.route_id(route) == case[0] == C.route_id(C.linear_route("split", case[1], case[2]))
    del launched[:]
    dx, dw, db = ops.linear_backward_split(dy, x, w, **kw)
    check_launches(launched, route, "linear")
    rx, rw, rb = linear_reference(dy, x, w, z)
    errs = dict(dx=_rel(dx, rx), db=_rel(db, rb))
    if route.wgrad is None:
        assert dw is None
    else:
        errs.update(dw=_rel(dw, rw))
    print(C.pytest_id(case), route, {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= TOL, errs


@pytest.mark.parametrize("case", C.CONV_SPLIT, ids=C.pytest_id)
def test_conv3x3_backward_split_leaf(launched, case):
    dy, x, w = conv_case(case, "split")
    route = ops.conv3x3_backward_route("split", *x.shape, dy.shape[3])
    assert C.route_id(route) == case[0] == C.route_id(C.conv_route("split", case[1], case[2]))
    del launched[:]
    dx, dw, db = ops.conv3x3_backward_split(dy, x, w, relu_in=True)
    check_launches(launched, route, "conv")
    rx, rw, rb = conv_reference(dy, x, w, True)
    errs = dict(dx=_rel(dx, rx), dw=_rel(dw, rw), db=_rel(db, rb))
    print(C.pytest_id(case), route, {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= TOL, errs
