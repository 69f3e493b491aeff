"""The cases of tests/test_backward_routes_gpu.py: one per leaf of vicasplat_amd/backward_routes.py, at the smallest shape that reaches it.
tests/test_backward_routes_cpu.py proves, without a GPU, that each case takes the route its id names.

A case is (id, shape, options); the id is the route's leaves joined by "-" in the order dx-[dgelu-]wgrad-db ("none" for a part that is not
wanted).  Options: need_dw; padded_dy (dy is a stride-8 view of a zero-padded buffer); strided_dy (dy is an NCHW tensor seen as NHWC);
scale_exp (the weight's exponent is handed in); dgelu (dgelu_z is given).
"""
from vicasplat_amd.backward_routes import conv3x3_backward_route, linear_backward_route

LINEAR16 = [      # (M, N, K)
    ("nt-tn256-colsum", (257, 256, 256), {}),                   # one slice, its last K tile ragged
    ("nt-tn256-colsum", (1100, 256, 256), {}),                  # two slices
    ("nt-tn_skinny-colsum", (1 << 20, 8, 64), {}),              # 2^20 rows: the route's own threshold
    ("nt-tn_skinny-colsum_padded", (1 << 20, 3, 64), dict(padded_dy=True)),
    ("nt-transposed-on_transpose", (100, 192, 64), {}),
    ("nt-none-colsum", (100, 192, 64), dict(need_dw=False)),
]
CONV16 = [        # (N, H, W, Cin, Cout)
    ("conv-tn-colsum", (1, 3, 5, 256, 256), {}),
    ("conv-tn_grouped-colsum", (1, 4, 4, 64, 256), {}),
    ("conv-transposed-on_transpose", (2, 16, 16, 64, 128), {}),
    # whole 256-tiles miss `tn` only through a strided x or dy; few pixels then make ONE slice: the un-sliced operands of the transposed arm
    ("conv-transposed-on_transpose", (1, 3, 5, 256, 256), dict(strided_dy=True)),
]
LINEAR_SPLIT = [
    ("pack_t-atn256-on_transpose", (100, 256, 256), dict(scale_exp=True)),
    ("padded-transposed-on_transpose", (300, 8, 128), {}),
    ("padded-epilogue-transposed-on_transpose", (64, 64, 128), dict(dgelu=True)),
    ("padded-pass-transposed-on_transpose", (200, 96, 256), dict(dgelu=True)),
    ("padded-none-colsum", (64, 64, 128), dict(need_dw=False)),
]
CONV_SPLIT = [
    ("conv-atn256-on_transpose", (1, 3, 5, 256, 256), {}),
    ("conv-stream-stream", (1, 1, 32, 64, 64), {}),
    ("conv-transposed-on_transpose", (2, 16, 16, 64, 128), {}),
]


def route_id(r) -> str:
    return "-".join(p or "none" for p in [r.dx] + ([r.dgelu] if r.dgelu else []) + [r.wgrad, r.db])


def pytest_id(case) -> str:
    name, shape, opt = case
    return "-".join([name, "x".join(map(str, shape))] + sorted(opt))


def linear_route(cls: str, shape, opt):
    """The route of a linear case from its shape and options alone: what the tensors of the GPU test amount to."""
    M, N, K = shape
    return linear_backward_route(cls, M, N, K, need_dw=opt.get("need_dw", True), dy_ld=8 if opt.get("padded_dy") else N,
                                 scale_exp_known=bool(opt.get("scale_exp")), dgelu=True if opt.get("dgelu") else None)


def conv_route(cls: str, shape, opt):
    return conv3x3_backward_route(cls, *shape, contiguous=not opt.get("strided_dy"))
