"""Float64 references (numpy) of the training step's element-wise kernels, with per-element magnitudes: GELU / GELU' / ReLU mask / SiLU /
split16 (csrc/backward.hip, split_bwd.hip, norm_rope.hip), the gated residual and its backward, the column sums, the bilinear x2 family
(csrc/conv.hip, split_bwd.hip) and the two rotary embeddings (csrc/norm_rope.hip rope_qk, csrc/rope2d.hip).  The yardstick of
tests/test_eltwise_edges_gpu.py, pinned to torch float64 by tests/test_eltwise_ref_cpu.py.

The method is that of tests/pointwise_f64.py: every output `k` comes with `k + "_mag"` (class V), the same code runs in float32
(dtype=np.float32: the restatement whose distance from float64 in units of 2^-24 mag is r32, R32_ELTWISE below) and `mutate=` plants one
deliberate defect.  A pure copy, a mask and split16 have magnitude 0: they must be bit exact (`same_bits`).

Criterion (`crit`), per element:  |got - ref| <= 4 max(r32, 1) 2^-24 mag, plus half an ulp of a 16-bit output, plus max(2^-22 |ref|,
2^-25) for a packed (hi, lo) output; the only absolute floor is underflow (2^-126 for an f32 output, half a subnormal step for a 16-bit
one), and only on elements of non-zero magnitude.
"""
import numpy as np
import torch

from pointwise_f64 import SUBNORMAL, U32, V, bound, gpu_factor, out_rows, ratio, round_to  # noqa: F401  (re-exported to the tests)

SQRT1_2 = 0.70710678118654752440
INV_SQRT_2PI = 0.3989422804014327
TWO_OVER_SQRT_PI = 1.1283791670955126

# r32 = max |f32 restatement - f64| / (2^-24 mag) per output over the edge inputs of tests/test_eltwise_edges_gpu.py, as printed by
# tests/test_eltwise_ref_cpu.py::test_f32_restatement_ratios, rounded up.  The GPU bound of an output is 4 max(r32, 1) 2^-24 mag.
R32_ELTWISE = dict(gelu=1.0, gelu_grad=1.0, silu=1.0, gated_out=1.0, gated_dy=1.0, dgate=1.9, colsum=6.1, up=1.0, up_t=1.0, rope_qk=1.0,
                   rope2d=1.0)

UNDERFLOW = {"f32": 2.0 ** -126, "f16": 2.0 ** -25, "bf16": 2.0 ** -134}


def _extras(ref, name, storage, packed):
    live = ref[name + "_mag"] > 0
    xabs = np.where(live, UNDERFLOW[storage] - SUBNORMAL[storage], 0.0)      # pointwise_f64.bound adds its own floor: the total is UNDERFLOW
    if packed:
        xabs = xabs + np.where(live, np.maximum(2.0 ** -25 - 2.0 ** -22 * np.abs(ref[name]), 0.0), 0.0)
    return (2.0 ** -22 if packed else 0.0), xabs


def allowance(ref, name, r32, storage="f32", packed=False):
    """The per-element allowance of the criterion (0 on elements of magnitude 0)."""
    extra, xabs = _extras(ref, name, storage, packed)
    return bound(ref, name, gpu_factor(r32), storage, extra) + xabs


def crit(got, ref, name, r32, storage="f32", packed=False):
    """max over the elements of |got - ref| / allowance (<= 1 passes); see the module docstring.  Elements of magnitude 0 must be exact."""
    extra, xabs = _extras(ref, name, storage, packed)
    return ratio(got, ref, name, gpu_factor(r32), storage, extra, xabs)


def units(got, ref, name, storage="f32"):
    """max |got - ref| / (2^-24 mag) over the elements of non-zero magnitude, the underflow floor of the criterion taken off the error."""
    got = np.asarray(got, np.float64).reshape(ref[name].shape)
    m = ref[name + "_mag"]
    ok = (m > 0) & np.isfinite(got)
    err = np.maximum(np.abs(got - ref[name].astype(np.float64)) - UNDERFLOW[storage], 0.0)
    return float((err[ok] / (U32 * m[ok])).max()) if ok.any() else 0.0


def _sum_rows(a):
    """Sum over axis 0 of a V [M, N], taken along the contiguous axis of the transpose: numpy then adds pairwise (blocks of 128), as the
    kernels' lanes, LDS reductions and atomics do, instead of row after row (M - 1 dependent roundings)."""
    return V(np.ascontiguousarray(a.v.T), np.ascontiguousarray(a.m.T)).sum(1)


def same_bits(got, ref):
    """got == ref element by element, the sign of zero included (float64 images of the stored values)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return got.shape == ref.shape and bool(((got == ref) & (np.signbit(got) == np.signbit(ref))).all())


def _erf(a):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(a))).numpy()


def _in(a, dtype):
    return V(np.asarray(a, np.float64).astype(dtype))


def _out(**kv):
    out = {}
    for k, a in kv.items():
        if isinstance(a, V):
            out[k], out[k + "_mag"] = a.v, np.asarray(a.m, np.float64)
        else:
            out[k] = a
    return out


_E = dict(over="ignore", invalid="ignore", divide="ignore", under="ignore")


# --------------------------------------------------------------------------------------------------------------------------------------
# activations
# --------------------------------------------------------------------------------------------------------------------------------------
def _one_plus_erf(x, mutate):
    e = (x * SQRT1_2).fn(_erf, lambda a: TWO_OVER_SQRT_PI * np.exp(-a * a))
    s = 1.0 + e
    if mutate == "erf_sat4":      # saturated one step early: |z| >= 4 -> 1 + erf = 0 / 2
        s = V(np.where(np.abs(x.v) >= 4, np.where(x.v < 0, 0.0, 2.0).astype(x.v.dtype), s.v), s.m)
    return s


def gelu(x, *, dtype=np.float64, mutate=None):
    """0.5 x (1 + erf(x / sqrt 2)) -> dict(gelu, gelu_mag)."""
    with np.errstate(**_E):
        xv = _in(x, dtype)
        return _out(gelu=0.5 * xv * _one_plus_erf(xv, mutate))


def gelu_grad(dy, x, *, dtype=np.float64, mutate=None):
    """dy (Phi(x) + x phi(x)) -> dict(gelu_grad, gelu_grad_mag)."""
    with np.errstate(**_E):
        g, xv = _in(dy, dtype), _in(x, dtype)
        d = 0.5 * _one_plus_erf(xv, mutate)
        if mutate != "no_zphi":
            d = d + xv * (INV_SQRT_2PI * (-0.5 * xv * xv).fn(np.exp, np.exp))
        return _out(gelu_grad=g * d)


def relu_mask(dy, x):
    """x > 0 ? dy : +0 (a copy or a zero: magnitude 0)."""
    dy, x = np.asarray(dy, np.float64), np.asarray(x, np.float64)
    return np.where(x > 0, dy, 0.0)


def silu(x, *, dtype=np.float64, mutate=None):
    """x / (1 + exp(-x)) -> dict(silu, silu_mag)."""
    with np.errstate(**_E):
        xv = _in(x, dtype)
        return _out(silu=xv / (1.0 + (-xv).fn(np.exp, np.exp)))


def split16(x):
    """f32 values -> (hi, lo) f16 as float64: hi = f16(x), lo = f16(x - hi); x - hi is exact in f32."""
    x32 = np.asarray(x, np.float64).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = x32.astype(np.float16)
        lo = (x32 - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


# --------------------------------------------------------------------------------------------------------------------------------------
# gated residual
# --------------------------------------------------------------------------------------------------------------------------------------
def _groups(M, gate_rows):
    return np.arange(M) // (gate_rows if gate_rows > 0 else M)


def gated_resid(x, y, gate=None, gate_rows=0, grp_in=0, grp_out=0, grp_off=0, *, dtype=np.float64, mutate=None):
    """out[m] = x[m] + (1 + gate[m // gate_rows]) y[yrow(m)]: x [M, C], y [rows, C] (the whole buffer), gate [G, C] or None
    -> dict(gated_out, gated_out_mag)."""
    M = np.asarray(x).shape[0]
    yr = out_rows(M, grp_in, grp_out, grp_off)
    xv, yv = _in(x, dtype), _in(np.asarray(y, np.float64)[yr], dtype)
    if gate is None:
        return _out(gated_out=xv + yv)
    grp = _groups(M, gate_rows) if mutate != "gate_grp_in" else np.minimum(np.arange(M) // max(grp_in, 1), np.asarray(gate).shape[0] - 1)
    return _out(gated_out=xv + (1.0 + _in(gate, dtype)[grp]) * yv)


def gated_chunk_rows(M, gate_rows, has_gate=True):
    """rows_per_chunk of vs_gated_resid_backward[_f32]'s launch (a block's 4 waves interleave the chunk's rows: more than 4 rows per chunk
    send a wave round its row loop again)."""
    gr = gate_rows if (has_gate and gate_rows > 0) else M
    G = -(-M // gr)
    chunks = max(1, min(1024 // G, -(-gr // 4)))
    return -(-gr // chunks)


def gated_nv(C):
    """NV of the gated_resid_backward_kernel instantiation that C selects (a lane owns columns 4 lane + 256 k, k < NV)."""
    return 1 if C <= 256 else 2 if C <= 512 else 3 if C <= 768 else 4 if C <= 1024 else 8


def gated_resid_backward(dout, y, gate=None, gate_rows=0, grp_in=0, grp_out=0, grp_off=0, *, dtype=np.float64, mutate=None):
    """-> dict(gated_dy [M, C] (row m is row yrow[m] of the dy buffer), dgate [G, C] (absent without a gate), yrow, untouched (rows of the
    buffer no m maps to), with `_mag`).  Without a gate dy is a copy of dout (magnitude 0: the rounding to the storage type only)."""
    dout = np.asarray(dout, np.float64)
    M, C = dout.shape
    rows = np.asarray(y).shape[0]
    yr = out_rows(M, grp_in, grp_out, grp_off)
    res = dict(yrow=yr, untouched=np.setdiff1d(np.arange(rows), yr))
    do = _in(dout, dtype)
    if gate is None:
        res.update(_out(gated_dy=do))
        return res
    gr = gate_rows if gate_rows > 0 else M
    grp, G = _groups(M, gr), np.asarray(gate).shape[0]
    dy = do * (1.0 + _in(gate, dtype)[grp])
    prod = do * _in(np.asarray(y, np.float64)[yr], dtype)
    keep = np.ones(M, bool)
    if mutate == "second_trip":      # the rows a wave takes after its first: chunk-local index >= 4
        keep = ((np.arange(M) - grp * gr) % gated_chunk_rows(M, gr)) < 4
    zero = V(np.zeros((C,), dtype))
    dg = V.stack([_sum_rows(prod[(grp == k) & keep]) if ((grp == k) & keep).any() else zero for k in range(G)], 0)
    if mutate == "masked_vec":      # the vector that holds columns >= 256 floor(C / 256) is never processed
        c0 = 256 * (C // 256)
        dg.v[:, c0:] = 0
        dy.v[:, c0:] = 0
    res.update(_out(gated_dy=dy, dgate=dg))
    return res


# --------------------------------------------------------------------------------------------------------------------------------------
# column sums
# --------------------------------------------------------------------------------------------------------------------------------------
def colsum_route(M, N, storage, ld, misaligned=False):
    """(kernel, row lanes, gridDim.y) of vs_colsum's dispatch: 'vec16' (N % 8 == 0, ld % 8 == 0, 16-byte aligned, 16-bit), 'vec32' (N % 4 ==
    0, ld % 4 == 0, aligned, f32), else 'scalar'."""
    cdiv = lambda a, b: -(-a // b)
    if storage != "f32" and N % 8 == 0 and ld % 8 == 0 and not misaligned:
        return "vec16", 16, max(1, min(max(1, 2048 // cdiv(N, 128)), cdiv(M, 64)))
    if storage == "f32" and N % 4 == 0 and ld % 4 == 0 and not misaligned:
        return "vec32", 8, max(1, min(max(1, 2048 // cdiv(N, 128)), cdiv(M, 32)))
    return "scalar", 4, min(max(256, 2048 // cdiv(N, 64)), cdiv(M, 64))


def colsum(x, *, dtype=np.float64, mutate=None, lanes=16, gy=1):
    """sum over the rows of x [M, N] -> dict(colsum, colsum_mag).  mutate='no_remainder': the rows the vector kernels' 4 x unrolled loop
    leaves to its remainder loop are dropped (thread (by, lane) takes rows by lanes + lane + j gy lanes)."""
    xv = _in(x, dtype)
    if mutate == "no_remainder":
        M, step = xv.v.shape[0], gy * lanes
        m = np.arange(M)
        n_start = -(-(M - m % step) // step)      # rows of the thread that owns row m
        xv = xv[(m // step) < 4 * (n_start // 4)]
    return _out(colsum=_sum_rows(xv))


# --------------------------------------------------------------------------------------------------------------------------------------
# bilinear x2, align_corners = True
# --------------------------------------------------------------------------------------------------------------------------------------
def _taps(n_in, dtype):
    """Per output index of one axis: i0, i1 (clamped) and the weight l of i1 as V; source position = dst ((in - 1) / (out - 1)) formed
    through V, so the weight's magnitude carries the rounding of the position (proportional to the size)."""
    n_out = 2 * n_in
    dst = V(np.arange(n_out).astype(dtype))
    r = V.lift(float(n_in - 1), dtype) / V.lift(float(n_out - 1), dtype)
    s = dst * r
    i0 = np.minimum(s.v.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, s - V(i0.astype(dtype))


def _ax(v, axis):
    shape = [1, 1, 1, 1]
    shape[axis] = -1
    return V(v.v.reshape(shape), v.m.reshape(shape))


def upsample2x(x, add=None, relu_add=False, *, dtype=np.float64, mutate=None):
    """x [N, H, W, C] -> dict(up [N, 2H, 2W, C], up_mag): lerp_y(lerp_x(.)) of the four neighbours, + add / + relu(add)."""
    with np.errstate(**_E):
        x = np.asarray(x, np.float64)
        N, H, W, C = x.shape
        y0, y1, ly = _taps(H, dtype)
        x0, x1, lx = _taps(W, dtype)
        if mutate == "x2_wrap":      # the 2 x 2 block's third source column (the right neighbour of its odd output) unclamped, wrapped
            xa = x0[0::2].repeat(2)
            third = (np.arange(2 * W) % 2 == 1) & (x0 == xa + 1)
            x1 = np.where(third, (xa + 2) % W, x1)
        xv = _in(x, dtype)
        lxb, lyb = _ax(lx, 2), _ax(ly, 1)
        top = xv[:, y0][:, :, x0] * (1.0 - lxb) + xv[:, y0][:, :, x1] * lxb
        bot = xv[:, y1][:, :, x0] * (1.0 - lxb) + xv[:, y1][:, :, x1] * lxb
        o = top * (1.0 - lyb) + bot * lyb
        if mutate == "relu_interp":
            o = V(np.maximum(o.v, 0), o.m)
        if add is not None:
            a = np.asarray(add, np.float64)
            o = o + _in(np.maximum(a, 0.0) if relu_add else a, dtype)
        return _out(up=o)


def _adjoint_axis(g, n_in, axis, dtype, window):
    """sum over the outputs of one axis: t[.., i, ..] = sum_o w(o, i) g[.., o, ..] over the candidates o = 2 i - window .. 2 i + window."""
    i0, i1, l = _taps(n_in, dtype)
    n_out = 2 * n_in
    acc = None
    for d in range(-window, window + 1):
        o = 2 * np.arange(n_in) + d
        ok = (o >= 0) & (o < n_out)
        oc = np.clip(o, 0, n_out - 1)
        lo = l[oc]
        i = np.arange(n_in)
        w = V.where(ok & (i0[oc] == i), 1.0 - lo, 0.0, dtype) + V.where(ok & (i1[oc] == i), lo, 0.0, dtype)
        w = V(np.where(w.v == 0, 0, w.v), np.where(w.v == 0, 0, w.m))
        idx = [slice(None)] * 4
        idx[axis] = oc
        term = _ax(w, axis) * g[tuple(idx)]
        acc = term if acc is None else acc + term
    return acc


def upsample2x_transpose(g, *, dtype=np.float64, mutate=None):
    """g [N, 2H, 2W, C] -> dict(up_t [N, H, W, C], up_t_mag): the transpose of upsample2x.  An input row receives from the output rows
    within +-2 of 2 y (the kernels scan +-3); mutate='window1' scans +-1."""
    with np.errstate(**_E):
        g = np.asarray(g, np.float64)
        N, Ho, Wo, C = g.shape
        win = 1 if mutate == "window1" else 3
        t = _adjoint_axis(_in(g, dtype), Wo // 2, 2, dtype, win)
        return _out(up_t=_adjoint_axis(t, Ho // 2, 1, dtype, win))


# --------------------------------------------------------------------------------------------------------------------------------------
# rotary embeddings
# --------------------------------------------------------------------------------------------------------------------------------------
def _pow_inv(base, e, dtype):
    """1 / base^e as V (e a V of exact exponents)."""
    lb = np.log(base)
    return 1.0 / e.fn(lambda a: np.asarray(base, a.dtype) ** a, lambda a: lb * np.asarray(base, a.dtype) ** a)


def _rotate(u, v, ang):
    cs, sn = ang.fn(np.cos, np.sin), ang.fn(np.sin, np.cos)
    return u * cs - v * sn, v * cs + u * sn


def rope_qk(buf, H, k_col, pos, kind=None, base2d=100.0, theta1d=30.0, direction=1.0, *, dtype=np.float64, mutate=None):
    """buf [rows, ld]: q at column 0 and k at column k_col, H heads of 64 each.  kind 0: halves of 32, pairs (i, i + 16), angle
    pos[half] / base2d^(i / 16); kind 1: pairs (2p, 2p + 1), angle pos[0] / theta1d^(2p / 64); kind 2: untouched.
    -> dict(rope_qk [rows, ld], rope_qk_mag): every column outside the two blocks, and every kind-2 row, is a copy (magnitude 0)."""
    with np.errstate(**_E):
        buf = np.asarray(buf, np.float64)
        rows, ld = buf.shape
        pos = np.asarray(pos, np.float64)
        kind = np.zeros(rows, np.int64) if kind is None else np.asarray(kind, np.int64)
        b = _in(buf, dtype)
        out_v, out_m = b.v.copy(), np.zeros(buf.shape, np.float64)
        p = np.arange(32)
        half, i = p >> 4, p & 15
        iu0, iv0 = half * 32 + i, half * 32 + i + 16
        iu1, iv1 = 2 * p, 2 * p + 1
        f0 = _pow_inv(base2d, V(i.astype(dtype)) / 16.0, dtype)
        f1 = _pow_inv(theta1d, V((2 * p).astype(dtype)) / 64.0, dtype)
        for r in range(rows):
            if kind[r] == 2:
                continue
            if kind[r] == 0:
                iu, iv, ang = iu0, iv0, V(pos[r][half].astype(dtype)) * f0
            else:
                iu, iv = (iu0, iv0) if mutate == "kind1_pairs16" else (iu1, iv1)
                ang = V(np.full(32, pos[r][0]).astype(dtype)) * f1
            for sel, col in enumerate((0, k_col)):
                d = direction
                if mutate == "inv_k_forward" and sel == 1 and direction < 0:
                    d = 1.0
                a = ang if d > 0 else -ang
                cu = col + 64 * np.arange(H)[:, None] + iu[None, :]
                cv = col + 64 * np.arange(H)[:, None] + iv[None, :]
                nu, nv = _rotate(b[r, cu], b[r, cv], a)
                out_v[r, cu], out_v[r, cv] = nu.v, nv.v
                out_m[r, cu], out_m[r, cv] = nu.m, nv.m
        return dict(rope_qk=out_v, rope_qk_mag=out_m)


def rope2d(tokens, pos, base=100.0, fwd=1.0, *, dtype=np.float64, mutate=None):
    """tokens [B, N, H, D] (D % 4 == 0), pos [B, N, 2]: D = [y half | x half]; in each half Q = D / 4 pairs (i, i + Q); angle = pos[half]
    (fwd / base^(i / Q)) -> dict(rope2d, rope2d_mag)."""
    with np.errstate(**_E):
        t = np.asarray(tokens, np.float64)
        B, N, H, D = t.shape
        Q = D // 4
        tv = _in(t.reshape(B, N, H, 2, 2, Q), dtype)
        inv = V.lift(float(fwd), dtype) * _pow_inv(base, V(np.arange(Q).astype(dtype)) / float(Q), dtype)      # [Q]
        p = V(np.asarray(pos, np.float64).astype(dtype).reshape(B, N, 1, 2, 1))
        ang = p * V(inv.v.reshape(1, 1, 1, 1, Q), inv.m.reshape(1, 1, 1, 1, Q))
        nu, nv = _rotate(tv[:, :, :, :, 0], tv[:, :, :, :, 1], ang)
        o = V.stack([nu, nv], 4)
        return dict(rope2d=o.v.reshape(B, N, H, D), rope2d_mag=np.asarray(o.m, np.float64).reshape(B, N, H, D))


# --------------------------------------------------------------------------------------------------------------------------------------
# edge inputs
# --------------------------------------------------------------------------------------------------------------------------------------
ACT_VALUES = [0.0, 1e-8, 1e-4, 0.5, 1.0, 2.0, 3.0, 4.0, 5.0, 5.5, 6.0, 8.0, 10.0, 13.0, 40.0]
TINY = {"f32": 2.0 ** -149, "f16": 2.0 ** -24, "bf16": 2.0 ** -133}      # the smallest subnormal of the type


def act_values(n, storage, extra=()):
    """n values cycling through +-ACT_VALUES (+-0 included) and +-extra, rounded to the storage type."""
    base = np.asarray(list(ACT_VALUES) + list(extra), np.float64)
    tab = np.stack([base, -base], 1).reshape(-1)
    return round_to(tab[np.arange(n) % tab.size], storage)


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def gated_inputs(M, C, G, rows, storage, seed=0):
    rng = np.random.default_rng(seed + 7919 * M + C)
    return dict(x=f32(rng.standard_normal((M, C))), y=round_to(rng.standard_normal((rows, C)), storage), gate=f32(0.5 * rng.standard_normal((G, C))),
                dout=f32(rng.standard_normal((M, C))))


def colsum_input(M, N, storage, seed=0):
    """Columns cycle through: ordinary, all zero, constant, alternating +-1e4 with a residue of 1e-3."""
    rng = np.random.default_rng(seed + 104729 * M + N)
    x = rng.standard_normal((M, N))
    m = np.arange(M)
    for c in range(N):
        k = c % 4
        if k == 1:
            x[:, c] = 0.0
        elif k == 2:
            x[:, c] = 0.3 * (1 + c % 5)
        elif k == 3:
            x[:, c] = np.where(m % 2 == 0, 1e4, -1e4) + 1e-3
    return round_to(x, storage)


def upsample_inputs(N, H, W, C, storage, seed=0):
    """x, add (with +-0 and negative values) and a cotangent g of the output's shape, values of the storage type."""
    rng = np.random.default_rng(seed + 31 * H + 7 * W + C + 1000 * min(N, 3))
    x = rng.standard_normal((N, H, W, C))
    add = rng.standard_normal((N, 2 * H, 2 * W, C))
    flat = add.reshape(-1)
    flat[0::7] = 0.0
    flat[3::7] = -0.0
    return round_to(x, storage), round_to(add, storage), round_to(rng.standard_normal((N, 2 * H, 2 * W, C)), storage)


ROPE_POS = [(0, 0), (15, 16), (16, 0)]
ROPE_T = [0, 1, 69]


def rope_qk_inputs(rows, H, k_col, ld, storage, mixed=True, seed=0):
    """buf [rows, ld], pos int [rows, 2], kind [rows] (0 / 1 / 2 cycling, or None)."""
    rng = np.random.default_rng(seed + 97 * rows + H + ld)
    buf = round_to(rng.standard_normal((rows, ld)), storage)
    kind = (np.arange(rows) % 3) if mixed else None
    pos = np.zeros((rows, 2), np.int64)
    for r in range(rows):
        if mixed and kind[r] == 1:
            pos[r] = (ROPE_T[(r // 3) % 3], 0)
        else:
            pos[r] = ROPE_POS[r % 3] if not mixed else ROPE_POS[(r // 3) % 3]
    return buf, pos, kind


def common16(a):
    """Values exact in f16, bf16 and f32 at once (bf16 rounding; nothing below 2^-10), so that one reference serves the three dtypes."""
    a = round_to(a, "bf16")
    return np.where(np.abs(a) < 2.0 ** -10, 0.0, a)


# --------------------------------------------------------------------------------------------------------------------------------------
# the cases (shared by the CPU measurement of r32 / the mutation check and by the GPU tests)
# --------------------------------------------------------------------------------------------------------------------------------------
ACT_N16, ACT_N32 = (8, 2040, 2048, 2056), (4, 1020, 1024, 1028)      # 8 per thread, 2048 per block / 4 per thread, 1024 per block
GATED_C = (4, 192, 256, 260, 512, 516, 768, 1024, 1028, 2048)
GATED_M = (1, 7, 33, 41)
GATED_DEEP = dict(M=256 * 37 + 11, C=192, gate_rows=37)      # 257 groups, the last ragged
GATED_ONE = dict(M=4101, C=4, gate_rows=4101)                # one group, 1024 chunks of 5 rows
COLSUM_N = (4, 8, 64, 100, 102, 128, 136, 1024)
COLSUM_M = (1, 7, 24, 25, 33, 47, 48, 49, 63, 64, 65, 129, 1000)
UP_HW = ((1, 1), (1, 5), (5, 1), (2, 2), (2, 3), (3, 2), (3, 3), (7, 9), (16, 12))
UP_N = (1, 3)
UP_C = dict(f16=(8, 24, 264), bf16=(8, 24, 264), f32=(4, 36, 132), packed=(32, 96))
UP_SPILL_BLOCK = dict(N=16385, H=2, W=2)                     # C = 8 (16-bit) / 4 (f32): 32 770 grid rows
UP_SPILL_POINT = dict(N=1, H=32769, W=1, C=4)                # the f32 per-output kernel: 65 538 grid rows
ROPE_ROWS, ROPE_H = (1, 3, 4, 5, 9), (1, 3, 12, 16)
ROPE2D_D, ROPE2D_B, ROPE2D_N, ROPE2D_H = (4, 64, 128), (1, 2), (1, 5), (1, 4)


def gated_cases(M):
    """(gate_rows or None, grp_in) of one M: no gate, 3 / 5 / 9 (ragged last groups included), M; the identity map (grp_in 0) and the
    camera-token map (grp_in = g, grp_out = g + 1, grp_off = 1) alternate, and both are used with gate_rows = M."""
    out, k = [], 0
    for gr in [None] + [r for r in (3, 5, 9) if r < M] + [M]:
        maps = (0, max(1, M // 2)) if gr in (None, M) else ((0,) if k % 2 else (gr,))
        k += 1
        out += [(gr, gi) for gi in maps]
    return out


def upsample_kernel(storage, H, W):
    """The kernel vs_upsample2x_nhwc launches: 'block16' / 'block32' (one thread per 2 x 2 outputs) or 'point32' (f32 with H or W of 1)."""
    if storage in ("f16", "bf16"):
        return "block16"
    return "block32" if H >= 2 and W >= 2 else "point32"


def upsample_grid_rows(kernel, N, H):
    return N * H * (2 if kernel == "point32" else 1)


def iter_gated(small_only=False):
    """dict(M, C, gate_rows (None: no gate), grp_in, grp_out, grp_off, rows, G, x, y, gate, dout): y holds values common to the three
    dtypes, so one reference serves them."""
    shapes = [(M, C) for C in GATED_C for M in GATED_M]
    cases = [(M, C, gr, gi) for M, C in shapes for gr, gi in gated_cases(M)]
    if not small_only:
        cases += [(GATED_DEEP["M"], GATED_DEEP["C"], GATED_DEEP["gate_rows"], 0), (GATED_ONE["M"], GATED_ONE["C"], GATED_ONE["gate_rows"], 0)]
    for M, C, gr, gi in cases:
        G = 1 if gr is None else -(-M // gr)
        rows = M if gi == 0 else -(-M // gi) * (gi + 1)
        z = gated_inputs(M, C, G, rows, "f32")
        z["y"] = common16(z["y"])
        z.update(M=M, C=C, gate_rows=gr, grp_in=gi, grp_out=gi + 1 if gi else 0, grp_off=1 if gi else 0, rows=rows, G=G)
        yield z


def gated_refs(z, dtype=np.float64, mutate=None):
    kw = dict(grp_in=z["grp_in"], grp_out=z["grp_out"], grp_off=z["grp_off"], dtype=dtype, mutate=mutate)
    gate, gr = (None, 0) if z["gate_rows"] is None else (z["gate"], z["gate_rows"])
    return dict(gated_resid(z["x"], z["y"], gate, gr, **kw), **gated_resid_backward(z["dout"], z["y"], gate, gr, **kw))


def iter_upsample(storage):
    """(N, H, W, C) of one storage class ('f16' / 'bf16' / 'f32' / 'packed'), the grid-spill cases last."""
    for H, W in UP_HW:
        if storage == "packed" and (H < 2 or W < 2):
            continue
        for N in UP_N:
            for C in UP_C[storage]:
                yield N, H, W, C
    if storage != "packed":
        yield UP_SPILL_BLOCK["N"], UP_SPILL_BLOCK["H"], UP_SPILL_BLOCK["W"], 4 if storage == "f32" else 8
    if storage == "f32":
        yield UP_SPILL_POINT["N"], UP_SPILL_POINT["H"], UP_SPILL_POINT["W"], UP_SPILL_POINT["C"]


def iter_rope_qk():
    """dict(rows, H, k_col, ld, mixed, buf, pos, kind): values common to the three dtypes."""
    for rows in ROPE_ROWS:
        for H in ROPE_H:
            for gap in (0, 64):
                for mixed in (True, False):
                    k_col = 64 * H + gap
                    ld = k_col + 64 * H + 64 * H + 8      # q | gap | k | v | spare columns
                    buf, pos, kind = rope_qk_inputs(rows, H, k_col, ld, "f32", mixed)
                    yield dict(rows=rows, H=H, k_col=k_col, ld=ld, mixed=mixed, buf=common16(buf), pos=pos, kind=kind)


def iter_rope2d():
    for D in ROPE2D_D:
        for B in ROPE2D_B:
            for N in ROPE2D_N:
                for H in ROPE2D_H:
                    rng = np.random.default_rng(D + 10 * B + 100 * N + H)
                    tok = common16(rng.standard_normal((B, N + 1, H, D)))      # one spare token: the tests rotate the view [:, :N]
                    pos = rng.integers(0, 1001, (B, N, 2))
                    pos[0, 0] = (1000, 0)
                    yield dict(B=B, N=N, H=H, D=D, tokens=tok, pos=pos)
