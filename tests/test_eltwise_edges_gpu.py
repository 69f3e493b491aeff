"""The training step's element-wise kernels against the float64 references of tests/eltwise_f64.py, at their own edges.  -m gpu.

Kernels: GELU / GELU' / ReLU mask (csrc/backward.hip 16-bit, split_bwd.hip f32), silu_cast (norm_rope.hip), split16, the gated residual
and its backward (all five NV instantiations, 16-bit and f32), the three column-sum kernels, the bilinear x2 family (16-bit block kernel,
f32 block kernel, f32 per-output kernel, packed output; the transposes) and the rotary embeddings rope_qk (norm_rope.hip) and rope2d.

Criterion, per element:  |gpu - ref| <= 4 max(r32, 1) 2^-24 mag  (eltwise_f64.R32_ELTWISE; r32 below); 16-bit outputs get half an ulp of
their type on top; packed (hi, lo) outputs are decoded as hi + lo and get max(2^-22 |ref|, 2^-25) for the pair's representation; the only
absolute floor is underflow (2^-126 for f32, half a subnormal step for 16-bit outputs).  Copies, masks and split16 are bit exact.  No
element of any case is left out; what a kernel must not touch (skipped yrow rows, the columns beside a slice, v columns, kind-2 rows, the
gap between q and k, a spare token) holds other values and must come back unchanged.  16-bit inputs are rounded to their type first.

The route each shape is there for is derived from the host-side dispatch conditions (eltwise_f64.gated_nv / gated_chunk_rows /
colsum_route / upsample_kernel / upsample_grid_rows) and asserted, not assumed.

The position of the last output column of the x2 kernels is exactly W - 1, so the clamped third source column min(x0 + 2, W - 1) only
ever carries the weight 0: no finite input can show a wrong clamp in a value.  test_upsample_zero_weight_column_does_not_spread_nan puts
a NaN where an unclamped, wrapped index would read, at the widths 2 and 3.

The f32 transpose is held to the reference directly and through the adjoint identity <up(x), g> = <x, up^T(g)>, both sides formed in
float64 from the GPU's own two outputs, within the two bounds summed over the elements.

Measured on an MI355X, max |gpu - ref| / (2^-24 mag) over all cases (`-s` prints them per test), beside r32:

    output      r32    gpu
    gelu        0.64   0.38
    gelu_grad   0.66   0.53
    silu        0.60   1.62
    gated_out   1.00   1.00
    gated_dy    0.99   0.99
    dgate       1.88   1.35
    colsum      6.08   6.16
    up          0.90   0.90
    up_t        0.49   0.33
    rope_qk     0.70   0.71
    rope2d      0.44   0.46

(f32 outputs; 16-bit and packed outputs: at most 1.00 of their allowance, which half an ulp of the type dominates.)  No kernel exceeded
4 max(r32, 1): the two kernels that use the fast __expf stay inside it as well (silu_cast: 1.62 units at x = -6, 0.82 at x = -40, against
0.53 with expf in its place; below x = -87 the result is under the 2^-126 floor; gelu_backward_kernel's outputs are 16-bit), so both keep it.
"""
import numpy as np
import pytest
import torch

import eltwise_f64 as ew

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
R32 = ew.R32_ELTWISE
SENTINEL = 7.0


def _dev():
    return torch.device("cuda:0")


def _t(a, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(_dev())


def _np(t):
    torch.cuda.synchronize()
    return t.double().cpu().numpy()


class Worst:
    """Worst measured units per output (f32 outputs) and worst error / allowance (every output), printed at the end of a test."""

    def __init__(self):
        self.u = {}

    def check(self, got, ref, name, storage="f32", packed=False, tag=()):
        r = ew.crit(got, ref, name, R32[name], storage, packed)
        key = name if storage == "f32" and not packed else f"{name} {'packed' if packed else storage} (of the allowance)"
        val = ew.units(got, ref, name) if storage == "f32" and not packed else r
        self.u[key] = max(self.u.get(key, 0.0), val)
        assert r <= 1.0, (name, storage, packed, tag, r, ew.units(got, ref, name, storage))

    def show(self, what):
        print(what, {k: round(v, 3) for k, v in self.u.items()})


# --------------------------------------------------------------------------------------------------------------------------------------
# GELU / GELU' / ReLU mask / SiLU / split16
# --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("st", ["f16", "bf16", "f32"])
def test_activations_match_float64(st):
    from vicasplat_amd import ops
    w = Worst()
    for n in (ew.ACT_N32 if st == "f32" else ew.ACT_N16):
        x = ew.act_values(n, st)
        dy = ew.round_to(1.0 + 0.25 * np.cos(np.arange(n)), st)
        xt, dyt = _t(x, DT[st]), _t(dy, DT[st])
        w.check(_np(ops.gelu16(xt)), ew.gelu(x), "gelu", st, tag=n)
        w.check(_np(ops.gelu_backward(dyt, xt)), ew.gelu_grad(dy, x), "gelu_grad", st, tag=n)
        # ReLU mask: the smallest subnormals of the type and both zeros first, a -0.0 among the gradients
        special = np.array([ew.TINY[st], -ew.TINY[st], -0.0, 0.0])
        xr = np.concatenate([special, x])[:n] if n > 4 else special
        dr = dy.copy()
        dr[::5] = -0.0
        xrt, drt = _t(xr, DT[st]), _t(dr, DT[st])
        assert _np(xrt)[0] > 0 > _np(xrt)[1]      # the subnormals reached the device as such
        ref = ew.relu_mask(dr, xr)
        assert ew.same_bits(_np(ops.relu_mask(drt, xrt)), ref), ("relu_mask", n)
        assert ew.same_bits(_np(drt), dr)      # ... and left the incoming gradient alone
        if st != "f32":
            assert ew.same_bits(_np(ops.relu_mask_(drt.clone(), xrt)), ref), ("relu_mask_", n)
    w.show(f"activations {st}")


@pytest.mark.parametrize("st", ["f32", "f16", "bf16"])
def test_silu_cast_matches_float64(st):
    from vicasplat_amd import ops
    w = Worst()
    for n in ew.ACT_N32:
        x = ew.act_values(n, "f32", extra=(88.0, 100.0))
        if n == max(ew.ACT_N32):
            assert {88.0, -88.0, 100.0, -100.0} <= set(x.tolist())
        w.check(_np(ops.silu_cast(_t(x), DT[st])), ew.silu(x), "silu", st, tag=n)
    w.show(f"silu {st}")


def test_split16_is_bit_exact():
    from vicasplat_amd import _lib as L, ops
    for n in ew.ACT_N32:
        x = ew.f32(ew.act_values(n, "f32") * (1.0 + 1e-4 * np.cos(np.arange(n))))
        xt = _t(x).reshape(1, n)
        if n % 8 == 0:
            hi, lo = ops.split16(xt)
        else:      # the ABI takes C % 4 == 0; the front-end asks for 8
            hi, lo = torch.empty((1, n), dtype=torch.float16, device=_dev()), torch.empty((1, n), dtype=torch.float16, device=_dev())
            L.call("vs_split16", _dev(), L.ptr(xt), xt.stride(0), L.ptr(hi), L.ptr(lo), hi.stride(0), 1, n)
        rh, rl = ew.split16(x)
        assert ew.same_bits(_np(hi).reshape(-1), rh) and ew.same_bits(_np(lo).reshape(-1), rl), n
    # rows of a wider buffer
    x = ew.f32(np.random.default_rng(0).standard_normal((5, 24)) * 3)
    hi, lo = ops.split16(_t(x)[:, 4:20])
    rh, rl = ew.split16(x[:, 4:20])
    assert ew.same_bits(_np(hi), rh) and ew.same_bits(_np(lo), rl)


# --------------------------------------------------------------------------------------------------------------------------------------
# gated residual
# --------------------------------------------------------------------------------------------------------------------------------------
def _gated_case(ops, z, k, w):
    M, C, gr = z["M"], z["C"], z["gate_rows"]
    ref = ew.gated_refs(z)
    kw = dict(grp_in=z["grp_in"], grp_out=z["grp_out"], grp_off=z["grp_off"])
    x, dout = _t(z["x"]), _t(z["dout"])
    gate = None if gr is None else _t(z["gate"])
    tag = (M, C, gr, z["grp_in"])
    for st in ("f16", "bf16", "f32"):
        wide = k % 2 == 1      # y / dy as column slices of a wider buffer
        ybuf = torch.full((z["rows"], C + 8 if wide else C), SENTINEL, dtype=DT[st], device=_dev())
        y = ybuf[:, 4:4 + C] if wide else ybuf
        y.copy_(_t(z["y"], DT[st]))
        assert (y.stride(0) != C) == wide
        w.check(_np(ops.gated_resid(x, y, gate, gr or 0, **kw)), ref, "gated_out", tag=tag + (st,))
        dybuf = torch.full_like(ybuf, SENTINEL)
        dy = dybuf[:, 4:4 + C] if wide else dybuf
        dgate = ops.gated_resid_backward(dout, y, gate, gr or 0, dy, **kw)
        full = _np(dy)
        if gr is None:      # no gate: a rounded copy
            assert dgate is None and ew.same_bits(full[ref["yrow"]], ew.round_to(z["dout"], st)), tag
        else:
            w.check(full[ref["yrow"]], ref, "gated_dy", st, tag=tag)
            w.check(_np(dgate), ref, "dgate", tag=tag + (st,))
        assert bool((full[ref["untouched"]] == SENTINEL).all()), tag
        if wide:
            side = _np(dybuf)
            assert bool((side[:, :4] == SENTINEL).all() and (side[:, 4 + C:] == SENTINEL).all()), tag


@pytest.mark.parametrize("C", ew.GATED_C)
def test_gated_residual_matches_float64(C):
    from vicasplat_amd import ops
    w = Worst()
    for k, z in enumerate(z for z in ew.iter_gated(small_only=True) if z["C"] == C):
        _gated_case(ops, z, k, w)
    w.show(f"gated residual C={C} NV={ew.gated_nv(C)}")


def test_gated_residual_shapes_reach_every_instantiation_and_ragged_group():
    assert sorted({ew.gated_nv(C) for C in ew.GATED_C}) == [1, 2, 3, 4, 8]
    assert {C % 256 != 0 for C in ew.GATED_C if C > 256} == {True, False}      # a masked last vector, and none
    cases = list(ew.gated_cases(41))
    assert any(gr is not None and 41 % gr for gr, _ in cases) and any(gi for _, gi in cases) and any(gr is None for gr, _ in cases)


@pytest.mark.parametrize("which", ["deep", "one_group"])
def test_gated_residual_backward_when_a_wave_takes_more_rows(which):
    from vicasplat_amd import ops
    spec = ew.GATED_DEEP if which == "deep" else ew.GATED_ONE
    rpc = ew.gated_chunk_rows(spec["M"], spec["gate_rows"])
    assert rpc > 4 and (which != "deep" or rpc > 8) and (which != "one_group" or rpc == 5)      # a wave takes 2 rows; 3 and more on the deep case
    assert which != "deep" or spec["M"] % spec["gate_rows"] == 11
    w = Worst()
    z = [z for z in ew.iter_gated() if z["M"] == spec["M"]]
    assert len(z) == 1
    _gated_case(ops, z[0], 0, w)
    w.show(f"gated residual {which} rows_per_chunk={rpc}")


# --------------------------------------------------------------------------------------------------------------------------------------
# column sums
# --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("st", ["f32", "f16", "bf16"])
def test_colsum_matches_float64(st):
    from vicasplat_amd import ops
    w, routes = Worst(), {}
    for N in ew.COLSUM_N:
        for M in ew.COLSUM_M:
            x = ew.colsum_input(M, N, st)
            ref = ew.colsum(x)
            assert bool((ref["colsum_mag"][1::4] == 0).all())      # the all-zero columns: exactly 0
            buf = torch.zeros((M, N + 16), dtype=DT[st], device=_dev())
            for layout, view in (("contiguous", _t(x, DT[st])), ("slice", buf[:, 8:8 + N]), ("offset1", buf[:, 1:1 + N])):
                if layout != "contiguous":
                    buf.fill_(SENTINEL)
                    view.copy_(_t(x, DT[st]))
                route = ew.colsum_route(M, N, st, view.stride(0), view.data_ptr() % 16 != 0)[0]
                routes.setdefault((N, layout), set()).add(route)
                w.check(_np(ops.colsum(view)), ref, "colsum", tag=(M, N, layout, route))
    vec = "vec32" if st == "f32" else "vec16"
    assert routes[(100, "contiguous")] == {"vec32" if st == "f32" else "scalar"} and routes[(102, "contiguous")] == {"scalar"}
    assert routes[(128, "contiguous")] == {vec} and routes[(128, "slice")] == {vec} and routes[(128, "offset1")] == {"scalar"}
    w.show(f"colsum {st}")


# --------------------------------------------------------------------------------------------------------------------------------------
# bilinear x2
# --------------------------------------------------------------------------------------------------------------------------------------
def _unpack(data, C):
    """int32 [rows, C] packed (hi, lo) f16 pairs in blocks of 32 columns (chunk g of a block holds k = 4g..4g+3, 16+4g..16+4g+3) -> hi + lo."""
    rows = data.shape[0]
    halves = data.view(torch.float16).reshape(rows, C // 32, 2, 32).double()
    pos = torch.arange(32)
    g, t = pos // 8, pos % 8
    k_of_pos = torch.where(t < 4, 4 * g + t, 16 + 4 * g + (t - 4))
    rec = torch.zeros(rows, C // 32, 32, dtype=torch.float64, device=data.device)
    rec[..., k_of_pos] = halves[:, :, 0] + halves[:, :, 1]
    return rec.reshape(rows, C)


def _up(ops, st, x, add, relu):
    """ops.upsample2x_nhwc in the storage class st -> float64 numpy."""
    dt = DT["f32" if st == "packed" else st]
    out = ops.upsample2x_nhwc(_t(x, dt), None if add is None else _t(add, dt), relu_add=relu, packed=st == "packed")
    if st == "packed":
        torch.cuda.synchronize()
        return _unpack(out.data.reshape(-1, x.shape[3]), x.shape[3]).cpu().numpy()
    return _np(out)


@pytest.mark.parametrize("st", ["f16", "bf16", "f32", "packed"])
def test_upsample_forward_matches_float64(st):
    from vicasplat_amd import ops
    w, kernels, spills = Worst(), set(), set()
    ist = "f32" if st == "packed" else st
    for N, H, W, C in ew.iter_upsample(st):
        kern = ew.upsample_kernel(ist, H, W)
        kernels.add(kern)
        if ew.upsample_grid_rows(kern, N, H) > 32768:
            spills.add(kern)
        x, add, _ = ew.upsample_inputs(N, H, W, C, ist)
        assert bool((add == 0).any() and (add < 0).any())
        for a, relu in ((None, False), (add, False), (add, True)):
            ref = ew.upsample2x(x, a, relu)
            w.check(_up(ops, st, x, a, relu), ref, "up", "f32" if st == "packed" else st, st == "packed", tag=(N, H, W, C, a is not None, relu))
    assert kernels == {"f16": {"block16"}, "bf16": {"block16"}, "f32": {"block32", "point32"}, "packed": {"block32"}}[st]
    assert spills == ({"block16"} if st in ("f16", "bf16") else {"block32", "point32"} if st == "f32" else set())
    assert -(-9 * (264 // 8) // 256) == 2 and -(-9 * (132 // 4) // 256) == 2      # W = 9 at the widest C: two blocks in x, the second partial
    w.show(f"upsample x2 {st}")


@pytest.mark.parametrize("st", ["f16", "bf16", "f32"])
def test_upsample_transpose_matches_float64(st):
    from vicasplat_amd import ops
    w, spill = Worst(), 0
    for N, H, W, C in ew.iter_upsample(st):
        spill += N * H > 32768
        x, _, g = ew.upsample_inputs(N, H, W, C, st)
        ref = ew.upsample2x_transpose(g)
        got = _np(ops.upsample2x_backward_nhwc(_t(g, DT[st])))
        w.check(got, ref, "up_t", st, tag=(N, H, W, C))
        if st == "f32":      # <up(x), g> = <x, up^T(g)> from the GPU's own two outputs, in float64
            fwd = ew.upsample2x(x)
            up = _up(ops, "f32", x, None, False)
            lhs, rhs = float((up * g).sum()), float((x * got).sum())
            lim = float((np.abs(g) * ew.allowance(fwd, "up", R32["up"])).sum() + (np.abs(x) * ew.allowance(ref, "up_t", R32["up_t"])).sum())
            assert abs(lhs - rhs) <= lim, (N, H, W, C, lhs, rhs, lim)
    assert spill == (2 if st == "f32" else 1)
    w.show(f"upsample x2 transpose {st}")


@pytest.mark.parametrize("W", [2, 3])
@pytest.mark.parametrize("st", ["f16", "bf16", "f32", "packed"])
def test_upsample_zero_weight_column_does_not_spread_nan(st, W):
    from vicasplat_amd import ops
    ist = "f32" if st == "packed" else st
    x, _, _ = ew.upsample_inputs(1, 2, W, 32, ist)
    x[:, :, 0, :] = np.nan      # where x0 + 2, unclamped and wrapped, would read
    ref = ew.upsample2x(x)
    nan = np.isnan(ref["up"])
    assert not nan[:, :, -1].any() and nan[:, :, 0].all()
    got = _up(ops, st, x, None, False).reshape(nan.shape)
    assert bool((np.isnan(got) == nan).all())
    fin = dict(up=np.where(nan, 0.0, ref["up"]), up_mag=np.where(nan, 0.0, ref["up_mag"]))
    assert ew.crit(np.where(nan, 0.0, got), fin, "up", R32["up"], ist, st == "packed") <= 1.0


# --------------------------------------------------------------------------------------------------------------------------------------
# rotary embeddings
# --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("st", ["f32", "f16", "bf16"])
def test_rope_qk_matches_float64(st):
    from vicasplat_amd import ops
    w, seen = Worst(), set()
    for z in ew.iter_rope_qk():
        rows, H, k_col = z["rows"], z["H"], z["k_col"]
        pos = _t(z["pos"], torch.int32)
        kind = None if z["kind"] is None else _t(z["kind"], torch.uint8)
        seen.add((rows % 4 != 0, k_col != 64 * H, z["kind"] is not None and 2 in z["kind"].tolist()))
        args = (z["buf"], H, k_col, z["pos"], z["kind"])
        fwd, inv = ew.rope_qk(*args, direction=1.0), ew.rope_qk(*args, direction=-1.0)
        buf = _t(z["buf"], DT[st])
        assert buf.stride(0) > k_col + 128 * H
        got_f = _np(ops.rope_qk(buf, H, k_col, pos, kind))      # everything outside the two blocks has magnitude 0: unchanged bit for bit
        w.check(got_f, fwd, "rope_qk", st, tag=(rows, H, k_col, "fwd"))
        w.check(_np(ops.rope_qk(_t(z["buf"], DT[st]), H, k_col, pos, kind, inverse=True)), inv, "rope_qk", st, tag=(rows, H, k_col, "inv"))
        # inverse(forward(x)) = x within the two bounds added (a forward error reaches both members of its pair)
        back = _np(ops.rope_qk(buf, H, k_col, pos, kind, inverse=True))
        a_f = ew.allowance(fwd, "rope_qk", R32["rope_qk"], st)
        back_ref = ew.rope_qk(fwd["rope_qk"], H, k_col, z["pos"], z["kind"], direction=-1.0)
        a_i = ew.allowance(back_ref, "rope_qk", R32["rope_qk"], st)
        cols = np.arange(z["ld"])
        k1 = np.zeros(rows, bool) if z["kind"] is None else (z["kind"] == 1)
        partner = np.where(k1[:, None], cols[None, :] ^ 1, cols[None, :] ^ 16)
        partner = np.minimum(partner, z["ld"] - 1)
        lim = np.where(fwd["rope_qk_mag"] > 0, a_i + a_f + np.take_along_axis(a_f, partner, 1), 0.0)
        assert bool((np.abs(back - z["buf"]) <= lim).all()), (rows, H, k_col, st)
    assert {(True, True, True), (False, False, False)} <= seen and any(s[0] and not s[2] for s in seen)
    w.show(f"rope_qk {st}")


@pytest.mark.parametrize("st", ["f32", "f16", "bf16"])
def test_rope2d_matches_float64(st):
    from vicasplat_amd.curope import rope_2d
    w = Worst()
    for z in ew.iter_rope2d():
        B, N, H, D = z["B"], z["N"], z["H"], z["D"]
        for fwd in (1.0, -1.0):
            buf = _t(z["tokens"], DT[st])
            view = buf[:, :N]
            assert view.stride(0) != N * H * D
            rope_2d(view, _t(z["pos"], torch.int64), 100.0, fwd)
            got = _np(buf)
            w.check(got[:, :N], ew.rope2d(z["tokens"][:, :N], z["pos"], 100.0, fwd), "rope2d", st, tag=(B, N, H, D, fwd))
            assert ew.same_bits(got[:, N], z["tokens"][:, N])      # the spare token
    assert int(max(z["pos"].max() for z in ew.iter_rope2d())) == 1000
    w.show(f"rope2d {st}")
