"""LayerNorm with AdaLN modulation (csrc/norm_rope.hip forward, csrc/backward.hip backward) against the float64 reference of
tests/pointwise_f64.py.  -m gpu.

Rows cycle through: mean 300 with unit spread (the ViT's massive-activation channels), a constant row (output = b (1 + scale) + shift),
spread 1e-5 (variance << eps), one channel at 1e4 among unit values, ordinary.  C = 1024, 768: the row-group kernels (a wave takes 4
rows, 8 with a modulation); 192, 2048 (the maximum), 4: the generic kernel.  M = 1, 7, 9, 33.  mod_rows = 3, 5, 9 put a group boundary
inside a wave's 8 rows; mod_rows = M is one group.  Outputs are written behind one extra row per group (grp_out = grp_in + 1, grp_off =
1); the skipped rows must stay untouched.

Criterion, per element:  |gpu - ref| <= B 2^-24 mag,  B = 4 r32 of the output (pointwise_f64.R32_LAYERNORM; r32 below); 16-bit outputs
get half an ulp of their type on top; the packed (hi, lo) output (out_dtype 3) is decoded as hi + lo and held to the f32 bound plus
max(2^-22 |ref|, 2^-25) for the pair's representation: lo = f16(y - hi) is within 2^-11 |lo| <= 2^-22 |y| while it is a normal f16
number and within half a subnormal step, 2^-25, below 2^-14 (measured without that term: up to 3.0 x the allowance, on elements with
|y| << 1 only; the packed format has scale 2^0, so this is the format's resolution, not the kernel's arithmetic).

Measured on an MI355X, max |gpu - ref| / (2^-24 mag) over all cases (`-s` prints them per case), beside r32:

    output   r32    gpu
    y        1.18   1.11   (f32; f16 / bf16: 1.00, packed: 0.73 of the allowance; dx16: 1.00 of the allowance)
    dx       1.05   0.98
    dw       1.06   0.79
    db       2.31   1.83
    dscale   1.18   0.86
    dshift   2.02   2.02
"""
import numpy as np
import pytest
import torch

import pointwise_f64 as pw

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
SHAPES = [(M, C) for C in (1024, 768, 192, 2048, 4) for M in (1, 7, 9, 33)]
SENTINEL = 7.0


def _dev():
    return torch.device("cuda:0")


def _t(a, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(_dev())


def _mods(M):
    """mod_rows of the cases of one shape: none, 3 / 5 / 9 (where they split the rows), one group."""
    return [0] + [r for r in (3, 5, 9) if r < M] + [M]


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


def _case(M, C, mod_rows):
    gi = mod_rows if mod_rows else max(1, M // 2)
    G = -(-M // gi)
    z = pw.layernorm_edge_inputs(M, C, G)
    orow = pw.out_rows(M, gi, gi + 1, 1)
    return z, gi, G, orow


@pytest.mark.parametrize("M,C", SHAPES)
def test_layernorm_forward_matches_float64(M, C):
    from vicasplat_amd import ops
    worst = {}
    for mod_rows in _mods(M):
        z, gi, G, orow = _case(M, C, mod_rows)
        x, w, b = _t(z["x"]), _t(z["w"]), _t(z["b"])
        kw = dict(scale=_t(z["scale"]), shift=_t(z["shift"]), mod_rows=mod_rows) if mod_rows else {}
        ref = pw.layernorm_forward(z["x"], z["w"], z["b"], **(dict(scale=z["scale"], shift=z["shift"], mod_rows=mod_rows) if mod_rows else {}))
        B = pw.gpu_factor(pw.R32_LAYERNORM["y"])
        grp = np.arange(M) // (mod_rows or M)
        flat = z["b"] * (1 + z["scale"][grp]) + z["shift"][grp] if mod_rows else np.broadcast_to(z["b"], (M, C))
        const = np.arange(M) % len(pw.LN_ROW_KINDS) == pw.LN_ROW_KINDS.index("constant")
        for odt in ("f32", "f16", "bf16") + (("packed",) if C % 32 == 0 else ()):
            rows = G * (gi + 1)
            if odt == "packed":
                out = ops.split_act(rows, C, _dev())
                out.data.fill_(0x3C003C00)
                ops.layernorm_mod(x, w, b, out, grp_in=gi, grp_out=gi + 1, grp_off=1, **kw)
                full, sent, st, extra = _unpack(out.data, C), float(_unpack(torch.full((1, C), 0x3C003C00, dtype=torch.int32, device=_dev()), C)[0, 0]), "f32", 2.0 ** -22
            else:
                out = torch.full((rows, C), SENTINEL, dtype=DT[odt], device=_dev())
                ops.layernorm_mod(x, w, b, out, grp_in=gi, grp_out=gi + 1, grp_off=1, **kw)
                full, sent, st, extra = out.double(), SENTINEL, odt, 0.0
            torch.cuda.synchronize()
            full = full.cpu().numpy()
            got = full[orow]
            xabs = np.maximum(2.0 ** -25 - 2.0 ** -22 * np.abs(ref["y"]), 0.0) if odt == "packed" else 0.0      # -> max(2^-22 |y|, 2^-25)
            r, u = pw.ratio(got, ref, "y", B, st, extra, xabs), pw.units(got, ref, "y")
            tag = "f32" if odt == "f32" else odt + " (of the allowance)"
            worst[tag] = max(worst.get(tag, 0.0), u if odt == "f32" else r)
            assert r <= 1.0, (mod_rows, odt, r, u)
            untouched = np.setdiff1d(np.arange(rows), orow)
            assert bool((full[untouched] == sent).all()), (mod_rows, odt)
            if const.any():      # a constant row: xhat = 0, the output is b (1 + scale) + shift up to the bound
                lim = (pw.bound(ref, "y", B, st, extra) + xabs)[const] + 1e-9
                assert bool((np.abs(got[const] - flat[const]) <= lim).all()), (mod_rows, odt)
    print(f"ln fwd M={M} C={C}", {k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("do_dt", ["f32", "f16"])
@pytest.mark.parametrize("M,C", SHAPES)
def test_layernorm_backward_matches_float64(M, C, do_dt):
    from vicasplat_amd import ops
    worst = {}
    for mod_rows in _mods(M):
        z, gi, G, orow = _case(M, C, mod_rows)
        x, w, b = _t(z["x"]), _t(z["w"]), _t(z["b"])
        dout = pw.round_to(z["dout"], do_dt)
        rows = G * (gi + 1)
        dfull = np.full((rows, C), np.nan)      # rows the forward never wrote carry no gradient: never read
        dfull[orow] = dout
        dfull_t = _t(dfull, DT[do_dt])
        kw = dict(scale=_t(z["scale"]), mod_rows=mod_rows) if mod_rows else {}
        rkw = dict(scale=z["scale"], mod_rows=mod_rows) if mod_rows else {}
        remap = dict(grp_in=gi, grp_out=gi + 1, grp_off=1)
        names = ("dx", "dw", "db") + (("dscale", "dshift") if mod_rows else ())

        def check(res, ref, which, tag):
            torch.cuda.synchronize()
            for name, t in zip(("dx", "dw", "db", "dscale", "dshift"), res):
                if name in which:
                    got = t.double().cpu().numpy()
                    r, u = pw.ratio(got, ref, name, pw.gpu_factor(pw.R32_LAYERNORM[name])), pw.units(got, ref, name)
                    worst[name] = max(worst.get(name, 0.0), u)
                    assert r <= 1.0, (tag, mod_rows, name, r, u)

        ref = pw.layernorm_backward(dout, z["x"], z["w"], z["b"], **rkw)
        check(ops.layernorm_backward(dfull_t, x, w, b, **kw, **remap), ref, names, "plain")
        # dx accumulated in place, and the residual-path gradient from its own buffer with a 16-bit copy of the sum
        ref_add = pw.layernorm_backward(dout, z["x"], z["w"], z["b"], dx_add=z["dx_add"], **rkw)
        check(ops.layernorm_backward(dfull_t, x, w, b, dx=_t(z["dx_add"]), accumulate_dx=True, **kw, **remap), ref_add, ("dx",), "accumulate_dx")
        for st16 in ("f16", "bf16"):
            dx16 = torch.full((M, C), SENTINEL, dtype=DT[st16], device=_dev())
            res = ops.layernorm_backward(dfull_t, x, w, b, dx_add=_t(z["dx_add"]), dx16=dx16, **kw, **remap)
            check(res, ref_add, names, "dx_add")
            r16 = pw.ratio(dx16.double().cpu().numpy(), ref_add, "dx", pw.gpu_factor(pw.R32_LAYERNORM["dx"]), st16)
            worst["dx16 (of the allowance)"] = max(worst.get("dx16 (of the allowance)", 0.0), r16)
            assert r16 <= 1.0, (st16, mod_rows, r16)
    print(f"ln bwd M={M} C={C} dout={do_dt}", {k: round(v, 3) for k, v in worst.items()})
