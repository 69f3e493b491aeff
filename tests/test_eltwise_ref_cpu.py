"""The float64 references of tests/eltwise_f64.py are right, and the criterion of tests/test_eltwise_edges_gpu.py has teeth.  No GPU.

1. Pinned: each reference equals torch in float64 (F.gelu and its autograd, F.silu, F.interpolate(mode="bilinear", align_corners=True)
   and its autograd for the transpose, autograd of the plain gated-residual expression, a plain column sum, the two rotary formulas
   written out in torch) to 1e-12 mag per element.
2. r32: the same code in float32 against float64, max |f32 - f64| / (2^-24 mag) per output over the edge inputs of the GPU tests
   (`-s` prints them; eltwise_f64.R32_ELTWISE holds them rounded up):

       gelu 0.64   gelu_grad 0.66   silu 0.60   gated_out 1.00   gated_dy 0.99   dgate 1.88   colsum 6.08   up 0.90   up_t 0.49
       rope_qk 0.70   rope2d 0.44

   Most stay at or below 1 (mag is a worst-case bound), so B = 4 for them.  The two row sums exceed it: a thread's, a block's and numpy's
   partial sums each round once more than the one rounding per sum that mag counts (the reference adds pairwise along the transposed
   column, as the kernels' lanes, LDS reductions and atomics do; row after row it was 152).  dgate gets B = 4 x 1.9, colsum 4 x 6.1.
3. Mutation check: each of the eleven planted defects exceeds the GPU criterion on a shape of the GPU tests (the factor is printed); the
   clean restatement stays inside it on every case.  The unclamped third source column of the 2 x 2 upsample kernels (x0 + 2 wrapped
   instead of min(x0 + 2, W - 1)) always carries the weight 0 -- the position of the last output column is exactly W - 1 -- so no finite
   input shows it in a value: it shows where that column holds a NaN, which must not spread to the outputs whose own four neighbours are
   finite.  The widths 2 and 3 are checked that way (here and on the GPU).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import eltwise_f64 as ew

T = torch.from_numpy


def _close(got, ref, name, rel=1e-12):
    got = np.asarray(got, np.float64).reshape(ref[name].shape)
    err, lim = np.abs(got - ref[name]), rel * ref[name + "_mag"] + 1e-300
    assert bool((err <= lim).all()), (name, float(err.max()), int(np.argmax((err - lim).reshape(-1))))


# --------------------------------------------------------------------------------------------------------------------------------------
# 1. pins
# --------------------------------------------------------------------------------------------------------------------------------------
def test_activation_references_equal_torch_float64():
    x = ew.act_values(240, "f32", extra=(88.0, 100.0))
    x = np.concatenate([x, np.random.default_rng(0).standard_normal(500) * 3])
    dy = ew.f32(np.random.default_rng(1).standard_normal(x.size))
    tx = T(x).requires_grad_()
    y = F.gelu(tx)
    _close(y.detach().numpy(), ew.gelu(x), "gelu")
    (g,) = torch.autograd.grad((y * T(dy)).sum(), tx)
    _close(g.numpy(), ew.gelu_grad(dy, x), "gelu_grad")
    _close(F.silu(T(x)).numpy(), ew.silu(x), "silu")
    m = ew.relu_mask(dy, x)
    (gr,) = torch.autograd.grad((F.relu(tx) * T(dy)).sum(), tx)
    assert ew.same_bits(m, np.where(x > 0, dy, 0.0)) and bool((gr.numpy() == m).all())
    hi, lo = ew.split16(x)
    thi = T(x).float().half()
    tlo = (T(x).float() - thi.float()).half()
    assert ew.same_bits(hi, thi.double().numpy()) and ew.same_bits(lo, tlo.double().numpy())


@pytest.mark.parametrize("M,C,gr,gi", [(33, 260, 5, 0), (41, 192, 9, 9), (7, 4, None, 3), (33, 516, 33, 16), (41, 8, 3, 3)])
def test_gated_residual_reference_equals_float64_autograd(M, C, gr, gi):
    G = 1 if gr is None else -(-M // gr)
    rows = M if gi == 0 else -(-M // gi) * (gi + 1)
    z = ew.gated_inputs(M, C, G, rows, "f16")
    z.update(gate_rows=gr, grp_in=gi, grp_out=gi + 1 if gi else 0, grp_off=1 if gi else 0)
    ref = ew.gated_refs(z)
    yr = ew.out_rows(M, z["grp_in"], z["grp_out"], z["grp_off"])
    assert bool((yr == ref["yrow"]).all()) and len(set(yr.tolist()) | set(ref["untouched"].tolist())) == rows
    x, y, gate = T(z["x"]), T(z["y"]).requires_grad_(), T(z["gate"]).requires_grad_()
    ysel = y[T(yr)]
    out = x + ysel if gr is None else x + (1 + gate[torch.arange(M) // gr]) * ysel
    _close(out.detach().numpy(), ref, "gated_out")
    grads = torch.autograd.grad((out * T(z["dout"])).sum(), (y,) if gr is None else (y, gate))
    _close(grads[0].numpy()[yr], ref, "gated_dy")
    assert bool((grads[0].numpy()[ref["untouched"]] == 0).all())
    if gr is not None:
        _close(grads[1].numpy(), ref, "dgate")
    else:
        assert "dgate" not in ref and ew.same_bits(ref["gated_dy"], z["dout"])


def test_colsum_reference_equals_torch_float64():
    x = ew.colsum_input(129, 12, "f32")
    ref = ew.colsum(x)
    _close(T(x).sum(0).numpy(), ref, "colsum")
    assert bool((ref["colsum"][1::4] == 0).all() and (ref["colsum_mag"][1::4] == 0).all())


def _torch_up(x, add, relu_add):
    o = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    return o if add is None else o + (F.relu(add) if relu_add else add)


@pytest.mark.parametrize("H,W", ew.UP_HW)
def test_upsample_references_equal_torch_float64(H, W):
    x, add, g = ew.upsample_inputs(3, H, W, 4, "f32")
    tx = T(x).requires_grad_()
    for a, r in ((None, False), (add, False), (add, True)):
        _close(_torch_up(tx, None if a is None else T(a), r).detach().numpy(), ew.upsample2x(x, a, r), "up", 1e-11)
    (gx,) = torch.autograd.grad((_torch_up(tx, None, False) * T(g)).sum(), tx)
    _close(gx.numpy(), ew.upsample2x_transpose(g), "up_t", 1e-11)


def _torch_rope_qk(buf, H, k_col, pos, kind, base2d, theta1d, direction):
    out = buf.clone()
    i = torch.arange(16, dtype=torch.float64)
    p = torch.arange(32, dtype=torch.float64)
    for r in range(buf.shape[0]):
        kd = 0 if kind is None else int(kind[r])
        if kd == 2:
            continue
        for col in (0, k_col):
            for h in range(H):
                blk = buf[r, col + 64 * h: col + 64 * h + 64]
                o = out[r, col + 64 * h: col + 64 * h + 64]
                if kd == 0:
                    for half in range(2):
                        a = direction * float(pos[r, half]) / base2d ** (i / 16)
                        u, v = blk[32 * half: 32 * half + 16], blk[32 * half + 16: 32 * half + 32]
                        o[32 * half: 32 * half + 16] = u * torch.cos(a) - v * torch.sin(a)
                        o[32 * half + 16: 32 * half + 32] = v * torch.cos(a) + u * torch.sin(a)
                else:
                    a = direction * float(pos[r, 0]) / theta1d ** (2 * p / 64)
                    u, v = blk[0::2], blk[1::2]
                    o[0::2] = u * torch.cos(a) - v * torch.sin(a)
                    o[1::2] = v * torch.cos(a) + u * torch.sin(a)
    return out


@pytest.mark.parametrize("direction", [1.0, -1.0])
def test_rope_references_equal_torch_float64(direction):
    for z in ew.iter_rope_qk():
        if z["rows"] not in (5, 9) or z["H"] not in (1, 3):
            continue
        ref = ew.rope_qk(z["buf"], z["H"], z["k_col"], z["pos"], z["kind"], direction=direction)
        _close(_torch_rope_qk(T(z["buf"]), z["H"], z["k_col"], z["pos"], z["kind"], 100.0, 30.0, direction).numpy(), ref, "rope_qk")
        touched = ref["rope_qk_mag"] > 0
        assert ew.same_bits(ref["rope_qk"][~touched], z["buf"][~touched])
        assert not touched[:, 64 * z["H"]: z["k_col"]].any() and not touched[:, z["k_col"] + 64 * z["H"]:].any()
        if z["kind"] is not None:
            assert not touched[z["kind"] == 2].any()
    for z in ew.iter_rope2d():
        B, N, H, D = z["B"], z["N"], z["H"], z["D"]
        tok, Q = T(z["tokens"][:, :N]), D // 4
        t = tok.reshape(B, N, H, 2, 2, Q)
        a = direction * T(z["pos"]).double().reshape(B, N, 1, 2, 1) / 100.0 ** (torch.arange(Q, dtype=torch.float64) / Q)
        u, v = t[:, :, :, :, 0], t[:, :, :, :, 1]
        exp = torch.stack([u * torch.cos(a) - v * torch.sin(a), v * torch.cos(a) + u * torch.sin(a)], 4).reshape(B, N, H, D)
        _close(exp.numpy(), ew.rope2d(z["tokens"][:, :N], z["pos"], 100.0, direction), "rope2d")


# --------------------------------------------------------------------------------------------------------------------------------------
# 2. / 3. the f32 restatement over the edge inputs: r32 units, or error / GPU bound
# --------------------------------------------------------------------------------------------------------------------------------------
def _score(got, ref, names, worst, as_ratio):
    for k in names:
        v = ew.crit(got[k], ref, k, ew.R32_ELTWISE[k]) if as_ratio else ew.units(got[k], ref, k)
        if not as_ratio:
            assert np.isfinite(ew.ratio(got[k], ref, k, 1e30)), k      # elements of magnitude 0 are exact
        worst[k] = max(worst.get(k, 0.0), v)


def _colsum_kw(M, N, st, mutate):
    if mutate is None:
        return {}
    kernel, lanes, gy = ew.colsum_route(M, N, st, N)
    return dict(lanes=lanes, gy=gy) if kernel != "scalar" else None


def _run_family(family, mutate=None, as_ratio=False):
    """{output: worst r32 units (or worst error / bound)} of one family over its edge inputs."""
    worst = {}
    f32 = dict(dtype=np.float32, mutate=mutate)
    if family == "act":
        for st, ns in (("f16", ew.ACT_N16), ("bf16", ew.ACT_N16), ("f32", ew.ACT_N32)):
            x = ew.act_values(max(ns), st)
            dy = ew.round_to(1.0 + 0.25 * np.cos(np.arange(x.size)), st)
            _score(ew.gelu(x, **f32), ew.gelu(x), ["gelu"], worst, as_ratio)
            _score(ew.gelu_grad(dy, x, **f32), ew.gelu_grad(dy, x), ["gelu_grad"], worst, as_ratio)
        x = ew.act_values(max(ew.ACT_N32), "f32", extra=(88.0, 100.0))
        _score(ew.silu(x, **f32), ew.silu(x), ["silu"], worst, as_ratio)
    elif family == "gated":
        for z in ew.iter_gated():
            names = ["gated_out"] + (["gated_dy", "dgate"] if z["gate_rows"] is not None else [])
            _score(ew.gated_refs(z, **f32), ew.gated_refs(z), names, worst, as_ratio)
    elif family == "colsum":
        for st in ("f32", "f16", "bf16"):
            for N in ew.COLSUM_N:
                for M in ew.COLSUM_M:
                    kw = _colsum_kw(M, N, st, mutate)
                    if kw is None:
                        continue
                    x = ew.colsum_input(M, N, st)
                    _score(ew.colsum(x, **f32, **kw), ew.colsum(x), ["colsum"], worst, as_ratio)
    elif family == "up":
        for N, H, W, C in ew.iter_upsample("f32"):
            x, add, g = ew.upsample_inputs(N, H, W, C, "f32")
            for a, r in ((None, False), (add, False), (add, True)):
                _score(ew.upsample2x(x, a, r, **f32), ew.upsample2x(x, a, r), ["up"], worst, as_ratio)
            _score(ew.upsample2x_transpose(g, **f32), ew.upsample2x_transpose(g), ["up_t"], worst, as_ratio)
    elif family == "rope":
        for z in ew.iter_rope_qk():
            for d in (1.0, -1.0):
                a = (z["buf"], z["H"], z["k_col"], z["pos"], z["kind"])
                _score(ew.rope_qk(*a, direction=d, **f32), ew.rope_qk(*a, direction=d), ["rope_qk"], worst, as_ratio)
        for z in ew.iter_rope2d():
            for d in (1.0, -1.0):
                a = (z["tokens"][:, :z["N"]], z["pos"], 100.0, d)
                _score(ew.rope2d(*a, **f32), ew.rope2d(*a), ["rope2d"], worst, as_ratio)
    return worst


FAMILIES = ("act", "gated", "colsum", "up", "rope")


@pytest.fixture(scope="module")
def clean():
    """Both measurements of the unmutated restatement, computed once."""
    return {f: (_run_family(f), _run_family(f, as_ratio=True)) for f in FAMILIES}


def test_f32_restatement_ratios(clean):
    """r32 per output over the edge inputs; the recorded values (eltwise_f64.R32_ELTWISE) are those, rounded up."""
    worst = {}
    for f in FAMILIES:
        worst.update(clean[f][0])
    print("r32 eltwise", {k: round(v, 2) for k, v in worst.items()})
    assert set(worst) == set(ew.R32_ELTWISE)
    for k, v in worst.items():
        assert v <= ew.R32_ELTWISE[k], (k, v)
        assert ew.R32_ELTWISE[k] == 1.0 or ew.R32_ELTWISE[k] - v < 0.1, (k, v)      # recorded = measured, rounded up


def test_clean_restatement_passes_the_gpu_criterion(clean):
    for f in FAMILIES:
        assert max(clean[f][1].values()) <= 1.0, (f, clean[f][1])


# defect -> (family, outputs that must exceed the bound)
MUTANTS = {"no_zphi": ("act", ("gelu_grad",)),                  # 1. GELU' without z phi(z)
           "erf_sat4": ("act", ("gelu", "gelu_grad")),          # 2. 1 + erf saturated at |z| >= 4
           "gate_grp_in": ("gated", ("gated_out",)),            # 3. the gate of group m // grp_in
           "second_trip": ("gated", ("dgate",)),                # 4. dgate without the rows of a wave's later trips
           "masked_vec": ("gated", ("dgate", "gated_dy")),      # 5. columns >= 256 floor(C / 256) skipped
           "no_remainder": ("colsum", ("colsum",)),             # 6. the rows after the 4 x unrolled loop dropped
           "window1": ("up", ("up_t",)),                        # 8. transpose scanning +-1 output rows / columns
           "kind1_pairs16": ("rope", ("rope_qk",)),             # 9. pairs (i, i + 16) for kind 1
           "inv_k_forward": ("rope", ("rope_qk",)),             # 10. the inverse rotating k forward
           "relu_interp": ("up", ("up",))}                      # 11. relu applied to the interpolated value as well


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutants_fail_the_gpu_criterion(mutant):
    family, outs = MUTANTS[mutant]
    r = _run_family(family, mutate=mutant, as_ratio=True)
    print(mutant, {k: f"{r[k]:.3g}x" for k in outs})
    for k in outs:
        assert r[k] > 1.0, (mutant, k, r[k])


def test_second_trip_mutant_is_caught_by_the_deep_and_the_single_group_case():
    """Mutant 4 needs more than 4 rows per chunk: only the two cases built for it reach that, and each catches it on its own."""
    seen = 0
    for z in ew.iter_gated():
        rpc = ew.gated_chunk_rows(z["M"], z["gate_rows"] or 0, z["gate_rows"] is not None)
        if z["gate_rows"] is None:
            continue
        got, ref = ew.gated_refs(z, dtype=np.float32, mutate="second_trip"), ew.gated_refs(z)
        caught = ew.crit(got["dgate"], ref, "dgate", ew.R32_ELTWISE["dgate"]) > 1.0
        assert caught == (rpc > 4), (z["M"], z["C"], z["gate_rows"], rpc)
        seen += caught
    assert seen == 2 and ew.gated_chunk_rows(**{k: ew.GATED_DEEP[k] for k in ("M", "gate_rows")}) > 8


@pytest.mark.parametrize("W", [2, 3])
def test_unclamped_third_column_mutant_spreads_a_nan(W):
    """Mutant 7: x0 + 2 (wrapped) instead of min(x0 + 2, W - 1).  Its weight is exactly 0, so it changes no finite value; with a NaN in the
    column it wrongly reads, the last output column -- whose own neighbours are finite -- turns NaN."""
    x, _, _ = ew.upsample_inputs(1, 2, W, 4, "f32")
    ref, mut = ew.upsample2x(x), ew.upsample2x(x, dtype=np.float32, mutate="x2_wrap")
    assert ew.crit(mut["up"], ref, "up", ew.R32_ELTWISE["up"]) <= 1.0      # invisible in values
    x[:, :, 0, :] = np.nan
    ref, clean_, mut = ew.upsample2x(x), ew.upsample2x(x, dtype=np.float32), ew.upsample2x(x, dtype=np.float32, mutate="x2_wrap")
    assert bool((np.isnan(ref["up"]) == np.isnan(clean_["up"])).all())
    assert not np.isnan(ref["up"][:, :, -1]).any() and np.isnan(mut["up"][:, :, -1]).all()
