"""Every forward GEMM route of csrc/gemm.hip / gemm256.h against the float64 reference of tests/gemm_f64.py evaluated on the same stored
values, at the tile, tail, seam, row-map, gate-group and alignment edges.  Goes through vicasplat_amd.ops (gemm, gemm_resid, gemm_qkv_rope,
_gemm_split with resid, packed A through SplitWeight, packed output through split_act's form).  -m gpu.

Operand classes: f16, bf16, f32x (the exact-f32 kernels, dtype 3), split.  The route a case reaches is the first part of its id, written by
hand in gemm_f64.CASES and compared with gemm_f64.plan() -- the transcription of the dispatcher -- in tests/test_gemm_ref_cpu.py:
    smallm<NW,MF>  gemm_smallm_kernel     skinny(ks)  gemm_skinny_kernel, ks K slices meeting through atomics
    g256           gemm256_kernel         mi8 / mi4 / mi2  gemm_kernel<., ., MI>      tail:...  the launch that finishes the last rows
Buffers come from gemm_f64.make_case: lda, ldw > K with NaN padding, NaN in every A row outside the input map, ldo > N, spare output rows,
everything outside [mapped rows] x [0, N) pre-filled with a sentinel that must survive bit for bit.

Two families per case.  lattice (epilogues 0 / 2 / 3): exact sums, the result must equal the float64 reference rounded once, BIT FOR BIT,
on every route, K slices through atomics included, and a second call returns the same bits.  real: max |error| over max |reference| on the
live elements within the bounds of the existing tests (gemm_f64.bound): f16 2e-3, bf16 1.2e-2, their epilogue 3 2e-5 + 1e-6 K / max|ref|,
their epilogue 2 1e-4 + 2e-5 sqrt(K) / max|ref|, split 6e-6, f32x 4e-6, RoPE 3e-3 / 1.6e-2 / 2e-5 / 2e-5, epilogue 5 3e-6.
Split class: a packed-A run is bit-identical to the f32-A run on every route (M <= 64 included), and a packed output is bit-identical to
packing the f32 output, the sentinel surviving elsewhere.

Every case prints a `FIG <id> <family> rel=...` line; a failure names the worst element's row and column, its 256 / 128 / 64 tile and
whether the row belongs to the main launch or the tail.

Measured on MI355X, largest max |error| / max |reference| over the file (lattice cases: 0 on every route, K slices through atomics
included; no MFMA path deviated on exactly representable sums; RoPE figures without the pos1000 cases, see below):
    f16    epi 0 4.3e-4   epi 1 4.6e-4   epi 2 3.0e-7   epi 3 2.1e-7   RoPE 4.2e-4
    bf16   epi 0 3.4e-3   epi 1 3.3e-3   epi 2 4.1e-7   epi 3 1.8e-7   RoPE 2.6e-3
    f32x   epi 0 3.3e-7   epi 1 3.3e-7   epi 2 3.7e-7   epi 3 3.1e-7   RoPE 3.9e-6
    split  epi 0 2.5e-7   epi 1 2.4e-7   epi 2 3.6e-7   epi 3 2.5e-7   RoPE 3.9e-6   epi 5 3.3e-7
Every quantity has a bound in an existing test, so none is derived from these figures.  The whole file (907 cases) takes 23 s.

FOUND AND FIXED: the four f32-class cases with the tag pos1000 (RoPE position 1000, far behind the epilogue's 64-entry table) measured
3.0e-5 .. 6.5e-5 against the bound 2e-5, on every route alike, worst in the rows with pos = 1000 of both kinds.  The epilogue formed the
angle in f32 as p * exp2(-(i / 16) * log2(base)) (v_exp_f32 of an f32 exponent, two f32 products, the conversion to revolutions), which
carries about p * 2e-7 rad: 1e-4 rad at p = 1000.  Positions >= 64 now take their frequency in revolutions as the product of two (hi, lo)
float pairs computed in double by the entry point, and the angle in two floats (sincos_far, gemm_common.h; GemmArgs::rope2_u ...); positions
below 64 keep their formula.  With it the four cases meet 2e-5 and the whole suite passes.
"""
import pytest
import torch

import gemm_f64 as G
from gemm_f64 import CASES, SENTINEL_PACKED, bound, build, gemm_f64, to_device, view2d

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _launch(c, ops, a_packed=None, out_packed=None):
    """One call of the case (device tensors) into a fresh copy of its initial output buffer.  -> (flat output buffer or None, [rows, N] view)."""
    M, N, K = c.M, c.N, c.K
    a_packed = c.a_packed if a_packed is None else a_packed
    out_packed = c.out_packed if out_packed is None else out_packed
    sp = c.cls == "split"
    Af = view2d(c.A, c.A_spec)
    Wf = view2d(c.W, c.W_spec)
    a = Af[:, :K] if c.a_grp is not None else Af[:M, :K]
    if sp:
        w = ops.SplitWeight(ops.split_pack_weight(Wf, c.scale_exp).data[:, :K], 2.0 ** -c.scale_exp, (N, K))
        if a_packed:      # the packed image of the whole [rows, lda] buffer (blocks of 32 k: its first K columns are the packed A)
            a = ops.SplitWeight(ops.split_pack_weight(Af, 0).data[:a.shape[0], :K], 1.0, (a.shape[0], K))
    else:
        w = Wf[:, :K]
    bias = None if c.bias is None else view2d(c.bias, c.bias_spec)[0]
    gate = None if c.gate is None else view2d(c.gate, c.gate_spec)
    resid = None if c.resid is None else view2d(c.resid, c.resid_spec)
    maps = dict(M=M)
    if c.grp is not None:
        maps.update(grp_in=c.grp[0], grp_out=c.grp[1], grp_off=c.grp[2])
    if c.a_grp is not None:
        maps.update(a_grp_in=c.a_grp[0], a_grp_out=c.a_grp[1], a_grp_off=c.a_grp[2])
    if c.contiguous_out and resid is not None:          # ops.gemm_resid (vs_gemm_resid for the 16-bit and f32 classes): a new [M, N] tensor
        assert resid.is_contiguous()
        return None, ops.gemm_resid(a, w, bias, resid, gate=gate, gate_rows=c.gate_rows if gate is not None else 0)
    if out_packed:
        buf = torch.full((c.out_rows * c.ldo,), SENTINEL_PACKED, dtype=torch.int32, device=c.A.device)
        out = ops.SplitWeight(view2d(buf, c.out_spec), 1.0, (c.out_rows, N))
    else:
        buf = c.out0.clone()
        out = view2d(buf, c.out_spec)
    gk = dict(gate=gate, gate_rows=c.gate_rows if gate is not None else 0)
    if sp:
        rope = dict(pos=c.pos, kind=c.kind, C=c.rope_C, base2d=G.ROPE_BASE2D, theta1d=G.ROPE_THETA1D) if c.epi == 4 else {}
        ops._gemm_split(a, w, bias, out, c.epi, resid=resid, **gk, **maps, **rope)
    elif c.epi == 4:
        ops.gemm_qkv_rope(a, w, bias, out, c.rope_C, c.pos, c.kind, G.ROPE_BASE2D, G.ROPE_THETA1D, **maps)
    else:
        ops.gemm(a, w, bias, out, c.epi, **gk, **maps)
    return buf, view2d(buf, c.out_spec)


def _where(c, got, ref, live):
    """The worst live element: row, column, its tiles, main launch or tail."""
    e = torch.nan_to_num((got.double() - ref).abs(), nan=float("inf"))
    e = torch.where(live, e, torch.zeros_like(e))
    i = int(e.argmax())
    r, n = divmod(i, e.shape[1])
    orow = G.map_rows(c.M, c.grp)
    ms = torch.nonzero(orow == r).flatten().tolist()
    m = ms[0] if ms else -1
    part = "main" if m < c.rows_main else "tail"
    return (f"worst at output row {r} (m = {m}, {part}; rows_main = {c.rows_main}), column {n}: got {float(got[r, n]):.9g} ref {float(ref[r, n]):.9g}; "
            f"tile256 ({m // 256}, {n // 256}) tile128 ({m // 128}, {n // 128}) tile64 ({m // 64}, {n // 64}); plan {c.plan}")


def _outside_untouched(c, buf):
    """Every element of the output allocation outside [mapped rows] x [0, N) still holds its initial bits."""
    touched = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    view2d(touched, c.out_spec)[c.live] = True
    init = c.out0 if buf.dtype != torch.int32 else torch.full_like(buf, SENTINEL_PACKED)
    return bool((buf[~touched] == init[~touched]).all())


def _check(case, family, ops, fig):
    cpu = build(case, family)
    c = to_device(cpu, _dev())
    ref = gemm_f64(c)
    live = c.live[:, None].expand(c.out_rows, c.N)
    buf, got = _launch(c, ops)
    assert bool(torch.isfinite(got[live].float()).all()), "NaN / inf in a live element: " + _where(c, got, ref, live)
    if buf is not None:
        assert _outside_untouched(c, buf), "wrote outside [mapped rows] x [0, N)"
    refmax = float(ref[live].abs().max())
    err = float((got.double() - ref)[live].abs().max()) / refmax
    tol = bound(c.cls, c.epi, c.K, refmax)
    print(f"FIG {case.id} {family} {c.cls} rel={err:.3e} bound={tol:.3e} refmax={refmax:.4g}")
    fig.append(err)
    if family == "lattice":
        want = ref.to(c.odt)
        assert torch.equal(got[live], want[live]), "lattice result is not the float64 result rounded once: " + _where(c, got, ref, live)
        buf2, got2 = _launch(c, ops)
        assert torch.equal(got2, got) and (buf is None or torch.equal(buf2, buf)), "a second call returned other bits"
    else:
        assert err <= tol, _where(c, got, ref, live)
    return c, buf, got


PLAIN = [c for c in CASES if c.group in ("route", "rowmap", "gate", "align", "rope", "tiny_w")]


@pytest.mark.parametrize("case", PLAIN, ids=[c.id for c in PLAIN])
def test_route_matches_float64(case):
    """Both families of the case against float64."""
    from vicasplat_amd import ops
    fig = []
    for family in case.families:
        c, _, _ = _check(case, family, ops, fig)
    if case.group == "tiny_w":
        assert c.scale_exp == 24 == ops.split_scale_exp(view2d(c.W, c.W_spec)[:, :c.K])


PACKED_A = [c for c in CASES if c.group == "packed_a"]


@pytest.mark.parametrize("case", PACKED_A, ids=[c.id for c in PACKED_A])
def test_packed_a_is_bit_identical_to_f32_a(case):
    """vs_gemm_split_packed against vs_gemm_split on the same values, and against float64, on every route of the split class."""
    from vicasplat_amd import ops
    for family in case.families:
        c, buf, got = _check(case, family, ops, [])
        buf32, got32 = _launch(c, ops, a_packed=False)
        assert torch.equal(buf, buf32), "packed-A run differs from the f32-A run"


PACKED_OUT = [c for c in CASES if c.group == "packed_out"]


@pytest.mark.parametrize("case", PACKED_OUT, ids=[c.id for c in PACKED_OUT])
def test_packed_output_is_the_packing_of_the_f32_output(case):
    """The packed (hi, lo) store against the f32 store of the same values.  out_packed takes part in the dispatch (the weight-streaming
    kernel has no packed store), so the two runs can reach different leaves for their last rows, i.e. other summation orders: the rows that
    both plans give to the same leaf must match bit for bit, every live row's hi + lo must meet the class bound against float64."""
    from vicasplat_amd import ops
    cpu = build(case, "real")
    c = to_device(cpu, _dev())
    live = c.live[:, None].expand(c.out_rows, c.N)
    ref = gemm_f64(c)
    refmax = float(ref[live].abs().max())
    tol = bound("split", c.epi, c.K, refmax)
    buf32, got32 = _launch(c, ops, out_packed=False)
    bufp, gotp = _launch(c, ops)
    assert _outside_untouched(c, bufp), "the packed store wrote outside [mapped rows] x [0, N)"
    val = G.unpack_split(gotp)
    err = float((val - ref)[live].abs().max()) / refmax
    print(f"FIG {case.id} real split rel={err:.3e} bound={tol:.3e}")
    assert err <= tol, _where(c, val, ref, live)
    p32, rows32 = G.plan_info("split", c.M, c.N, c.K, c.epi, case.resid, False, False)
    same = c.M if G.leaves_of(p32) == G.leaves_of(c.plan) else (min(rows32, c.rows_main) if G.leaves_of(p32)[0] == G.leaves_of(c.plan)[0] else 0)
    assert same > 0 or c.M <= 64, (p32, c.plan)          # only the <= 64-row launches have no leaf in common
    clean = torch.where(live, got32, torch.zeros_like(got32)).contiguous()
    want = ops.split_pack_weight(clean, 0).data
    rows = G.map_rows(c.M, c.grp, _dev())[:same]
    assert torch.equal(gotp[rows], want[rows]), "packed output differs from packing the f32 output"
