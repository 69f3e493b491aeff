"""The float64 GEMM reference, the input families and the route plan of tests/gemm_f64.py, checked without a GPU:

  * on tiny shapes the reference equals a naive triple loop in Python floats (row maps, gate groups, every epilogue, RoPE);
  * the lattice family's preconditions hold for every lattice case of the table: integer operands with |.| <= 3, every sum below 2^24,
    the split packing of such a weight exact in hi with lo == 0, and float64 -> 16-bit of the (f32-exact) result one rounding;
  * every planted error of gemm_f64.MUTANTS moves the metric to >= 10x the bound asserted for the class on the real family, and breaks
    bit-equality on the lattice family;
  * every dispatcher leaf of a class is the plan() of at least one case of that class, and the route written in every case id is its plan().
"""
import math

import pytest
import torch

import gemm_f64 as G
from gemm_f64 import CASES, CLASSES, LEAVES, MUTANTS, build, gemm_f64, leaves_of, make_case, map_rows, plan, view2d


# ------------------------------------------------------------------------------------------------------------------------------------
# the reference against a naive loop
# ------------------------------------------------------------------------------------------------------------------------------------
def _naive(c):
    """{(output row, n): value} by loops over Python floats, straight from the header's contract."""
    A, W = view2d(c.A, c.A_spec).double().tolist(), view2d(c.W, c.W_spec).double().tolist()
    bias = None if c.bias is None else view2d(c.bias, c.bias_spec)[0].double().tolist()
    gate = None if c.gate is None else view2d(c.gate, c.gate_spec).double().tolist()
    out0 = view2d(c.out0, c.out_spec).double().tolist()
    res = None if c.resid is None else view2d(c.resid, c.resid_spec).double().tolist()

    def row(m, grp):
        return m if grp is None else (m // grp[0]) * grp[1] + grp[2] + m % grp[0]

    got = {}
    for m in range(c.M):
        ar, orow = row(m, c.a_grp), row(m, c.grp)
        z = []
        for n in range(c.N):
            s = 0.0
            for k in range(c.K):
                s += A[ar][k] * W[n][k]
            z.append(s + (bias[n] if bias is not None else 0.0))
        if c.epi == 1:
            z = [0.5 * v * (1.0 + math.erf(v / math.sqrt(2.0))) for v in z]
        elif c.epi == 2:
            src = res if res is not None else out0
            z = [src[orow][n] + (1.0 + (gate[m // c.gate_rows][n] if gate is not None else 0.0)) * z[n] for n in range(c.N)]
        elif c.epi == 5:
            zz = res[orow]
            z = [z[n] * (0.5 * (1.0 + math.erf(zz[n] / math.sqrt(2.0))) + zz[n] * math.exp(-0.5 * zz[n] ** 2) / math.sqrt(2.0 * math.pi))
                 for n in range(c.N)]
        elif c.epi == 4:
            p0, p1 = int(c.pos[orow, 0]), int(c.pos[orow, 1])
            kd = 0 if c.kind is None else int(c.kind[orow])
            r = list(z)
            for h in range(2 * c.rope_C // 64):
                b = h * 64
                if kd == 0:
                    for half, p in ((0, p0), (1, p1)):
                        for i in range(16):
                            ang = p * G.ROPE_BASE2D ** (-i / 16.0)
                            u, v = z[b + half * 32 + i], z[b + half * 32 + i + 16]
                            r[b + half * 32 + i], r[b + half * 32 + i + 16] = u * math.cos(ang) - v * math.sin(ang), v * math.cos(ang) + u * math.sin(ang)
                elif kd == 1:
                    for q in range(32):
                        ang = p0 * G.ROPE_THETA1D ** (-2.0 * q / 64.0)
                        u, v = z[b + 2 * q], z[b + 2 * q + 1]
                        r[b + 2 * q], r[b + 2 * q + 1] = u * math.cos(ang) - v * math.sin(ang), v * math.cos(ang) + u * math.sin(ang)
            z = r
        for n in range(c.N):
            got[(orow, n)] = z[n]
    return got


TINY = [("f16", 5, 19, 64, 0, {}), ("bf16", 5, 19, 64, 1, dict(grp=(2, 4, 1), a_grp=(3, 5, 2))),
        ("f32x", 7, 18, 32, 2, dict(gate_rows=3, grp=(2, 3, 1), a_grp=(2, 4, 1), gate_ld_odd=True, off_gate=1, off_out=1, ldo_odd=True)),
        ("split", 7, 18, 32, 2, dict(resid=True, gate_rows=2, off_resid=1, off_bias=1)), ("f16", 6, 17, 64, 3, dict(bias=False)),
        ("split", 23, 192, 32, 4, dict(rope_C=64, rope_far=True, grp=(5, 7, 2), a_grp=(4, 5, 1))), ("f16", 9, 128, 64, 4, dict(rope_C=64, rope_kinds=False)),
        ("split", 6, 20, 64, 5, dict(resid=True))]


@pytest.mark.parametrize("family", ["lattice", "real"])
@pytest.mark.parametrize("cls,M,N,K,epi,kw", TINY, ids=["%s-e%d-%dx%dx%d" % (t[0], t[4], t[1], t[2], t[3]) for t in TINY])
def test_reference_equals_a_naive_triple_loop(cls, M, N, K, epi, kw, family):
    c = make_case(cls, M, N, K, epi, family=family, seed=3, **kw)
    img = gemm_f64(c)
    want = _naive(c)
    out0 = view2d(c.out0, c.out_spec).double()
    scale = max(abs(v) for v in want.values())
    for r in range(c.out_rows):
        for n in range(N):
            if (r, n) in want:
                assert abs(float(img[r, n]) - want[(r, n)]) <= 1e-12 * scale, (r, n)
            else:
                assert float(img[r, n]) == float(out0[r, n]) == G.SENTINEL, (r, n)
    assert set(r for r, _ in want) == set(torch.nonzero(c.live).flatten().tolist())


def test_make_case_guards_every_buffer():
    """NaN in the padding columns of A and W and in every A row outside the input map; the sentinel in every output element outside
    [mapped rows] x [0, N); the offsets and strides asked for."""
    c = make_case("split", 75, 83, 64, 2, family="real", resid=True, grp=(37, 40, 2), a_grp=(37, 39, 1), gate_rows=16, gate_ld_odd=True,
                  ldo_odd=True, off_out=1, off_resid=1, off_gate=1, off_bias=1)
    A = view2d(c.A, c.A_spec)
    arow = map_rows(c.M, c.a_grp)
    assert bool(torch.isfinite(A[arow, :c.K]).all()) and bool(torch.isnan(A[:, c.K:]).all())
    dead = torch.ones(A.shape[0], dtype=torch.bool)
    dead[arow] = False
    assert int(dead.sum()) >= 3 and bool(torch.isnan(A[dead]).all())
    W = view2d(c.W, c.W_spec)
    assert bool(torch.isfinite(W[:, :c.K]).all()) and bool(torch.isnan(W[:, c.K:]).all())
    assert c.ldo % 4 != 0 and c.gate_spec[3] % 4 != 0 and c.out_spec[0] == c.resid_spec[0] == c.gate_spec[0] == c.bias_spec[0] == 1
    assert bool((c.out0 == G.SENTINEL).all()) and int((~c.live).sum()) >= 3
    assert c.lda > c.K and c.ldw > c.K and c.ldo > c.N and c.lda % 8 == 0


# ------------------------------------------------------------------------------------------------------------------------------------
# lattice preconditions
# ------------------------------------------------------------------------------------------------------------------------------------
LATTICE_CASES = [c for c in CASES if "lattice" in c.families]
CPU_WORK = 1 << 27        # M N K up to which the float64 reference of a case is also evaluated here


@pytest.mark.parametrize("case", LATTICE_CASES, ids=[c.id for c in LATTICE_CASES])
def test_lattice_preconditions(case):
    from vicasplat_amd import ops
    c = build(case, "lattice")
    K = c.K
    a = view2d(c.A, c.A_spec)[map_rows(c.M, c.a_grp), :K].float()
    w = view2d(c.W, c.W_spec)[:, :K].float()
    for t in (a, w):
        assert bool((t == t.round()).all()) and float(t.abs().max()) <= G.LAT_AW
    # every partial sum is an integer of magnitude <= 9 K; with bias, the gate factor (multiples of 1/2, at most 2) and the residual the
    # result is a multiple of 1/2 below 2^24 / 2 as well: exact in f32 in any order
    top = 2 * (G.LAT_AW ** 2 * K + G.LAT_BIAS) + G.LAT_RESID
    assert G.LAT_AW ** 2 * K < 2 ** 24 and 2 * top < 2 ** 24
    if c.bias is not None:
        b = view2d(c.bias, c.bias_spec)
        assert bool((b == b.round()).all()) and float(b.abs().max()) <= G.LAT_BIAS
    if c.gate is not None:
        gt = view2d(c.gate, c.gate_spec)
        assert bool(((2 * gt) == (2 * gt).round()).all()) and float(gt.min()) >= -0.5 and float(gt.max()) <= 1.0
    if c.cls == "split":      # the packing of a lattice weight: hi exact, lo == 0 (activations: scale 2^0, the same argument)
        e = ops.split_scale_exp(w)
        assert e == c.scale_exp
        ws = w * 2.0 ** e
        assert torch.equal(ws.half().float(), ws) and torch.equal(a.half().float(), a)
    if case.M * case.N * case.K <= CPU_WORK:
        img = gemm_f64(c)
        live = img[c.live]
        assert float(live.abs().max()) <= top and bool(((2 * live) == (2 * live).round()).all())
        assert torch.equal(live.float().double(), live)                                  # f32-exact ...
        if c.odt != torch.float32:
            assert torch.equal(live.to(c.odt), live.float().to(c.odt))                   # ... so float64 -> 16-bit is one rounding


# ------------------------------------------------------------------------------------------------------------------------------------
# mutants
# ------------------------------------------------------------------------------------------------------------------------------------
MUTANT_CASES = [
    ("f16", 100, 83, 256, 0, dict(grp=(37, 40, 2), a_grp=(37, 39, 1))),
    ("bf16", 100, 83, 256, 2, dict(gate_rows=17, grp=(37, 40, 2), a_grp=(37, 39, 1))),
    ("f32x", 70, 144, 128, 1, dict(grp=(1, 4, 2), a_grp=(1, 3, 1))),
    ("split", 100, 83, 128, 2, dict(resid=True, gate_rows=16)),
    ("split", 100, 83, 128, 3, dict(grp=(37, 40, 2), a_grp=(37, 39, 1))),
    ("f16", 129, 128, 8192, 2, dict(gate_rows=64)),                       # skinny(ks=4): bias_every_slice
    ("split", 300, 128, 2048, 2, dict(gate_rows=65)),
    ("f16", 75, 192, 64, 4, dict(rope_C=64, grp=(37, 40, 2), a_grp=(37, 39, 1))),
    ("bf16", 75, 192, 64, 4, dict(rope_C=64, grp=(37, 40, 2), a_grp=(37, 39, 1))),
    ("split", 75, 384, 64, 4, dict(rope_C=128, grp=(37, 40, 2), a_grp=(37, 39, 1))),
    ("f32x", 75, 192, 64, 4, dict(rope_C=64, grp=(37, 40, 2), a_grp=(37, 39, 1))),
    ("split", 80, 96, 128, 5, dict(resid=True)),
]
MUTANT_IDS = ["%s-e%d-%dx%dx%d" % (t[0], t[4], t[1], t[2], t[3]) for t in MUTANT_CASES]


def _live_rel(c, img, ref):
    """The metric of tests/test_gemm_routes_gpu.py: max |error| over max |reference| on the reference's live elements; an element that
    the mutant did not write at all (or wrote elsewhere) counts with its full size."""
    live = c.live[:, None].expand_as(ref)
    d = torch.nan_to_num((img - ref).abs()[live], nan=float("inf"))        # a NaN read from a guard row is as wrong as it gets
    return float(d.max() / ref[live].abs().max())


@pytest.mark.parametrize("cls,M,N,K,epi,kw", MUTANT_CASES, ids=MUTANT_IDS)
def test_every_mutant_is_rejected_tenfold_on_the_real_family(cls, M, N, K, epi, kw):
    c = make_case(cls, M, N, K, epi, family="real", seed=1, **kw)
    ref = gemm_f64(c)
    tol = G.bound(cls, epi, K, float(ref[c.live].abs().max()))
    for mu in MUTANTS:
        if not G.mutant_applies(c, mu):
            continue
        e = _live_rel(c, gemm_f64(c, mutant=mu), ref)
        assert e >= 10 * tol, (mu, e, tol)


@pytest.mark.parametrize("cls,M,N,K,epi,kw", [t for t in MUTANT_CASES if t[4] in (0, 2, 3)], ids=[i for i, t in zip(MUTANT_IDS, MUTANT_CASES) if t[4] in (0, 2, 3)])
def test_every_mutant_breaks_bit_equality_on_the_lattice_family(cls, M, N, K, epi, kw):
    c = make_case(cls, M, N, K, epi, family="lattice", seed=1, **kw)
    ref = gemm_f64(c)
    for mu in MUTANTS:
        if not G.mutant_applies(c, mu):
            continue
        img = gemm_f64(c, mutant=mu)
        assert not torch.equal(img.to(c.odt), ref.to(c.odt)), mu


def test_mutants_cover_the_list():
    """Every mutant applies to at least one case of MUTANT_CASES."""
    applies = set()
    for cls, M, N, K, epi, kw in MUTANT_CASES:
        c = make_case(cls, M, N, K, epi, family="real", seed=1, **kw)
        applies |= {mu for mu in MUTANTS if G.mutant_applies(c, mu)}
    assert applies == set(MUTANTS), set(MUTANTS) - applies


# ------------------------------------------------------------------------------------------------------------------------------------
# routes
# ------------------------------------------------------------------------------------------------------------------------------------
def test_route_in_every_case_id_is_its_plan():
    for c in CASES:
        p = plan(c.cls, c.M, c.N, c.K, c.epi, c.resid, c.kw.get("a_packed", False), c.kw.get("out_packed", False))
        assert "+".join(leaves_of(p)) == c.route and c.id.startswith(c.route + "-" + c.cls + "-"), (c.id, p)


@pytest.mark.parametrize("cls", CLASSES)
def test_every_leaf_of_a_class_is_the_plan_of_a_case(cls):
    seen = set()
    for c in CASES:
        if c.cls == cls:
            seen.update(leaves_of(plan(c.cls, c.M, c.N, c.K, c.epi, c.resid, c.kw.get("a_packed", False), c.kw.get("out_packed", False))))
    assert seen == set(LEAVES[cls]), (set(LEAVES[cls]) - seen, seen - set(LEAVES[cls]))


def test_plan_examples_from_the_dispatcher_comments():
    """Shapes whose route the comments of csrc/routes.h spell out."""
    assert plan("f16", 2056, 4096, 1024, 0) == "mi8(rows=2048)+tail:smallm<NW8,MF1>"         # "peeling the 8 leftover rows makes it one"
    assert plan("split", 2056, 1024, 1024, 2) == "mi2(rows=2056)"                            # "64-row tiles ... double the workgroups"
    assert plan("f16", 16684, 1024, 512, 2) == "g256(rows=16384)+tail:mi4(ks=2)"
    assert plan("f16", 16684, 1024, 512, 2, resid=True) == "g256(rows=16384)+tail:mi4(ks=1)"
    assert plan("f32x", 65, 64, 64, 0) == "g256(rows=65)" and plan("f32x", 64, 64, 64, 4) == "g256(rows=64)"
    assert plan("split", 40, 128, 64, 0, a_packed=True) == "smallm<NW8,MF4>"                 # a packed A with M <= 64 goes to the weight-streaming kernel
    assert plan("f16", 40, 128, 64, 4) == "skinny(ks=1)" and plan("split", 40, 128, 64, 0, out_packed=True) == "skinny(ks=1)"
