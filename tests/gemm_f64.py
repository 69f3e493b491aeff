"""Float64 restatement of the forward GEMM entry points (include/vicasplat_hip.h: vs_gemm_bias_act, vs_gemm_resid, vs_gemm_qkv_rope,
vs_gemm_split, vs_gemm_split_packed), the guarded input generator and the route plan shared by tests/test_gemm_ref_cpu.py and
tests/test_gemm_routes_gpu.py.

  * `gemm_f64`   -- plain torch, float64, from the stored values (the f16 / bf16 / f32 tensors as the kernel sees them):
    A[arow(m)] @ W^T (+ bias) and the epilogue, written into a copy of the initial output buffer at row(m).  It returns the whole
    [out_rows, ldo] image, so "nothing outside [mapped rows] x [0, N) was written" is part of the comparison.  `mutant=` plants one
    error (MUTANTS) for the tests of the tests; leave it None.
  * `make_case`  -- one seeded input set in guarded buffers: lda, ldw > K with NaN padding columns, NaN in every A row outside the input
    row map, ldo > N and spare output rows pre-filled with a sentinel, optional odd strides and pointers offset by one element.  Every view
    lies inside one allocation, so nothing is ever out of bounds.
  * `plan`       -- a line-by-line transcription of the dispatcher, csrc/routes.h (gemm_plan, tail_step, skinny_step, smallm_step): the
    kernels a call reaches, e.g. "g256(rows=16384)+tail:mi4(ks=2)".  tests/test_routes_cpu.py compiles routes.h for the host and compares
    the two string for string; the GPU tests name their routes from this copy, since there may be no compiler where they run.
  * `CASES`      -- the table of tests/test_gemm_routes_gpu.py; the first part of every id is the route written down by hand, which
    tests/test_gemm_ref_cpu.py compares with plan().

Two input families.  "lattice": A, W integers in [-3, 3], bias / resid small integers, gate in {-0.5, 0, 0.5, 1}: every partial sum is an
integer of magnitude <= 9 K < 2^24 (times the power of two of the split packing), so f32 accumulation is exact in any order, through f32
atomics too, and the epilogues 0 / 2 / 3 must reproduce the float64 result bit for bit.  "real": the asymmetric random operands of
tests/test_ops_gpu.py (a transposed write or swapped operand does not survive them), with one 32-wide k block raised so that losing it
shows; only this family exercises the lo terms of the split class, the accumulation error, GELU / GELU' and RoPE.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch

SENTINEL = -1024.0           # exactly representable in f16 and bf16
SENTINEL_PACKED = 0x12345678
STORAGE = {"f16": torch.float16, "bf16": torch.bfloat16, "f32x": torch.float32, "split": torch.float32}
CLASSES = ("f16", "bf16", "f32x", "split")
ROPE_BASE2D, ROPE_THETA1D = 100.0, 30.0
ROPE_POS = (0, 63, 64, 1000)  # the 64-entry (sin, cos) table of the epilogue: its last entry, the first fallback position, a far one (rope_far)
LAT_AW, LAT_BIAS, LAT_RESID = 3, 8, 16
LAT_GATE = (-0.5, 0.0, 0.5, 1.0)


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------------------------------
# route plan: csrc/routes.h, the function transcribed (VS_DETERMINISTIC unset)
# ------------------------------------------------------------------------------------------------------------------------------------
def _smallm(rows, K2):                                            # smallm_step
    one, deep = rows <= 16, K2 // 32 >= 64
    return "smallm<NW%d,MF%d>" % (16 if deep else 8, 1 if one else 4)


def _skinny(rows, N, K2, epi, resid):                             # skinny_step
    gy, gx = cdiv(rows, 64), cdiv(N, 64)
    ks = 1
    if epi == 2 and not resid:
        while ks < 8 and gx * gy * ks * 2 <= 384 and K2 // 64 // (ks * 2) >= 32:
            ks *= 2
    return "skinny(ks=%d)" % ks


def _tail(sp, rem, N, K2, epi, resid, ap, op):                    # tail_step
    ks = 1
    if epi == 2 and rem > 64 and not resid:
        tiles = cdiv(rem, 128) * cdiv(N, 128)
        while ks < 8 and (K2 // 32) % (ks * 2) == 0 and K2 // 32 // (ks * 2) >= 8 and tiles * ks * 2 <= 512:
            ks *= 2
    if rem <= 256 and K2 % 64 == 0 and (rem > 64 or epi in (4, 5) or op) and (sp or (not ap and not op)):     # skinny_takes and ...
        return "tail:" + _skinny(rem, N, K2, epi, resid)
    if rem <= 64 and epi not in (4, 5) and not op and (sp or not ap):   # smallm_takes
        return "tail:" + _smallm(rem, K2)
    return "tail:mi4(ks=%d)" % ks


def plan_info(cls, M, N, K, epi, resid=False, a_packed=False, out_packed=False):
    """-> (plan string, rows of the main launch).  K as given to the ABI; it doubles for the f32 and split classes (gemm_entry,
    gemm.hip: f32 rows are addressed in 2-byte units)."""
    assert cls in CLASSES
    K2 = 2 * K if cls in ("f32x", "split") else K
    ap, op = a_packed, out_packed
    if cls == "f32x":                                             # gemm_plan, the f32 class: no tail
        if M <= 64 and epi != 4:
            return _smallm(M, K2), M
        return ("g256(rows=%d)" % M if K2 % 128 == 0 else "mi4(rows=%d)" % M), M
    sp = cls == "split"
    if M <= 64 and epi not in (4, 5) and not op and (sp or not ap):   # gemm_plan: smallm_takes
        return _smallm(M, K2), M
    if M <= 256 and K2 % 64 == 0 and (sp or (not ap and not op)):     # skinny_takes
        return _skinny(M, N, K2, epi, resid), M
    if K2 % 128 == 0 and M >= 256:                                # whole rounds of 256 x 256 tiles + a tail
        tn, mt = cdiv(N, 256), M // 256
        full, rounds_all = mt * tn, (cdiv(M, 256) * tn + 255) // 256
        mt_main = mt
        if full > 256 and full % 256 != 0:
            mt_main = (full // 256) * 256 // tn
        rows_main = mt_main * 256
        rem = M - rows_main
        tiles4 = cdiv(rem, 128) * cdiv(N, 128)
        cost_split = float((mt_main * tn + 255) // 256) + (0.31 * float((tiles4 + 767) // 768) if rem > 0 else 0.0)
        tiles_one = cdiv(M, 256) * tn
        nearly_full = tiles_one * 100 >= rounds_all * 256 * 95
        split = (not nearly_full) and rem > 0 and mt_main > 0 and cost_split < float(rounds_all) - 0.05
        if split or tiles_one * 100 >= rounds_all * 256 * 70:
            if not split:
                return "g256(rows=%d)" % M, M
            return "g256(rows=%d)+%s" % (rows_main, _tail(sp, rem, N, K2, epi, resid, ap, op)), rows_main
    tiles_n = cdiv(N, 128)                                        # 256 x 128 or 128 x 128 tiles, a tail of <= half a tile peeled
    t8 = cdiv(M, 256) * tiles_n
    mi = 8 if t8 >= 256 else 4
    bm, slots = 32 * mi, 256 * (2 if mi == 8 else 3)
    rem = M % bm
    full = (M // bm) * tiles_n
    split = full > 0 and 0 < rem <= bm // 2 and ((full + tiles_n + slots - 1) // slots > (full + slots - 1) // slots or
                                                 (full + tiles_n + 255) // 256 > (full + 255) // 256)
    m_main = M - rem if split else M
    tail = "+" + _tail(sp, rem, N, K2, epi, resid, ap, op) if split else ""
    if sp:                                                        # 64-row tiles for small residual-epilogue GEMMs
        tiles4 = cdiv(m_main, 128) * tiles_n
        if mi == 4 and epi == 2 and tiles4 <= 192 and m_main > 64:
            return "mi2(rows=%d)%s" % (m_main, tail), m_main
    return "mi%d(rows=%d)%s" % (mi, m_main, tail), m_main


def plan(cls, M, N, K, epi, resid=False, a_packed=False, out_packed=False) -> str:
    return plan_info(cls, M, N, K, epi, resid, a_packed, out_packed)[0]


def leaves_of(p: str):
    """Leaf names of a plan string: the row counts dropped, e.g. "g256(rows=16384)+tail:mi4(ks=2)" -> ["g256", "tail:mi4(ks=2)"]."""
    out = []
    for part in p.split("+"):
        i = part.find("(rows=")
        out.append(part if i < 0 else part[:i])
    return out


def plan_ksplit(p: str) -> int:
    """Number of K slices whose partial sums meet in `out` through atomics on some launch of the plan (1: none)."""
    ks = 1
    for part in p.split("+"):
        i = part.find("(ks=")
        if i >= 0:
            ks = max(ks, int(part[i + 4:part.index(")", i)]))
    return ks


# Every leaf the dispatcher has for a class; tests/test_gemm_ref_cpu.py asserts that each is the plan of at least one case of that class.
_SMALLM = ["smallm<NW8,MF1>", "smallm<NW16,MF1>", "smallm<NW8,MF4>", "smallm<NW16,MF4>"]
_TILE16 = _SMALLM + ["skinny(ks=1)", "skinny(ks=2)", "skinny(ks=4)", "g256", "mi8", "mi4", "tail:smallm<NW8,MF1>", "tail:smallm<NW8,MF4>",
                     "tail:skinny(ks=1)", "tail:mi4(ks=1)", "tail:mi4(ks=2)"]
LEAVES = {"f16": _TILE16, "bf16": _TILE16, "split": _TILE16 + ["mi2"], "f32x": _SMALLM + ["g256", "mi4"]}


# ------------------------------------------------------------------------------------------------------------------------------------
# row maps, views
# ------------------------------------------------------------------------------------------------------------------------------------
def map_rows(M, grp, device=None, shift=0):
    """row(m) = (m // grp_in) * grp_out + grp_off + m % grp_in for m < M (grp None: identity).  shift: the group index is taken from
    m + shift (a planted off-by-one at the group boundaries)."""
    m = torch.arange(M, device=device)
    if grp is None:
        return m
    gi, go, off = grp
    return ((m + shift) // gi) * go + off + m % gi


def view2d(buf, spec):
    """The [rows, cols] view (row stride ld, first element at off) of a flat buffer: spec = (off, rows, cols, ld)."""
    off, rows, cols, ld = spec
    return torch.as_strided(buf, (rows, cols), (ld, 1), off)


def _gelu(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def _dgelu(z):
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def rope_f64(x, pos, kind, C, partner_shift=0):
    """x [M, N] float64, pos [M, 2], kind [M] (None: all 2-D) -> q | k columns [0, 2C) rotated per head of 64, the rest untouched.
    kind 0: 2-D, pairs (i, i + 16) of each 32, first 32 by pos[:, 0], second by pos[:, 1], frequency base^(-i / 16); kind 1: 1-D, pairs
    (2p, 2p + 1), pos[:, 0], frequency theta^(-2p / 64); kind 2: none.  partner_shift: the planted wrong partner column."""
    M = x.shape[0]
    out = x.clone()
    h = x[:, :2 * C].reshape(M, -1, 64)
    p = pos.double()
    inv2 = ROPE_BASE2D ** (-torch.arange(16, dtype=torch.float64, device=x.device) / 16)
    r2 = h.clone()
    for half in range(2):
        ang = p[:, half, None, None] * inv2
        c, s = ang.cos(), ang.sin()
        iu = torch.arange(half * 32, half * 32 + 16, device=x.device)
        iv = (iu + 16 + partner_shift) % 64
        u, v = h[..., iu], h[..., iv]
        r2[..., iu] = u * c - v * s
        r2[..., iu + 16] = v * c + u * s
    inv1 = ROPE_THETA1D ** (-torch.arange(0, 64, 2, dtype=torch.float64, device=x.device) / 64)
    ang = p[:, 0, None, None] * inv1
    c, s = ang.cos(), ang.sin()
    r1 = h.clone()
    u, v = h[..., 0::2], h[..., 1::2]
    r1[..., 0::2] = u * c - v * s
    r1[..., 1::2] = v * c + u * s
    k = torch.zeros(M, dtype=torch.long, device=x.device) if kind is None else kind.long()
    sel = torch.where((k == 1)[:, None, None], r1, torch.where((k == 2)[:, None, None], h, r2))
    out[:, :2 * C] = sel.reshape(M, 2 * C)
    return out


MUTANTS = ("kblock_dropped", "kblock_twice", "rows_swapped_16", "gate_next_group", "out_map_off_by_one", "a_map_off_by_one", "bias_off_16",
           "rope_partner_off_16", "pos_by_input_row", "bias_every_slice", "lo_dropped")


def mutant_applies(c, mutant) -> bool:
    """Whether the planted error exists for the case (a gate error needs a gate with two groups, ...).  lo_dropped is a real-family
    mutant: lattice operands have lo == 0 by construction (asserted in tests/test_gemm_ref_cpu.py)."""
    return {"kblock_dropped": True, "kblock_twice": True,
            "rows_swapped_16": c.M > 16,
            "gate_next_group": c.epi == 2 and c.gate is not None and cdiv(c.M, c.gate_rows) > 1,
            "out_map_off_by_one": c.grp is not None and c.M > c.grp[0],
            "a_map_off_by_one": c.a_grp is not None and c.M > c.a_grp[0],
            "bias_off_16": c.bias is not None and c.N > 16,
            "rope_partner_off_16": c.epi == 4,
            "pos_by_input_row": c.epi == 4 and c.grp is not None,
            "bias_every_slice": c.bias is not None and c.epi == 2 and plan_ksplit(c.plan) > 1,
            "lo_dropped": c.cls == "split" and c.family == "real"}[mutant]


def gemm_f64(c, mutant=None, device=None):
    """The float64 image of the whole output buffer, [out_rows, ldo_cols] (= the initial buffer with the live elements replaced), on
    `device` (default: where the case's tensors are).  For a packed output the image is the f32 result the packing is taken of, with NaN
    where nothing is written."""
    dev = c.A.device if device is None else device
    M, N, K = c.M, c.N, c.K
    A = view2d(c.A, c.A_spec).to(dev).double()
    W = view2d(c.W, c.W_spec).to(dev).double()[:, :K]
    if mutant == "lo_dropped":
        A, W = A.float().half().double(), (W * 2.0 ** c.scale_exp).float().half().double() * 2.0 ** -c.scale_exp
    arow = map_rows(M, c.a_grp, dev, shift=1 if mutant == "a_map_off_by_one" else 0)
    Am = A[arow.clamp(max=A.shape[0] - 1)][:, :K]          # (the clamp only ever acts on a mutant's map)
    kb = c.probe_kblock
    if mutant == "kblock_dropped":
        Am = Am.clone()
        Am[:, kb * 32:(kb + 1) * 32] = 0.0
    acc = Am @ W.t()
    if mutant == "kblock_twice":
        acc = acc + Am[:, kb * 32:(kb + 1) * 32] @ W[:, kb * 32:(kb + 1) * 32].t()
    if mutant == "rows_swapped_16":
        m0 = ((M - 17) // 32) * 32 if M >= 32 else 0              # a 16-row fragment and the next, inside the last whole 32 rows
        n16 = min(16, M - m0 - 16)
        acc = acc.clone()
        acc[m0:m0 + n16], acc[m0 + 16:m0 + 16 + n16] = acc[m0 + 16:m0 + 16 + n16].clone(), acc[m0:m0 + n16].clone()
    z = acc
    if c.bias is not None:
        b = view2d(c.bias, c.bias_spec).to(dev).double()[0]
        if mutant == "bias_off_16":
            b = b[(torch.arange(N, device=dev) + 16) % N]
        z = acc + b * (plan_ksplit(c.plan) if mutant == "bias_every_slice" else 1)
    orow = map_rows(M, c.grp, dev, shift=1 if mutant == "out_map_off_by_one" else 0)
    out0 = view2d(c.out0, c.out_spec).to(dev)
    inside = orow < out0.shape[0]                              # (false only for a mutant's map)
    orow = orow.clamp(max=out0.shape[0] - 1)
    img = torch.full(out0.shape, float("nan"), dtype=torch.float64, device=dev) if c.out_packed else out0.double().clone()
    epi = c.epi
    if epi in (0, 3):
        val = z
    elif epi == 1:
        val = _gelu(z)
    elif epi == 2:
        src = view2d(c.resid, c.resid_spec).to(dev).double() if c.resid is not None else out0.double()
        if c.gate is not None:
            g = view2d(c.gate, c.gate_spec).to(dev).double()
            gi = torch.arange(M, device=dev) // c.gate_rows
            if mutant == "gate_next_group":
                gi = (gi + 1) % cdiv(M, c.gate_rows)
            z = (1.0 + g[gi]) * z
        val = src[orow] + z
    elif epi == 4:
        pos, kind = c.pos.to(dev), (None if c.kind is None else c.kind.to(dev))
        prow = arow.clamp(max=pos.shape[0] - 1) if mutant == "pos_by_input_row" else orow
        val = rope_f64(z, pos[prow], None if kind is None else kind[prow], c.rope_C, 16 if mutant == "rope_partner_off_16" else 0)
    elif epi == 5:
        val = z * _dgelu(view2d(c.resid, c.resid_spec).to(dev).double()[orow])
    else:
        raise ValueError(epi)
    img[orow[inside]] = val[inside]
    return img


# ------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------------
def _flat(n, fill, dtype):
    return torch.full((n,), fill, dtype=dtype)


def make_case(cls, M, N, K, epi, *, family="real", resid=False, a_packed=False, out_packed=False, grp=None, a_grp=None, gate=None,
              gate_rows=0, gate_ld_odd=False, ldo_odd=False, off_out=0, off_resid=0, off_gate=0, off_bias=0, bias=True, rope_C=0,
              rope_kinds=True, rope_far=False, w_amax=0.0, contiguous_out=False, seed=0):
    """One input set (CPU tensors; `to_device` moves it).  K as given to the ABI.  grp / a_grp: (grp_in, grp_out, grp_off) or None.
    gate: None = "epilogue 2 has one" (False: none); gate_rows 0 = one group.  contiguous_out: out (and resid) are plain [M, N] tensors
    (what ops.gemm_resid takes; off_resid still applies).  Returns a namespace of flat buffers and (off, rows, cols, ld) view specs:
    A (every column, lda wide: NaN beyond K and in rows outside the input map), W, bias, gate, resid, out0 (the initial output buffer),
    pos / kind per OUTPUT row, plus the call's scalars, `plan`, `rows_main` and `live` (bool [out_rows], rows inside the output map)."""
    assert family in ("lattice", "real") and cls in CLASSES
    dt = STORAGE[cls]
    g = torch.Generator().manual_seed(seed * 7919 + M * 31 + N * 17 + K + epi)
    lattice = family == "lattice"
    if epi == 5:
        assert cls == "split" and resid and grp is None
        bias, gate = False, False
    if gate is None:
        gate = epi == 2
    odt = dt if epi in (0, 1, 4) else torch.float32
    lda = ldw = K + 32
    arow = map_rows(M, a_grp)
    a_rows = int(arow.max()) + 4
    p, rows_main = plan_info(cls, M, N, K, epi, resid, a_packed, out_packed)
    nkb = K // 32
    probe_kblock = nkb // 2 if nkb > 1 else 0

    def rnd(shape, scale=1.0):
        return torch.randn(shape, generator=g) * scale

    def ints(shape, lim):
        return torch.randint(-lim, lim + 1, shape, generator=g).float()

    if lattice:
        a, w = ints((M, K), LAT_AW), ints((N, K), LAT_AW)
    else:
        a = rnd((M, K), 0.1 if epi == 5 else 1.0) + 0.1 * torch.arange(K).float() / K
        w = rnd((N, K)) / math.sqrt(K) + 0.05 * torch.arange(N).float()[:, None] / N
        if nkb > 2:                # one 32-wide block carries as much as the rest of K together: a kernel that loses or repeats it is far off
            a[:, probe_kblock * 32:(probe_kblock + 1) * 32] *= math.sqrt(nkb)
        if w_amax:                 # the largest weight put at w_amax (the split packing's scale_exp is a function of it)
            w = w * (w_amax / float(w.abs().max()))
    A = _flat(a_rows * lda, float("nan"), dt)
    Av = view2d(A, (0, a_rows, lda, lda))
    Av[arow, :K] = a.to(dt)
    Wb = _flat((N + 1) * ldw, float("nan"), dt)
    view2d(Wb, (0, N, ldw, ldw))[:, :K] = w.to(dt)
    c = SimpleNamespace(cls=cls, M=M, N=N, K=K, epi=epi, family=family, a_packed=a_packed, out_packed=out_packed, grp=grp, a_grp=a_grp,
                        plan=p, rows_main=rows_main, probe_kblock=probe_kblock, rope_C=rope_C, contiguous_out=contiguous_out,
                        A=A, A_spec=(0, a_rows, lda, lda), W=Wb, W_spec=(0, N, ldw, ldw), lda=lda, ldw=ldw, dt=dt, odt=odt)
    wl = view2d(Wb, c.W_spec)[:, :K].float()
    amax = float(wl.abs().max())
    c.scale_exp = max(-24, min(24, 13 - math.frexp(amax)[1] + 1)) if amax != 0.0 and math.isfinite(amax) else 0   # = ops.split_scale_exp
    # bias
    c.bias = None
    if bias:
        c.bias = _flat(off_bias + N + 3, float("nan"), torch.float32)
        c.bias_spec = (off_bias, 1, N, N)
        view2d(c.bias, c.bias_spec)[0] = ints((N,), LAT_BIAS) if lattice else rnd((N,))
    # output buffer, residual
    orow = map_rows(M, grp)
    if contiguous_out:
        assert grp is None and not out_packed and off_out == 0
        out_rows, ldo = M, N
    else:
        out_rows = int(orow.max()) + 4
        ldo = N + 32 if out_packed else (cdiv(N, 4) * 4 + (5 if ldo_odd else 4))
    c.out_rows, c.ldo = out_rows, ldo
    c.out_spec = (off_out, out_rows, N, ldo)
    c.live = torch.zeros(out_rows, dtype=torch.bool)
    c.live[orow] = True
    if out_packed:
        assert cls == "split" and N % 64 == 0 and off_out == 0 and epi in (0, 1, 3, 4)
        c.out0 = _flat(out_rows * ldo, SENTINEL, torch.float32)          # the float image; the device buffer is int32 SENTINEL_PACKED
    else:
        c.out0 = _flat(off_out + out_rows * ldo + 3, SENTINEL, odt)
    r = (ints((M, N), LAT_RESID) if lattice else rnd((M, N), 1.5 if epi == 5 else 1.0)) if epi in (2, 5) else None
    c.resid = None
    if epi in (2, 5) and resid:
        c.resid = _flat(off_resid + out_rows * ldo + 3, float("nan"), torch.float32)
        c.resid_spec = (off_resid, out_rows, N, ldo)
        view2d(c.resid, c.resid_spec)[orow] = r
    elif epi == 2:
        view2d(c.out0, c.out_spec)[orow] = r
    # gate
    c.gate, c.gate_rows = None, (gate_rows if gate_rows > 0 else M)
    if gate:
        G = cdiv(M, c.gate_rows)
        gld = cdiv(N, 4) * 4 + (5 if gate_ld_odd else 4)
        c.gate = _flat(off_gate + (G + 1) * gld + 3, float("nan"), torch.float32)
        c.gate_spec = (off_gate, G, N, gld)
        view2d(c.gate, c.gate_spec)[:] = (torch.tensor(LAT_GATE)[torch.randint(0, 4, (G, N), generator=g)] if lattice else rnd((G, N), 0.5))
    # RoPE: per OUTPUT row; the table edge and fallback positions and the three kinds are dealt so that every 16-row fragment mixes them
    c.pos = c.kind = None
    if epi == 4:
        assert rope_C > 0 and rope_C % 64 == 0 and N >= 2 * rope_C and N % 64 == 0
        pos = torch.randint(0, 17, (out_rows, 2), generator=g).int()
        rr = torch.arange(out_rows)
        for j, pv in enumerate(ROPE_POS if rope_far else ROPE_POS[:3]):      # (the far position: cases of their own, see CASES)
            pos[rr % 7 == j, 0] = pv
            pos[rr % 5 == j, 1] = pv
        c.pos = pos.contiguous()
        if rope_kinds:
            kind = torch.zeros(out_rows, dtype=torch.uint8)
            kind[rr % 6 == 1] = 1
            kind[rr % 11 == 3] = 2
            c.kind = kind
    return c


TENSORS = ("A", "W", "bias", "gate", "resid", "out0", "pos", "kind", "live")


def to_device(c, device):
    d = SimpleNamespace(**vars(c))
    for k in TENSORS:
        t = getattr(c, k)
        setattr(d, k, None if t is None else t.to(device))
    return d


def unpack_split(data):
    """int32 [rows, N] packed (hi, lo) image (vs_split_pack_weight, scale 2^0) -> float64 hi + lo.  Per block of 32 k: 32 halves hi, then 32
    halves lo; inside a block chunk g (8 halves) holds k = {4g .. 4g+3, 16+4g .. 16+4g+3}."""
    rows, N = data.shape
    h = data.contiguous().view(torch.float16).reshape(rows, 2 * N)
    k = torch.arange(N, device=data.device)
    kk = k % 32
    hi = (k // 32) * 64 + ((kk % 16) // 4) * 8 + (kk >= 16).long() * 4 + kk % 4
    return h[:, hi].double() + h[:, hi + 32].double()


def bound(cls, epi, K, refmax):
    """The relative bound (max |error| over max |reference|, live elements) per class and epilogue: the bounds of test_gemm_epilogues
    (tests/test_ops_gpu.py: 2e-3 / 1.2e-2; epilogue 3: 2e-5 max|ref| + 1e-6 K; epilogue 2: 1e-4 max|ref| + 2e-5 sqrt K),
    test_gemm_qkv_rope_fused (3e-3 / 1.6e-2), tests/test_split_path_gpu.py (6e-6; RoPE 2e-5), tests/test_f32_path_gpu.py (4e-6; RoPE 2e-5)
    and test_linear_backward_split_with_gelu_derivative_in_the_epilogue (tests/test_split_bwd_gpu.py: 3e-6)."""
    if cls in ("f16", "bf16"):
        if epi == 3:
            return 2e-5 + 1e-6 * K / refmax
        if epi == 2:
            return 1e-4 + 2e-5 * math.sqrt(K) / refmax
        if epi == 4:
            return 3e-3 if cls == "f16" else 1.6e-2
        return 2e-3 if cls == "f16" else 1.2e-2
    if epi == 4:
        return 2e-5
    if cls == "split":
        return 3e-6 if epi == 5 else 6e-6
    return 4e-6




# ------------------------------------------------------------------------------------------------------------------------------------
# the table of tests/test_gemm_routes_gpu.py
# ------------------------------------------------------------------------------------------------------------------------------------
B16 = ("f16", "bf16")
TILE = B16 + ("split",)           # the classes that share launch()
EP = (0, 1, 2, "2r", 3)           # "2r": epilogue 2 with the residual in a second buffer
MI_OF = {"smallm": 16, "skinny": 16, "mi2": 32, "mi4": 64, "mi8": 128, "g256": 128}   # rows of a wave tile = 16 * MI of the fast epilogue


def _kfor(cls, K, Ksplit=None, Kf32=None):
    return Ksplit if (cls == "split" and Ksplit) else Kf32 if (cls == "f32x" and Kf32) else K


def _cases():
    """Every case: id = "<route>-<cls>-<M>x<N>x<K>-e<epi>[r][-tag]".  route is written by hand (leaf names, no row counts) -- a string, or a
    dict {epilogue key or class or (class, epilogue key): route, "*": default} where the dispatcher tells them apart."""
    cs = []

    def route_of(route, cls, ekey):
        if isinstance(route, dict):
            for k in ((cls, ekey), ekey, cls, "*"):
                if k in route:
                    return route_of(route[k], cls, ekey)
            raise KeyError((cls, ekey))
        return route

    def add(group, route, classes, M, N, K, epis=EP, Ksplit=None, Kf32=None, tag="", families=("lattice", "real"), **kw):
        for cls in classes:
            k = _kfor(cls, K, Ksplit, Kf32)
            for ekey in epis:
                epi, resid = (2, True) if ekey == "2r" else (ekey, False)
                if epi == 5:
                    resid = True
                kw2 = dict(kw)
                if ekey == "2r" and cls != "split":          # ops.gemm_resid: plain [M, N] tensors, no row map
                    if kw2.get("grp") or kw2.get("a_grp") or kw2.get("ldo_odd") or kw2.get("off_out"):
                        continue
                    kw2["contiguous_out"] = True
                fams = tuple(f for f in families if f == "real" or epi in (0, 2, 3))
                r = route_of(route, cls, ekey)
                cid = "%s-%s-%dx%dx%d-e%s%s" % (r, cls, M, N, k, ekey, ("-" + tag) if tag else "")
                cs.append(SimpleNamespace(id=cid, group=group, route=r, cls=cls, M=M, N=N, K=k, epi=epi, resid=resid, families=fams, kw=kw2))

    ALL = CLASSES
    # ---- routes ----
    # the weight-streaming kernel: NW8/MF1, NW16/MF1, NW8/MF4, NW16/MF4, and the deep seam K2 / 32 = 62 | 64
    add("route", "smallm<NW8,MF1>", ALL, 1, 16, 64)
    add("route", "smallm<NW16,MF1>", ALL, 16, 48, 2048, Ksplit=1024, Kf32=1024)
    add("route", "smallm<NW8,MF4>", ALL, 17, 83, 64)
    add("route", "smallm<NW16,MF4>", ALL, 64, 144, 2048, Ksplit=1024, Kf32=1024)
    add("route", "smallm<NW8,MF1>", ALL, 16, 48, 1984, epis=(0, 2), Ksplit=992, Kf32=992)
    # skinny: K slices over workgroups (epilogue 2 in place) 1, 2, 4; with resid given: 1
    add("route", "skinny(ks=1)", TILE, 65, 64, 64)
    add("route", "skinny(ks=1)", TILE, 256, 83, 64)
    add("route", {2: "skinny(ks=2)", "2r": "skinny(ks=1)"}, TILE, 200, 3072, 4096, epis=(2, "2r"), Ksplit=2048)
    add("route", {2: "skinny(ks=4)", "2r": "skinny(ks=1)"}, TILE, 129, 128, 8192, epis=(2, "2r"), Ksplit=4096)
    # skinny with M <= 64: the epilogues the weight-streaming kernel does not have
    add("route", "skinny(ks=1)", ("split",), 40, 128, 64, epis=(5,))
    add("route", "skinny(ks=1)", TILE, 40, 128, 64, epis=(4,), rope_C=64)
    # 128-row tiles alone; 64-row tiles (split class, epilogue 2)
    t4 = {"*": "mi4", ("split", 2): "mi2", ("split", "2r"): "mi2"}
    add("route", t4, TILE, 257, 128, 64)
    add("route", t4, TILE, 300, 144, 192, Ksplit=96)
    add("route", "mi4", ("f32x",), 300, 144, 96)
    add("route", "mi2", ("split",), 385, 256, 64, epis=(2, "2r"))
    add("route", "mi4", ("split",), 1000, 256, 64, epis=(5,))
    # 128-row tiles + tails
    add("route", "mi4+tail:smallm<NW8,MF1>", TILE, 4100, 1024, 64, epis=(0, 1, 2, "2r", 3), Ksplit=96)
    add("route", "mi4+tail:skinny(ks=1)", TILE, 4100, 1024, 64, epis=(4,), Ksplit=96, rope_C=256)
    add("route", "mi4+tail:skinny(ks=1)", ("split",), 4100, 1024, 64, epis=(5,))
    # 256 x 128 tiles + tails
    add("route", "mi8+tail:smallm<NW8,MF1>", TILE, 2056, 4096, 64, Ksplit=96)
    add("route", "mi8+tail:skinny(ks=1)", TILE, 2056, 4096, 64, epis=(4,), Ksplit=96, rope_C=1024)
    add("route", "mi8+tail:skinny(ks=1)", ("split",), 2056, 4096, 64, epis=(5,))
    add("route", "mi8+tail:skinny(ks=1)", ("f16",), 8292, 4096, 64)
    add("route", "mi8+tail:skinny(ks=1)", ("split",), 8257, 4096, 96)
    # 256 x 256 tiles: one launch, a partly filled last tile row, the f32 class with M < 256; + tails
    add("route", "g256", ("f16", "split", "f32x"), 3072, 4096, 128, epis=(0, 2), Ksplit=64, Kf32=64)
    add("route", "g256", ("f16", "split", "f32x"), 3072, 4096, 128, epis=(4,), Ksplit=64, Kf32=64, rope_C=1024)
    add("route", "g256", ("split",), 3072, 4096, 64, epis=(5,))
    add("route", "g256", ALL, 3100, 4096, 128, epis=(1, "2r", 3), Ksplit=64, Kf32=64)
    add("route", "g256", ("f32x",), 65, 64, 64)
    add("route", "g256", ("f32x",), 257, 83, 64, epis=(0, 2))
    add("route", "g256+tail:smallm<NW8,MF4>", TILE, 16448, 1024, 128, Ksplit=64)
    add("route", "g256+tail:skinny(ks=1)", ("f16", "split"), 16576, 1024, 128, epis=(0, 1, 2, "2r", 3), Ksplit=64)
    add("route", "g256+tail:skinny(ks=1)", ("f16", "split"), 16576, 1024, 128, epis=(4,), Ksplit=64, rope_C=256)
    add("route", "g256+tail:mi4(ks=1)", ("f16", "split"), 16684, 1024, 128, Ksplit=64)
    add("route", "g256+tail:mi4(ks=1)", ("f16", "split"), 16684, 1024, 128, epis=(4,), Ksplit=64, rope_C=256)
    add("route", "g256+tail:mi4(ks=1)", ("split",), 16684, 1024, 64, epis=(5,))
    add("route", {2: "g256+tail:mi4(ks=2)", "2r": "g256+tail:mi4(ks=1)"}, TILE, 16684, 1024, 512, epis=(2, "2r"), Ksplit=256)
    # ---- row maps: grp_in in {1, 37, 257}, grp_out > grp_in, grp_off > 0, the same for the input map; group boundaries off the tile
    # edges and off the main / tail seam (16384 and 2048 are no multiples of 37 or 257)
    for gi in (1, 37, 257):
        kw = dict(grp=(gi, gi + 3, 2), a_grp=(gi, gi + 2, 1), tag="grp%d" % gi)
        add("rowmap", "smallm<NW8,MF4>", ALL, 17, 83, 64, epis=(0, 2), **kw)
        add("rowmap", "skinny(ks=1)", TILE, 200, 144, 64, epis=(0, 2), **kw)
        add("rowmap", t4, TILE, 300, 144, 64, epis=(0, 2), **kw)
        add("rowmap", "mi4", ("f32x",), 300, 144, 96, epis=(0, 2), **kw)
        add("rowmap", "g256", ("f32x",), 300, 144, 64, epis=(0, 2), **kw)
        if gi > 1:
            add("rowmap", "g256+tail:mi4(ks=1)", ("f16", "split"), 16684, 1024, 128, epis=(0, 2), Ksplit=64, **kw)
            add("rowmap", "mi8+tail:smallm<NW8,MF1>", ("f16", "split"), 2056, 4096, 64, epis=(0, 2), Ksplit=96, **kw)
            add("rowmap", "mi4+tail:smallm<NW8,MF1>", ("bf16", "split"), 4100, 1024, 64, epis=(0, 2), Ksplit=96, **kw)
    # ---- gate groups at the seam of the fast epilogue's "two gate groups per lane": gate_rows in {1, 16 MI - 1, 16 MI, 16 MI + 1, 257},
    # the last group partial, gate_ld padded; once each with gate_ld % 4 != 0 and with the gate pointer off by one float
    gate_shapes = [("smallm<NW8,MF4>", ALL, 64, 144, 64, {}), ("skinny(ks=1)", TILE, 200, 144, 64, {}), ("mi2", ("split",), 385, 256, 64, {}),
                   ("mi4", B16, 300, 144, 64, {}), ("mi4", ("f32x",), 300, 144, 96, {}),
                   ("mi8+tail:smallm<NW8,MF1>", ("f16", "split"), 2056, 4096, 64, dict(Ksplit=96)),
                   ("g256", ("f16", "split", "f32x"), 3072, 4096, 128, dict(Ksplit=64, Kf32=64))]
    for route, classes, M, N, K, kk in gate_shapes:
        w = MI_OF[route.split("+")[0].split("<")[0].split("(")[0]]
        for gr in (1, w - 1, w, w + 1, 257):
            add("gate", route, classes, M, N, K, epis=(2,), gate_rows=gr, tag="gate%d" % gr, **kk)
        add("gate", route, classes, M, N, K, epis=(2,), gate_rows=w, gate_ld_odd=True, tag="gate%d-ldodd" % w, **kk)
        add("gate", route, classes, M, N, K, epis=(2,), gate_rows=w + 1, off_gate=1, tag="gate%d-off1" % (w + 1), **kk)
    # ---- partly filled last column tile and the non-vector half of the epilogue: N = 83 / 144 with ldo % 4 != 0, out / resid / bias off by
    # one element, no bias
    for N in (83, 144):
        shapes = [("smallm<NW8,MF4>", ALL, 17, 64, {}), ("skinny(ks=1)", TILE, 200, 64, {}), (t4, TILE, 300, 64, {}),
                  ("mi4", ("f32x",), 300, 96, {}), ("g256", ("f32x",), 300, 64, {})]
        for route, classes, M, K, kk in shapes:
            add("align", route, classes, M, N, K, epis=(0, 1, 2, 3), ldo_odd=True, tag="ldo-odd", **kk)
            add("align", route, classes, M, N, K, epis=(0, 1, 2, 3), off_out=1, tag="out-off1", **kk)
            add("align", route, classes, M, N, K, epis=(0, 2), ldo_odd=True, off_out=1, off_bias=1, tag="all-off1", **kk)
            add("align", route, classes, M, N, K, epis=(0, 2), bias=False, tag="nobias", **kk)
            add("align", route, classes, M, N, K, epis=("2r",), off_resid=1, tag="resid-off1", **kk)
    # ---- RoPE: the three kinds mixed inside every 16-row fragment, pos in {0, 63, 64} and random below 17 (make_case), C = 64 with N = 192 (one 128-wide
    # tile holds q, k and part of v), C = 128 with N = 3 C, under a row map (pos is indexed by OUTPUT row), on a tail route
    for C in (64, 128):
        for kw in (dict(), dict(grp=(37, 40, 2), a_grp=(37, 39, 1), tag="grp37")):
            add("rope", "skinny(ks=1)", TILE, 200, 3 * C, 64, epis=(4,), rope_C=C, **kw)
            add("rope", "mi4", TILE, 300, 3 * C, 64, epis=(4,), rope_C=C, **kw)
            add("rope", "g256", ("f32x",), 300, 3 * C, 64, epis=(4,), rope_C=C, **kw)
            add("rope", "mi4", ("f32x",), 300, 3 * C, 96, epis=(4,), rope_C=C, **kw)
    add("rope", "skinny(ks=1)", TILE, 200, 192, 64, epis=(4,), rope_C=64, rope_kinds=False, tag="nokind")
    # position 1000, far behind the table, in cases of its own: an f32 angle p * base^(-i / 16) carries about p * 2e-7 rad, 1e-4 rad at p = 1000 --
    # above what 2e-5 of max |ref| allows the f32 classes; the epilogue takes such positions through sincos_far (gemm_common.h)
    far = dict(rope_C=64, rope_far=True, tag="pos1000")
    add("rope", "skinny(ks=1)", TILE, 200, 192, 64, epis=(4,), **far)
    add("rope", "mi4", TILE, 300, 192, 64, epis=(4,), **far)
    add("rope", "g256", ("f32x",), 300, 192, 64, epis=(4,), **far)
    add("rope", "mi4", ("f32x",), 300, 192, 96, epis=(4,), **far)
    add("rope", "mi4+tail:skinny(ks=1)", ("f16", "split"), 4100, 1024, 64, epis=(4,), Ksplit=96, rope_C=256, grp=(257, 260, 2), tag="grp257")
    # ---- split class: packed A (bit-identical to the f32-A run, M <= 64 included) and packed output (= packing the f32 output), per route.
    # Where the K slices of epilogue 2 meet through atomics the sums depend on the order, so those routes run the lattice family.
    sp = ("split",)
    for route, M, N, K, epis in (("smallm<NW8,MF4>", 40, 128, 64, (0, 2)), ("smallm<NW16,MF1>", 16, 48, 1024, (0,)), ("skinny(ks=1)", 200, 128, 64, (0, 2)),
                                 ({0: "mi4", 2: "mi2"}, 300, 128, 64, (0, 2)), ("mi4+tail:smallm<NW8,MF1>", 4100, 1024, 96, (0, 2)),
                                 ("mi8+tail:smallm<NW8,MF1>", 2056, 4096, 96, (0,)), ("mi8+tail:skinny(ks=1)", 8257, 4096, 96, (2,)),
                                 ("g256", 3072, 4096, 64, (0, 2)), ("g256+tail:smallm<NW8,MF4>", 16448, 1024, 64, (0,)),
                                 ("g256+tail:skinny(ks=1)", 16576, 1024, 64, (2,)), ("g256+tail:mi4(ks=1)", 16684, 1024, 64, (0, 2))):
        add("packed_a", route, sp, M, N, K, epis=epis, a_packed=True, families=("real",), tag="packed-a")
    add("packed_a", "mi4+tail:skinny(ks=1)", sp, 4100, 1024, 96, epis=(4,), a_packed=True, rope_C=256, families=("real",), tag="packed-a")
    add("packed_a", "g256+tail:mi4(ks=2)", sp, 16684, 1024, 256, epis=(2,), a_packed=True, families=("lattice",), tag="packed-a")
    add("packed_a", "skinny(ks=2)", sp, 200, 3072, 2048, epis=(2,), a_packed=True, families=("lattice",), tag="packed-a")
    for route, M, N, K in (("skinny(ks=1)", 40, 128, 64), ("skinny(ks=1)", 200, 128, 64), ("mi4", 300, 128, 64), ("mi4+tail:skinny(ks=1)", 4100, 1024, 96),
                           ("mi8+tail:skinny(ks=1)", 2056, 4096, 96), ("g256", 3072, 4096, 64), ("g256+tail:skinny(ks=1)", 16448, 1024, 64),
                           ("g256+tail:mi4(ks=1)", 16684, 1024, 64)):
        add("packed_out", route, sp, M, N, K, epis=(0, 1, 3), out_packed=True, families=("real",), tag="packed-out")
    add("packed_out", "skinny(ks=1)", sp, 200, 192, 64, epis=(4,), out_packed=True, rope_C=64, families=("real",), tag="packed-out")
    add("packed_out", "mi4", sp, 300, 384, 64, epis=(4,), out_packed=True, rope_C=128, families=("real",), tag="packed-out")
    # one case with tiny weights: the largest at 1.5 * 2^-11, where split_scale_exp reaches its clamp of 24
    add("tiny_w", "mi4", sp, 300, 144, 96, epis=(0,), w_amax=1.5 * 2.0 ** -11, families=("real",), tag="tiny-w")
    ids = [c.id for c in cs]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return cs


CASES = _cases()


def build(case, family, seed=0):
    """make_case of a table entry."""
    return make_case(case.cls, case.M, case.N, case.K, case.epi, family=family, resid=case.resid, seed=seed, **case.kw)
