"""Every attention route of csrc/attention.hip / attention_bwd.hip, forward and backward, against the float64 reference of
tests/attention_f64.py evaluated on the same stored values, at the tile, mask and segment edges.  Goes through vicasplat_amd.ops (the
ctypes C ABI).  -m gpu.

Operand classes: f16, bf16 (resident / 64-query / 128-query kernels; backward through the atomic entry and the direct 16-bit entry),
f32x (the exact-f32 kernel, dtype 3, forward only), split (f32 in; f32 and packed out; split backward), sp (packed q | k | v in; f32 and
packed out).  The route a case is meant to reach is the first part of its id:
    res     attention_res_kernel            k1      attention_kernel<*,1>           k2      attention_kernel<*,2>
    split1  attention_split_kernel<1>       split2  attention_split_kernel<2>       sp      attention_sp_kernel<3>
    sweep / fam: lengths across the tile edges and every input family of attention_route_cases.FAMILIES, all classes (16-bit: res when the
    case is plain and short, k1 otherwise; f32x: attention_f32_kernel).
The thresholds between the routes are attention_route of csrc/routes.h; tests/test_routes_cpu.py proves on the CPU that every case of
tests/attention_route_cases.py reaches the route its id names, and that every route is reached.
Inputs come from attention_f64.make_case, whose planted boundary keys make a mask / segment / tile error move out, lse and the gradients
by >= 10x every bound used here (asserted on the CPU in tests/test_attention_ref_cpu.py).

Bounds (max |error| over max |reference|, whole tensor, live rows): forward f16 3e-3, bf16 2e-2, split / sp 6e-6, f32x 3e-6; backward
f16 6e-3, bf16 3e-2, split 1e-5; lse (log2 units) split / sp / f32x 1e-4 -- the bounds of test_ops_gpu.py, test_split_path_gpu.py,
test_split_bwd_gpu.py and test_f32_path_gpu.py.  lse of the 16-bit classes: 4 x the largest deviation measured over this file, never above
one storage rounding of the row sum, 2^-11 / ln 2 = 7.0e-4 (f16) and 2^-8 / ln 2 = 5.6e-3 (bf16):
    measured maxima on MI355X: f16 5.62e-6 (fam-L257-plain_peaked), bf16 5.69e-6 (fam-L257-seg_uneven_peaked) -> asserted 2.2e-5 / 2.3e-5
    (attention_f64.LSE16_MEASURED / LSE16_BOUND).  Other measured maxima over the file: out f16 4.3e-4, bf16 3.5e-3, split 1.3e-6,
    sp 1.4e-6, f32x 1.9e-6; backward dq f16 3.8e-3, bf16 2.6e-2, split 3.1e-6; lse split 7.4e-6, sp 8.1e-6, f32x 1.3e-5.
The packed output of both split kernels is bit-identical to packing the f32 output, under masks and segments too.  (This file found that
attention_split_kernel's was not: its epilogue contracted o * 1/l and the subtraction of hi into one fma, so lo came from the unrounded
product and differed by one f16 unit; the epilogue now rounds the product first.)
"""
from types import SimpleNamespace

import pytest
import torch

from attention_f64 import LSE16_BOUND, STORAGE, attention_f64, make_case, rel
from attention_route_cases import ALL, CASES, FAMILIES, PERMUTE_CASES

pytestmark = pytest.mark.gpu

TOL_OUT = {"f16": 3e-3, "bf16": 2e-2, "f32x": 3e-6, "split": 6e-6, "sp": 6e-6}
TOL_LSE = {"f16": LSE16_BOUND["f16"], "bf16": LSE16_BOUND["bf16"], "f32x": 1e-4, "split": 1e-4, "sp": 1e-4}
TOL_BWD = {"f16": 6e-3, "bf16": 3e-2, "split": 1e-5}
SENTINEL = -1024.0          # exactly representable in f16 and bf16


def _dev():
    return torch.device("cuda:0")


def _storage(cls):
    return cls if cls in ("f16", "bf16") else "f32"


class _Run:
    """One case on the device in one operand class: buffers with the row strides of a packed projection (q in a [rows, C + 64] buffer,
    k | v side by side in a [rows, 2C] buffer), every output pre-filled with a sentinel."""

    def __init__(self, cls, c):
        from vicasplat_amd import ops
        self.ops, self.cls, self.c, d = ops, cls, c, _dev()
        self.dt = dt = STORAGE[_storage(cls)]
        self.C = C = c.q.shape[1]
        self.H = c.kw["H"]
        qbuf = torch.zeros(c.q.shape[0], C + 64, dtype=dt, device=d)
        kvbuf = torch.zeros(c.k.shape[0], 2 * C, dtype=dt, device=d)
        qbuf[:, :C], kvbuf[:, :C], kvbuf[:, C:] = c.q.to(d), c.k.to(d), c.v.to(d)
        if cls == "sp":
            qp, kvp = ops.split_pack_weight(qbuf, 0).data, ops.split_pack_weight(kvbuf, 0).data
            self.q, self.k, self.v = qp[:, :C], kvp[:, :C], kvp[:, C:]
        else:
            self.q, self.k, self.v = qbuf[:, :C], kvbuf[:, :C], kvbuf[:, C:]
        self.qf, self.kf, self.vf = qbuf[:, :C], kvbuf[:, :C], kvbuf[:, C:]          # the plain views (split backward reads f32)
        self.dout = c.dout.to(dt).to(d)
        self.kw = {k: (v.to(d) if torch.is_tensor(v) else v) for k, v in c.kw.items()}
        self.odt = dt if cls in ("f16", "bf16") else torch.float32
        self.q_live, self.k_live = c.q_live.to(d), c.k_live.to(d)

    def forward(self, packed_out=False):
        ops, d = self.ops, _dev()
        rows = self.q.shape[0]
        lse = torch.full((rows, self.H), SENTINEL, dtype=torch.float32, device=d)
        if packed_out:
            out = ops.split_act(rows, self.C, d)
            out.data.fill_(0x12345678)
        else:
            out = torch.full((rows, self.C), SENTINEL, dtype=self.odt, device=d)
        ops.attention(self.q, self.k, self.v, out, lse=lse, split=self.cls in ("split", "sp"), **self.kw)
        return out, lse

    def backward(self, out, lse, direct=False):
        """-> dq, dk, dv.  16-bit: the atomic entry (f32 dk / dv from zero) or, direct, vs_attention_backward16 into sentinel-filled 16-bit
        buffers; split: dk_out / dv_out always given, sentinel-filled (with key segments the call zeroes them)."""
        ops, d, C = self.ops, _dev(), self.C
        dq = torch.full((self.q.shape[0], C), SENTINEL, dtype=self.odt, device=d)
        if self.cls == "split":
            dk = torch.full((self.k.shape[0], C), SENTINEL, dtype=torch.float32, device=d)
            dv = torch.full((self.k.shape[0], C), SENTINEL, dtype=torch.float32, device=d)
            ops.attention_backward_split(self.qf, self.kf, self.vf, out, self.dout, lse, dq_out=dq, dk_out=dk, dv_out=dv, max_keys=self.c.max_keys, **self.kw)
            return dq, dk, dv
        if direct:
            dk = torch.full((self.k.shape[0], C), SENTINEL, dtype=self.odt, device=d)
            dv = torch.full((self.k.shape[0], C), SENTINEL, dtype=self.odt, device=d)
            ops.attention_backward(self.q, self.k, self.v, out, self.dout, lse, dq_out=dq, dk_out=dk, dv_out=dv, **self.kw)
            return dq, dk, dv
        _, dk, dv = ops.attention_backward(self.q, self.k, self.v, out, self.dout, lse, dq_out=dq, max_keys=self.c.max_keys, **self.kw)
        return dq, dk, dv

    def reference(self, with_grad):
        c, d = self.c, _dev()
        return attention_f64(c.q.to(d), c.k.to(d), c.v.to(d), dout=self.dout.float() if with_grad else None, **c.kw)


def _where(name, got, ref, live, H):
    """Coordinates of the worst element: (row, head, column within the head) -- printed with a failure."""
    e = (got.double() - ref).abs()
    e = torch.where(live[:, None].expand_as(e), e, torch.zeros_like(e))
    i = int(e.argmax())
    r, col = divmod(i, e.shape[1])
    per = e.shape[1] // H
    return f"{name}: worst at row {r}, head {col // per}, col {col % per}: got {float(got[r, col]):.6g} ref {float(ref[r, col]):.6g}"


def _check_case(cls, c, tag):
    run = _Run(cls, c)
    H, ql, kl = run.H, run.q_live, run.k_live
    has_bwd = cls in TOL_BWD
    ref = run.reference(has_bwd)
    out, lse = run.forward()
    fig = dict(out=rel(out[ql], ref["out"][ql]), lse=float((lse[ql].double() - ref["lse"][ql]).abs().max()))
    fails = []
    if not fig["out"] <= TOL_OUT[cls]:
        fails.append(_where("out", out, ref["out"], ql, H))
    if not fig["lse"] <= TOL_LSE[cls]:
        fails.append(_where("lse", lse, ref["lse"], ql, H))
    # rows of no batch item are not written; a second call returns the same bits
    assert bool((out[~ql] == SENTINEL).all()) and bool((lse[~ql] == SENTINEL).all()), "forward wrote rows outside the batch items"
    out2, lse2 = run.forward()
    assert torch.equal(out, out2) and torch.equal(lse, lse2), "forward is not deterministic"
    if cls in ("split", "sp"):             # the packed output against the packed image of the f32 output, masks and segments included
        outp, lsep = run.forward(packed_out=True)
        want = run.ops.split_pack_weight(torch.where(ql[:, None], out, torch.zeros_like(out)), 0).data
        assert torch.equal(lsep, lse) and bool((outp.data[~ql] == 0x12345678).all())
        assert torch.equal(outp.data[ql], want[ql]), "packed output differs from packing the f32 output"
    if has_bwd:
        dq, dk, dv = run.backward(out, lse)
        # With a single visible key per query dq and dk are exactly zero (p = 1, dp = delta) and the metric has no denominator; the error
        # is then the cancellation p (dp - delta), so it is measured against the size of one term, scale * max|delta| * max|k| (resp. |q|),
        # delta = dout . out per (row, head).
        delta = float((c.dout.to(_dev())[ql].double() * ref["out"][ql]).reshape(-1, H, 64).sum(-1).abs().max()) * c.kw["scale"]
        zero_ref = []            # gradients measured against that term size instead of max |reference| (named in the FIG line)
        floor = dict(dq=delta * float(c.k[c.k_live].abs().max()), dk=delta * float(c.q[c.q_live].abs().max()), dv=0.0)
        for nm, got, rf, live in (("dq", dq, ref["dq"], ql), ("dk", dk, ref["dk"], kl), ("dv", dv, ref["dv"], kl)):
            den = float(rf[live].abs().max())
            if den == 0.0:
                den, zero_ref = floor[nm], zero_ref + [nm]
            fig[nm] = float((got[live].double() - rf[live]).abs().max()) / den
            if not fig[nm] <= TOL_BWD[cls]:
                fails.append(_where(nm, got, rf, live, H))
        assert bool((dq[~ql] == SENTINEL).all()), "backward wrote dq rows outside the batch items"
        seg = "kv_seg" in c.kw
        if seg:          # dk / dv meet through atomics under key segments; dq is stored by its one owner on every entry
            assert torch.equal(run.backward(out, lse)[0], dq), "dq is not deterministic under key segments"
        if cls == "split":
            if seg:      # accumulated from the zero fill of the call: unreferenced rows end as zero
                assert bool((dk[~kl] == 0).all()) and bool((dv[~kl] == 0).all())
            else:        # plain stores: rows of no batch item untouched, and no atomics -> the same bits again
                assert bool((dk[~kl] == SENTINEL).all()) and bool((dv[~kl] == SENTINEL).all())
                dq2, dk2, dv2 = run.backward(out, lse)
                assert torch.equal(dq, dq2) and torch.equal(dk, dk2) and torch.equal(dv, dv2), "split backward is not deterministic"
        else:
            assert bool((dk[~kl] == 0).all()) and bool((dv[~kl] == 0).all())
            if not seg:  # the direct entry: the atomic entry's f32 sums rounded once, plain stores, deterministic
                dq16, dk16, dv16 = run.backward(out, lse, direct=True)
                assert torch.equal(dq16, dq)
                assert torch.equal(dk16[kl], dk[kl].to(run.dt)) and torch.equal(dv16[kl], dv[kl].to(run.dt)), "direct dk / dv != atomic dk / dv rounded once"
                assert bool((dk16[~kl] == SENTINEL).all()) and bool((dv16[~kl] == SENTINEL).all())
                dq2, dk2, dv2 = run.backward(out, lse, direct=True)
                assert torch.equal(dq16, dq2) and torch.equal(dk16, dk2) and torch.equal(dv16, dv2), "direct backward is not deterministic"
    print(f"FIG {tag} {cls} " + " ".join(f"{k}={v:.3e}" for k, v in fig.items()) + (f" zero-reference:{','.join(zero_ref)}" if has_bwd and zero_ref else ""))
    assert not fails, (tag, cls, fig, fails)
    return run, out, lse


PARAMS = [pytest.param(cls, kw, id=f"{cid}-{cls}") for cid, classes, kw in CASES for cls in classes]


@pytest.mark.parametrize("cls,kw", PARAMS)
def test_route_matches_float64(cls, kw, request):
    c = make_case(seed=kw["Lq"], storage=_storage(cls), **kw)
    _check_case(cls, c, request.node.callspec.id)


@pytest.mark.parametrize("fam", ["plain", "ragged", "camera3", "seg_uneven", "seg_uneven_ragged"])
@pytest.mark.parametrize("L", [37, 257])
@pytest.mark.parametrize("cls", ALL)
def test_padded_batch_rows_do_not_leak(cls, L, fam, request):
    """q_batch_rows > Lq and (without segments) k_batch_rows > Lk, the rows between the batch items NaN in q, k, v and dout: every check of
    _check_case holds (live results finite and right, rows of no item bit-untouched or zero), and out / lse equal, bit for bit, what the
    same call returns on compacted buffers."""
    c = make_case(nbatch=3, H=2, Lq=L, pad=5, nan_pad=True, seed=L, storage=_storage(cls), **FAMILIES[fam])
    run, out, lse = _check_case(cls, c, request.node.callspec.id)
    assert bool(torch.isfinite(out[run.q_live].float()).all()) and bool(torch.isfinite(lse[run.q_live]).all())
    kw = dict(c.kw, q_batch_rows=L)
    k, v, k_live = c.k, c.v, c.k_live
    if "kv_seg" not in c.kw:
        kw.update(k_batch_rows=L)
        k, v, k_live = c.k[c.k_live], c.v[c.k_live], torch.ones(3 * L, dtype=torch.bool)
    c0 = SimpleNamespace(q=c.q[c.q_live], k=k, v=v, dout=c.dout[c.q_live], kw=kw, max_keys=c.max_keys, q_live=torch.ones(3 * L, dtype=torch.bool),
                         k_live=k_live, nks=c.nks, storage=c.storage)
    if "kv_seg" in c.kw:          # key rows are not padded under segments, but rows no segment reads are NaN: keep them out of the packing
        c0.k, c0.v = torch.nan_to_num(k), torch.nan_to_num(v)
    run0 = _Run(cls, c0)
    out0, lse0 = run0.forward()
    assert torch.equal(out[run.q_live], out0) and torch.equal(lse[run.q_live], lse0)
    if cls in TOL_BWD and "kv_seg" not in c.kw:
        direct = cls != "split"
        g, g0 = run.backward(out, lse, direct=direct), run0.backward(out0, lse0, direct=direct)
        for a, b, live in zip(g, g0, (run.q_live, run.k_live, run.k_live)):
            assert torch.equal(a[live], b)


@pytest.mark.parametrize("cid,cls,kw", PERMUTE_CASES)
def test_permuting_batch_items_permutes_the_result(cid, cls, kw):
    """An XCD / grid remap that crossed batch items would not survive this: the items in another order give the same bits in that order."""
    c = make_case(seed=7, storage=_storage(cls), **kw)
    nb, L = kw["nbatch"], kw["Lq"]
    out, lse = _Run(cls, c).forward()
    perm = torch.tensor([(3 * b + 1) % nb for b in range(nb)]) if nb % 3 else torch.arange(nb).flip(0)
    rows = (perm[:, None] * L + torch.arange(L)[None, :]).reshape(-1)
    ckw = dict(c.kw)
    if "q_kvlen" in ckw:
        ckw["q_kvlen"] = ckw["q_kvlen"].reshape(nb, L)[perm].reshape(-1).contiguous()
    cp = SimpleNamespace(q=c.q[rows], k=c.k[rows], v=c.v[rows], dout=c.dout[rows], kw=ckw, max_keys=0, q_live=c.q_live, k_live=c.k_live,
                         nks=c.nks, storage=c.storage)
    outp, lsep = _Run(cls, cp).forward()
    rows = rows.to(out.device)
    assert torch.equal(outp, out[rows]) and torch.equal(lsep, lse[rows])
