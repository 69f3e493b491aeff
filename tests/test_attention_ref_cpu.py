"""The float64 attention reference (tests/attention_f64.py) is right, and the inputs of tests/test_attention_routes_gpu.py are sharp enough:
every deliberate mask / segment / tile / scale error below, applied to the REFERENCE, moves the suite's own metrics by at least ten times
the tolerance of every operand class.  Runs without a GPU.

Asserted per mutation: "forward" = max(out, lse) and "backward" = max(dq, dk, dv), each over its own tolerance, are both >= 10.  Which
metric carries the rejection depends on the family and length and is printed per mutation (`-s`: "<ratio>x via <forward>/<backward>").
Over all families, lengths and storage types: the forward rejection is through lse in most cases and through out in the rest (short key
sets, where one key is a large share of a row), for every mutation in the list; the backward rejection is through dv or dk (the planted
boundary keys dominate them) and otherwise dq (scale=0.125: always dk first).
"""
import math

import pytest
import torch
import torch.nn.functional as F

from attention_f64 import FAMILIES, HD, LN2, TOLERANCES, attention_f64, key_rows, make_case, rel

# (nbatch, H, L).  The fam-L100 / fam-L257 cases of the GPU file are these inputs exactly but for H (same generator, nbatch and seed = L); 17
# and 129 stand for its length sweep (nbatch 2, seed = L, and only the three families the sweep uses), 1032 for the long routes.  The GPU
# file's other shapes (H 16, nbatch 4 / 7 / 11, Lq != Lk, the other sweep lengths) come from the same generator with the same planting
# rule but are not re-run here.
SHAPES = [(2, 1, 17), (3, 1, 100), (2, 1, 129), (2, 1, 257), (2, 1, 1032)]
SWEEP_LENGTHS, SWEEP_FAMILIES = (17, 129), ("plain", "ragged", "seg_uneven")


def _sdpa(c, kw):
    """torch's own scaled_dot_product_attention (float64, boolean mask) on the gathered keys of every batch item."""
    H, Lq = kw["H"], kw["Lq"]
    outs = []
    for b in range(kw["nbatch"]):
        idx = key_rows(b, Lk=kw.get("Lk", 0), k_batch_rows=kw.get("k_batch_rows", 0), kv_seg=kw.get("kv_seg"))
        nk = idx.numel()
        mask = torch.ones(Lq, nk, dtype=torch.bool)
        if "q_kvlen" in kw:
            mask = torch.arange(nk)[None, :] < kw["q_kvlen"][b * Lq:(b + 1) * Lq, None]
        r0 = b * kw["q_batch_rows"]
        qb = c.q[r0:r0 + Lq].double().reshape(Lq, H, HD).transpose(0, 1)
        kb = c.k[idx].double().reshape(nk, H, HD).transpose(0, 1)
        vb = c.v[idx].double().reshape(nk, H, HD).transpose(0, 1)
        outs.append(F.scaled_dot_product_attention(qb, kb, vb, attn_mask=mask[None], scale=kw["scale"]).transpose(0, 1).reshape(Lq, H * HD))
    return outs


@pytest.mark.parametrize("fam", ["plain", "ragged", "camera3", "seg_prod2", "seg_uneven_ragged", "seg_overlap", "ragged_scale03"])
@pytest.mark.parametrize("nb,H,L,pad", [(2, 2, 37, 0), (3, 1, 100, 5), (1, 2, 257, 0)])
def test_reference_agrees_with_torch_sdpa(fam, nb, H, L, pad):
    c = make_case(nbatch=nb, H=H, Lq=L, pad=pad, nan_pad=True, seed=3, **FAMILIES[fam])
    r = attention_f64(c.q, c.k, c.v, **c.kw)
    for b, ob in enumerate(_sdpa(c, c.kw)):
        r0 = b * c.kw["q_batch_rows"]
        assert float((r["out"][r0:r0 + L] - ob).abs().max()) <= 1e-12
    assert torch.isnan(r["out"][~c.q_live]).all() and torch.isfinite(r["lse"][c.q_live]).all()


def test_reference_lse_is_the_log2_logsumexp_and_exact_on_a_uniform_row():
    c = make_case(nbatch=2, H=2, Lq=40, seed=1, **FAMILIES["ragged_uniform"])
    r = attention_f64(c.q, c.k, c.v, **c.kw)
    lens = c.kw["q_kvlen"].reshape(2, 40)
    for b in range(2):
        # the zero query: every visible score is 0
        assert float((r["lse"][b * 40 + 39] - math.log2(int(lens[b, 39]))).abs().max()) <= 1e-12
        # the query whose 24 visible keys are identical: lse = score * log2(e) + log2(24)
        s = (c.q[b * 40 + 38].double().reshape(2, HD) * c.k[b * 40].double().reshape(2, HD)).sum(-1) * 0.125
        assert int(lens[b, 38]) == 24
        assert float((r["lse"][b * 40 + 38] - (s / LN2 + math.log2(24))).abs().max()) <= 1e-12


def test_reference_gradients_pass_gradcheck_and_sum_over_shared_rows():
    c = make_case(nbatch=2, H=1, Lq=5, seed=2, **FAMILIES["seg_overlap"])
    kw = dict(c.kw, q_kvlen=torch.tensor([5, 1, 7, 3, 6, 2, 7, 7, 4, 1], dtype=torch.int32))

    q, k, v = (t.double().requires_grad_() for t in (c.q, c.k, c.v))
    for name in ("out", "lse"):
        assert torch.autograd.gradcheck(lambda a, b_, c_: attention_f64(a, b_, c_, **kw)[name], (q, k, v), eps=1e-6, atol=1e-7)
    # the dq / dk / dv the helper returns are the gradients of that same forward, scattered to key rows
    out = attention_f64(q, k, v, **kw)["out"]
    gq, gk, gv = torch.autograd.grad((out * c.dout.double()).sum(), (q, k, v))
    r = attention_f64(c.q, c.k, c.v, dout=c.dout, **kw)
    for got, want in ((r["dq"], gq), (r["dk"], gk), (r["dv"], gv)):
        assert float((got - want).abs().max()) <= 1e-12
    assert int(c.k_live.sum()) < sum(c.nks)          # rows really are shared between the two items


# ------------------------------------------------------------------------------------------------------------------------------------
# mutation check
# ------------------------------------------------------------------------------------------------------------------------------------
def _keep_nonempty(new, old):
    """A mutated mask never leaves a query without keys (that would be a NaN, not a wrong number)."""
    empty = ~new.any(1)
    new[empty] = old[empty]
    return new


def _mutations(c):
    """(name, keyword overrides for attention_f64) of every deliberate error that applies to this case."""
    kw, muts = c.kw, []
    nks = c.nks
    if "q_kvlen" in kw:
        lens = kw["q_kvlen"].reshape(kw["nbatch"], kw["Lq"]).long()
        nk = torch.tensor(nks)[:, None]
        eff = torch.minimum(lens, nk)
        for nm, delta, sel in (("prefix-1", -1, eff >= 2), ("prefix-1(>16)", -1, eff > 16), ("prefix+1", 1, eff < nk),
                               ("prefix+1(>16)", 1, (eff < nk) & (eff > 16))):
            if sel.any():
                muts.append((nm, dict(q_kvlen=torch.where(sel, eff + delta, eff).to(torch.int32).reshape(-1))))
    if min(nks) >= 2:
        def drop_last(b, m):
            old = m.clone()
            m[:, -1] = False
            return _keep_nonempty(m, old)
        muts.append(("last-key-dropped", dict(mask_edit=drop_last)))
    if "kv_seg" in kw:
        seg = kw["kv_seg"]
        # (without a prefix mask, or with one of the two empty, the order of the keys cannot matter)
        if "q_kvlen" in kw and bool(((seg[:, 1] != seg[:, 3]) & (seg[:, 1] > 0) & (seg[:, 3] > 0)).any()):
            muts.append(("segments-swapped", dict(kv_seg=seg[:, [2, 3, 0, 1]].contiguous())))
        # (an empty SECOND segment read as one key puts that key behind every prefix a mask allows: no visible change under a mask)
        if bool((seg[:, 1] == 0).any()) or ("q_kvlen" not in kw and bool((seg[:, 3] == 0).any())):
            s1 = seg.clone()
            s1[:, 1] = s1[:, 1].clamp(min=1)
            s1[:, 3] = s1[:, 3].clamp(min=1)
            muts.append(("empty-segment-read-as-1", dict(kv_seg=s1)))
    if min(nks) > 32:
        for nm, tile in (("tile-skipped(first)", lambda nk: 0), ("tile-skipped(middle)", lambda nk: nk // 32), ("tile-skipped(last)", lambda nk: (nk - 1) // 16)):
            def skip(b, m, tile=tile):
                old, t = m.clone(), tile(m.shape[1])
                m[:, 16 * t:16 * t + 16] = False
                return _keep_nonempty(m, old)
            muts.append((nm, dict(mask_edit=skip)))
    if kw["scale"] != 0.125:
        muts.append(("scale=0.125", dict(scale=0.125)))
    return muts


@pytest.mark.parametrize("storage", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_every_mutation_is_rejected_tenfold(fam, storage):
    worst, via = {}, {}
    for nb, H, L in SHAPES:
        if (storage != "bf16" and L == 1032) or (L in SWEEP_LENGTHS and fam not in SWEEP_FAMILIES):
            continue                       # bf16 has the widest bounds; the long case is run where it is hardest
        c = make_case(nbatch=nb, H=H, Lq=L, seed=L, storage=storage, **FAMILIES[fam])
        good = attention_f64(c.q, c.k, c.v, dout=c.dout, **c.kw)
        t_out, t_lse, t_bwd = TOLERANCES[storage]
        muts = _mutations(c)
        assert muts or L == 17, fam
        for nm, over in muts:
            bad = attention_f64(c.q, c.k, c.v, dout=c.dout, **dict(c.kw, **over))
            ql = c.q_live
            r = dict(out=rel(bad["out"][ql], good["out"][ql]) / t_out, lse=float((bad["lse"][ql] - good["lse"][ql]).abs().max()) / t_lse,
                     dq=rel(bad["dq"][ql], good["dq"][ql]) / t_bwd, dk=rel(bad["dk"], good["dk"]) / t_bwd, dv=rel(bad["dv"], good["dv"]) / t_bwd)
            fwd, bwd = max(r["out"], r["lse"]), max(r["dq"], r["dk"], r["dv"])
            worst[nm] = min(worst.get(nm, float("inf")), fwd, bwd)
            by = max(("out", "lse"), key=r.get) + "/" + max(("dq", "dk", "dv"), key=r.get)
            via.setdefault(nm, set()).add(by)
            assert fwd >= 10 and bwd >= 10, (fam, storage, L, nm, {k: round(x, 1) for k, x in r.items()})
    print(fam, storage, {k: f"{x:.0f}x via {'+'.join(sorted(via[k]))}" for k, x in worst.items()})


def test_mutations_cover_the_list():
    """Every error of the list is exercised by at least one family (a family only skips the ones that cannot apply to it)."""
    seen = set()
    for fam in FAMILIES:
        seen |= {nm for nm, _ in _mutations(make_case(nbatch=3, H=1, Lq=100, seed=100, **FAMILIES[fam]))}
    assert seen == {"prefix-1", "prefix-1(>16)", "prefix+1", "prefix+1(>16)", "last-key-dropped", "segments-swapped", "empty-segment-read-as-1",
                    "tile-skipped(first)", "tile-skipped(middle)", "tile-skipped(last)", "scale=0.125"}
