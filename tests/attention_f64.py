"""Float64 restatement of the fused attention operator (include/vicasplat_hip.h: vs_attention_lse and its backward entries), written
from the header's contract, plus the input generator shared by tests/test_attention_ref_cpu.py and tests/test_attention_routes_gpu.py.

  * `attention_f64`  -- plain torch, float64, one batch item at a time: builds the boolean key mask and the gathered K / V from exactly the
    ABI arguments (nbatch, H, Lq, Lk, q_batch_rows, k_batch_rows, kv_seg, q_kvlen, scale) on [rows, ld] buffers and returns out, lse
    (log2 domain) and, given dout, dq / dk / dv by torch autograd with dk / dv scattered back to key ROWS (rows shared between batch
    items under key segments sum).  It runs on whichever device its inputs are on.
  * `make_case`      -- seeded inputs of one (shape, mask, segments, value regime) family on padded [rows, ld] buffers, with dominant keys
    planted on the mask / segment / tile boundaries so that an off-by-one there moves out, lse and the gradients far beyond any class's
    tolerance (tests/test_attention_ref_cpu.py asserts that this holds, mutation by mutation).
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch

from attention_route_cases import FAMILIES  # noqa: F401  (the input families: make_case keywords by name)

HD = 64                      # head dimension of every attention kernel
LN2 = math.log(2.0)
STORAGE = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


def key_rows(b: int, *, Lk: int, k_batch_rows: int, kv_seg) -> torch.Tensor:
    """Rows of k / v that batch item b attends to, in key order: the two segments of kv_seg[b] concatenated, or b*k_batch_rows + [0, Lk)."""
    if kv_seg is None:
        return torch.arange(b * k_batch_rows, b * k_batch_rows + Lk)
    b0, l0, b1, l1 = (int(x) for x in kv_seg[b])
    return torch.cat([torch.arange(b0, b0 + l0), torch.arange(b1, b1 + l1)])


def key_mask(b: int, nk: int, *, Lq: int, q_kvlen) -> torch.Tensor:
    """[Lq, nk] bool: query i of item b sees the first min(nk, q_kvlen[b*Lq + i]) keys (all of them without q_kvlen)."""
    if q_kvlen is None:
        return torch.ones(Lq, nk, dtype=torch.bool)
    lens = torch.as_tensor(q_kvlen).reshape(-1)[b * Lq:(b + 1) * Lq].cpu().long().clamp(max=nk)
    return torch.arange(nk)[None, :] < lens[:, None]


def attention_f64(q, k, v, *, nbatch, H, Lq, Lk=0, q_batch_rows, k_batch_rows=0, kv_seg=None, q_kvlen=None, scale=0.125, dout=None,
                  mask_edit=None):
    """q / k / v (/ dout): [rows, ld >= H*64] tensors of any float dtype; head h at columns [h*64, (h+1)*64).  Returns a dict of float64
    tensors on q's device: out [q rows, H*64] and lse [q rows, H] (NaN in rows that belong to no batch item), and with dout also dq (NaN
    likewise) and dk, dv [k rows, H*64] (zero in rows no query attends to).  lse = log2 sum_j exp(scale * q . k_j) over the visible keys.
    Called without dout on inputs that require grad, out and lse stay attached to the autograd graph (for torch.autograd.gradcheck).
    mask_edit(b, mask) -> mask is for the tests of the tests (deliberately wrong references); leave it None."""
    dev, C = q.device, H * HD
    graph = dout is None and any(t.requires_grad for t in (q, k, v))
    if kv_seg is not None:
        kv_seg = torch.as_tensor(kv_seg).cpu().reshape(-1, 4).tolist()
    res = dict(out=torch.full((q.shape[0], C), float("nan"), dtype=torch.float64, device=dev),
               lse=torch.full((q.shape[0], H), float("nan"), dtype=torch.float64, device=dev))
    if dout is not None:
        res.update(dq=torch.full((q.shape[0], C), float("nan"), dtype=torch.float64, device=dev),
                   dk=torch.zeros((k.shape[0], C), dtype=torch.float64, device=dev),
                   dv=torch.zeros((v.shape[0], C), dtype=torch.float64, device=dev))
    for b in range(nbatch):
        idx = key_rows(b, Lk=Lk, k_batch_rows=k_batch_rows, kv_seg=kv_seg).to(dev)
        nk = idx.numel()
        mask = key_mask(b, nk, Lq=Lq, q_kvlen=q_kvlen)
        if mask_edit is not None:
            mask = mask_edit(b, mask.clone())
        mask = mask.to(dev)
        r0 = b * q_batch_rows
        qb, kb, vb = q[r0:r0 + Lq, :C].double().reshape(Lq, H, HD), k[idx, :C].double().reshape(nk, H, HD), v[idx, :C].double().reshape(nk, H, HD)
        if not graph:
            qb, kb, vb = (t.detach().requires_grad_(dout is not None) for t in (qb, kb, vb))
        s = torch.einsum("qhd,khd->hqk", qb, kb) * scale
        s = s.masked_fill(~mask[None], float("-inf"))
        ob = torch.einsum("hqk,khd->qhd", torch.softmax(s, -1), vb).reshape(Lq, C)
        lb = (torch.logsumexp(s, -1) / LN2).t()
        if graph:
            rows = torch.arange(r0, r0 + Lq, device=dev)
            res["out"], res["lse"] = res["out"].index_copy(0, rows, ob), res["lse"].index_copy(0, rows, lb)
        else:
            res["out"][r0:r0 + Lq] = ob.detach()
            res["lse"][r0:r0 + Lq] = lb.detach()
        if dout is not None:
            gq, gk, gv = torch.autograd.grad((ob * dout[r0:r0 + Lq, :C].double()).sum(), (qb, kb, vb))
            res["dq"][r0:r0 + Lq] = gq.reshape(Lq, C)
            res["dk"].index_add_(0, idx, gk.reshape(nk, C))
            res["dv"].index_add_(0, idx, gv.reshape(nk, C))
    return res


# ------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------------
PLANTED_LENS = (1, 2, 15, 16, 17)          # plus Lk - 1 and Lk


def ragged_lens(nbatch, Lq, nk, g):
    """Per-query key-prefix lengths: uniform in [1, nk], with 1, 2, 15, 16, 17, nk - 1 and nk planted (as far as they are in range and Lq has
    room), the full length first so that every item keeps an unmasked row."""
    lens = torch.randint(1, nk + 1, (nbatch, Lq), generator=g)
    want = [nk] + [x for x in PLANTED_LENS + (nk - 1,) if 1 <= x < nk]
    for b in range(nbatch):
        for j, x in enumerate(want[:Lq]):
            lens[b, (j * 7 + b) % Lq if Lq >= 7 * len(want) else j] = x
    return lens


def camera_lens(nbatch, Lq, nk, T):
    """The production blocked-causal pattern of T frames: token 0 of frame t sees the frames up to its own, every other query everything."""
    n = Lq // T
    lens = torch.full((nbatch, Lq), nk, dtype=torch.int64)
    for t in range(T):
        lens[:, t * n] = min(nk, (t + 1) * n)
    return lens


def make_segments(kind, nbatch, L, Rk):
    """[nbatch, 4] key segments {base0, len0, base1, len1} over Rk = nbatch * L key rows (batch item b owns rows [b*L, (b+1)*L))."""
    short = {100: 37, 257: 16}.get(L, max(1, L // 3))
    seg = []
    for b in range(nbatch):
        nxt, nx2 = ((b + 1) % nbatch) * L, ((b + 2) % nbatch) * L
        if kind == "prod2":            # two views: all keys of the other view, second segment empty
            s = [nxt, L, 0, 0]
        elif kind == "zero_first":     # the empty segment in front
            s = [nx2, 0, nxt, L]
        elif kind == "uneven":         # len0 != len1, both orders; the short one starts inside another item's rows
            sb = min(nx2 + 1, Rk - short)
            s = [nxt, L, sb, short] if b % 2 == 0 else [sb, short, nxt, L]
        elif kind == "twice":          # the same rows twice
            s = [b * L, L, b * L, L]
        elif kind == "overlap":        # long runs across item borders (no row twice within an item): key rows collect gradient from several items
            l0 = min(Rk, L + L // 2)
            s0 = min(b * (L // 2), Rk - l0)
            s = [s0, l0, s0 + l0, min(L // 4 + 1, Rk - s0 - l0)] if s0 + l0 < Rk else [s0, l0, 0, min(L // 4 + 1, s0)]
        else:
            raise ValueError(kind)
        seg.append(s)
    return seg


def _plant(qv, kv, dout, idx, probe_row, positions, H, scale, used, nvis, idx_is_rows=False):
    """Make key positions `positions` of the key list idx (idx_is_rows: key ROWS `positions`, wherever they are) dominant for query row probe_row: in every head, k = q * t / (scale |q|^2) with
    t = the natural logsumexp of the row's visible scores, i.e. one planted key weighs as much as everything the row saw before.  The
    probe row's dout is raised eightfold (once) so that its share of dq / dk / dv stands out of the tensor maximum the metric divides by."""
    rows = [r for r in positions if r not in used] if idx_is_rows else [int(idx[p]) for p in positions if int(idx[p]) not in used]
    if not rows:
        return
    qr = qv[probe_row].double().reshape(H, HD)
    kk = kv[idx[:nvis]].double().reshape(nvis, H, HD)
    t = torch.logsumexp(torch.einsum("hd,khd->hk", qr, kk) * scale, -1)                  # [H]
    n2 = (qr * qr).sum(-1)
    if float(n2.min()) == 0.0:
        return
    newk = (qr * (t / (scale * n2))[:, None]).reshape(H * HD).float()
    for r in rows:
        kv[r] = newk
        used.add(r)
    if ("dout", probe_row) not in used:
        dout[probe_row] *= 8.0
        used.add(("dout", probe_row))


def make_case(*, nbatch, H, Lq, Lk=None, mask="none", seg=None, regime="randn", scale=0.125, pad=0, nan_pad=False, seed=0, storage="f32"):
    """One seeded input set.  mask: "none" | "ragged" | "camera<T>"; seg: None or a make_segments kind (then Lk is Lq, the item length);
    regime: "randn" (score std ~ 1) | "peaked" (score std ~ 6: the running maximum moves in late key tiles) | "uniform" (randn plus one
    zero query per item -- uniform softmax, lse = log2 n exactly -- and, under a mask, one query whose visible keys are all identical);
    pad: extra rows per batch item in q / dout and (without segments) k / v, NaN-filled with nan_pad; storage: values are rounded to this
    type (returned as float32 tensors that hold exactly representable values).
    Returns a namespace: q, k, v, dout float32 [rows, H*64]; kw = the ABI keyword arguments (kv_seg / q_kvlen as int32 tensors or absent);
    max_keys; q_live / k_live bool row masks (rows of a batch item / rows some query attends to)."""
    Lk = Lq if Lk is None else Lk
    assert seg is None or Lk == Lq
    g = torch.Generator().manual_seed(seed)
    C = H * HD
    qbr, kbr = Lq + pad, Lk + (pad if seg is None else 0)
    Rq, Rk = nbatch * qbr, nbatch * kbr
    amp = math.sqrt(6.0) if regime == "peaked" else 1.0
    q = torch.randn(Rq, C, generator=g) * amp
    k = torch.randn(Rk, C, generator=g) * amp
    v = torch.randn(Rk, C, generator=g)
    dout = torch.randn(Rq, C, generator=g)
    kv_seg = make_segments(seg, nbatch, Lk, Rk) if seg is not None else None
    idxs = [key_rows(b, Lk=Lk, k_batch_rows=kbr, kv_seg=kv_seg) for b in range(nbatch)]
    nks = [int(i.numel()) for i in idxs]
    lens = None
    if mask == "ragged":
        lens = torch.stack([ragged_lens(1, Lq, nks[b], g)[0] for b in range(nbatch)])
    elif mask.startswith("camera"):
        lens = torch.stack([camera_lens(1, Lq, nks[b], int(mask[6:]))[0] for b in range(nbatch)])
    else:
        assert mask == "none", mask
    used: set = set()
    for b in range(nbatch):
        nk, idx, r0 = nks[b], idxs[b], b * qbr
        eff = lens[b].clamp(max=nk) if lens is not None else torch.full((Lq,), nk)
        rows = list(range(Lq))
        if regime == "uniform":
            u0 = Lq - 1
            q[r0 + u0] = 0.0
            rows.remove(u0)
            if lens is not None and Lq >= 2:
                n_same = min(24, nk)
                lens[b, Lq - 2] = n_same
                eff[Lq - 2] = n_same
                k[idx[:n_same]] = k[idx[0]].clone()
                used.update(int(r) for r in idx[:n_same])
                rows.remove(Lq - 2)
        full = [r for r in rows if int(eff[r]) == nk]
        if full:                   # the last key, one key of the first and of a middle 16-key tile: visible to an unmasked row only
            pos = sorted({nk - 1} | ({3, (nk // 32) * 16 + 5} if nk > 32 else set()))
            _plant(q, k, dout, idx, r0 + full[0], pos, H, scale, used, nk)
            if kv_seg is not None:  # the row an empty segment points at: a kernel that reads one key of it must move the result
                for sb, sl in ((kv_seg[b][0], kv_seg[b][1]), (kv_seg[b][2], kv_seg[b][3])):
                    if sl == 0 and len(full) > 1 and sb not in used:
                        _plant(q, k, dout, idx, r0 + full[1], [sb], H, scale, used, nk, idx_is_rows=True)
        seen = set()
        for r in rows:             # masked rows with prefix > 16: the last visible key and the first hidden one
            n = int(eff[r])
            if 16 < n < nk and n not in seen and len(seen) < 4:
                seen.add(n)
                _plant(q, k, dout, idx, r0 + r, [n - 1, n], H, scale, used, n)
    dt = STORAGE[storage]
    q, k, v, dout = (t.to(dt).float() for t in (q, k, v, dout))
    q_live = torch.zeros(Rq, dtype=torch.bool)
    k_live = torch.zeros(Rk, dtype=torch.bool)
    for b in range(nbatch):
        q_live[b * qbr:b * qbr + Lq] = True
        k_live[idxs[b]] = True
    if nan_pad:
        q[~q_live] = float("nan")
        dout[~q_live] = float("nan")
        k[~k_live] = float("nan")
        v[~k_live] = float("nan")
    kw = dict(nbatch=nbatch, H=H, Lq=Lq, q_batch_rows=qbr, scale=scale)
    if kv_seg is None:
        kw.update(Lk=Lk, k_batch_rows=kbr)
    else:
        kw.update(kv_seg=torch.tensor(kv_seg, dtype=torch.int32))
    if lens is not None:
        kw.update(q_kvlen=lens.to(torch.int32).reshape(-1).contiguous())
    return SimpleNamespace(q=q, k=k, v=v, dout=dout, kw=kw, max_keys=max(nks) if kv_seg is not None else 0, q_live=q_live, k_live=k_live,
                           nks=nks, storage=storage)


def rel(a, b):
    """The suite's metric: max |a - b| over max |b|."""
    a, b = a.double(), b.double().to(a.device)
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


# Per storage class: (forward out, lse [log2 units], backward dq / dk / dv) -- the project's bounds (tests/test_ops_gpu.py,
# test_split_path_gpu.py, test_split_bwd_gpu.py, test_f32_path_gpu.py); the 16-bit lse entries are the derived ceilings 2^-11 / ln 2 and
# 2^-8 / ln 2 that the asserted lse bound may never exceed.
TOLERANCES = {"f16": (3e-3, 2.0 ** -11 / LN2, 6e-3), "bf16": (2e-2, 2.0 ** -8 / LN2, 3e-2), "f32": (6e-6, 1e-4, 1e-5)}

# lse of the 16-bit classes: largest |lse - float64 lse| (log2 units) measured on MI355X over every case of
# tests/test_attention_routes_gpu.py (f16: fam-L257-plain_peaked, bf16: fam-L257-seg_uneven_peaked).  The kernels keep scores, running
# maximum and row sum in f32, so the deviation is f32 round-off of a value of size ~ 50, two orders below the derived ceiling.  Asserted:
# 4 x the measured maximum, never above one storage rounding of the row sum (TOLERANCES[...][1]).
LSE16_MEASURED = {"f16": 5.62e-6, "bf16": 5.69e-6}
LSE16_BOUND = {c: min(4 * LSE16_MEASURED[c], TOLERANCES[c][1]) for c in LSE16_MEASURED}
