"""The distillation teacher without a GPU: the float64 restatement (tests/teacher_f64.py) against the REAL reference's float64 run
(tests/golden/teacher_tiny.npz), the mutants that restatement must tell apart, the module's state_dict, what it refuses, the new header,
the anchor sampler and the loss keyword.

Criterion of the restatement: per output (pts3d and conf of both views), max |restatement f64 - fixture f64| / max |fixture f64| must be
below 1e-3 of the reference's own f32 - f64 difference, normalised the same way (stored in the fixture: 1.3e-6, 4.5e-7, 2.3e-6, 2.2e-6).
Measured: 0.0 for all four outputs and for all 26 block checksums -- the restatement repeats the reference's float64 arithmetic bit for bit
on this input (the f32-formed RoPE angles included).

Mutants, each rejected by that bound (measured max over the four outputs, bound <= 2.4e-9): norm_y dropped 3e14, the key side of the
cross-attention not rotated 1.2e-1, dec_blocks2 replaced by dec_blocks 5.9, branch 2 reading the current step's branch 1 2.8, hook 6
moved to 5 2.9e-1, dec_norm on one branch only 6.2e-1.  "Query and key positions swapped in the cross-attention RoPE" cannot be rejected by
any input: the two views of a call share one patch grid, so the two position tables are equal and the swap is the identity; the test
asserts exactly that (bit-equal outputs) and rejects the neighbouring mistake, the key side left unrotated, instead.
The tail's mutants are f32 mistakes (in float64 exp(d) - 1 at d = 1e-6 is good to 1e-10) and are judged as a kernel is, in f32 by the GPU
test's criterion 4 max(r32, 1) 2^-24 mag: exp(d) - 1 on a d = 1e-6 input (no transform: behind a transform the translation's magnitude
covers so small a point) and conf without the + 1 miss it by factors of a thousand and more (`-s` prints the units; the single-pixel shape
holds the zero vector alone and shows neither).  conf without the + 1 is a mistake in any dtype and is ALSO rejected by the fixture's bound:
the restatement's float64 confidences without it are 0.30 / 0.24 of max |f64| away from the fixture's (bounds 4.5e-10 / 2.2e-9).

r32, the torch-f32 composition's own ratio on the GPU test's inputs (`-s` prints it per case): 44.0 to 44.4 units of 2^-24 mag wherever the
d = 88 edge is planted, where half an f32 step of d alone moves expm1(d) by 44 units; 0 on the single-pixel shape (the zero vector).
"""
import json
import os

import numpy as np
import pytest
import torch

import teacher_f64 as T

G = os.path.join(os.path.dirname(__file__), "golden")
OUTS = (("pts1", 0, "pts3d"), ("conf1", 0, "conf"), ("pts2", 1, "pts3d"), ("conf2", 1, "conf"))


@pytest.fixture(scope="module")
def fixture():
    from vicasplat_amd.synthetic import golden_weights
    z = np.load(os.path.join(G, "teacher_tiny.npz"))
    W = golden_weights(json.load(open(os.path.join(G, "shapes_teacher_tiny.json"))), seed=int(z["cfg_seed"]))
    img = T.teacher_input(int(z["cfg_B"]), int(z["cfg_H"]), int(z["cfg_W"]), int(z["cfg_seed"]))
    return z, W, img


def _errs(z, res):
    return {k: float(np.abs(res[v][f].numpy() - z["f64_" + k]).max() / np.abs(z["f64_" + k]).max()) for k, v, f in OUTS}


def _bounds(z):
    return {k: 1e-3 * float(z["ref_err_" + k]) for k, _, _ in OUTS}


def test_restatement_meets_the_reference_float64(fixture):
    z, W, img = fixture
    sums = {}
    res = T.teacher_forward(W, img, T.TINY["enc_num_heads"], T.TINY["dec_num_heads"], torch.float64,
                            probe=lambda n, t: sums.__setitem__(n, T.checksum(t).numpy()))
    errs, bounds = _errs(z, res), _bounds(z)
    names = [str(n) for n in z["f64_block_names"]]
    drift = max(float(np.abs(sums[n] - row).max() / row[1]) for n, row in zip(names, z["f64_blocks"]))
    print("restatement f64 vs reference f64:", errs, "bounds", bounds, "worst block checksum", drift)
    assert len(names) == T.TINY["enc_depth"] + 2 * T.TINY["dec_depth"] and set(names) == set(sums)
    for k in errs:
        assert 0 < bounds[k] and errs[k] <= bounds[k], (k, errs[k], bounds[k])
    assert drift <= max(bounds.values())
    # what the fixture records about itself: magnitudes below the saturation of expm1 (d = 88.7), the reference's own f32 error
    assert all(float(z["mag_" + k]) < 1e3 for k, _, _ in OUTS) and all(1e-8 < float(z["ref_err_" + k]) < 1e-5 for k, _, _ in OUTS)


@pytest.mark.parametrize("mutant", [m for m in T.MUTANTS if m != "swap_cross_pos"])
def test_network_mutants_are_rejected(fixture, mutant):
    z, W, img = fixture
    errs, bounds = _errs(z, T.teacher_forward(W, img, 2, 1, torch.float64, mutant=mutant)), _bounds(z)
    print(mutant, errs)
    assert any(errs[k] > bounds[k] for k in errs), (mutant, errs)
    assert max(errs.values()) > 1e3 * max(bounds.values()), (mutant, errs)      # and not by a hair


def test_conf_without_the_plus_one_is_rejected_by_the_fixture_bound(fixture):
    z, W, img = fixture
    res = T.teacher_forward(W, img, 2, 1, torch.float64)
    bounds = _bounds(z)
    for v, k in ((0, "conf1"), (1, "conf2")):
        assert torch.equal(T.tail(res[v]["raw"])["conf"], res[v]["conf"])
        m = T.tail(res[v]["raw"], mutant="conf_no_plus_1")["conf"]
        e = float(np.abs(m.numpy() - z["f64_" + k]).max() / np.abs(z["f64_" + k]).max())
        print(k, "without the + 1:", e, "bound", bounds[k])
        assert e > 1e3 * bounds[k]


def test_swapped_cross_positions_cannot_be_seen_on_a_shared_grid(fixture):
    """Both views of a call have one image size, so the query's and the key's position tables are the same table: handing each side the
    other's is the identity.  (The mistake next to it that CAN be seen, the key side not rotated, is among the rejected mutants.)"""
    z, W, img = fixture
    a = T.teacher_forward(W, img, 2, 1, torch.float64)
    b = T.teacher_forward(W, img, 2, 1, torch.float64, mutant="swap_cross_pos")
    for v in (0, 1):
        assert torch.equal(a[v]["raw"], b[v]["raw"])


CASES = [(n, H, W, dt, tr) for (n, H, W) in ((1, 1, 1), (3, 3, 5), (2, 16, 65)) for dt in (torch.float32, torch.float16) for tr in (False, True)]


@pytest.mark.parametrize("n,H,W,dtype,with_transform", CASES)
def test_tail_torch_f32_ratio_and_mutants(n, H, W, dtype, with_transform):
    """r32 on the inputs of tests/test_teacher_points_gpu.py, and the tail's two mutants against that test's criterion."""
    raw = T.tail_edge_input(n, H, W, dtype, seed=n * 100 + W)
    tr = T.tail_transforms(n, seed=W) if with_transform else None
    ref = T.tail(raw.double(), None if tr is None else tr.double(), f32_overflow=True)
    assert not torch.isnan(ref["pts"]).any() and not torch.isnan(ref["conf"]).any()
    p32, c32 = T.tail_torch_f32(raw, tr)
    r32 = T.tail_ratio(p32, c32, ref)
    print(f"tail n={n} {H}x{W} {str(dtype)[6:]} transform={with_transform}: torch f32 {r32:.3f} units of 2^-24 mag")
    assert r32 < 100      # the composition is an f32 evaluation: at d = 88 half an f32 step of d moves expm1(d) by 44 units, a few more follow
    lim = 4 * max(r32, 1.0)
    if H * W >= 8:
        m = T.tail(raw.float(), tr, mutant="conf_no_plus_1")
        assert T.tail_ratio(m["pts"], m["conf"], ref) > 1e3 * lim
        # exp(d) - 1 shows where the issue plants it: at d = 1e-6 (f32 and f16 input), the point itself the output (behind a transform the
        # translation's magnitude covers the error of so small a point, and the criterion rightly lets it pass)
        if tr is None:
            m = T.tail(raw.float(), tr, mutant="exp_minus_1")
            u = T.tail_ratio(m["pts"], m["conf"], ref)
            print(f"    exp(d) - 1 in f32: {u:.3g} units, bound {lim:.3g}")
            assert u > 100 * lim
    # float64 rounded once to f32 (what the kernel does): half an f32 step of the value, at most one unit of 2^-24 mag
    assert T.tail_ratio(ref["pts"].float(), ref["conf"].float(), ref) <= 1.0


def test_tail_zero_and_small_distances():
    raw = torch.zeros(1, 1, 3, 4, dtype=torch.float64)
    raw[0, 0, 1, :3] = torch.tensor([6e-7, 0.0, -8e-7], dtype=torch.float64)
    raw[0, 0, 2, 3] = -float("inf")
    t = T.tail(raw)
    assert bool((t["pts"][0, 0, 0] == 0).all()) and float(t["conf"][0, 0, 2]) == 1.0 and float(t["conf"][0, 0, 0]) == 2.0
    d = 1e-6
    assert abs(float(t["pts"][0, 0, 1].norm()) / np.expm1(d) - 1) < 1e-12
    # exp(d) - 1 in f32 at d = 1e-6: an error of percents, where expm1 is good to an f32 rounding
    e = T.tail(raw.float(), mutant="exp_minus_1")["pts"][0, 0, 1].double().norm() / np.expm1(d) - 1
    assert abs(float(e)) > 1e-3


def test_state_dict_is_the_reference_abi():
    from vicasplat_amd.model.distiller import DUST3R_SHAPE, Dust3R
    for name, cfg in (("tiny", T.TINY), ("full", DUST3R_SHAPE)):
        with torch.device("meta"):
            m = Dust3R(**cfg)
        sd = {k: list(v.shape) for k, v in m.state_dict().items()}
        assert sd == json.load(open(os.path.join(G, f"shapes_teacher_{name}.json"))), name
        assert not m.training and not any(p.requires_grad for p in m.parameters())
        assert not m.train().training      # stays in eval mode
    names = {k.split(".")[0] for k in sd}
    assert names == {"mask_token", "patch_embed", "enc_blocks", "enc_norm", "decoder_embed", "dec_blocks", "dec_blocks2", "dec_norm",
                     "downstream_head1", "downstream_head2"}
    blk = {k[len("dec_blocks2.0."):].rsplit(".", 1)[0] for k in sd if k.startswith("dec_blocks2.0.")}
    assert blk == {"norm1", "attn.qkv", "attn.proj", "norm2", "norm3", "norm_y", "cross_attn.projq", "cross_attn.projk", "cross_attn.projv",
                   "cross_attn.proj", "mlp.fc1", "mlp.fc2"}


def test_checkpoint_without_the_second_decoder_loads_strictly(fixture):
    from vicasplat_amd.model.distiller import Dust3R
    _, W, _ = fixture
    m = Dust3R(**T.TINY)
    half = {k: v for k, v in W.items() if not k.startswith("dec_blocks2.")}
    assert len(half) < len(W)
    m.load_state_dict(half, strict=True)
    sd = m.state_dict()
    for k in sd:
        if k.startswith("dec_blocks2."):
            assert torch.equal(sd[k], W[k.replace("dec_blocks2", "dec_blocks")]), k
    m.load_state_dict(W, strict=True)
    assert torch.equal(m.state_dict()["dec_blocks2.3.mlp.fc1.weight"], W["dec_blocks2.3.mlp.fc1.weight"])
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in W.items() if k != "dec_norm.weight"}, strict=True)


def test_checkpoint_file_with_its_training_arguments_loads(fixture, tmp_path):
    """The published checkpoints hold {'args': argparse.Namespace, 'model': state_dict, ...}: the loader reads them with the weights-only
    unpickler (that one class admitted) and refuses a file that smuggles in anything else."""
    import argparse
    from vicasplat_amd.model.distiller import Dust3R, load_checkpoint
    _, W, _ = fixture
    path = str(tmp_path / "teacher.pth")
    torch.save({"args": argparse.Namespace(model="AsymmetricCroCo3DStereo(...)", lr=1e-4), "model": W, "epoch": 3}, path)
    m = load_checkpoint(Dust3R(**T.TINY), path)
    sd = m.state_dict()
    assert all(torch.equal(sd[k], W[k]) for k in W) and not any(p.requires_grad for p in m.parameters())
    torch.save({"args": T.checksum, "model": W}, path)      # a function object: not admitted
    with pytest.raises(Exception, match="(?i)weights_only|unsupported|global"):
        load_checkpoint(Dust3R(**T.TINY), path)


def test_what_the_teacher_refuses():
    from vicasplat_amd.model.distiller import Dust3R, get_distiller
    with pytest.raises(NotImplementedError, match="mast3r"):
        get_distiller("mast3r")
    with pytest.raises(ValueError):
        get_distiller("croco")
    m = Dust3R(**T.TINY)
    ctx = dict(image=torch.zeros(1, 2, 3, 32, 32))
    with pytest.raises(NotImplementedError, match="symmetrize_batch"):
        m(ctx, symmetrize_batch=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(ctx)
    with pytest.raises(ValueError, match="operand class"):
        m.set_compute_dtype(torch.bfloat16)
    with pytest.raises(NotImplementedError, match="head_dim 64"):
        Dust3R(**dict(T.TINY, dec_embed_dim=96))


def test_teacher_header_parses_with_its_prefix():
    from vicasplat_amd import _lib
    inc = os.path.join(os.path.dirname(__file__), "..", "include")
    sigs = _lib.parse_header(open(os.path.join(inc, "vicasplat_teacher.h")).read(), prefix="vst_")
    assert set(sigs) == {"vst_points_conf"}
    restype, argtypes, takes_stream = sigs["vst_points_conf"]
    assert len(argtypes) == 9 and takes_stream
    L = _lib.lib()
    # null pointers and bad sizes come back as an error code with a message, not as a crash
    assert L.vst_points_conf(None, 0, None, 1, 1, 1, None, None, None) < 0 and b"vst_points_conf" in L.vs_last_error()


def test_sample_anchor_frames_draws_what_the_reference_draws():
    from vicasplat_amd import callers
    z = np.load(os.path.join(G, "teacher_anchors.npz"))
    for b in (1, 3):
        for v, tc in ((2, 1), (5, 1), (8, 1), (5, 4), (8, 4)):
            frames = torch.arange(b * v, dtype=torch.float32).reshape(b, v, 1, 1, 1)
            np.random.seed(100 * b + v)
            anchors, idx, seg = callers.sample_anchor_frames(frames, temporal_compression=tc, n_frames=2)
            tag = f"B{b}_V{v}_tc{tc}"
            assert idx.dtype == torch.int64 and np.array_equal(idx.numpy(), z[tag + "_idx"]), tag
            assert np.array_equal(seg.numpy(), z[tag + "_segment_idx"]) and np.array_equal(anchors.reshape(b, 2).numpy(), z[tag + "_anchors"]), tag
            assert bool((seg[:, 1] == seg[:, 0] + 1).all()) and int(idx.min()) >= 0 and int(idx.max()) < v      # adjacent segments, in range
    with pytest.raises(ValueError, match="two frames"):
        callers.sample_anchor_frames(torch.zeros(1, 12, 1, 1, 1))      # 3 segments of 4 frames and no n_frames


def test_points_already_in_the_first_frame_skip_the_einsum():
    from vicasplat_amd import callers
    g = torch.Generator().manual_seed(3)
    B, V, H, W = 2, 3, 6, 7
    out = dict(gaussian_centers=torch.randn(B, V, H, W, 3, generator=g), confidence=1 + torch.rand(B, V, H, W, generator=g))
    gt = [dict(pts3d=torch.randn(B, H, W, 3, generator=g) + torch.tensor([0.0, 0.0, 2.0]), conf=1 + torch.rand(B, H, W, generator=g)) for _ in (0, 1)]
    E = torch.eye(4).repeat(B, V, 1, 1)
    q, _ = torch.linalg.qr(torch.randn(B, V, 3, 3, generator=g))
    E[..., :3, :3], E[..., :3, 3] = q, torch.randn(B, V, 3, generator=g)
    frame_idx = segment_idx = torch.tensor([[1, 2], [0, 1]])
    fn = callers.Regr3D(backend="torch")
    base = callers.distillation_loss(out, gt[0], gt[1], frame_idx, segment_idx, E, 0.5, fn)
    Ea = E[torch.arange(B), frame_idx[:, 0]]
    moved = [dict(pts3d=torch.einsum("bij,bhwj->bhwi", Ea[:, :3, :3], g_["pts3d"]) + Ea[:, None, None, :3, 3], conf=g_["conf"]) for g_ in gt]
    pre = callers.distillation_loss(out, moved[0], moved[1], frame_idx, segment_idx, E, 0.5, fn, pts_in_first_frame=True)
    assert torch.equal(base, pre)
    assert not torch.equal(base, callers.distillation_loss(out, gt[0], gt[1], frame_idx, segment_idx, E, 0.5, fn, pts_in_first_frame=True))
