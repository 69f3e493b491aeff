"""The HIP view-overlap counts (csrc/overlap.hip behind geometry.epipolar_lines.view_overlap_counts) against the float64 restatement of
tests/overlap_f64.py and the real reference's counts in tests/golden/view_overlap.npz, and EvaluationIndexGenerator.test_step on the
device against the reference's index.  -m gpu.

Sizes 1 x 1, 1 x 7, 7 x 1, 16 x 16, 17 x 23 (a partial last wave), 32 x 48; the cases of overlap_f64 (the 16-frame trajectory with all ordered
pairs, identical cameras and i = j, a pure rotation with bit-equal positions, cameras facing away, forward motion, a sideways pair with
o_z exactly 0, K_i != K_j, a non-rigid extrinsic, a NaN camera among finite ones, an origin 1e-5 and one 1e-6 from the other camera, and
the exact-edge pair whose frame-line coordinate IS the f32 bound: held to the reference's f32 counts bit for bit); f32 and f64 inputs.
Criterion: every count in [sure, sure + ambiguous] of the restatement; equal to the reference's f64 count wherever a pair has no ambiguous ray.
Measured on an MI355X (`-s` prints it per case): every count of every case, f32 and f64 inputs, 0 rays from the reference's count.
"""
import numpy as np
import pytest
import torch

import overlap_f64 as O

pytestmark = pytest.mark.gpu
G = O.golden()
CASES = O.cases(G)
SENTINEL = -12345
_REF = {}


def _dev():
    return torch.device("cuda:0")


def _reference(name, h, w):
    """(E, K, pairs, sure, ambiguous, the reference's f64 counts) of one case and size; computed once and shared."""
    if (name, h, w) not in _REF:
        _, E, K, pairs, key, sl = next(c for c in CASES if c[0] == name)
        _, sure, amb = O.counts(E, K, h, w, pairs)
        _REF[(name, h, w)] = (E, K, pairs, sure, amb, G[f"{key}_ref64_{h}x{w}"][sl])
    return _REF[(name, h, w)]


def _run(E, K, shape, pairs, dtype=torch.float32):
    from vicasplat_amd.geometry.epipolar_lines import view_overlap_counts
    out = view_overlap_counts(torch.tensor(E, dtype=dtype, device=_dev()), torch.tensor(K, dtype=dtype, device=_dev()), shape,
                              torch.tensor(pairs, dtype=torch.int32, device=_dev()).reshape(-1, 2))
    assert out.dtype == torch.int32 and out.is_cuda
    return out.cpu().numpy()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_counts_against_the_restatement_and_the_reference(name, dtype):
    worst = 0
    for h, w in O.SIZES:
        E, K, pairs, sure, amb, ref = _reference(name, h, w)
        got = _run(E, K, (h, w), pairs, dtype)
        if name == "edge":      # exact in f32 only: its c_y is the f32 bound; held to the reference's own f32 counts, bit for bit
            if dtype == torch.float32:
                assert np.array_equal(got, G[f"spec_ref32_{h}x{w}"][-2:]), (h, w, got)
            continue
        assert ((got >= sure) & (got <= sure + amb)).all(), (name, h, w, got, sure, amb)
        assert np.array_equal(got[amb == 0], ref[amb == 0]), (name, h, w)
        worst = max(worst, int(np.abs(got - ref).max()))
    print(f"{name} {dtype}: at most {worst} rays from the reference's count")
    if name == "identical":
        assert (got == 32 * 48).all()
    if name == "away":
        assert (got == 0).all()


def test_pair_lists_sentinel_and_guards():
    """P in {0, 1, 2, 480}, repeated and shuffled pairs, an out-of-range index, counts inside a guarded buffer at an aligned and at a
    misaligned offset, two runs, a pair alone against the same pair in a batch."""
    from vicasplat_amd import _lib as L
    h, w = 17, 23
    E, K, pairs, sure, amb, ref = _reference("trajectory", h, w)
    g = np.random.default_rng(0)
    order = g.permutation(np.concatenate([np.arange(256), g.integers(0, 256, 224)]))       # 480 pairs, repeats, shuffled
    big = np.array(pairs)[order]
    got = _run(E, K, (h, w), big)
    assert ((got >= sure[order]) & (got <= sure[order] + amb[order])).all() and np.array_equal(got, _run(E, K, (h, w), big))
    full = _run(E, K, (h, w), pairs)
    assert np.array_equal(got, full[order])
    for k in (3, 100):
        assert _run(E, K, (h, w), [pairs[k]])[0] == full[k]
    assert np.array_equal(_run(E, K, (h, w), pairs[5:7]), full[5:7])
    bad = np.array([pairs[9], (16, 0), pairs[10], (0, -1), pairs[11]])
    assert _run(E, K, (h, w), bad).tolist() == [full[9], -1, full[10], -1, full[11]]
    assert _run(E, K, (h, w), np.zeros((0, 2))).shape == (0,)
    # the raw entry on a guarded buffer
    Ed, Kd = torch.tensor(E, dtype=torch.float32, device=_dev()), torch.tensor(K, dtype=torch.float32, device=_dev())
    prs = torch.tensor(big, dtype=torch.int32, device=_dev())
    for offset in (64, 67):
        buf = torch.full((offset + 480 + 64,), SENTINEL, dtype=torch.int32, device=_dev())
        L.call("vso_view_overlap_counts", _dev(), L.ptr(Ed), L.ptr(Kd), 0, 16, h, w, L.ptr(prs), 480, L.ptr(buf[offset:]))
        out = buf.cpu().numpy()
        assert (out[:offset] == SENTINEL).all() and (out[offset + 480:] == SENTINEL).all() and np.array_equal(out[offset:offset + 480], got)


def test_a_nan_camera_among_finite_ones():
    """The NaN camera's pairs inside a list of finite pairs: theirs is what IEEE gives (no comparison with a NaN holds: 0), and every finite
    pair keeps the count it has alone."""
    h, w = 17, 23
    E, K, named = O.special()
    finite = named["other_k"] + named["scaled"] + named["forward"]
    mixed = finite[:3] + [named["nan"][0]] + finite[3:6] + [named["nan"][1]] + finite[6:]
    got = _run(E, K, (h, w), mixed)
    alone = _run(E, K, (h, w), finite)
    assert got[3] == 0 and got[7] == 0 and np.array_equal(np.delete(got, [3, 7]), alone)
    for k, pair in enumerate(finite):
        assert _run(E, K, (h, w), [pair])[0] == alone[k]


def test_more_than_one_chunk_per_pair():
    """64 x 64 = two chunks of VSO_CHUNK rays per pair: the atomics of both land on the pair's count."""
    from vicasplat_amd import _lib as L
    from vicasplat_amd.geometry.epipolar_lines import view_overlap_counts
    assert 64 * 64 == 2 * L.VSO_CHUNK
    E, K, pairs = G["traj_E"], G["traj_K"], O.all_pairs(16)[::5]
    got = _run(E, K, (64, 64), pairs)
    want = view_overlap_counts(torch.tensor(E).float(), torch.tensor(K).float(), (64, 64), torch.tensor(pairs), backend="torch").numpy()
    _, sure, amb = O.counts(E, K, 64, 64, pairs)
    assert ((got >= sure) & (got <= sure + amb)).all() and ((want >= sure) & (want <= sure + amb)).all()


def test_no_synchronisation_graph_capture_and_the_mean():
    from vicasplat_amd.geometry.epipolar_lines import overlap_from_counts, view_overlap, view_overlap_counts
    h, w = 17, 23
    E, K, pairs, *_ = _reference("trajectory", h, w)
    Ed, Kd = torch.tensor(E, dtype=torch.float32, device=_dev()), torch.tensor(K, dtype=torch.float32, device=_dev())
    prs = torch.tensor(pairs, dtype=torch.int32, device=_dev())
    eager = view_overlap_counts(Ed, Kd, (h, w), prs)          # (also loads the library before the detector is armed)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = view_overlap_counts(Ed, Kd, (h, w), prs)
        share = view_overlap(Ed, Kd, (h, w), prs)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(again, eager) and share.dtype == torch.float32
    # counts / N exactly as torch's own mean of the flags gives it on the device
    flags = torch.arange(h * w, device=_dev())[None] < eager[:, None]
    assert torch.equal(share, torch.stack([f.float().mean() for f in flags]))
    assert torch.equal(overlap_from_counts(eager, h * w), share)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        view_overlap_counts(Ed, Kd, (h, w), prs)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = view_overlap_counts(Ed, Kd, (h, w), prs)
    out.fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_generator_on_the_device_reproduces_the_reference_index(tmp_path):
    gen, text = O.run_generator(G, tmp_path, None, _dev())
    assert text == str(G["index_json"])
