"""The HIP trajectory metrics (csrc/trajectory.hip behind ops.trajectory_metrics / callers.camera_eval_metrics) against the float64
restatement of tests/trajectory_f64.py.  -m gpu.

Shapes: V = 1, 2 (degenerate by construction), 3, 4, 8, 9, 64 (one pose per lane), 65 (the first second trip), 130 (three trips);
B = 1 and B = 5 with degenerate and valid scenes mixed in one batch; delta = 1, 3; f64 and f32 inputs (f32: against the restatement run on
the same values promoted).  Inputs: every family of trajectory_f64.families / degenerate_families -- random walks with perturbed poses
under a random similarity, the closed-form square (repeated singular values and a zero one), planar walks (V = 3 is always planar), the
reflection, the exact similarity near and 1e3 away from the origin, the estimate bit-equal to the truth, positions on a coordinate axis, a
NaN and an inf element.  No case is exempted from any comparison.

Criterion: valid equal to the restatement's; every output within 4 max(R64, 1) 2^-52 mag of it (trajectory_f64.R64 per output: 4 units
for the three metrics, 35.6 for R, 8 for t, 13.6 for c, in units of their magnitudes); R orthonormal with det +1; degenerate scenes
exactly 0 with the identity alignment; two runs bit-equal; a scene alone bit-equal to the same scene inside a batch.
Measured on an MI355X, max |gpu - ref| / (2^-52 mag) over all cases (`-s` prints it per V):

    output      R64     bound   gpu
    ate         0.617   4.0     0.66
    rpe_trans   0.577   4.0     0.94
    rpe_rot     0.279   4.0     2.23
    R           8.881   35.6    5.50
    t           1.928   8.0     1.87
    c           3.365   13.6    4.42
    R R^T - I (units of 2^-52): 5.0, against the 16 allowed
"""
import numpy as np
import pytest
import torch

import trajectory_f64 as T

pytestmark = pytest.mark.gpu

VS = (1, 2, 3, 4, 8, 9, 64, 65, 130)
# R is built from two orthonormal triples, each orthogonal to the Jacobi threshold 2^-52 and normalised by a rounded division: a few units
# per entry of R R^T; 16 leaves room for the six products behind an entry
ORTHO_UNITS = 16.0
IDENTITY = np.concatenate([np.eye(3).ravel(), np.zeros(3), [1.0]])


def _dev():
    return torch.device("cuda:0")


def _run(P, Q, delta, dtype=torch.float64):
    """ops.trajectory_metrics on the device -> (metrics [B, 3], valid [B], align [B, 13]) as numpy."""
    from vicasplat_amd import ops
    p, q = torch.tensor(P, dtype=dtype, device=_dev()), torch.tensor(Q, dtype=dtype, device=_dev())
    m, v, a = ops.trajectory_metrics(p, q, delta, return_alignment=True)
    assert m.dtype == torch.float64 and v.dtype == torch.int32 and a.dtype == torch.float64
    return m.cpu().numpy(), v.cpu().numpy(), a.cpu().numpy()


_REF = {}


def _reference(name, V, delta, f32):
    """(P, Q, ref) of one case; computed once and shared."""
    key = (name, V, delta, f32)
    if key not in _REF:
        fam = T.degenerate_families(V)
        if V >= 3:
            fam.update(T.families(V))
        P, Q = fam[name]
        if f32:
            P, Q = P.astype(np.float32).astype(np.float64), Q.astype(np.float32).astype(np.float64)
        _REF[key] = (P, Q, T.metrics(P, Q, delta))
    return _REF[key]


def _names(V):
    return list(T.degenerate_families(V)) + (list(T.families(V)) if V >= 3 else [])


def _check_scene(m, v, a, ref, tag, worst):
    assert v == ref[1], (tag, v, ref[3])
    if not ref[1]:
        assert not m.any() and np.array_equal(a, IDENTITY), (tag, m, a)
        return
    assert T.well_posed(ref), (tag, ref[3])
    R, t, c = a[:9].reshape(3, 3), a[9:12], a[12]
    u = [T.units(m[k], ref[0][k], ref[4][k]) for k in range(3)] + list(T.alignment_units(R, t, c, ref))
    for k, n in enumerate(T.OUTPUTS):
        worst[n] = max(worst.get(n, 0.0), u[k])
    ortho = float(np.abs(R @ R.T - np.eye(3)).max() / T.EPS)
    worst["ortho"] = max(worst.get("ortho", 0.0), ortho)
    assert np.isfinite(m).all() and np.isfinite(a).all(), tag
    for k, n in enumerate(T.OUTPUTS):
        assert u[k] <= T.gpu_factor(n), (tag, n, u[k])
    assert ortho <= ORTHO_UNITS and abs(np.linalg.det(R) - 1.0) <= ORTHO_UNITS * T.EPS, (tag, ortho, np.linalg.det(R))


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("delta", [1, 3])
@pytest.mark.parametrize("V", VS)
def test_every_family_alone_and_in_a_batch(V, delta, f32):
    """Each family as a batch of one, then five of them -- degenerate and valid mixed -- as one batch: the same bits."""
    dtype = torch.float32 if f32 else torch.float64
    worst, alone = {}, {}
    names = _names(V)
    for name in names:
        P, Q, ref = _reference(name, V, delta, f32)
        finite = bool(np.isfinite(P).all() and np.isfinite(Q).all())
        assert ref[1] == 1 or T.plainly_degenerate(ref, V, delta, finite), (name, V, delta, ref[3])
        m, v, a = _run(P[None], Q[None], delta, dtype)
        _check_scene(m[0], v[0], a[0], ref, (name, V, delta, f32), worst)
        alone[name] = (m[0], v[0], a[0])
    mixed = ([n for n in names if n in ("walk", "planar", "reflection", "square", "exact_far")][:3] + ["axis", "nan"])
    mixed = [mixed[i] for i in (0, 3, 1, 4, 2)] if len(mixed) == 5 else (mixed * 5)[:5]       # valid and degenerate scenes interleaved
    Pb = np.stack([_reference(n, V, delta, f32)[0] for n in mixed])
    Qb = np.stack([_reference(n, V, delta, f32)[1] for n in mixed])
    m, v, a = _run(Pb, Qb, delta, dtype)
    m2, v2, a2 = _run(Pb, Qb, delta, dtype)
    assert np.array_equal(m, m2, equal_nan=True) and np.array_equal(v, v2) and np.array_equal(a, a2, equal_nan=True)      # two runs: the same bits
    for k, n in enumerate(mixed):
        assert np.array_equal(m[k], alone[n][0]) and v[k] == alone[n][1] and np.array_equal(a[k], alone[n][2]), (n, V, delta, f32)
    print(f"trajectory V={V} delta={delta} {'f32' if f32 else 'f64'}", {k: round(x, 3) for k, x in worst.items()})


def test_closed_form_square_on_the_device():
    P, Q = T.square_case()
    m, v, a = _run(P[None], Q[None], 1)
    mag = T.metrics(P, Q)[4]
    assert v[0] == 1 and max(T.units(m[0, k], T.SQUARE["out"][k], mag[k]) for k in range(3)) <= 4.0, m
    assert T.units(a[0, :9].reshape(3, 3), np.eye(3), 1.0) <= T.gpu_factor("R") and T.units(a[0, 12], T.SQUARE["c"], T.SQUARE["c"]) <= T.gpu_factor("c")


def test_no_alignment_buffer_and_empty_batch():
    from vicasplat_amd import ops
    P, Q, ref = _reference("walk", 9, 1, False)
    p, q = torch.tensor(P[None], device=_dev()), torch.tensor(Q[None], device=_dev())
    m, v = ops.trajectory_metrics(p, q)
    m3, v3, _ = ops.trajectory_metrics(p, q, return_alignment=True)
    assert torch.equal(m, m3) and torch.equal(v, v3)
    m0, v0, a0 = ops.trajectory_metrics(p[:0], q[:0], return_alignment=True)
    assert m0.shape == (0, 3) and v0.shape == (0,) and a0.shape == (0, 13)
    # delta >= V through the wrapper: every scene degenerate
    m, v = ops.trajectory_metrics(p, q, delta=9)
    assert int(v[0]) == 0 and not m.any()
    m, v = ops.trajectory_metrics(p, q, delta=8)
    assert int(v[0]) == 1 and T.units(m[0].cpu().numpy(), T.metrics(P, Q, 8)[0], ref[4]) <= 4.0


def test_wrapper_checks():
    from vicasplat_amd import ops
    p = torch.eye(4, device=_dev(), dtype=torch.float64).repeat(2, 5, 1, 1)
    with pytest.raises(ValueError, match=r"\[B, V, 4, 4\]"):
        ops.trajectory_metrics(p[0], p[0])
    with pytest.raises(ValueError, match="ground truth of shape"):
        ops.trajectory_metrics(p, p[:, :4])
    with pytest.raises(ValueError, match="one dtype"):
        ops.trajectory_metrics(p, p.float())
    with pytest.raises(ValueError, match="f32 or f64"):
        ops.trajectory_metrics(p.half(), p.half())
    with pytest.raises(ValueError, match="contiguous"):
        ops.trajectory_metrics(p.transpose(-1, -2), p.transpose(-1, -2))
    with pytest.raises(ValueError, match="delta"):
        ops.trajectory_metrics(p, p, delta=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.trajectory_metrics(p.cpu(), p)


def test_camera_eval_metrics_on_device_tensors():
    """callers.camera_eval_metrics on HIP tensors: device float64 tensors equal to the ops call, under the synchronisation detector."""
    from vicasplat_amd import callers, ops
    names = ["walk", "axis", "planar", "nan", "exact_far"]
    Pb = np.stack([_reference(n, 8, 1, True)[0] for n in names])
    Qb = np.stack([_reference(n, 8, 1, True)[1] for n in names])
    p, q = torch.tensor(Pb, dtype=torch.float32, device=_dev()), torch.tensor(Qb, dtype=torch.float32, device=_dev())
    m, v = ops.trajectory_metrics(p, q)          # (also loads the library before the detector is armed)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ate, rt, rr, valid = callers.camera_eval_metrics(p, q, return_valid=True)
        one = callers.camera_eval_metrics(p[0], q[0])
        strided = callers.camera_eval_metrics(p, q, 2)
        mixed = callers.camera_eval_metrics(p.double(), q)          # the narrower side is promoted
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch_side = callers.camera_eval_metrics(p, q, backend="torch")          # (torch's SVD may wait for the device: outside the detector)
    for t in (ate, rt, rr) + one + strided + mixed:
        assert t.is_cuda and t.dtype == torch.float64
    assert ate.shape == (5,) and one[0].shape == () and valid.dtype == torch.bool and valid.tolist() == [True, False, True, False, True]
    assert torch.equal(torch.stack([ate, rt, rr], -1), m) and torch.equal(valid, v != 0)
    assert torch.equal(torch.stack(one), m[0]) and torch.equal(torch.stack(mixed, -1), m)
    ms, _ = ops.trajectory_metrics(p[:, ::2].contiguous(), q[:, ::2].contiguous())
    assert torch.equal(torch.stack(strided, -1), ms)
    ref = T.metrics_batch(Pb, Qb)
    got = torch.stack(torch_side, -1).cpu().numpy()
    assert (np.abs(got - ref["out"]) <= 256.0 * T.EPS * ref["mag"]).all()          # the torch backend on the device: its own sums and SVD


def test_capture_into_a_graph():
    """The entry is asynchronous and has no workspace: a captured launch replays to the same bits."""
    from vicasplat_amd import ops
    P, Q, _ = _reference("walk", 65, 1, False)
    p, q = torch.tensor(P[None], device=_dev()), torch.tensor(Q[None], device=_dev())
    eager, _ = ops.trajectory_metrics(p, q)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.trajectory_metrics(p, q)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        m, v = ops.trajectory_metrics(p, q)
    m.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(m, eager) and int(v[0]) == 1
