"""Float64 restatement (numpy) of the trajectory metrics ATE / RPE-trans / RPE-rot as src/evaluation/metrics.py:185-265 asks evo for them
(ape and rpe with align=True, correct_scale=True, delta in frames, all_pairs=True), from the published algorithm (Umeyama 1991 for the
alignment).  UNVERIFIED against evo: the package is not available offline, so nothing here is pinned to its numbers.  Independent of
vicasplat_amd/callers.py.  The yardstick of tests/test_trajectory_gpu.py and tests/test_trajectory_cpu.py.

One scene: estimated camera-to-world poses P [V, 4, 4], ground truth Q [V, 4, 4]; x_i, y_i their positions, Rp_i, Rq_i their rotation
blocks, used as given (the reference passes them through a quaternion and back; test_trajectory_cpu measures what that moves).
  mu_x, mu_y the means; sigma_x^2 = (1/V) sum |x_i - mu_x|^2; C = (1/V) sum (y_i - mu_y)(x_i - mu_x)^T = U diag(d) V^T (numpy.linalg.svd,
  d descending); S = I with S_33 = -1 when det U det V < 0; R = U S V^T, c = tr(diag(d) S) / sigma_x^2, t = mu_y - c R mu_x.
  degenerate (valid = 0, all outputs 0, alignment identity): fewer than two d_k > 2^-52 (evo's absolute test), V < 3, delta >= V, or any
  non-finite element of P or Q.
  ATE = sqrt(mean |c R x_i + t - y_i|^2).
  RPE over (i, j = i + delta): A = Rq_i^T Rq_j, a = Rq_i^T (y_j - y_i), B = Rp_i^T Rp_j, b = c Rp_i^T (x_j - x_i), E_R = A^T B,
  E_t = A^T (b - a); RPE-trans = sqrt(mean |E_t|^2), RPE-rot = sqrt(mean theta^2), theta = atan2(|w| / 2, (tr E_R - 1) / 2) in degrees with
  w = (E32 - E23, E13 - E31, E21 - E12) (acos loses half the digits at theta -> 0).
The three sums over the poses that feed the SVD (means, sigma_x^2, C) and the two sums of squares are accumulated in numpy.longdouble, so
that the restatement's own summation error stays below one unit at V = 130; every other operation is float64, each rounded once, in the
order written in `metrics` (products summed left to right).

Units.  An output is compared in units of 2^-52 mag: mag = max |y_i| + c max |x_i| + |t| for ATE, RPE-trans and t (the magnitude of the
operands of the residual c R x_i + t - y_i), 180 / pi for RPE-rot (one unit = 2^-52 rad), 1 for R, c for c.

R64 is the restatement's own rounding floor, per output: the largest change of the output (the three metrics, and R, t, c mapped back), in
those units, when both trajectories are re-expressed under the 24 proper signed axis permutations of the world frame -- exact in floating
point, and the metrics are invariant under them.  The three metrics stay below one unit; R, t and c carry the SVD's own error times the
condition of the rotation, d_1 / (d_2 + S_33 d_3), which the case builders keep at 5 or less.  `mutant=` plants one deliberate defect (MUTANTS).
"""
import itertools

import numpy as np

EPS = 2.0 ** -52
DEG = 180.0 / np.pi
NAMES = ("ate", "rpe_trans", "rpe_rot")
MUTANTS = ("no_scale", "no_s33", "swapped", "rpe_no_scale", "mean_not_rms", "c_vm1", "sigma_vm1", "pairs_from_0", "acos")
OUTPUTS = NAMES + ("R", "t", "c")
# measured by tests/test_trajectory_cpu.py::test_permutation_spread_is_within_r64 over every case family (printed there with -s: 0.617,
# 0.577, 0.279, 8.881, 1.928, 3.365), per output, rounded up to one place
R64 = dict(ate=0.7, rpe_trans=0.6, rpe_rot=0.3, R=8.9, t=2.0, c=3.4)


def gpu_factor(key):
    """B of the GPU criterion |gpu - ref| <= B 2^-52 mag for output `key` (OUTPUTS)."""
    return 4.0 * max(R64[key], 1.0)


def _ld(a):
    return np.asarray(a, dtype=np.longdouble)


def _mv(M, v):
    """M v for M [..., 3, 3], v [..., 3]: (M_r0 v_0 + M_r1 v_1) + M_r2 v_2."""
    return (M[..., :, 0] * v[..., None, 0] + M[..., :, 1] * v[..., None, 1]) + M[..., :, 2] * v[..., None, 2]


def _mtv(M, v):
    """M^T v: (M_0c v_0 + M_1c v_1) + M_2c v_2."""
    return (M[..., 0, :] * v[..., None, 0] + M[..., 1, :] * v[..., None, 1]) + M[..., 2, :] * v[..., None, 2]


def _mtm(A, B):
    """A^T B: out[r, c] = (A_0r B_0c + A_1r B_1c) + A_2r B_2c."""
    return (A[..., 0, :, None] * B[..., 0, None, :] + A[..., 1, :, None] * B[..., 1, None, :]) + A[..., 2, :, None] * B[..., 2, None, :]


def _sq(v):
    return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


def _zero():
    return np.zeros(3), 0, (np.eye(3), np.zeros(3), 1.0), np.zeros(3), np.ones(3)


def metrics(P, Q, delta=1, mutant=None):
    """(out [3] = ate, rpe_trans, rpe_rot; valid; (R, t, c); d [3]; mag [3]) of one scene, all float64."""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    V = P.shape[0]
    assert P.shape == Q.shape == (V, 4, 4) and delta >= 1
    if V < 3 or delta >= V or not (np.isfinite(P).all() and np.isfinite(Q).all()):
        return _zero()
    x, y, Rp, Rq = P[:, :3, 3], Q[:, :3, 3], P[:, :3, :3], Q[:, :3, :3]
    if mutant == "swapped":       # the truth aligned to the estimate
        x, y, Rp, Rq = y, x, Rq, Rp
    mux, muy = np.float64(_ld(x).sum(0) / V), np.float64(_ld(y).sum(0) / V)
    dx, dy = x - mux, y - muy
    sig2 = np.float64((_ld(dx) * _ld(dx)).sum() / (V - 1 if mutant == "sigma_vm1" else V))
    C = np.float64((_ld(dy)[:, :, None] * _ld(dx)[:, None, :]).sum(0) / (V - 1 if mutant == "c_vm1" else V))
    U, d, Vt = np.linalg.svd(C)
    if int((d > EPS).sum()) < 2:
        z = _zero()
        return z[0], 0, z[2], d, z[4]
    s = -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 and mutant != "no_s33" else 1.0
    R = (U * np.array([1.0, 1.0, s])) @ Vt
    c = ((d[0] + d[1]) + s * d[2]) / sig2
    if mutant == "no_scale":
        c = 1.0
    t = muy - c * _mv(R, mux)
    res = (c * _mv(R, x) + t) - y
    e = _sq(res)
    i = np.zeros(V - 1, dtype=int) if mutant == "pairs_from_0" else np.arange(V - delta)
    j = np.arange(1, V) if mutant == "pairs_from_0" else i + delta
    A, a = _mtm(Rq[i], Rq[j]), _mtv(Rq[i], y[j] - y[i])
    B, b = _mtm(Rp[i], Rp[j]), (1.0 if mutant == "rpe_no_scale" else c) * _mtv(Rp[i], x[j] - x[i])
    E, Et = _mtm(A, B), _mtv(A, b - a)
    w = np.stack([E[:, 2, 1] - E[:, 1, 2], E[:, 0, 2] - E[:, 2, 0], E[:, 1, 0] - E[:, 0, 1]], -1)
    cs = 0.5 * (((E[:, 0, 0] + E[:, 1, 1]) + E[:, 2, 2]) - 1.0)
    theta = np.arccos(np.clip(cs, -1.0, 1.0)) if mutant == "acos" else np.arctan2(0.5 * np.sqrt(_sq(w)), cs)
    deg, et = theta * DEG, _sq(Et)
    if mutant == "mean_not_rms":
        out = np.array([np.sqrt(e).mean(), np.sqrt(et).mean(), np.abs(deg).mean()])
    else:
        out = np.array([np.sqrt(np.float64(_ld(e).sum() / V)), np.sqrt(np.float64(_ld(et).sum() / len(i))),
                        np.sqrt(np.float64(_ld(deg * deg).sum() / len(i)))])
    m = np.sqrt(_sq(y)).max() + c * np.sqrt(_sq(x)).max() + np.sqrt(_sq(t))
    return out, 1, (R, t, c), d, np.array([m, m, DEG])


def metrics_batch(P, Q, delta=1):
    """The scenes of P, Q [B, V, 4, 4] one by one -> dict of stacked arrays: out [B, 3], valid [B], R [B, 3, 3], t [B, 3], c [B], d [B, 3],
    mag [B, 3]."""
    rows = [metrics(p, q, delta) for p, q in zip(P, Q)]
    return dict(out=np.stack([r[0] for r in rows]), valid=np.array([r[1] for r in rows]), R=np.stack([r[2][0] for r in rows]),
                t=np.stack([r[2][1] for r in rows]), c=np.array([r[2][2] for r in rows]), d=np.stack([r[3] for r in rows]),
                mag=np.stack([r[4] for r in rows]))


def units(got, ref, mag):
    """max |got - ref| / (2^-52 mag), elementwise magnitudes broadcast; 0 for empty arrays."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    u = np.abs(got - ref) / (EPS * np.broadcast_to(mag, got.shape))
    return float(u.max()) if u.size else 0.0


def alignment_units(got_R, got_t, got_c, ref):
    """(units of R, t, c) of one scene against the tuple `metrics` returned: R in units of 1, t of mag, c of c."""
    (R, t, c), mag = ref[2], ref[4]
    return units(got_R, R, 1.0), units(got_t, t, mag[0]), units(got_c, c, abs(c))


# ---- the 24 proper signed axis permutations ----
def signed_permutations():
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            G = np.zeros((3, 3))
            for r in range(3):
                G[r, perm[r]] = signs[r]
            if np.linalg.det(G) > 0:
                out.append(G)
    assert len(out) == 24
    return out


def transform_world(P, G):
    """The trajectory P [V, 4, 4] re-expressed in the world frame G (a signed permutation: exact)."""
    out = np.array(P, np.float64, copy=True)
    out[:, :3, :3] = G @ P[:, :3, :3]
    out[:, :3, 3] = P[:, :3, 3] @ G.T
    return out


def permutation_spread(P, Q, delta=1):
    """{output: the largest change of it, in its units, over the 24 re-expressions of the world frame} (OUTPUTS)."""
    ref = metrics(P, Q, delta)
    worst = dict.fromkeys(OUTPUTS, 0.0)
    for G in signed_permutations():
        got = metrics(transform_world(P, G), transform_world(Q, G), delta)
        assert got[1] == ref[1]
        if not ref[1]:
            assert not got[0].any()
            continue
        (R, t, c) = got[2]
        u = [units(got[0][k], ref[0][k], ref[4][k]) for k in range(3)] + list(alignment_units(G.T @ R @ G, G.T @ t, c, ref))
        worst = {k: max(worst[k], v) for k, v in zip(OUTPUTS, u)}
    return worst


# ---- case builders: every one returns (P, Q) [V, 4, 4] float64 ----
def _rot(axis_angle):
    a = np.asarray(axis_angle, np.float64)
    th = np.linalg.norm(a)
    if th == 0:
        return np.eye(3)
    k = a / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def poses(R, p):
    V = len(p)
    out = np.tile(np.eye(4), (V, 1, 1))
    out[:, :3, :3], out[:, :3, 3] = R, p
    return out


def similarity(P, s, R0, t0):
    """The trajectory under x -> s R0 x + t0 (rotations R0 Rp)."""
    return poses(R0 @ P[:, :3, :3], s * (P[:, :3, 3] @ R0.T) + t0)


def walk(V, seed, planar=False):
    """Ground truth: a random walk with steps of order 1 and slowly turning cameras."""
    g = np.random.default_rng(seed)
    step = g.normal(size=(V, 3))
    if planar:
        step[:, 2] = 0.0
    y = np.cumsum(step, 0)
    R, rots = np.eye(3), []
    for _ in range(V):
        R = R @ _rot(0.3 * g.normal(size=3))
        rots.append(R)
    return poses(np.stack(rots), y)


def walk_case(V, seed, noise=0.05, planar=False):
    """A walk and its estimate: the truth under a random similarity, every pose perturbed (positions by `noise`, rotations by 2 * noise rad)."""
    g = np.random.default_rng(1000 + seed)
    Q = walk(V, seed, planar)
    P = similarity(Q, float(g.uniform(0.3, 3.0)), _rot(g.normal(size=3)), g.normal(size=3) * 2.0)
    P[:, :3, :3] = P[:, :3, :3] @ np.stack([_rot(2 * noise * g.normal(size=3)) for _ in range(V)])
    # planar: the estimate stays in the image of the plane (up to rounding: d_3 is noise of the order of 1e-17, or 0)
    P[:, :3, 3] += (noise * g.normal(size=(V, 2))) @ _plane_basis(P) if planar else noise * g.normal(size=(V, 3))
    return P, Q


def _plane_basis(P):
    """Two orthonormal directions spanning the plane of the positions of P (planar trajectories)."""
    x = P[:, :3, 3] - P[:, :3, 3].mean(0)
    return np.linalg.svd(x)[2][:2]


def square_case():
    """The closed form: y the corners (+-1, +-1, 0) in cyclic order, x = y + (0, 0, +-1) alternating, rotations the identity.
    d = (1, 1, 0), R = I, c = 2/3, ATE = sqrt(2/3), RPE-trans = sqrt(20)/3, RPE-rot = 0."""
    y = np.array([[1.0, 1.0, 0.0], [-1.0, 1.0, 0.0], [-1.0, -1.0, 0.0], [1.0, -1.0, 0.0]])
    x = y + np.array([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [0.0, 0.0, 1.0], [0.0, 0.0, -1.0]])
    eye = np.tile(np.eye(3), (4, 1, 1))
    return poses(eye, x), poses(eye, y)


SQUARE = dict(d=(1.0, 1.0, 0.0), c=2.0 / 3.0, out=(np.sqrt(2.0 / 3.0), np.sqrt(20.0) / 3.0, 0.0))


def reflection_case(V=8, seed=0):
    """x = diag(1, 1, -1) y with the rotations shared: the best ROTATION is not the reflection (S_33 = -1), ATE > 0, RPE-rot = 0."""
    Q = walk(V, 70 + seed)
    return poses(Q[:, :3, :3], Q[:, :3, 3] * np.array([1.0, 1.0, -1.0])), Q


def exact_case(V=8, seed=0, offset=0.0):
    """The estimate is exactly a similarity of the truth (up to the rounding of applying it); `offset` moves both far from the origin."""
    g = np.random.default_rng(90 + seed)
    Q = walk(V, 90 + seed)
    Q[:, :3, 3] += offset * np.array([1.0, -1.0, 0.5])
    P = similarity(Q, 1.7, _rot(g.normal(size=3)), g.normal(size=3) + offset * np.array([-0.5, 1.0, 1.0]))
    return P, Q


def identical_case(V=8, seed=0):
    """P == Q bit for bit: every relative rotation error is exactly the identity up to the rounding of A^T A."""
    Q = walk(V, 110 + seed)
    return Q.copy(), Q


def axis_case(V=8, seed=0):
    """Positions on the first coordinate axis: C has one non-zero entry, d_2 = d_3 = 0 exactly under any SVD."""
    g = np.random.default_rng(130 + seed)
    Q = walk(V, 130 + seed)
    P = walk(V, 131 + seed)
    Q[:, 1:3, 3] = 0.0
    P[:, 1:3, 3] = 0.0
    P[:, 0, 3] = 2.0 * Q[:, 0, 3] + 0.1 * g.normal(size=V)
    return P, Q


def nan_case(V=8, seed=0, where=(2, 1, 3), truth=False):
    P, Q = walk_case(V, 150 + seed)
    (Q if truth else P)[where] = np.nan
    return P, Q


def _pick(make, seed, min_d3=0.0):
    """make(seed), the seed stepped until the case is well posed with room to spare (rounding the poses to f32 keeps it so), and the rotation
    well conditioned: R, t and c are compared too, and neither numpy's SVD nor any other gives R better than its condition allows."""
    for k in range(64):
        P, Q = make(seed + 7919 * k)
        d = metrics(P, Q)[3]
        if d[1] - d[2] >= 0.2 * d[0] and d[2] >= min_d3 * d[0]:      # R is conditioned like d_1 / (d_2 + S_33 d_3): at most 5 here, whatever S_33 is
            return P, Q
    raise AssertionError("no well-posed case in 64 draws")


def families(V):
    """{name: (P, Q)} of every non-degenerate family that exists at V poses (V >= 3)."""
    out = {"walk": _pick(lambda s: walk_case(V, s), V), "walk_noisy": _pick(lambda s: walk_case(V, s, noise=0.3), 200 + V),
           "planar": _pick(lambda s: walk_case(V, s, planar=True), 300 + V),
           "exact_far": _pick(lambda s: exact_case(V, s, offset=1e3), V), "exact": _pick(lambda s: exact_case(V, s), V),
           "identical": _pick(lambda s: identical_case(V, s), V)}
    if V >= 4:      # three points lie in a plane, and a plane's mirror image is a rotation of it
        out["reflection"] = _pick(lambda s: reflection_case(V, s), V, min_d3=0.02)
    if V == 4:
        out["square"] = square_case()
    return out


def degenerate_families(V):
    """{name: (P, Q)} of the degenerate families at V poses (any V >= 1)."""
    out = {"axis": axis_case(V, V), "nan": nan_case(V, V, where=(V // 2, 1, 3))}
    P, Q = walk_case(V, 170 + V)
    Q[V - 1, 3, 0] = np.inf       # an element no formula reads: "any non-finite input element of the scene"
    out["inf_bottom_row"] = (P, Q)
    return out


def well_posed(ref, floor=0.1):
    """The condition every non-degenerate test case meets (asserted on the restatement itself): d_2 >= 1e-6 d_1 and d_2 + d_3 >= 0.1 d_1."""
    d = ref[3]
    return bool(ref[1] == 1 and d[1] >= 1e-6 * d[0] and d[1] + d[2] >= floor * d[0])


def plainly_degenerate(ref, V, delta=1, finite=True):
    """The condition every degenerate test case meets: d_2 = 0 exactly, V < 3, delta >= V, or a non-finite element."""
    return bool(ref[1] == 0 and (V < 3 or delta >= V or not finite or ref[3][1] == 0.0))
