"""A numpy restatement of the view-overlap closed form of include/vicasplat_overlap.h, with ONE code path that runs in float64 or in float32,
and the case builders of tests/test_overlap_cpu.py, tests/test_overlap_gpu.py and tests/golden/gen_view_overlap_golden.py.

`flags` returns, per ray, the flag and an `ambiguous` mark.  Every compared quantity carries a propagated magnitude `mag` next to its value: a
first-order running bound of its rounding error in units of 2^-24 (an input or an operation's result adds its own size; a product adds
|a| mag_b + |b| mag_a; a quotient adds (mag_a + |q| mag_b) / |b| and, since a quotient is only known as well as its denominator is, becomes
unknown (mag = inf) when 4 x 2^-24 mag_b reaches |b| / 2: a near-zero d_z o_s - d_s o_z marks the ray and does not fake a sure decision).
A comparison is `unknown` when the quantity lies within FACTOR 2^-24 mag of its threshold, FACTOR = 4 max(r32, 1); the flag is then
evaluated in three-valued logic, and a ray is ambiguous when the unknown comparisons can change its flag.  A count of an f32 implementation
must lie in [sure, sure + ambiguous], sure = the rays whose flag is true whatever the unknown comparisons give.

r32 is this restatement's own f32 - f64 gap of each compared quantity in units of 2^-24 mag, at its maximum over the case list.  Measured on
the CPU (tests/test_overlap_cpu.py::test_r32_is_measured prints it):

    proj_o 0.274  proj_d 0.106  t 0.339  other 0.401  z 0.350  d_z 0.243  o_z 0.772  o_norm 0.465     (all below 1, so FACTOR = 4)
    largest ambiguous share of a case's ray-pairs: 2.7e-3 (near_origin; the case `edge` apart, which is exact in f32 only and wholly ambiguous); the reference's own f32 and f64 counts differ by at most 1 ray

When at_camera holds (|o| < 1e-6) the frame-line terms use o = 0 exactly, with mag 0: the stated deviation of DESIGN.md section 7.

Mutants (planted defects for the CPU test): "no_eps32", "strict_bounds" (`>` for `>=` and `<` for `<=` in in_bounds), "no_oz_check", "no_at_camera", "drop_line0" .. "drop_line3", "swap_xy", "swap_ij",
"corners".
"""
from __future__ import annotations

import os

import numpy as np

EPS = 1e-6
EPS32 = float(np.finfo(np.float32).eps)
INFINITY = 1e8
U = 2.0 ** -24
# bounds of the measured gaps above: max over the case list of |f32 - f64| / (2^-24 mag) per compared quantity (test_r32_is_measured asserts they are not exceeded)
R32 = {"t": 1.0, "other": 1.0, "z": 1.0, "proj_d": 1.0, "proj_o": 1.0, "d_z": 1.0, "o_z": 1.0, "o_norm": 1.0}
FACTOR = 4.0 * max(max(R32.values()), 1.0)
MUTANTS = ("no_eps32", "strict_bounds", "no_oz_check", "no_at_camera", "drop_line0", "drop_line1", "drop_line2", "drop_line3", "swap_xy", "swap_ij", "corners")
K_GENERIC = np.array([[0.9, 0.0, 0.5], [0.0, 1.2, 0.5], [0.0, 0.0, 1.0]])
SIZES = ((1, 1), (1, 7), (7, 1), (16, 16), (17, 23), (32, 48))


class Q:
    """A value in the working dtype and its propagated magnitude (float64): the rounding error is about 2^-24 mag."""

    def __init__(self, v, e):
        self.v, self.e = v, np.asarray(e, np.float64)

    @staticmethod
    def of(v, dtype, exact=False):
        v = np.asarray(v, np.float64).astype(dtype)
        return Q(v, np.zeros(v.shape) if exact else np.abs(v.astype(np.float64)))

    def _a(self):
        return np.abs(self.v.astype(np.float64))

    def __add__(self, o):
        r = self.v + o.v
        return Q(r, self.e + o.e + np.abs(r.astype(np.float64)))

    def __sub__(self, o):
        r = self.v - o.v
        return Q(r, self.e + o.e + np.abs(r.astype(np.float64)))

    def __mul__(self, o):
        r = self.v * o.v
        return Q(r, self._a() * o.e + o._a() * self.e + np.abs(r.astype(np.float64)))

    def __truediv__(self, o):
        q = self.v / o.v
        aq, ab = np.abs(q.astype(np.float64)), o._a()
        rel = np.where(o.e == 0, 0.0, 4.0 * U * o.e / ab)
        e = (self.e + np.where(self.e + o.e == 0, 0.0, aq * o.e)) / (ab * (1.0 - rel)) + aq
        return Q(q, np.where(rel < 0.5, e, np.inf))

    def sqrt(self):
        r = np.sqrt(self.v)
        ar = np.abs(r.astype(np.float64))
        return Q(r, np.where(self.e == 0, 0.0, self.e / (2.0 * ar)) + ar)


class B3:
    """A three-valued truth: lo <= hi; lo = true whatever the unknown comparisons give, hi = true for some outcome of them."""

    def __init__(self, lo, hi):
        self.lo, self.hi = lo, hi

    def __and__(self, o):
        return B3(self.lo & o.lo, self.hi & o.hi)

    def __or__(self, o):
        return B3(self.lo | o.lo, self.hi | o.hi)

    def __invert__(self):
        return B3(~self.hi, ~self.lo)


def _cmp(q: Q, op: str, tau: float, factor: float) -> B3:
    t = np.asarray(tau, np.float64).astype(q.v.dtype)      # the threshold in the working dtype, as torch casts a Python scalar
    base = {">": q.v > t, ">=": q.v >= t, "<": q.v < t, "<=": q.v <= t}[op]
    if factor is None:
        return B3(base, base)
    sure = np.abs(q.v.astype(np.float64) - float(t)) > factor * U * q.e       # false for an unknown magnitude (inf, NaN)
    unknown = ~np.isnan(q.v) & ~sure
    return B3(base & ~unknown, base | unknown)


def _in_bounds(q: Q, factor, strict=False) -> B3:
    return _cmp(q, ">" if strict else ">=", -EPS, factor) & _cmp(q, "<" if strict else "<=", 1 + EPS, factor)


def _nan_to_num(q: Q) -> Q:
    v = np.nan_to_num(q.v, nan=0.0, posinf=INFINITY, neginf=-INFINITY)
    return Q(v, np.where(np.isfinite(q.e), q.e, np.inf))


def _adjugate(A):
    adj = np.empty((3, 3))
    for r in range(3):
        for c in range(3):
            r1, r2, c1, c2 = (c + 1) % 3, (c + 2) % 3, (r + 1) % 3, (r + 2) % 3
            adj[r, c] = A[r1, c1] * A[r2, c2] - A[r1, c2] * A[r2, c1]
    return adj, (A[0, 0] * adj[0, 0] + A[0, 1] * adj[1, 0]) + A[0, 2] * adj[2, 0]


def pair_constants(E, K, i, j):
    """(R, o, K_i^-1, c_f [4]) in float64: M = inv(E_j) E_i by the affine inverse, 3 x 3 by the adjugate."""
    Ei, Ej, Ki, Kj = (np.asarray(a, np.float64) for a in (E[i], E[j], K[i], K[j]))
    with np.errstate(all="ignore"):
        adj, det = _adjugate(Ej[:3, :3])
        R = np.array([[(adj[r, 0] * Ei[0, c] + adj[r, 1] * Ei[1, c]) + adj[r, 2] * Ei[2, c] for c in range(3)] for r in range(3)]) / det
        dt = Ei[:3, 3] - Ej[:3, 3]
        o = np.array([(adj[r, 0] * dt[0] + adj[r, 1] * dt[1]) + adj[r, 2] * dt[2] for r in range(3)]) / det
        kadj, kdet = _adjugate(Ki)
        cf = np.array([(v - Kj[a, 2]) / Kj[a, a] for a in (0, 1) for v in (0.0, 1.0)])
        return R, o, kadj / kdet, cf


def _core(E, K, h, w, i, j, dtype, mutant, factor, record):
    """(lo, hi) [h w] of the three-valued flag; factor None: every comparison decided as the working dtype decides it (lo == hi)."""
    if mutant == "swap_ij":
        i, j = j, i
    T, strict = np.dtype(dtype).type, mutant == "strict_bounds"
    R64, o64, Kinv64, cf64 = pair_constants(E, K, i, j)
    Kj64 = np.asarray(K[j], np.float64)
    N = h * w
    with np.errstate(all="ignore"):
        c = lambda v, exact=False: Q.of(np.full(1, v), T, exact)
        R = [[c(R64[r, k]) for k in range(3)] for r in range(3)]
        o = [c(o64[k]) for k in range(3)]
        Ki = [[c(Kinv64[r, k]) for k in range(3)] for r in range(3)]
        Kj = [[c(Kj64[r, k]) for k in range(3)] for r in range(2)]
        cf = [c(v) for v in cf64]
        eps32 = c(0.0 if mutant == "no_eps32" else EPS32, exact=True)

        def projects_inside(p, name):
            den = p[2] + eps32
            q = [_nan_to_num(p[k] / den) for k in range(3)]
            x = (Kj[0][0] * q[0] + Kj[0][1] * q[1]) + Kj[0][2] * q[2]
            y = (Kj[1][0] * q[0] + Kj[1][1] * q[1]) + Kj[1][2] * q[2]
            if record is not None:
                record[name + "_x"], record[name + "_y"] = x, y
            return _in_bounds(x, factor, strict) & _in_bounds(y, factor, strict)

        # ---- the pair's own flags
        o_norm = ((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]).sqrt()
        at = _cmp(o_norm, "<", EPS, factor)
        if mutant == "no_at_camera":
            at = B3(np.zeros(1, bool), np.zeros(1, bool))
        origin_valid = projects_inside(o, "proj_o") & _cmp(o[2], ">", -EPS, factor)
        if mutant != "no_oz_check":
            origin_valid = origin_valid & ~_cmp(o[2], "<", EPS, factor)
        at_base = bool(o_norm.v[0] < T(EPS)) and mutant != "no_at_camera"      # the plain decision in the working dtype
        at_unknown = bool(at.lo[0] != at.hi[0])
        o_given = o
        if at_base:
            o = [c(0.0, exact=True) for _ in range(3)]

        # ---- the rays: the grid is formed in f32, as sample_image_grid forms it, whatever the working dtype
        n = np.arange(N)
        half = np.float32(0.0 if mutant == "corners" else 0.5)
        x32 = ((n % w).astype(np.float32) + half) / np.float32(w)
        y32 = ((n // w).astype(np.float32) + half) / np.float32(h)
        if mutant == "swap_xy":
            x32, y32 = ((n // w).astype(np.float32) + half) / np.float32(h), ((n % w).astype(np.float32) + half) / np.float32(w)
        x, y = Q.of(x32, T), Q.of(y32, T)
        u = [(Ki[r][0] * x + Ki[r][1] * y) + Ki[r][2] for r in range(3)]
        norm = ((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]).sqrt()
        u = [v / norm for v in u]
        d = [(R[r][0] * u[0] + R[r][1] * u[1]) + R[r][2] * u[2] for r in range(3)]
        valid_inf = projects_inside(d, "proj_d") & _cmp(d[2], ">", -EPS, factor)
        valid_0 = valid_inf if at_base else B3(np.broadcast_to(origin_valid.lo, (N,)), np.broadcast_to(origin_valid.hi, (N,)))

        any_f = B3(np.zeros(N, bool), np.zeros(N, bool))
        for f in range(4):
            if mutant == f"drop_line{f}":
                continue
            s, q_ = (0, 1) if f < 2 else (1, 0)
            den = d[2] * o[s] - d[s] * o[2]
            t = (cf[f] * o[2] - o[s]) / (d[s] - cf[f] * d[2])
            num = Kj[q_][q_] * (o[q_] * (cf[f] * d[2] - d[s]) + d[q_] * (o[s] - cf[f] * o[2]))
            other = Kj[q_][2] + num / den
            z = o[2] + t * d[2]
            if record is not None:
                record[f"t{f}"], record[f"other{f}"], record[f"z{f}"] = t, other, z
            any_f = any_f | (_in_bounds(other, factor, strict) & _cmp(z, ">", -EPS, factor) & _cmp(t, ">", -EPS, factor))
        if record is not None:
            record["d_z"], record["o_z"], record["o_norm"] = d[2], o_given[2], o_norm
        out = (valid_0 & valid_inf) | any_f
        lo, hi = np.broadcast_to(out.lo, (N,)), np.broadcast_to(out.hi, (N,))
        if at_unknown:      # |o| too close to eps to tell which of the two forms applies: nothing about this pair is sure
            lo, hi = np.zeros(N, bool), np.ones(N, bool)
        return lo.copy(), hi.copy()


def flags(E, K, h, w, i, j, dtype=np.float64, mutant=None, factor=FACTOR, record=None):
    """(flag [h w] bool, ambiguous [h w] bool) of the ordered pair (i -> j) in the working dtype.  record: a dict that receives the compared
    quantities (Q: value and magnitude)."""
    flag, _ = _core(E, K, h, w, i, j, dtype, mutant, None, record)
    lo, hi = _core(E, K, h, w, i, j, dtype, mutant, factor, None)
    assert (lo <= flag).all() and (flag <= hi).all()
    return flag, lo != hi


def counts(E, K, h, w, pairs, dtype=np.float64, mutant=None, factor=FACTOR):
    """(count, sure, ambiguous) [P] int: the plain count, the rays that overlap whatever the unknown comparisons give, and the ambiguous rays.
    An f32 implementation of the closed form must count within [sure, sure + ambiguous]."""
    out = np.zeros((len(pairs), 3), np.int64)
    for k, (i, j) in enumerate(pairs):
        flag, amb = flags(E, K, h, w, int(i), int(j), dtype, mutant, factor)
        out[k] = flag.sum(), (flag & ~amb).sum(), amb.sum()
    return out[:, 0], out[:, 1], out[:, 2]


# ---- case builders: every entry is rounded to f32, so that f32 and f64 inputs hold the same values -----------------------------------------
def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def rotation(yaw=0.0, pitch=0.0, roll=0.0):
    """Camera-to-world rotation: yaw about y, then pitch about x, then roll about z (radians)."""
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    return Ry @ Rx @ Rz


def pose(Rm, t, scale=1.0):
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = scale * np.asarray(Rm), t
    return E


def trajectory(V=16, seed=0, yaw_step=0.06, step=(0.15, 0.0, 0.05), wobble=0.02):
    """(E [V, 4, 4], K [V, 3, 3]): a generic walk that turns while it moves (yaw_step per frame: a number or [V] increments), with the
    generic intrinsics."""
    g = np.random.default_rng(seed)
    yaw = np.cumsum(np.broadcast_to(np.asarray(yaw_step, np.float64), (V,))) - np.broadcast_to(yaw_step, (V,))[0]
    E = np.stack([pose(rotation(yaw[k] + wobble * g.normal(), wobble * g.normal(), wobble * g.normal()),
                       np.asarray(step) * k + wobble * g.normal(size=3)) for k in range(V)])
    return _f32(E), _f32(np.repeat(K_GENERIC[None], V, 0))




def special():
    """(E [16, 4, 4], K [16, 3, 3], {name: [(i, j), ...]}): the hand-made cameras; the first nine are paired with camera 0 (the identity pose)."""
    I = np.eye(3)
    E = np.stack([pose(I, (0, 0, 0)), pose(I, (0, 0, 0)), pose(rotation(0.35, 0.05), (0, 0, 0)), pose(rotation(np.pi), (0, 0, -1.0)),
                  pose(I, (0, 0, 0.5)), pose(I, (0.5, 0, 0)), pose(rotation(0.09, -0.03), (0.2, 0.05, 0.1)),
                  pose(rotation(-0.14, 0.02, 0.05), (0.1, 0.0, 0.2), scale=2.0), pose(rotation(0.1), (0.1, 0.1, 0.1))])
    E[3, :3, :3] = np.diag([-1.0, 1.0, -1.0])      # exactly half a turn about y
    E[8, 0, 3] = np.nan
    K = np.repeat(K_GENERIC[None], 9, 0)
    K[6] = [[1.3, 0, 0.45], [0, 0.8, 0.55], [0, 0, 1]]
    # the forward camera's epipole off the image centre: with both at the centre the diagonal rays of a square grid pass exactly through the
    # image corners, where two frame lines decide at once
    K[4] = [[0.9, 0, 0.48], [0, 1.2, 0.53], [0, 0, 1]]
    # near_origin: the origin of camera 10's rays sits 1e-5 in front of camera 9; eps32 is 1.2 % of the projection's denominator there and
    # pulls the projected origin from x = 1.006, outside camera 9's image, to 0.994, inside it.  Camera 9 has a skew, which the frame lines do
    # not read: for them the origin projects well inside, so no frame line is crossed within t > -eps and valid_0 alone decides.  near_plane: the origin of camera 12's rays sits 1.06e-6 from camera 11 with o_z = 0.9e-6 < eps, projecting inside.
    # edge: camera 15 looks along camera 13's and 14's axis from one unit to the side, so that at 1 x 1 the one ray crosses the frame line
    # x = 1 at other = c_y exactly, and c_y is the f32 bound itself: -f32(1e-6) for camera 13, f32(1 + 1e-6) for camera 14
    I4 = pose(I, (0, 0, 0))
    E = np.concatenate([E, np.stack([I4, pose(I, (0.118e-5, 0.2e-5, 1.0e-5)), I4, pose(I, (0.4e-6, 0.4e-6, 0.9e-6)), I4, I4,
                                     pose(I, (1.0, 0, 0))])])
    K = np.concatenate([K, np.repeat(K_GENERIC[None], 7, 0)])
    K[9] = [[0.9, 2.0, 0.5], [0, 1.2, 0.5], [0, 0, 1]]
    K[11] = [[0.5, 0, 0.5], [0, 0.5, 0.5], [0, 0, 1]]
    K[13] = [[1, 0, 0.5], [0, 1, -float(np.float32(EPS))], [0, 0, 1]]
    K[14] = [[1, 0, 0.5], [0, 1, float(np.float32(1 + EPS))], [0, 0, 1]]
    K[15] = [[1, 0, 0.5], [0, 1, 0.5], [0, 0, 1]]
    pairs = {"identical": [(0, 0), (0, 1), (1, 0)], "rotated": [(0, 2), (2, 0)], "away": [(0, 3), (3, 0)], "forward": [(0, 4), (4, 0)],
             "sideways": [(0, 5), (5, 0)], "other_k": [(0, 6), (6, 0)], "scaled": [(0, 7), (7, 0), (6, 7), (7, 6)], "nan": [(0, 8), (8, 0)],
             "near_origin": [(10, 9)], "near_plane": [(12, 11)], "edge": [(15, 13), (15, 14)]}
    return _f32(E), _f32(K), pairs


def all_pairs(V):
    return [(i, j) for i in range(V) for j in range(V)]


SCENE_V, SCENE_SHAPE = 24, (16, 16)
# the configuration of the evaluation-index golden: small distances, so that 24 frames hold whole walks
SCENE_CFG = dict(num_target_views=3, min_distance=2, max_distance=6, min_overlap=0.6, max_overlap=0.9, save_previews=False, seed=7)
# turn per frame (radians) of the five scenes.  A walk that barely turns overlaps by more than max_overlap at every distance of the band, so
# "none" finds nothing; "later" turns on its last five frames only, so that a start frame among the first twelve finds nothing
SCENE_YAW = {"first": 0.08, "later": [0.0] * 19 + [0.08] * 5, "none": 0.002, "max_distance": 0.03, "repeat": 0.16}


def scene(kind, seed=0):
    """(E, K) of one seeded scene of the evaluation-index golden."""
    return trajectory(SCENE_V, seed, yaw_step=SCENE_YAW[kind], step=(0.04, 0.0, 0.02), wobble=0.004)


# ---- what the CPU and the GPU tests share ------------------------------------------------------------------------------------------------
def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "view_overlap.npz"))


def cases(G):
    """[(name, E, K, pairs, key prefix, slice of the golden's pair list)]: the trajectory with all ordered pairs, then the hand-made cases."""
    out = [("trajectory", G["traj_E"], G["traj_K"], all_pairs(16), "traj", slice(None))]
    at = 0
    for name, pairs in special()[2].items():
        out.append((name, G["spec_E"], G["spec_K"], pairs, "spec", slice(at, at + len(pairs))))
        at += len(pairs)
    return out


def run_generator(G, tmp_path, backend, device):
    """The five scenes of the golden through vicasplat_amd's EvaluationIndexGenerator -> (the generator, the JSON it saved)."""
    import torch
    from vicasplat_amd.evaluation import EvaluationIndexGenerator, EvaluationIndexGeneratorCfg
    gen = EvaluationIndexGenerator(EvaluationIndexGeneratorCfg(output_path=tmp_path, **dict(SCENE_CFG, seed=int(G["cfg_seed"]))), backend=backend)
    h, w = SCENE_SHAPE
    for name, E, K in zip(G["scene_names"], G["scene_E"], G["scene_K"]):
        batch = dict(target=dict(image=torch.zeros(1, SCENE_V, 3, h, w, device=device),
                                 extrinsics=torch.tensor(E, dtype=torch.float32, device=device)[None],
                                 intrinsics=torch.tensor(K, dtype=torch.float32, device=device)[None]), scene=[str(name)])
        gen.test_step(batch, 0)
    gen.save_index()
    return gen, (tmp_path / "evaluation_index.json").read_text()
