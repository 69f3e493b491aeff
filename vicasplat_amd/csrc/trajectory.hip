// Trajectory metrics: ATE / RPE-trans / RPE-rot of camera_eval_metrics (src/evaluation/metrics.py:148-265), batched over scenes, float64.
// Declared in include/vicasplat_metrics.h (prefix vsm_), where the algorithm is written out.
//
//   one 64-lane wave per scene, grid B.  Poses are strided over the lanes (V > 64: several trips); each lane accumulates its poses in
//   index order and a fixed xor butterfly combines the lanes, so every lane ends with the same bits.  No LDS, no atomics, no workspace.
//   pass 1   the position sums and the finiteness of all 32 V input elements; V < 3, delta >= V or a non-finite element end the scene here
//   pass 2   sigma_x^2 and C around the means
//   svd      every lane, redundantly and uniformly: cyclic one-sided Jacobi on the columns of C (at most kMaxSweeps sweeps of three
//            rotations; a NaN fails every comparison and so rotates nothing), singular values = column norms, sorted descending with their
//            vectors; u_3 and v_3 are COMPLETED from the first two (u_1 x u_2, v_1 x v_2) and only their signs are read off the Jacobi
//            columns -- a zero or rounding-noise d_3 (planar trajectories) still gives orthonormal U and V
//   pass 3   the ATE residuals and the RPE pairs (i, i + delta)
// The sums that feed the SVD carry the rounding error of every addition and (by fma) of every product in a second word, so C and
// sigma_x^2 are correctly rounded up to their last bit whatever V is: the rotation is conditioned like 1 / (d_2 + d_3) on C.  The sums of
// squares of pass 3 carry the additions' error.  Floating-point contraction is off in this file: every product and sum below is
// rounded once, in the order written, which is the order of tests/trajectory_f64.py.
// The same inputs give the same bits, alone or inside a batch.
#include "common.h"

#include "../../include/vicasplat_metrics.h"

#pragma clang fp contract(off)

namespace {

constexpr int kWave = 64;
constexpr int kMaxSweeps = 16;               // 3 x 3 Jacobi converges quadratically: 4-6 sweeps in practice
constexpr double kTiny = 0x1p-52;            // evo's absolute rank test; also the relative orthogonality at which Jacobi stops rotating
constexpr double kDeg = 180.0 / 3.14159265358979323846;
constexpr int kDtypeF32 = 0, kDtypeF64 = 5;

struct dd {
    double hi, lo;
};

__device__ __forceinline__ void two_sum(double a, double b, double &s, double &e) {
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}

__device__ __forceinline__ void dd_add(dd &acc, double v) {
    double s, e;
    two_sum(acc.hi, v, s, e);
    acc.hi = s;
    acc.lo += e;
}

// acc += a * b, the product's rounding error included
__device__ __forceinline__ void dd_add_prod(dd &acc, double a, double b) {
    const double p = a * b;
    const double pe = fma(a, b, -p);
    dd_add(acc, p);
    acc.lo += pe;
}

// the sum over the wave, the same bits on every lane (the butterfly's additions commute; lane 0's value is broadcast all the same)
__device__ __forceinline__ dd dd_wave_sum(dd v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double oh = __shfl_xor(v.hi, m, kWave), ol = __shfl_xor(v.lo, m, kWave);
        double s, e;
        two_sum(v.hi, oh, s, e);
        v.hi = s;
        v.lo = (v.lo + ol) + e;
    }
    v.hi = __shfl(v.hi, 0, kWave);
    v.lo = __shfl(v.lo, 0, kWave);
    return v;
}

// (hi + lo) / n, rounded once
__device__ __forceinline__ double dd_div(dd v, double n) {
    double s, e;
    two_sum(v.hi, v.lo, s, e);
    const double q = s / n;
    return q + (fma(-q, n, s) + e) / n;
}

__device__ __forceinline__ bool finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

__device__ __forceinline__ double dot3(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__device__ __forceinline__ void cross3(const double *a, const double *b, double *o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// M v, M row-major
__device__ __forceinline__ void mv(const double (&M)[3][3], const double *v, double *o) {
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = (M[r][0] * v[0] + M[r][1] * v[1]) + M[r][2] * v[2];
}

// M^T v
__device__ __forceinline__ void mtv(const double (&M)[3][3], const double *v, double *o) {
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (M[0][c] * v[0] + M[1][c] * v[1]) + M[2][c] * v[2];
}

// A^T B
__device__ __forceinline__ void mtm(const double (&A)[3][3], const double (&B)[3][3], double (&O)[3][3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) O[r][c] = (A[0][r] * B[0][c] + A[1][r] * B[1][c]) + A[2][r] * B[2][c];
}

template <typename T>
__device__ __forceinline__ void load_pos(const T *pose, double *x) {
    x[0] = (double)pose[3];
    x[1] = (double)pose[7];
    x[2] = (double)pose[11];
}

template <typename T>
__device__ __forceinline__ void load_rot(const T *pose, double (&R)[3][3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[r][c] = (double)pose[4 * r + c];
}

// one Jacobi rotation of the columns p, q of A (and of W with them); false: they are orthogonal already (or not comparable: NaN)
template <int P, int Q>
__device__ __forceinline__ bool rotate(double (&A)[3][3], double (&W)[3][3]) {
    const double alpha = dot3(A[P], A[P]), beta = dot3(A[Q], A[Q]), gamma = dot3(A[P], A[Q]);
    if (!(fabs(gamma) > kTiny * (sqrt(alpha) * sqrt(beta)))) return false;
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double ap = A[P][r], aq = A[Q][r], wp = W[P][r], wq = W[Q][r];
        A[P][r] = cs * ap - sn * aq;
        A[Q][r] = sn * ap + cs * aq;
        W[P][r] = cs * wp - sn * wq;
        W[Q][r] = sn * wp + cs * wq;
    }
    return true;
}

template <int P, int Q>
__device__ __forceinline__ void sort_pair(double (&A)[3][3], double (&W)[3][3], double *d) {
    if (d[P] < d[Q]) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double a = A[P][r], w = W[P][r];
            A[P][r] = A[Q][r];
            A[Q][r] = a;
            W[P][r] = W[Q][r];
            W[Q][r] = w;
        }
        const double t = d[P];
        d[P] = d[Q];
        d[Q] = t;
    }
}

__device__ __forceinline__ void write_degenerate(int lane, int b, double *metrics, int *valid, double *align) {
    if (lane != 0) return;
    metrics[3 * (size_t)b] = metrics[3 * (size_t)b + 1] = metrics[3 * (size_t)b + 2] = 0.0;
    valid[b] = 0;
    if (align) {
        double *o = align + 13 * (size_t)b;
#pragma unroll
        for (int k = 0; k < 12; ++k) o[k] = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
        o[12] = 1.0;
    }
}

template <typename T>
__global__ void __launch_bounds__(kWave) trajectory_metrics_kernel(const T *__restrict__ pred, const T *__restrict__ gt, int V, int delta,
                                                                   double *__restrict__ metrics, int *__restrict__ valid,
                                                                   double *__restrict__ align) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const T *P = pred + (size_t)b * V * 16, *Q = gt + (size_t)b * V * 16;
    const double Vd = (double)V;

    // ---- pass 1: the position sums, and is every element finite
    dd sx[3] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}}, sy[3] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
    bool bad = false;
    for (int i = lane; i < V; i += kWave) {
        const T *p = P + (size_t)i * 16, *q = Q + (size_t)i * 16;
#pragma unroll
        for (int e = 0; e < 16; ++e) bad |= !(finite((double)p[e]) && finite((double)q[e]));
        double x[3], y[3];
        load_pos(p, x);
        load_pos(q, y);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            dd_add(sx[k], x[k]);
            dd_add(sy[k], y[k]);
        }
    }
    if (V < 3 || delta >= V || __ballot(bad) != 0ull) {      // uniform: every lane leaves
        write_degenerate(lane, b, metrics, valid, align);
        return;
    }
    double mux[3], muy[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        mux[k] = dd_div(dd_wave_sum(sx[k]), Vd);
        muy[k] = dd_div(dd_wave_sum(sy[k]), Vd);
    }

    // ---- pass 2: sigma_x^2 and C[r][c] = mean (y - mu_y)_r (x - mu_x)_c
    dd s2 = {0.0, 0.0}, sc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) sc[k] = {0.0, 0.0};
    for (int i = lane; i < V; i += kWave) {
        double x[3], y[3];
        load_pos(P + (size_t)i * 16, x);
        load_pos(Q + (size_t)i * 16, y);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            x[k] -= mux[k];
            y[k] -= muy[k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) dd_add_prod(s2, x[k], x[k]);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) dd_add_prod(sc[3 * r + c], y[r], x[c]);
    }
    const double sig2 = dd_div(dd_wave_sum(s2), Vd);
    // A[k] = column k of C, W[k] = column k of the right singular vectors (the identity to start with)
    double A[3][3], W[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) A[c][r] = dd_div(dd_wave_sum(sc[3 * r + c]), Vd);

    // ---- the 3 x 3 SVD: C W = A with orthogonal columns
    for (int sweep = 0; sweep < kMaxSweeps; ++sweep) {
        bool any = rotate<0, 1>(A, W);
        any |= rotate<0, 2>(A, W);
        any |= rotate<1, 2>(A, W);
        if (!any) break;
    }
    double d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = sqrt(dot3(A[k], A[k]));
    sort_pair<0, 1>(A, W, d);
    sort_pair<1, 2>(A, W, d);
    sort_pair<0, 1>(A, W, d);
    const int rank = (d[0] > kTiny) + (d[1] > kTiny) + (d[2] > kTiny);
    if (rank < 2) {      // uniform: every lane holds the same d
        write_degenerate(lane, b, metrics, valid, align);
        return;
    }
    double u1[3], u2[3], u3[3], v3[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        u1[r] = A[0][r] / d[0];
        u2[r] = A[1][r] / d[1];
    }
    cross3(u1, u2, u3);
    cross3(W[0], W[1], v3);
    const double nu = sqrt(dot3(u3, u3)), nv = sqrt(dot3(v3, v3));
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        u3[r] /= nu;
        v3[r] /= nv;
    }
    // U = [u1 u2 su u3], V = [w0 w1 sv v3] with the signs of the Jacobi columns: det U = su, det V = sv, S_33 = su sv, so the third term of
    // U S V^T is u3 v3^T whatever the signs are, and only tr(diag(d) S) reads S_33
    const double su = dot3(A[2], u3) < 0.0 ? -1.0 : 1.0, sv = dot3(W[2], v3) < 0.0 ? -1.0 : 1.0;
    const double s33 = su * sv;
    double R[3][3], t[3], Rmu[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[r][c] = (u1[r] * W[0][c] + u2[r] * W[1][c]) + u3[r] * v3[c];
    const double scale = ((d[0] + d[1]) + s33 * d[2]) / sig2;
    mv(R, mux, Rmu);
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = muy[k] - scale * Rmu[k];

    // ---- pass 3: ATE residuals and RPE pairs
    dd se = {0.0, 0.0}, st = {0.0, 0.0}, sr = {0.0, 0.0};
    const int npairs = V - delta;
    for (int i = lane; i < V; i += kWave) {
        const T *pi = P + (size_t)i * 16, *qi = Q + (size_t)i * 16;
        double xi[3], yi[3], Rx[3], res[3];
        load_pos(pi, xi);
        load_pos(qi, yi);
        mv(R, xi, Rx);
#pragma unroll
        for (int k = 0; k < 3; ++k) res[k] = (scale * Rx[k] + t[k]) - yi[k];
        dd_add(se, dot3(res, res));
        if (i < npairs) {
            const T *pj = pi + (size_t)delta * 16, *qj = qi + (size_t)delta * 16;      // j = i + delta < V
            double xj[3], yj[3], Rpi[3][3], Rpj[3][3], Rqi[3][3], Rqj[3][3], RA[3][3], RB[3][3], E[3][3], a[3], bt[3], Et[3];
            load_pos(pj, xj);
            load_pos(qj, yj);
            load_rot(pi, Rpi);
            load_rot(pj, Rpj);
            load_rot(qi, Rqi);
            load_rot(qj, Rqj);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                xj[k] -= xi[k];
                yj[k] -= yi[k];
            }
            mtm(Rqi, Rqj, RA);
            mtv(Rqi, yj, a);
            mtm(Rpi, Rpj, RB);
            mtv(Rpi, xj, bt);
#pragma unroll
            for (int k = 0; k < 3; ++k) bt[k] = scale * bt[k] - a[k];
            mtm(RA, RB, E);
            mtv(RA, bt, Et);
            const double w[3] = {E[2][1] - E[1][2], E[0][2] - E[2][0], E[1][0] - E[0][1]};
            const double sn = 0.5 * sqrt(dot3(w, w)), cs = 0.5 * (((E[0][0] + E[1][1]) + E[2][2]) - 1.0);
            const double deg = atan2(sn, cs) * kDeg;
            dd_add(st, dot3(Et, Et));
            dd_add(sr, deg * deg);
        }
    }
    const double ate = sqrt(dd_div(dd_wave_sum(se), Vd));
    const double rpe_t = sqrt(dd_div(dd_wave_sum(st), (double)npairs));
    const double rpe_r = sqrt(dd_div(dd_wave_sum(sr), (double)npairs));
    if (lane == 0) {
        metrics[3 * (size_t)b] = ate;
        metrics[3 * (size_t)b + 1] = rpe_t;
        metrics[3 * (size_t)b + 2] = rpe_r;
        valid[b] = 1;
        if (align) {
            double *o = align + 13 * (size_t)b;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c) o[3 * r + c] = R[r][c];
                o[9 + r] = t[r];
            }
            o[12] = scale;
        }
    }
}

}  // namespace

extern "C" int vsm_trajectory_metrics(const void *pred, const void *gt, int32_t dtype, int32_t B, int32_t V, int32_t delta, double *metrics,
                                      int32_t *valid, double *align, vs_stream_t stream_) {
    const char *who = "vsm_trajectory_metrics";
    VS_CHECK(pred && gt && metrics && valid, "%s: null pointer (pred, gt, metrics and valid are required; align may be null)", who);
    VS_CHECK(dtype == kDtypeF32 || dtype == kDtypeF64, "%s: dtype %d is neither %d (f32) nor %d (f64)", who, dtype, kDtypeF32, kDtypeF64);
    VS_CHECK(B >= 0 && V >= 1 && delta >= 1, "%s: B = %d, V = %d, delta = %d: B must not be negative, V and delta must be at least 1", who, B, V,
             delta);
    if (B == 0) return 0;
    const hipStream_t stream = (hipStream_t)stream_;
    if (dtype == kDtypeF32)
        hipLaunchKernelGGL(trajectory_metrics_kernel<float>, dim3(B), dim3(kWave), 0, stream, (const float *)pred, (const float *)gt, V, delta,
                           metrics, valid, align);
    else
        hipLaunchKernelGGL(trajectory_metrics_kernel<double>, dim3(B), dim3(kWave), 0, stream, (const double *)pred, (const double *)gt, V, delta,
                           metrics, valid, align);
    VS_HIP(hipGetLastError());
    return 0;
}
