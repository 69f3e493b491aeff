// View-overlap counts: for each ordered camera pair (i -> j), how many rays of camera i have an epipolar segment that crosses the image of
// camera j -- project_rays(...)["overlaps_image"].sum() of src/geometry/epipolar_lines.py:157-251 with near = far = None, the hot path of
// src/evaluation/evaluation_index_generator.py.  Declared in include/vicasplat_overlap.h (prefix vso_), where the closed form is written out.
//
//   grid = P x ceil(N / VSO_CHUNK) workgroups of VSO_THREADS threads; a workgroup takes VSO_CHUNK consecutive rays of one pair, a lane one
//   ray per trip.
//   prologue  every lane, redundantly and uniformly, in float64: M = inv(E_j) E_i (affine inverse, 3 x 3 by the adjugate), K_i^-1, the four
//             c_f; rounded once to f32 and moved to scalar registers (readfirstlane), with K_j and the pair's own flags
//   rays      f32, every operation rounded once in the order of the header (contraction is off in this file; division and square root
//             are the correctly rounded ones: see the Makefile's flags for this object and the #error below)
//   count     ballot + popcount per wave and trip, the waves summed in LDS, one integer atomicAdd per workgroup onto counts[p], which the
//             host zeroed with hipMemsetAsync on the same stream.  A pair with an index outside [0, V): -1, written by its first workgroup.
// Integer sums only: the same inputs give the same bits, alone or inside a list.
#include "common.h"

#include "../../include/vicasplat_overlap.h"

#pragma clang fp contract(off)

#ifdef __FAST_MATH__
#error "overlap.hip needs correctly rounded f32 division and square root: do not compile it with fast-math"
#endif

namespace {

constexpr int kWave = 64;
constexpr int kThreads = VSO_THREADS;
constexpr int kChunk = VSO_CHUNK;
constexpr int kDtypeF32 = 0, kDtypeF64 = 5;
constexpr float kEps = 1e-6f;                     // f32(1e-6): torch casts the Python scalar to the tensor's dtype
constexpr float kOnePlusEps = (float)(1.0 + 1e-6);   // `1 + epsilon` is formed in Python, then cast
constexpr float kEps32 = 0x1p-23f;                // torch.finfo(torch.float32).eps
constexpr float kInfinity = 1e8f;                 // project_camera_space's stand-in for +-inf

// a wave-uniform f32 value into a scalar register
__device__ __forceinline__ float uni(double v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, (float)v)));
}

__device__ __forceinline__ float nan_to_num(float v) {
    if (v != v) return 0.0f;
    if (v == __builtin_inff()) return kInfinity;
    if (v == -__builtin_inff()) return -kInfinity;
    return v;
}

__device__ __forceinline__ bool in_bounds(float v) { return v >= -kEps && v <= kOnePlusEps; }

// in_bounds(project(p)) for the camera whose first two intrinsic rows are k0, k1
__device__ __forceinline__ bool projects_inside(float px, float py, float pz, const float *k0, const float *k1) {
    const float den = pz + kEps32;
    const float q0 = nan_to_num(px / den), q1 = nan_to_num(py / den), q2 = nan_to_num(pz / den);
    const float x = (k0[0] * q0 + k0[1] * q1) + k0[2] * q2;
    const float y = (k1[0] * q0 + k1[1] * q1) + k1[2] * q2;
    return in_bounds(x) && in_bounds(y);
}

// one frame line: s the line's own axis, q the other; den = d_z o_s - d_s o_z
__device__ __forceinline__ bool crosses_line(float c, float os, float oq, float oz, float ds, float dq, float dz, float fo, float co,
                                             float den) {
    const float t = (c * oz - os) / (ds - c * dz);
    const float num = fo * (oq * (c * dz - ds) + dq * (os - c * oz));
    const float other = co + num / den;
    const float z = oz + t * dz;
    return in_bounds(other) && z > -kEps && t > -kEps;
}

template <typename T>
__global__ void __launch_bounds__(kThreads) view_overlap_kernel(const T *__restrict__ extrinsics, const T *__restrict__ intrinsics, int V, int H,
                                                                 int W, int chunks, const int *__restrict__ pairs, int *__restrict__ counts) {
    __shared__ int wave_count[kThreads / kWave];
    const int p = blockIdx.x / chunks, chunk = blockIdx.x - p * chunks;
    const int i = pairs[2 * (size_t)p], j = pairs[2 * (size_t)p + 1];
    if (i < 0 || i >= V || j < 0 || j >= V) {      // uniform over the pair's workgroups: nobody adds to counts[p]
        if (chunk == 0 && threadIdx.x == 0) counts[p] = -1;
        return;
    }

    // ---- the pair's constants, float64
    const T *Ei = extrinsics + (size_t)i * 16, *Ej = extrinsics + (size_t)j * 16;
    const T *Ki = intrinsics + (size_t)i * 9, *Kj = intrinsics + (size_t)j * 9;
    double A[3][3], B[3][3], dt[3], adj[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            A[r][c] = (double)Ej[4 * r + c];
            B[r][c] = (double)Ei[4 * r + c];
        }
        dt[r] = (double)Ei[4 * r + 3] - (double)Ej[4 * r + 3];
    }
    // adj(A)[r][c] = cofactor(c, r); inv(A) = adj(A) / det(A)
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;
            adj[r][c] = A[r1][c1] * A[r2][c2] - A[r1][c2] * A[r2][c1];
        }
    const double det = (A[0][0] * adj[0][0] + A[0][1] * adj[1][0]) + A[0][2] * adj[2][0];
    float R[3][3], o[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) R[r][c] = uni(((adj[r][0] * B[0][c] + adj[r][1] * B[1][c]) + adj[r][2] * B[2][c]) / det);
        o[r] = uni(((adj[r][0] * dt[0] + adj[r][1] * dt[1]) + adj[r][2] * dt[2]) / det);
    }
    float Kinv[3][3];
    {
        double K[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) K[r][c] = (double)Ki[3 * r + c];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;
                adj[r][c] = K[r1][c1] * K[r2][c2] - K[r1][c2] * K[r2][c1];
            }
        const double dk = (K[0][0] * adj[0][0] + K[0][1] * adj[1][0]) + K[0][2] * adj[2][0];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) Kinv[r][c] = uni(adj[r][c] / dk);
    }
    float k0[3], k1[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        k0[c] = uni((double)Kj[c]);
        k1[c] = uni((double)Kj[3 + c]);
    }
    const double fx = (double)Kj[0], cx = (double)Kj[2], fy = (double)Kj[4], cy = (double)Kj[5];
    const float cf[4] = {uni((0.0 - cx) / fx), uni((1.0 - cx) / fx), uni((0.0 - cy) / fy), uni((1.0 - cy) / fy)};

    // ---- the pair's own flags, f32
    const bool at_camera = sqrtf((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]) < kEps;
    const bool origin_valid = projects_inside(o[0], o[1], o[2], k0, k1) && o[2] > -kEps && !(o[2] < kEps);
    const float ox = at_camera ? 0.0f : o[0], oy = at_camera ? 0.0f : o[1], oz = at_camera ? 0.0f : o[2];

    // ---- the rays
    const int N = H * W;
    const float fw = (float)W, fh = (float)H;
    const int first = chunk * kChunk, last = min(first + kChunk, N);
    int count = 0;
    for (int base = first; base < last; base += kThreads) {      // uniform trip count: the ballot below sees every lane
        const int n = base + (int)threadIdx.x;
        bool overlaps = false;
        if (n < last) {
            const int r = n / W, c = n - r * W;
            const float x = ((float)c + 0.5f) / fw, y = ((float)r + 0.5f) / fh;
            float u0 = (Kinv[0][0] * x + Kinv[0][1] * y) + Kinv[0][2];
            float u1 = (Kinv[1][0] * x + Kinv[1][1] * y) + Kinv[1][2];
            float u2 = (Kinv[2][0] * x + Kinv[2][1] * y) + Kinv[2][2];
            const float norm = sqrtf((u0 * u0 + u1 * u1) + u2 * u2);
            u0 = u0 / norm;
            u1 = u1 / norm;
            u2 = u2 / norm;
            const float dx = (R[0][0] * u0 + R[0][1] * u1) + R[0][2] * u2;
            const float dy = (R[1][0] * u0 + R[1][1] * u1) + R[1][2] * u2;
            const float dz = (R[2][0] * u0 + R[2][1] * u1) + R[2][2] * u2;

            const bool valid_inf = projects_inside(dx, dy, dz, k0, k1) && dz > -kEps;
            const bool valid_0 = at_camera ? valid_inf : origin_valid;
            const float den_x = dz * ox - dx * oz, den_y = dz * oy - dy * oz;
            const bool any_f = crosses_line(cf[0], ox, oy, oz, dx, dy, dz, k1[1], k1[2], den_x) ||
                               crosses_line(cf[1], ox, oy, oz, dx, dy, dz, k1[1], k1[2], den_x) ||
                               crosses_line(cf[2], oy, ox, oz, dy, dx, dz, k0[0], k0[2], den_y) ||
                               crosses_line(cf[3], oy, ox, oz, dy, dx, dz, k0[0], k0[2], den_y);
            overlaps = (valid_0 && valid_inf) || any_f;
        }
        count += __popcll(__ballot(overlaps));
    }
    const int wave = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) wave_count[wave] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < kThreads / kWave; ++w) total += wave_count[w];
        if (total != 0) atomicAdd(counts + p, total);
    }
}

}  // namespace

extern "C" int vso_view_overlap_counts(const void *extrinsics, const void *intrinsics, int32_t dtype, int32_t V, int32_t H, int32_t W,
                                       const int32_t *pairs, int32_t P, int32_t *counts, vs_stream_t stream_) {
    const char *who = "vso_view_overlap_counts";
    VS_CHECK(dtype == kDtypeF32 || dtype == kDtypeF64, "%s: dtype %d is neither %d (f32) nor %d (f64)", who, dtype, kDtypeF32, kDtypeF64);
    VS_CHECK(V >= 1 && H >= 1 && W >= 1 && P >= 0, "%s: V = %d, H = %d, W = %d, P = %d: V, H and W must be at least 1, P must not be negative", who,
             V, H, W, P);
    VS_CHECK((int64_t)H * W <= (int64_t)1 << 30, "%s: H W = %lld rays exceed 2^30", who, (long long)((int64_t)H * W));
    if (P == 0) return 0;
    VS_CHECK(extrinsics && intrinsics && pairs && counts, "%s: null pointer (extrinsics, intrinsics, pairs and counts are required when P > 0)",
             who);
    const int chunks = vs::cdiv(H * W, kChunk);
    VS_CHECK((int64_t)P * chunks <= 2147483647LL, "%s: P = %d pairs of %d ray chunks exceed the grid limit 2^31 - 1", who, P, chunks);
    const hipStream_t stream = (hipStream_t)stream_;
    VS_HIP(hipMemsetAsync(counts, 0, (size_t)P * sizeof(int32_t), stream));
    const dim3 grid((unsigned)((int64_t)P * chunks));
    if (dtype == kDtypeF32)
        hipLaunchKernelGGL(view_overlap_kernel<float>, grid, dim3(kThreads), 0, stream, (const float *)extrinsics, (const float *)intrinsics, V, H,
                           W, chunks, pairs, counts);
    else
        hipLaunchKernelGGL(view_overlap_kernel<double>, grid, dim3(kThreads), 0, stream, (const double *)extrinsics, (const double *)intrinsics, V,
                           H, W, chunks, pairs, counts);
    VS_HIP(hipGetLastError());
    return 0;
}
