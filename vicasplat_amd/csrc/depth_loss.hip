// Depth-smoothness loss: LossDepth of src/loss/loss_depth.py:34-60, forward and backward, f32.  Declared in include/vicasplat_loss.h
// (prefix vsl_).
//
//   logs     log(near), log(far), once per view (correctly rounded: formed in f64).
//   tile     one workgroup per (view, band of kBandRows rows, chunk of kChunkCols columns).  It stages the normalised depth d (and the three
//            colour planes when the bilateral weights are on) of its tile plus a halo in LDS -- 16-byte loads when every row is 16-byte
//            aligned (W % 4 == 0), scalar loads otherwise --, then forms every difference term that touches its pixels ONCE: the weighted
//            term t, |t| into the loss partial of the tile that owns the term (the tile that holds its first pixel), and dL/dt = sign(t)
//            weight / count x the bilateral weight into LDS.  Last, each pixel GATHERS its own 1 + s terms per side and direction from LDS
//            (torch's order: diff backward of diff backward), adds the two directions, divides by lf - ln, applies the clamp's subgradient
//            and writes the gradient for an upstream factor of 1.  There is no scatter and there are no float atomics.
//   finish   one workgroup: the tiles' partials in a fixed order (in f64: they are few), the two means, the weight.
//   scale    the backward: grad_loss x the gradient image.
// The same inputs give the same bits.
#include "common.h"

#include "../../include/vicasplat_loss.h"

namespace {

constexpr int kThreads = 256;
// ops.DEPTH_SMOOTH_BAND_ROWS / ops.DEPTH_SMOOTH_CHUNK_COLS (vicasplat_amd/ops.py) are the twins of the next two: change them together (the
// tests take their tile-edge shapes from there).
constexpr int kBandRows = 16;
constexpr int kChunkCols = 64;
constexpr int kHaloRows = 2;      // 1 + s rows above and below
constexpr int kHaloCols = 4;      // 1 + s columns are needed left and right; four keep every 16-byte load aligned
constexpr int kTileRows = kBandRows + 2 * kHaloRows;
constexpr int kTileCols = kChunkCols + 2 * kHaloCols;
constexpr int kTermCols = kChunkCols + 2;      // x terms of a tile: those that start at its columns and at the two columns left of it
constexpr int kTermRows = kBandRows + 2;       // y terms: likewise, two rows above
static_assert(kBandRows * (kChunkCols / 4) == kThreads, "the gather gives each thread four consecutive pixels of one row");

struct Args {
    const float *depth, *image;
    float *gimg;      // null: the loss alone
    int H, W, second;
    float sigma, kx, ky;      // kx = weight / count of x terms, ky likewise: d loss / d |t|
};

// torch.minimum / torch.maximum: a NaN operand gives NaN (fminf / fmaxf would drop it)
__device__ __forceinline__ float min_t(float a, float b) { return (a != a || b != b) ? a + b : (a < b ? a : b); }
__device__ __forceinline__ float max_t(float a, float b) { return (a != a || b != b) ? a + b : (a > b ? a : b); }

__device__ __forceinline__ float normalise(float x, float ln, float lf, float den) { return (max_t(min_t(x, lf), ln) - ln) / den; }

// d |t| / dt times k, as torch forms it: k * sgn(t)
__device__ __forceinline__ float sign_times(float t, float k) { return t > 0.f ? k : t < 0.f ? -k : t == 0.f ? k * 0.f : t; }

__global__ void __launch_bounds__(kThreads) depth_smooth_logs_kernel(const float *__restrict__ near, const float *__restrict__ far, int N,
                                                                     float *__restrict__ logs) {
    const int n = blockIdx.x * kThreads + threadIdx.x;
    if (n < N) {
        // through f64: the correctly rounded f32 logarithm, so that "depth equals log far" names one f32 value on every device (the clamp's
        // tie passes half the gradient); two logarithms per view cost nothing
        logs[2 * n] = (float)log((double)near[n]);
        logs[2 * n + 1] = (float)log((double)far[n]);
    }
}

template <bool VEC, bool IMG>
__global__ void __launch_bounds__(kThreads) depth_smooth_tile_kernel(Args a, const float *__restrict__ logs, float *__restrict__ part) {
    constexpr int kColourRows = IMG ? 3 * kTileRows : 1;
    __shared__ __attribute__((aligned(16))) float sd[kTileRows][kTileCols];
    __shared__ __attribute__((aligned(16))) float sc[kColourRows][kTileCols];      // plane ch at rows ch * kTileRows ...
    __shared__ float ssx[kBandRows][kTermCols];
    __shared__ float ssy[kTermRows][kChunkCols];
    __shared__ float sm[4][2];
    const int n = blockIdx.z, r0 = blockIdx.y * kBandRows, c0 = blockIdx.x * kChunkCols, tid = threadIdx.x;
    const int H = a.H, W = a.W, s = a.second;
    const float ln = logs[2 * n], lf = logs[2 * n + 1], den = lf - ln;
    const size_t plane = (size_t)H * W;
    const float *dep = a.depth + (size_t)n * plane;
    const float *img = IMG ? a.image + (size_t)n * 3 * plane : nullptr;

    // ---- stage the tile: LDS row r is image row r0 - kHaloRows + r, LDS column c is image column c0 - kHaloCols + c; zeros outside the image
    if (VEC) {
        for (int idx = tid; idx < kTileRows * (kTileCols / 4); idx += kThreads) {
            const int r = idx / (kTileCols / 4), q = idx % (kTileCols / 4);
            const int gi = r0 - kHaloRows + r, gj = c0 - kHaloCols + 4 * q;
            const bool in = gi >= 0 && gi < H && gj >= 0 && gj < W;      // W % 4 == 0 and gj % 4 == 0: gj < W puts gj + 3 inside too
            const size_t off = in ? (size_t)gi * W + gj : 0;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (in) {
                v = *reinterpret_cast<const float4 *>(dep + off);
                v.x = normalise(v.x, ln, lf, den);
                v.y = normalise(v.y, ln, lf, den);
                v.z = normalise(v.z, ln, lf, den);
                v.w = normalise(v.w, ln, lf, den);
            }
            *reinterpret_cast<float4 *>(&sd[r][4 * q]) = v;
            if (IMG) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (in) c = *reinterpret_cast<const float4 *>(img + ch * plane + off);
                    *reinterpret_cast<float4 *>(&sc[ch * kTileRows + r][4 * q]) = c;
                }
            }
        }
    } else {
        for (int idx = tid; idx < kTileRows * kTileCols; idx += kThreads) {
            const int r = idx / kTileCols, c = idx % kTileCols;
            const int gi = r0 - kHaloRows + r, gj = c0 - kHaloCols + c;
            const bool in = gi >= 0 && gi < H && gj >= 0 && gj < W;
            const size_t off = in ? (size_t)gi * W + gj : 0;
            sd[r][c] = in ? normalise(dep[off], ln, lf, den) : 0.f;
            if (IMG) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) sc[ch * kTileRows + r][c] = in ? img[ch * plane + off] : 0.f;
            }
        }
    }
    __syncthreads();

    // ---- the terms.  An x term (i, k) spans the columns k .. k + 1 + s of row i; it exists when those lie inside the image.
    float acc[2] = {0.f, 0.f};
    for (int idx = tid; idx < kBandRows * kTermCols; idx += kThreads) {
        const int ty = idx / kTermCols, kk = idx % kTermCols;
        const int i = r0 + ty, k = c0 - 2 + kk;
        const int r = ty + kHaloRows, c = kk - 2 + kHaloCols;
        float g = 0.f;
        if (i < H && k >= 0 && k + 1 + s < W) {
            float t = sd[r][c + 1] - sd[r][c];
            if (s) t = (sd[r][c + 2] - sd[r][c + 1]) - t;
            float w = 1.f;
            if (IMG) {
                auto cdiff = [&](int cc) {
                    return max_t(max_t(sc[r][cc + 1] - sc[r][cc], sc[kTileRows + r][cc + 1] - sc[kTileRows + r][cc]),
                                 sc[2 * kTileRows + r][cc + 1] - sc[2 * kTileRows + r][cc]);
                };
                float cm = cdiff(c);
                if (s) cm = max_t(cdiff(c + 1), cm);
                w = expf(-cm * a.sigma);
                t *= w;
            }
            if (k >= c0) acc[0] += fabsf(t);      // the tile that holds the term's first pixel counts it
            g = sign_times(t, a.kx);
            if (IMG) g *= w;
        }
        ssx[ty][kk] = g;
    }
    for (int idx = tid; idx < kTermRows * kChunkCols; idx += kThreads) {
        const int rr = idx / kChunkCols, tx = idx % kChunkCols;
        const int k = r0 - 2 + rr, j = c0 + tx;
        const int r = rr - 2 + kHaloRows, c = tx + kHaloCols;
        float g = 0.f;
        if (j < W && k >= 0 && k + 1 + s < H) {
            float t = sd[r + 1][c] - sd[r][c];
            if (s) t = (sd[r + 2][c] - sd[r + 1][c]) - t;
            float w = 1.f;
            if (IMG) {
                auto cdiff = [&](int rw) {
                    return max_t(max_t(sc[rw + 1][c] - sc[rw][c], sc[kTileRows + rw + 1][c] - sc[kTileRows + rw][c]),
                                 sc[2 * kTileRows + rw + 1][c] - sc[2 * kTileRows + rw][c]);
                };
                float cm = cdiff(r);
                if (s) cm = max_t(cdiff(r + 1), cm);
                w = expf(-cm * a.sigma);
                t *= w;
            }
            if (k >= r0) acc[1] += fabsf(t);
            g = sign_times(t, a.ky);
            if (IMG) g *= w;
        }
        ssy[rr][tx] = g;
    }

    // ---- the tile's two partial sums, in a fixed order
    const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        float v = acc[q];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
        if (lane == 0) sm[wv][q] = v;
    }
    __syncthreads();      // also: ssx and ssy are complete
    if (tid < 2) {
        const size_t wg = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        part[2 * wg + tid] = (sm[0][tid] + sm[1][tid]) + (sm[2][tid] + sm[3][tid]);
    }
    if (!a.gimg) return;

    // ---- the gradient: pixel (i, j) gathers the terms it takes part in
    const int ty = tid / (kChunkCols / 4), tx0 = (tid % (kChunkCols / 4)) * 4;
    const int i = r0 + ty, j0 = c0 + tx0;
    if (i >= H || j0 >= W) return;
    float g[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int tx = tx0 + e, kk = tx + 2, rr = ty + 2;
        float gx, gy;
        if (s) {
            gx = (ssx[ty][kk - 2] - ssx[ty][kk - 1]) - (ssx[ty][kk - 1] - ssx[ty][kk]);
            gy = (ssy[rr - 2][tx] - ssy[rr - 1][tx]) - (ssy[rr - 1][tx] - ssy[rr][tx]);
        } else {
            gx = ssx[ty][kk - 1] - ssx[ty][kk];
            gy = ssy[rr - 1][tx] - ssy[rr][tx];
        }
        g[e] = (gx + gy) / den;
    }
    // through the clamp: maximum(minimum(x, lf), ln); a tie passes half, the losing side an exact zero
    auto through_clamp = [&](float grad, float x) {
        const float m = min_t(x, lf);
        const float f = (m < ln ? 0.f : m == ln ? 0.5f : 1.f) * (x > lf ? 0.f : x == lf ? 0.5f : 1.f);
        return f == 0.f ? 0.f : grad * f;
    };
    const size_t off = (size_t)i * W + j0;
    float *out = a.gimg + (size_t)n * plane + off;
    if (VEC) {
        const float4 x = *reinterpret_cast<const float4 *>(dep + off);
        *reinterpret_cast<float4 *>(out) =
            make_float4(through_clamp(g[0], x.x), through_clamp(g[1], x.y), through_clamp(g[2], x.z), through_clamp(g[3], x.w));
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (j0 + e < W) out[e] = through_clamp(g[e], dep[off + e]);
    }
}

__global__ void __launch_bounds__(1024) depth_smooth_finish_kernel(const float *__restrict__ part, int nparts, float weight, float count_x,
                                                                   float count_y, float *__restrict__ loss) {
    __shared__ double sm[16][2];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double t[2] = {0.0, 0.0};
    for (int p = tid; p < nparts; p += 1024) {
        t[0] += (double)part[2 * (size_t)p];
        t[1] += (double)part[2 * (size_t)p + 1];
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) t[q] += __shfl_xor(t[q], m, 64);
        if (lane == 0) sm[wv][q] = t[q];
    }
    __syncthreads();
    if (tid == 0) {
        double s0 = 0.0, s1 = 0.0;
        for (int w = 0; w < 16; ++w) { s0 += sm[w][0]; s1 += sm[w][1]; }
        *loss = weight * ((float)s0 / count_x + (float)s1 / count_y);      // each mean: the sum over its count, as torch's
    }
}

template <bool VEC>
__global__ void __launch_bounds__(kThreads) depth_smooth_scale_kernel(const float *unit, const float *__restrict__ grad_loss, int64_t count,
                                                                      float *out) {
    const float up = grad_loss[0];
    const int64_t step = (int64_t)gridDim.x * kThreads;
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < count; p += step) {
        if (VEC) {
            float4 v = reinterpret_cast<const float4 *>(unit)[p];
            v.x *= up; v.y *= up; v.z *= up; v.w *= up;
            reinterpret_cast<float4 *>(out)[p] = v;
        } else {
            out[p] = up * unit[p];
        }
    }
}

struct Shape {
    int bands, chunks;
    int64_t tiles, words;      // workspace: logs [N][2] | partials [tiles][2]
};

int shape_of(const char *who, int32_t N, int32_t H, int32_t W, Shape *sh) {
    VS_CHECK(N > 0 && H > 0 && W > 0, "%s: N = %d, H = %d, W = %d must be positive", who, N, H, W);
    sh->bands = vs::cdiv(H, kBandRows);
    sh->chunks = vs::cdiv(W, kChunkCols);
    sh->tiles = (int64_t)N * sh->bands * sh->chunks;
    VS_CHECK(N <= 65535 && sh->bands <= 65535 && sh->tiles <= INT32_MAX / 2, "%s: N = %d views of %d x %d are too many tiles for one launch", who, N,
             H, W);
    sh->words = 2 * (int64_t)N + 2 * sh->tiles;
    return 0;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int64_t vsl_depth_smooth_workspace_bytes(int32_t N, int32_t H, int32_t W) {
    Shape sh;
    if (shape_of("vsl_depth_smooth_workspace_bytes", N, H, W, &sh)) return -1;
    return sh.words * 4;
}

extern "C" int vsl_depth_smooth_forward(const float *depth, const float *near, const float *far, const float *image, int32_t N, int32_t H,
                                        int32_t W, float sigma_image, int32_t use_second_derivative, float weight, void *workspace,
                                        int64_t workspace_bytes, float *loss, float *d_depth_unit, vs_stream_t stream_) {
    const char *who = "vsl_depth_smooth_forward";
    VS_CHECK(depth && near && far && loss, "%s: null pointer (depth, near, far and loss are required)", who);
    Shape sh;
    if (shape_of(who, N, H, W, &sh)) return -1;
    const int s = use_second_derivative != 0;
    VS_CHECK(H >= 2 + s && W >= 2 + s, "%s: %d x %d is too small: a %s difference needs at least %d rows and columns (an empty mean is NaN in torch)",
             who, H, W, s ? "second" : "first", 2 + s);
    VS_CHECK(workspace, "%s: null workspace (size: vsl_depth_smooth_workspace_bytes)", who);
    VS_CHECK(workspace_bytes >= sh.words * 4, "%s: workspace of %lld bytes, %lld needed", who, (long long)workspace_bytes, (long long)sh.words * 4);
    VS_CHECK(((uintptr_t)workspace & 3) == 0, "%s: workspace is not 4-byte aligned", who);
    const hipStream_t stream = (hipStream_t)stream_;
    float *logs = (float *)workspace, *part = logs + 2 * (size_t)N;
    const float count_x = (float)((int64_t)N * H * (W - 1 - s)), count_y = (float)((int64_t)N * (H - 1 - s) * W);
    Args a;
    a.depth = depth; a.image = image; a.gimg = d_depth_unit;
    a.H = H; a.W = W; a.second = s;
    a.sigma = sigma_image; a.kx = weight / count_x; a.ky = weight / count_y;
    hipLaunchKernelGGL(depth_smooth_logs_kernel, dim3(vs::cdiv(N, kThreads)), dim3(kThreads), 0, stream, near, far, N, logs);
    VS_HIP(hipGetLastError());
    const bool vec = W % 4 == 0 && aligned16(depth) && (!image || aligned16(image)) && (!d_depth_unit || aligned16(d_depth_unit));
    const dim3 grid(sh.chunks, sh.bands, N), block(kThreads);
    if (image) {
        if (vec) hipLaunchKernelGGL((depth_smooth_tile_kernel<true, true>), grid, block, 0, stream, a, logs, part);
        else hipLaunchKernelGGL((depth_smooth_tile_kernel<false, true>), grid, block, 0, stream, a, logs, part);
    } else {
        if (vec) hipLaunchKernelGGL((depth_smooth_tile_kernel<true, false>), grid, block, 0, stream, a, logs, part);
        else hipLaunchKernelGGL((depth_smooth_tile_kernel<false, false>), grid, block, 0, stream, a, logs, part);
    }
    VS_HIP(hipGetLastError());
    hipLaunchKernelGGL(depth_smooth_finish_kernel, dim3(1), dim3(1024), 0, stream, part, (int)sh.tiles, weight, count_x, count_y, loss);
    VS_HIP(hipGetLastError());
    return 0;
}

extern "C" int vsl_depth_smooth_backward(const float *d_depth_unit, const float *grad_loss, int32_t N, int32_t H, int32_t W, float *d_depth,
                                         vs_stream_t stream_) {
    const char *who = "vsl_depth_smooth_backward";
    VS_CHECK(d_depth_unit && grad_loss && d_depth, "%s: null pointer", who);
    VS_CHECK(N > 0 && H > 0 && W > 0, "%s: N = %d, H = %d, W = %d must be positive", who, N, H, W);
    const int64_t count = (int64_t)N * H * W;
    const bool vec = count % 4 == 0 && aligned16(d_depth_unit) && aligned16(d_depth);
    const int64_t items = vec ? count / 4 : count;
    const int64_t want = vs::cdiv64(items, kThreads);
    const int grid = (int)(want < 2048 ? want : 2048);      // grid-stride beyond
    if (vec) hipLaunchKernelGGL(depth_smooth_scale_kernel<true>, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream_, d_depth_unit, grad_loss, items, d_depth);
    else hipLaunchKernelGGL(depth_smooth_scale_kernel<false>, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream_, d_depth_unit, grad_loss, items, d_depth);
    VS_HIP(hipGetLastError());
    return 0;
}
