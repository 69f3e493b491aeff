// LPIPS-VGG (lpips.LPIPS(net="vgg", version="0.1") in eval mode; src/loss/loss_lpips.py:27-54, src/evaluation/metrics.py:37-44): the glue
// around the 13 split-class convolutions (vs_conv3x3_split_nhwc and its data gradient), forward and backward.
//
//   vs_lpips_prep            NCHW image -> optional 2x - 1 -> scaling layer (x - shift) / scale -> NHWC, channels zero-padded to 32
//   vs_lpips_prep_backward   the conv1_1 data gradient (NHWC, 32 channels) -> NCHW image gradient (first 3 channels, / scale, x 2 if normalized)
//   vs_lpips_maxpool         2 x 2 stride-2 max-pool, NHWC
//   vs_lpips_maxpool_backward  pool gradient routed to the first maximum of each window + the tap's head gradient, times the tap's ReLU mask
//   vs_lpips_head_forward    the five taps of both images -> per-image distance (unit-normalised channel vectors, weighted squared
//                            differences, spatial mean, sum over taps)
//   vs_lpips_head_backward   dL/df of either image at the five taps, times the tap's ReLU mask
//
// Conventions (ABI 10):
//   * zero-norm pixels: where a tap's whole channel vector is 0, d n / d f = I / (r + eps) with the rank-one term dropped (torch autograd
//     returns NaN there: the backward of sqrt at 0 is 0 / 0).  Such a pixel is a dead ReLU column, so its ReLU mask zeroes the result anyway.
//   * max-pool ties go to the first maximum in row-major window order, as torch's max_pool2d does (a NaN wins, as there).
//   * gradient scale: the backward runs on a power-of-two scaled gradient, so the split class's f16 (hi, lo) halves of the data gradients stay
//     normal.  Image n's upstream gradient g[n] = m 2^e (frexp) enters the heads as m 2^scale_log2, and vs_lpips_prep_backward multiplies by
//     2^(e - scale_log2); every step between is linear, so the scale cancels exactly.
// Determinism: no atomics.  The head forward writes one f32 partial per workgroup; lpips_reduce_kernel sums them in a fixed order in f64.
#include <cmath>

#include "common.h"

// No contraction of a * b - c * d into an FMA: the heads' differences n0 - n1 must be exactly 0 when the two images' taps are equal (an
// FMA keeps the rounding error of one product), so that LPIPS(x, x) and its gradient are exactly 0.
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kTaps = 5;
constexpr int kCin0 = 32;             // conv1_1 input channels after padding (vs_conv3x3_split_nhwc: Cin % 32 == 0)
constexpr int kChunk = 128;           // head forward: pixels per workgroup
constexpr float kEps = 1e-10f;        // lpips normalize_tensor
constexpr int kTapC[kTaps] = {64, 128, 256, 512, 512};

// lpips ScalingLayer (lpips/pretrained_networks / lpips.py: shift, scale buffers)
__device__ __forceinline__ float lp_shift(int c) { return c == 0 ? -0.030f : (c == 1 ? -0.088f : -0.188f); }
__device__ __forceinline__ float lp_scale(int c) { return c == 0 ? 0.458f : (c == 1 ? 0.448f : 0.450f); }

__global__ void __launch_bounds__(kThreads) lpips_prep_kernel(const float *__restrict__ img, int64_t P, int HW, int normalize,
                                                              float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= P) return;
    const int64_t n = i / HW, p = i - n * HW;
    const float *src = img + n * 3 * HW + p;
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float x = src[(int64_t)c * HW];
        if (normalize) x = 2.f * x - 1.f;
        v[c] = (x - lp_shift(c)) / lp_scale(c);
    }
    float4 *o = reinterpret_cast<float4 *>(out + i * kCin0);
    o[0] = make_float4(v[0], v[1], v[2], 0.f);
#pragma unroll
    for (int k = 1; k < kCin0 / 4; ++k) o[k] = make_float4(0.f, 0.f, 0.f, 0.f);
}

__global__ void __launch_bounds__(kThreads) lpips_prep_backward_kernel(const float *__restrict__ g32, const float *__restrict__ g, int64_t P,
                                                                       int HW, int normalize, int scale_log2, float *__restrict__ dimg) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= P) return;
    const int64_t n = i / HW, p = i - n * HW;
    int e;
    frexpf(g[n], &e);
    const float4 d = *reinterpret_cast<const float4 *>(g32 + i * kCin0);
    const float dv[3] = {d.x, d.y, d.z};
    float *dst = dimg + n * 3 * HW + p;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = dv[c] / lp_scale(c);
        dst[(int64_t)c * HW] = ldexpf(normalize ? 2.f * v : v, e - scale_log2);
    }
}

// window order (0,0) (0,1) (1,0) (1,1); strict > keeps the first maximum (torch: `val > maxval || isnan(val)`)
__device__ __forceinline__ int first_max(float a0, float a1, float a2, float a3, float *m) {
    int k = 0;
    float v = a0;
    if (a1 > v || isnan(a1)) { v = a1; k = 1; }
    if (a2 > v || isnan(a2)) { v = a2; k = 2; }
    if (a3 > v || isnan(a3)) { v = a3; k = 3; }
    *m = v;
    return k;
}

// thread = (pooled pixel, 4 channels); H, W of the INPUT (even)
__global__ void __launch_bounds__(kThreads) lpips_maxpool_kernel(const float *__restrict__ x, int64_t total, int Ho, int Wo, int C,
                                                                 float *__restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int C4 = C / 4;
    const int64_t q = i / C4;
    const int c4 = (int)(i - q * C4);
    const int64_t n = q / ((int64_t)Ho * Wo);
    const int rem = (int)(q - n * Ho * Wo), oy = rem / Wo, ox = rem - oy * Wo;
    const int W = 2 * Wo;
    const float *p00 = x + ((n * 2 * Ho + 2 * oy) * W + 2 * ox) * C + c4 * 4;
    const float4 a = *reinterpret_cast<const float4 *>(p00), b = *reinterpret_cast<const float4 *>(p00 + C);
    const float4 c = *reinterpret_cast<const float4 *>(p00 + (int64_t)W * C), d = *reinterpret_cast<const float4 *>(p00 + (int64_t)W * C + C);
    float4 r;
    first_max(a.x, b.x, c.x, d.x, &r.x);
    first_max(a.y, b.y, c.y, d.y, &r.y);
    first_max(a.z, b.z, c.z, d.z, &r.z);
    first_max(a.w, b.w, c.w, d.w, &r.w);
    *reinterpret_cast<float4 *>(y + q * C + c4 * 4) = r;
}

// dx[window j] = (x_j > 0) ? g_add_j + (j == first max ? dy : 0) : 0
__global__ void __launch_bounds__(kThreads) lpips_maxpool_backward_kernel(const float *__restrict__ dy, const float *__restrict__ x,
                                                                          const float *__restrict__ g_add, int64_t total, int Ho, int Wo,
                                                                          int C, float *__restrict__ dx) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int C4 = C / 4;
    const int64_t q = i / C4;
    const int c4 = (int)(i - q * C4);
    const int64_t n = q / ((int64_t)Ho * Wo);
    const int rem = (int)(q - n * Ho * Wo), oy = rem / Wo, ox = rem - oy * Wo;
    const int W = 2 * Wo;
    const int64_t o = ((n * 2 * Ho + 2 * oy) * W + 2 * ox) * C + c4 * 4;
    const int64_t off[4] = {o, o + C, o + (int64_t)W * C, o + (int64_t)W * C + C};
    float xv[4][4], gv[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float4 t = *reinterpret_cast<const float4 *>(x + off[j]);
        xv[j][0] = t.x; xv[j][1] = t.y; xv[j][2] = t.z; xv[j][3] = t.w;
        const float4 u = g_add ? *reinterpret_cast<const float4 *>(g_add + off[j]) : make_float4(0.f, 0.f, 0.f, 0.f);
        gv[j][0] = u.x; gv[j][1] = u.y; gv[j][2] = u.z; gv[j][3] = u.w;
    }
    const float4 d4 = *reinterpret_cast<const float4 *>(dy + q * C + c4 * 4);
    const float dv[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float m;
        const int arg = first_max(xv[0][k], xv[1][k], xv[2][k], xv[3][k], &m);
#pragma unroll
        for (int j = 0; j < 4; ++j) gv[j][k] = xv[j][k] > 0.f ? gv[j][k] + (j == arg ? dv[k] : 0.f) : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) *reinterpret_cast<float4 *>(dx + off[j]) = make_float4(gv[j][0], gv[j][1], gv[j][2], gv[j][3]);
}

// Lane layout of the heads: a pixel's C channels are spread over LP = min(64, C / 4) lanes, V float4 per lane; 64 / LP pixels per wave.
template <int C>
struct HeadShape {
    static constexpr int LP = C / 4 < 64 ? C / 4 : 64;
    static constexpr int V = C / (4 * LP);
    static constexpr int PPW = 64 / LP;
};

template <int LP>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int s = LP / 2; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

__device__ __forceinline__ float dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// One tap: per pixel d = sum_c w_c (f0_c / (r0 + eps) - f1_c / (r1 + eps))^2; one partial (the workgroup's sum over kChunk pixels) per
// workgroup at partials[n * nblk + blk].
template <int C>
__global__ void __launch_bounds__(kThreads) lpips_head_forward_kernel(const float *__restrict__ f0, const float *__restrict__ f1,
                                                                      const float *__restrict__ lin, int HW, int nblk,
                                                                      float *__restrict__ partials) {
    using S = HeadShape<C>;
    __shared__ float red[kThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int sub = lane % S::LP, grp = lane / S::LP;
    const int n = blockIdx.y, blk = blockIdx.x;
    float4 w[S::V];
#pragma unroll
    for (int v = 0; v < S::V; ++v) w[v] = *reinterpret_cast<const float4 *>(lin + (v * S::LP + sub) * 4);
    float acc = 0.f;
    for (int k = wid * S::PPW + grp; k < kChunk; k += 4 * S::PPW) {
        const int pix = blk * kChunk + k;
        const bool ok = pix < HW;
        const size_t base = ((size_t)n * HW + (ok ? pix : 0)) * C;
        float4 a[S::V], b[S::V];
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int v = 0; v < S::V; ++v) {
            const size_t o = base + (v * S::LP + sub) * 4;
            a[v] = ok ? *reinterpret_cast<const float4 *>(f0 + o) : make_float4(0.f, 0.f, 0.f, 0.f);
            b[v] = ok ? *reinterpret_cast<const float4 *>(f1 + o) : make_float4(0.f, 0.f, 0.f, 0.f);
            s0 += dot4(a[v], a[v]);
            s1 += dot4(b[v], b[v]);
        }
        s0 = group_sum<S::LP>(s0);
        s1 = group_sum<S::LP>(s1);
        const float i0 = 1.f / (sqrtf(s0) + kEps), i1 = 1.f / (sqrtf(s1) + kEps);
        float d = 0.f;
#pragma unroll
        for (int v = 0; v < S::V; ++v) {
            const float dx = a[v].x * i0 - b[v].x * i1, dy = a[v].y * i0 - b[v].y * i1;
            const float dz = a[v].z * i0 - b[v].z * i1, dw = a[v].w * i0 - b[v].w * i1;
            d += w[v].x * (dx * dx) + w[v].y * (dy * dy) + w[v].z * (dz * dz) + w[v].w * (dw * dw);
        }
        acc += group_sum<S::LP>(d);      // identical in every lane of the group
    }
    // one copy per pixel group, then the wave's groups in butterfly order, then the four waves in order
    float t = sub == 0 ? acc : 0.f;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) t += __shfl_xor(t, s);
    if (lane == 0) red[wid] = t;
    __syncthreads();
    if (tid == 0) partials[(size_t)n * nblk + blk] = (red[0] + red[1]) + (red[2] + red[3]);
}

struct TapLayout {
    int HW[kTaps], nblk[kTaps];
    int64_t off[kTaps];     // partials of tap s start at off[s] (N * nblk[s] of them)
};

// One workgroup per image: per tap the partials summed in f64 in a fixed order, / HW (spatial mean), summed over the taps.
__global__ void __launch_bounds__(kThreads) lpips_reduce_kernel(const float *__restrict__ partials, TapLayout t, float *__restrict__ out) {
    __shared__ double red[kThreads];
    const int n = blockIdx.x, tid = threadIdx.x;
    double total = 0.0;
    for (int s = 0; s < kTaps; ++s) {
        const float *src = partials + t.off[s] + (int64_t)n * t.nblk[s];
        double v = 0.0;
        for (int i = tid; i < t.nblk[s]; i += kThreads) v += (double)src[i];
        red[tid] = v;
        __syncthreads();
        for (int w = kThreads / 2; w > 0; w >>= 1) {
            if (tid < w) red[tid] += red[tid + w];
            __syncthreads();
        }
        total += red[0] / (double)t.HW[s];
        __syncthreads();
    }
    if (tid == 0) out[n] = (float)total;
}

// One tap: u = dL/dn0 = G 2 w (n0 - n1) = -dL/dn1 with G = mantissa(g[n]) * gscale (gscale = 2^scale_log2 / HW); then
// dL/df = u / t - f (sum_c u_c f_c) / (r t^2), t = r + eps (the rank-one term dropped at r = 0), times the ReLU mask f > 0.
template <int C>
__global__ void __launch_bounds__(kThreads) lpips_head_backward_kernel(const float *__restrict__ f0, const float *__restrict__ f1,
                                                                       const float *__restrict__ lin, const float *__restrict__ g, int HW,
                                                                       float gscale, float *__restrict__ d0, float *__restrict__ d1) {
    using S = HeadShape<C>;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int sub = lane % S::LP, grp = lane / S::LP;
    const int n = blockIdx.y;
    const int pix = (blockIdx.x * 4 + wid) * S::PPW + grp;
    const bool ok = pix < HW;
    int e;
    const float G = frexpf(g[n], &e) * gscale;
    float4 w[S::V], a[S::V], b[S::V];
    const size_t base = ((size_t)n * HW + (ok ? pix : 0)) * C;
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int v = 0; v < S::V; ++v) {
        const size_t o = base + (v * S::LP + sub) * 4;
        w[v] = *reinterpret_cast<const float4 *>(lin + (v * S::LP + sub) * 4);
        a[v] = ok ? *reinterpret_cast<const float4 *>(f0 + o) : make_float4(0.f, 0.f, 0.f, 0.f);
        b[v] = ok ? *reinterpret_cast<const float4 *>(f1 + o) : make_float4(0.f, 0.f, 0.f, 0.f);
        s0 += dot4(a[v], a[v]);
        s1 += dot4(b[v], b[v]);
    }
    s0 = group_sum<S::LP>(s0);
    s1 = group_sum<S::LP>(s1);
    const float r0 = sqrtf(s0), r1 = sqrtf(s1), t0 = r0 + kEps, t1 = r1 + kEps;
    const float i0 = 1.f / t0, i1 = 1.f / t1;
    float4 u[S::V];
    float p0 = 0.f, p1 = 0.f;
#pragma unroll
    for (int v = 0; v < S::V; ++v) {
        const float g2 = 2.f * G;
        u[v] = make_float4(g2 * w[v].x * (a[v].x * i0 - b[v].x * i1), g2 * w[v].y * (a[v].y * i0 - b[v].y * i1),
                           g2 * w[v].z * (a[v].z * i0 - b[v].z * i1), g2 * w[v].w * (a[v].w * i0 - b[v].w * i1));
        p0 += dot4(u[v], a[v]);
        p1 += dot4(u[v], b[v]);      // (sum of u1 f1 = -p1)
    }
    p0 = group_sum<S::LP>(p0);
    p1 = group_sum<S::LP>(p1);
    if (!ok) return;
    // side 0: d = u / t0 - a p0 / (r0 t0^2); side 1: u1 = -u, d = -u / t1 + b p1 / (r1 t1^2)
    const float k0 = r0 > 0.f ? p0 / (r0 * t0 * t0) : 0.f, k1 = r1 > 0.f ? p1 / (r1 * t1 * t1) : 0.f;
#pragma unroll
    for (int v = 0; v < S::V; ++v) {
        const size_t o = base + (v * S::LP + sub) * 4;
        if (d0) {
            float4 r;
            r.x = a[v].x > 0.f ? u[v].x * i0 - a[v].x * k0 : 0.f;
            r.y = a[v].y > 0.f ? u[v].y * i0 - a[v].y * k0 : 0.f;
            r.z = a[v].z > 0.f ? u[v].z * i0 - a[v].z * k0 : 0.f;
            r.w = a[v].w > 0.f ? u[v].w * i0 - a[v].w * k0 : 0.f;
            *reinterpret_cast<float4 *>(d0 + o) = r;
        }
        if (d1) {
            float4 r;
            r.x = b[v].x > 0.f ? b[v].x * k1 - u[v].x * i1 : 0.f;
            r.y = b[v].y > 0.f ? b[v].y * k1 - u[v].y * i1 : 0.f;
            r.z = b[v].z > 0.f ? b[v].z * k1 - u[v].z * i1 : 0.f;
            r.w = b[v].w > 0.f ? b[v].w * k1 - u[v].w * i1 : 0.f;
            *reinterpret_cast<float4 *>(d1 + o) = r;
        }
    }
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

int check_shape(int32_t N, int32_t H, int32_t W, const char *who) {
    VS_CHECK(N > 0 && H > 0 && W > 0, "%s: N = %d, H = %d, W = %d must be positive", who, N, H, W);
    VS_CHECK(H % 16 == 0 && W % 16 == 0, "%s: H = %d and W = %d must be multiples of 16 (four 2 x 2 max-pools)", who, H, W);
    VS_CHECK((int64_t)H * W <= INT32_MAX / 64 && (int64_t)N * H * W * 64 <= (int64_t)1 << 40, "%s: image too large", who);
    return 0;
}

TapLayout tap_layout(int32_t N, int32_t H, int32_t W) {
    TapLayout t;
    int64_t off = 0;
    for (int s = 0; s < kTaps; ++s) {
        t.HW[s] = (H >> s) * (W >> s);
        t.nblk[s] = vs::cdiv(t.HW[s], kChunk);
        t.off[s] = off;
        off += (int64_t)N * t.nblk[s];
    }
    return t;
}

int64_t workspace_floats(int32_t N, int32_t H, int32_t W) {
    const TapLayout t = tap_layout(N, H, W);
    return t.off[kTaps - 1] + (int64_t)N * t.nblk[kTaps - 1];
}

int check_taps(const float *const *f0, const float *const *f1, const float *const *lin, const char *who) {
    VS_CHECK(f0 && f1 && lin, "%s: null tap array (f0, f1 and lin each hold 5 device pointers)", who);
    for (int s = 0; s < kTaps; ++s) {
        VS_CHECK(f0[s] && f1[s] && lin[s], "%s: null pointer for tap %d", who, s + 1);
        VS_CHECK(aligned16(f0[s]) && aligned16(f1[s]) && aligned16(lin[s]), "%s: tap %d: 16-byte alignment required", who, s + 1);
    }
    return 0;
}

// one launch of KERNEL<C> for tap s (C = kTapC[s])
#define VS_LPIPS_TAP_LAUNCH(s, KERNEL, grid, stream, ...)                                                   \
    switch (kTapC[s]) {                                                                                     \
        case 64: hipLaunchKernelGGL((KERNEL<64>), grid, dim3(kThreads), 0, stream, __VA_ARGS__); break;     \
        case 128: hipLaunchKernelGGL((KERNEL<128>), grid, dim3(kThreads), 0, stream, __VA_ARGS__); break;   \
        case 256: hipLaunchKernelGGL((KERNEL<256>), grid, dim3(kThreads), 0, stream, __VA_ARGS__); break;   \
        default: hipLaunchKernelGGL((KERNEL<512>), grid, dim3(kThreads), 0, stream, __VA_ARGS__); break;    \
    }

}  // namespace

extern "C" int64_t vs_lpips_workspace_bytes(int32_t N, int32_t H, int32_t W) {
    if (check_shape(N, H, W, "vs_lpips_workspace_bytes")) return -1;
    return workspace_floats(N, H, W) * (int64_t)sizeof(float);
}

extern "C" int vs_lpips_prep(const float *img, int32_t N, int32_t H, int32_t W, int32_t normalize, float *out, vs_stream_t stream) {
    VS_CHECK(img && out, "vs_lpips_prep: null pointer (img and out are required)");
    if (check_shape(N, H, W, "vs_lpips_prep")) return -1;
    VS_CHECK(aligned16(out), "vs_lpips_prep: out must be 16-byte aligned");
    const int64_t P = (int64_t)N * H * W;
    hipLaunchKernelGGL(lpips_prep_kernel, dim3((unsigned)vs::cdiv64(P, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, img, P, H * W,
                       normalize ? 1 : 0, out);
    VS_HIP(hipGetLastError());
    return 0;
}

extern "C" int vs_lpips_prep_backward(const float *g32, const float *g, int32_t N, int32_t H, int32_t W, int32_t normalize, int32_t scale_log2,
                                      float *dimg, vs_stream_t stream) {
    VS_CHECK(g32 && g && dimg, "vs_lpips_prep_backward: null pointer (g32, g and dimg are required)");
    if (check_shape(N, H, W, "vs_lpips_prep_backward")) return -1;
    VS_CHECK(aligned16(g32), "vs_lpips_prep_backward: g32 must be 16-byte aligned");
    VS_CHECK(scale_log2 >= 0 && scale_log2 <= 64, "vs_lpips_prep_backward: scale_log2 = %d must be in [0, 64]", scale_log2);
    const int64_t P = (int64_t)N * H * W;
    hipLaunchKernelGGL(lpips_prep_backward_kernel, dim3((unsigned)vs::cdiv64(P, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, g32, g, P,
                       H * W, normalize ? 1 : 0, scale_log2, dimg);
    VS_HIP(hipGetLastError());
    return 0;
}

static int pool_args(const void *a, const void *b, const void *c, int32_t N, int32_t H, int32_t W, int32_t C, const char *who) {
    VS_CHECK(a && b, "%s: null pointer", who);
    VS_CHECK(N > 0 && H > 0 && W > 0 && C > 0 && H % 2 == 0 && W % 2 == 0 && C % 4 == 0,
             "%s: N = %d, H = %d, W = %d, C = %d: positive, H and W even, C a multiple of 4", who, N, H, W, C);
    VS_CHECK((int64_t)N * H * W * C <= (int64_t)1 << 40, "%s: tensor too large", who);
    VS_CHECK(aligned16(a) && aligned16(b) && aligned16(c), "%s: 16-byte alignment required", who);
    return 0;
}

extern "C" int vs_lpips_maxpool(const float *x, int32_t N, int32_t H, int32_t W, int32_t C, float *y, vs_stream_t stream) {
    if (pool_args(x, y, nullptr, N, H, W, C, "vs_lpips_maxpool")) return -1;
    const int64_t total = (int64_t)N * (H / 2) * (W / 2) * (C / 4);
    hipLaunchKernelGGL(lpips_maxpool_kernel, dim3((unsigned)vs::cdiv64(total, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, x, total,
                       H / 2, W / 2, C, y);
    VS_HIP(hipGetLastError());
    return 0;
}

extern "C" int vs_lpips_maxpool_backward(const float *dy, const float *x, const float *g_add, int32_t N, int32_t H, int32_t W, int32_t C,
                                         float *dx, vs_stream_t stream) {
    if (pool_args(dy, x, g_add, N, H, W, C, "vs_lpips_maxpool_backward")) return -1;
    VS_CHECK(dx && aligned16(dx), "vs_lpips_maxpool_backward: dx must be a 16-byte aligned device pointer");
    const int64_t total = (int64_t)N * (H / 2) * (W / 2) * (C / 4);
    hipLaunchKernelGGL(lpips_maxpool_backward_kernel, dim3((unsigned)vs::cdiv64(total, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, dy,
                       x, g_add, total, H / 2, W / 2, C, dx);
    VS_HIP(hipGetLastError());
    return 0;
}

extern "C" int vs_lpips_head_forward(const float *const *f0, const float *const *f1, const float *const *lin, int32_t N, int32_t H, int32_t W,
                                     float *workspace, float *out, vs_stream_t stream_) {
    if (check_taps(f0, f1, lin, "vs_lpips_head_forward")) return -1;
    if (check_shape(N, H, W, "vs_lpips_head_forward")) return -1;
    VS_CHECK(workspace && out, "vs_lpips_head_forward: null workspace or out (workspace size: vs_lpips_workspace_bytes)");
    VS_CHECK(N <= 65535, "vs_lpips_head_forward: N = %d exceeds 65535 images per call", N);
    const hipStream_t stream = (hipStream_t)stream_;
    const TapLayout t = tap_layout(N, H, W);
    for (int s = 0; s < kTaps; ++s) {
        VS_LPIPS_TAP_LAUNCH(s, lpips_head_forward_kernel, dim3(t.nblk[s], N), stream, f0[s], f1[s], lin[s], t.HW[s], t.nblk[s], workspace + t.off[s]);
        VS_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(lpips_reduce_kernel, dim3(N), dim3(kThreads), 0, stream, (const float *)workspace, t, out);
    VS_HIP(hipGetLastError());
    return 0;
}

extern "C" int vs_lpips_head_backward(const float *const *f0, const float *const *f1, const float *const *lin, const float *g, int32_t N,
                                      int32_t H, int32_t W, int32_t scale_log2, float *const *d0, float *const *d1, vs_stream_t stream_) {
    if (check_taps(f0, f1, lin, "vs_lpips_head_backward")) return -1;
    if (check_shape(N, H, W, "vs_lpips_head_backward")) return -1;
    VS_CHECK(g, "vs_lpips_head_backward: null g (the upstream gradient, [N] on the device)");
    VS_CHECK(d0 || d1, "vs_lpips_head_backward: null d0 and d1");
    VS_CHECK(N <= 65535, "vs_lpips_head_backward: N = %d exceeds 65535 images per call", N);
    VS_CHECK(scale_log2 >= 0 && scale_log2 <= 64, "vs_lpips_head_backward: scale_log2 = %d must be in [0, 64]", scale_log2);
    for (int s = 0; s < kTaps; ++s) {
        VS_CHECK(!d0 || (d0[s] && aligned16(d0[s])), "vs_lpips_head_backward: d0[%d] must be a 16-byte aligned device pointer", s);
        VS_CHECK(!d1 || (d1[s] && aligned16(d1[s])), "vs_lpips_head_backward: d1[%d] must be a 16-byte aligned device pointer", s);
    }
    const hipStream_t stream = (hipStream_t)stream_;
    const TapLayout t = tap_layout(N, H, W);
    for (int s = 0; s < kTaps; ++s) {
        const int ppb = 4 * (64 / (kTapC[s] / 4 < 64 ? kTapC[s] / 4 : 64));     // pixels per workgroup (HeadShape::PPW x 4 waves)
        const float gscale = (float)(std::ldexp(1.0, scale_log2) / (double)t.HW[s]);
        VS_LPIPS_TAP_LAUNCH(s, lpips_head_backward_kernel, dim3(vs::cdiv(t.HW[s], ppb), N), stream, f0[s], f1[s], lin[s], g, t.HW[s], gscale,
                                               d0 ? d0[s] : nullptr, d1 ? d1[s] : nullptr);
        VS_HIP(hipGetLastError());
    }
    return 0;
}
