// SSIM on (image, channel) planes: the evaluation metric of the reference (skimage structural_similarity, src/evaluation/metrics.py:46-62)
// and its differentiable SSIM loss (src/loss/loss_ssim.py:129-190), forward and backward.
//
// Both are one map on the VALID window positions: map pixel q (0 <= q < H - ws + 1 per axis) reads input q .. q + ws - 1.  The loss
// convolves without padding, so that is its definition.  The metric filters with reflect padding and then crops (ws - 1) / 2 pixels from
// every edge; the map pixels that survive the crop read no reflected sample, so it is the same valid map (with cov_norm and its own C1/C2).
//
// Taps: the caller's ws taps, zero-padded to 11 and centred (tap j of the padded window reads input q + j + off, off = (ws - 1) / 2 - 5 <= 0):
// every loop below runs 11 taps; the padded taps read a clamped, finite sample and multiply it by zero.
//
// Precision: every workgroup subtracts one sample of its tile (cx, cy) from X and Y before it forms the products, so E[x^2] - mu^2 cancels
// on the tile's local variation rather than on the full intensity (a flat bright plane has zero variance exactly).  The shift is undone
// exactly for a window of total weight T (wsum): v_x = E'[u^2] - mu'^2 + (1 - T)(2 cx mu' + cx^2 T) with u = x - cx, mu' = F u.  T is 1
// for the metric (skimage's float64 taps sum to 1) and the float64 square of the taps' sum for the loss (its float32 window does not).
//
// Determinism: no atomics.  Every workgroup writes one f32 partial per quantity; ssim_reduce_kernel sums them in a fixed order in f64.
#include "common.h"

namespace {

constexpr int kTaps = 11;
constexpr int kThreads = 256;
constexpr float kEps2 = 1.1920928955078125e-07f * 1.1920928955078125e-07f;     // torch.finfo(float32).eps ** 2 (loss_ssim.py:107)

struct SsimTaps {
    float w[kTaps];
};

struct SsimParams {
    int H, W, Mh, Mw, off, P;
    float cov_norm, c1, c2, inv_count, wsum, defect;     // defect = 1 - wsum, formed in double
};

__device__ __forceinline__ int clampi(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// The means and (co)variances of one map pixel from the five moments of the shifted samples u = x - cx, v = y - cy.
struct Moments {
    float m1, m2, v1, v2, v12;
};

__device__ __forceinline__ Moments moments(float mu, float mv, float euu, float evv, float euv, float cx, float cy, const SsimParams &p) {
    const float T = p.wsum, d = p.defect;
    return Moments{mu + cx * T, mv + cy * T, p.cov_norm * ((euu - mu * mu) + d * (2.f * cx * mu + cx * cx * T)),
                   p.cov_norm * ((evv - mv * mv) + d * (2.f * cy * mv + cy * cy * T)),
                   p.cov_norm * ((euv - mu * mv) + d * (cy * mu + cx * mv + cx * cy * T))};
}

// Forward: tile of kFH x kFW map pixels, 256 threads; X and Y tiles with their 10-sample halo in LDS, horizontal pass of the five
// products into LDS, vertical pass in registers.
constexpr int kFW = 32, kFH = 32;
constexpr int kFIW = kFW + kTaps - 1, kFIH = kFH + kTaps - 1;

__global__ void __launch_bounds__(kThreads) ssim_forward_kernel(const float *__restrict__ x, const float *__restrict__ y, SsimTaps taps,
                                                                SsimParams p, int components, int tiles_x, int ntiles,
                                                                float *__restrict__ partials) {
    __shared__ float sx[kFIH][kFIW], sy[kFIH][kFIW];
    __shared__ float sh[5][kFIH][kFW];
    __shared__ float red[4][kThreads / 64];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x;
    const int ox0 = (tile % tiles_x) * kFW, oy0 = (tile / tiles_x) * kFH;
    for (int plane = blockIdx.y; plane < p.P; plane += gridDim.y) {
        const size_t base = (size_t)plane * p.H * p.W;
        const size_t oc = base + (size_t)clampi(oy0 + p.off + kFIH / 2, p.H) * p.W + clampi(ox0 + p.off + kFIW / 2, p.W);
        const float cx = x[oc], cy = y[oc];
        __syncthreads();
        for (int i = tid; i < kFIH * kFIW; i += kThreads) {
            const int r = i / kFIW, c = i % kFIW;
            const size_t o = base + (size_t)clampi(oy0 + p.off + r, p.H) * p.W + clampi(ox0 + p.off + c, p.W);
            sx[r][c] = x[o] - cx;
            sy[r][c] = y[o] - cy;
        }
        __syncthreads();
        for (int i = tid; i < kFIH * kFW; i += kThreads) {
            const int r = i / kFW, c = i % kFW;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
#pragma unroll
            for (int j = 0; j < kTaps; ++j) {
                const float w = taps.w[j], u = sx[r][c + j], v = sy[r][c + j];
                a0 += w * u;
                a1 += w * v;
                a2 += w * (u * u);
                a3 += w * (v * v);
                a4 += w * (u * v);
            }
            sh[0][r][c] = a0;
            sh[1][r][c] = a1;
            sh[2][r][c] = a2;
            sh[3][r][c] = a3;
            sh[4][r][c] = a4;
        }
        __syncthreads();
        float acc_s = 0.f, acc_b = 0.f, acc_c = 0.f, acc_t = 0.f;
        const int c = tid % kFW;
#pragma unroll
        for (int k = 0; k < kFH / (kThreads / kFW); ++k) {
            const int r = tid / kFW + k * (kThreads / kFW);
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
#pragma unroll
            for (int j = 0; j < kTaps; ++j) {
                const float w = taps.w[j];
                a0 += w * sh[0][r + j][c];
                a1 += w * sh[1][r + j][c];
                a2 += w * sh[2][r + j][c];
                a3 += w * sh[3][r + j][c];
                a4 += w * sh[4][r + j][c];
            }
            if (oy0 + r >= p.Mh || ox0 + c >= p.Mw) continue;
            const Moments m = moments(a0, a1, a2, a3, a4, cx, cy, p);
            const float A1 = 2.f * m.m1 * m.m2 + p.c1, B1 = m.m1 * m.m1 + m.m2 * m.m2 + p.c1;
            const float A2 = 2.f * m.v12 + p.c2, B2 = m.v1 + m.v2 + p.c2;
            const float l = A1 / B1;
            acc_s += l * (A2 / B2);
            if (components) {     // loss_ssim.py:105-124
                const float v1 = fmaxf(m.v1, kEps2), v2 = fmaxf(m.v2, kEps2);
                const float sgn = m.v12 > 0.f ? 1.f : (m.v12 < 0.f ? -1.f : 0.f);
                const float s12 = sgn * fminf(sqrtf(v1 * v2), fabsf(m.v12));
                const float c3 = 0.5f * p.c2;
                const float s1s2 = sqrtf(v1) * sqrtf(v2);
                acc_b += l;
                acc_c += fminf((2.f * s1s2 + p.c2) / (v1 + v2 + p.c2), 0.98f);
                acc_t += fminf((s12 + c3) / (s1s2 + c3), 0.98f);
            }
        }
        // fixed-order reduction: wave butterfly, then the four wave sums in order
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            acc_s += __shfl_xor(acc_s, s);
            acc_b += __shfl_xor(acc_b, s);
            acc_c += __shfl_xor(acc_c, s);
            acc_t += __shfl_xor(acc_t, s);
        }
        if ((tid & 63) == 0) {
            red[0][tid >> 6] = acc_s;
            red[1][tid >> 6] = acc_b;
            red[2][tid >> 6] = acc_c;
            red[3][tid >> 6] = acc_t;
        }
        __syncthreads();
        const int nq = components ? 4 : 1;
        if (tid < nq) {
            const float v = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
            partials[((size_t)tid * p.P + plane) * ntiles + tile] = v;
        }
    }
}

// One workgroup per image: per quantity and channel, the tile partials summed in f64 in a fixed order, divided by the map size (the
// per-plane mean), then averaged over the channels (the per-image mean).
__global__ void __launch_bounds__(kThreads) ssim_reduce_kernel(const float *__restrict__ partials, int N, int C, int ntiles, int nq,
                                                               double inv_count, float *__restrict__ out_plane, float *__restrict__ out_image) {
    __shared__ double red[kThreads];
    const int n = blockIdx.x, tid = threadIdx.x, P = N * C;
    for (int q = 0; q < nq; ++q) {
        double img = 0.0;
        for (int ch = 0; ch < C; ++ch) {
            const int plane = n * C + ch;
            const float *src = partials + ((size_t)q * P + plane) * ntiles;
            double s = 0.0;
            for (int t = tid; t < ntiles; t += kThreads) s += (double)src[t];
            red[tid] = s;
            __syncthreads();
            for (int w = kThreads / 2; w > 0; w >>= 1) {
                if (tid < w) red[tid] += red[tid + w];
                __syncthreads();
            }
            const double v = red[0] * inv_count;
            __syncthreads();
            if (tid == 0 && out_plane) out_plane[(size_t)q * P + plane] = (float)v;
            img += v;
        }
        if (tid == 0 && out_image) out_image[(size_t)q * N + n] = (float)(img / C);
    }
}

// Backward: tile of kBH x kBW INPUT pixels.  The map pixels whose window covers the tile are the tile grown by 10 on the low side of each
// axis; their moments need the input grown by 10 more (a 10-pixel halo on both sides).  Per map pixel the partials of
// g_ssim * S + g_struct * structure with respect to (mu_x, mu_y, E[x^2], E[y^2], E[xy]) go to LDS; the transposed window (flipped index)
// brings them back to the input pixels: dX = F^T a_mx + 2 X F^T a_xx + Y F^T a_xy, dY = F^T a_my + 2 Y F^T a_yy + X F^T a_xy.
constexpr int kBW = 32, kBH = 16;
constexpr int kBMW = kBW + kTaps - 1, kBMH = kBH + kTaps - 1;       // map pixels
constexpr int kBIW = kBMW + kTaps - 1, kBIH = kBMH + kTaps - 1;     // input pixels
constexpr int kBPix = (kBMW * kBMH + kThreads - 1) / kThreads;      // map pixels per thread

// a[0], a[1] are the partials for the means of the SHIFTED samples (what the tile's transposed pass multiplies by u and v): with X = u + cx,
// F^T a_mx + 2 X F^T a_xx + Y F^T a_xy = F^T (a_mx + 2 cx a_xx + cy a_xy) + 2 u F^T a_xx + v F^T a_xy.
__device__ __forceinline__ void ssim_partials(const Moments &m, float su, float sv, const SsimParams &p, float gs, float gt, float *a) {
    const float A1 = 2.f * m.m1 * m.m2 + p.c1, B1 = m.m1 * m.m1 + m.m2 * m.m2 + p.c1;
    const float A2 = 2.f * m.v12 + p.c2, B2 = m.v1 + m.v2 + p.c2;
    const float l = A1 / B1, cs = A2 / B2;
    // gradient with respect to (mu_x, mu_y) held fixed in v, then (v1, v2, v12)
    float g1 = gs * 2.f * cs * (m.m2 - l * m.m1) / B1;
    float g2 = gs * 2.f * cs * (m.m1 - l * m.m2) / B1;
    float gv1 = -gs * l * cs / B2, gv2 = gv1, gv12 = gs * 2.f * l / B2;
    if (gt != 0.f) {      // structure map of loss_ssim.py:107-120 under torch autograd's conventions
        const float v1 = fmaxf(m.v1, kEps2), v2 = fmaxf(m.v2, kEps2);
        const float sgn = m.v12 > 0.f ? 1.f : (m.v12 < 0.f ? -1.f : 0.f);
        const float P = sqrtf(v1 * v2), Q = fabsf(m.v12);
        const float s12 = sgn * fminf(P, Q);
        const float c3 = 0.5f * p.c2;
        const float r1 = sqrtf(v1), r2 = sqrtf(v2);
        const float D = r1 * r2 + c3;
        const float st = (s12 + c3) / D;
        if (st <= 0.98f) {                                   // clamp(max=0.98) passes the gradient up to the bound
            const float dM = gt * sgn / D;                   // sign() contributes nothing
            const float wP = P < Q ? 1.f : (P == Q ? 0.5f : 0.f);
            const float dP = dM * wP, dQ = dM * (1.f - wP);
            const float dS1S2 = -gt * st / D;
            gv12 += dQ * sgn;
            const float dprod = dP / (2.f * P);
            const float dv1 = dprod * v2 + dS1S2 * r2 / (2.f * r1);
            const float dv2 = dprod * v1 + dS1S2 * r1 / (2.f * r2);
            if (m.v1 >= kEps2) gv1 += dv1;                  // clamp(min=eps) passes the gradient from the bound up
            if (m.v2 >= kEps2) gv2 += dv2;
        }
    }
    gv1 *= p.cov_norm;
    gv2 *= p.cov_norm;
    gv12 *= p.cov_norm;
    a[0] = g1 - 2.f * su * gv1 - sv * gv12;
    a[1] = g2 - 2.f * sv * gv2 - su * gv12;
    a[2] = gv1;
    a[3] = gv2;
    a[4] = gv12;
}

__global__ void __launch_bounds__(kThreads) ssim_backward_kernel(const float *__restrict__ x, const float *__restrict__ y, SsimTaps taps,
                                                                 SsimParams p, int tiles_x, const float *__restrict__ g_ssim,
                                                                 const float *__restrict__ g_struct, float *__restrict__ dx,
                                                                 float *__restrict__ dy) {
    __shared__ float sx[kBIH][kBIW], sy[kBIH][kBIW];
    __shared__ float sh[5 * kBIH * kBMW];          // horizontal products [5][kBIH][kBMW]; then the partials a [5][kBMH][kBMW]
    __shared__ float st[5][kBMH][kBW];             // transposed horizontal pass of a
    const int tid = threadIdx.x;
    const int tile = blockIdx.x;
    const int rx0 = (tile % tiles_x) * kBW, ry0 = (tile / tiles_x) * kBH;
    const int qx0 = rx0 - (kTaps - 1) - p.off, qy0 = ry0 - (kTaps - 1) - p.off;     // first map pixel of the tile
    for (int plane = blockIdx.y; plane < p.P; plane += gridDim.y) {
        const size_t base = (size_t)plane * p.H * p.W;
        const float gs = (g_ssim ? g_ssim[plane] : 0.f) * p.inv_count;
        const float gt = (g_struct ? g_struct[plane] : 0.f) * p.inv_count;
        const size_t oc = base + (size_t)clampi(ry0 + kBH / 2, p.H) * p.W + clampi(rx0 + kBW / 2, p.W);
        const float cx = x[oc], cy = y[oc];
        __syncthreads();
        for (int i = tid; i < kBIH * kBIW; i += kThreads) {
            const int r = i / kBIW, c = i % kBIW;
            const size_t o = base + (size_t)clampi(ry0 - (kTaps - 1) + r, p.H) * p.W + clampi(rx0 - (kTaps - 1) + c, p.W);
            sx[r][c] = x[o] - cx;
            sy[r][c] = y[o] - cy;
        }
        __syncthreads();
        for (int i = tid; i < kBIH * kBMW; i += kThreads) {
            const int r = i / kBMW, c = i % kBMW;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
#pragma unroll
            for (int j = 0; j < kTaps; ++j) {
                const float w = taps.w[j], u = sx[r][c + j], v = sy[r][c + j];
                a0 += w * u;
                a1 += w * v;
                a2 += w * (u * u);
                a3 += w * (v * v);
                a4 += w * (u * v);
            }
            const int o = r * kBMW + c;
            sh[0 * kBIH * kBMW + o] = a0;
            sh[1 * kBIH * kBMW + o] = a1;
            sh[2 * kBIH * kBMW + o] = a2;
            sh[3 * kBIH * kBMW + o] = a3;
            sh[4 * kBIH * kBMW + o] = a4;
        }
        __syncthreads();
        float a[kBPix][5];
#pragma unroll
        for (int k = 0; k < kBPix; ++k) {
            const int i = tid + k * kThreads;
#pragma unroll
            for (int e = 0; e < 5; ++e) a[k][e] = 0.f;
            if (i >= kBMH * kBMW) continue;
            const int r = i / kBMW, c = i % kBMW;
            if (qy0 + r < 0 || qy0 + r >= p.Mh || qx0 + c < 0 || qx0 + c >= p.Mw) continue;
            float mo[5];
#pragma unroll
            for (int e = 0; e < 5; ++e) {
                float s = 0.f;
#pragma unroll
                for (int j = 0; j < kTaps; ++j) s += taps.w[j] * sh[e * kBIH * kBMW + (r + j) * kBMW + c];
                mo[e] = s;
            }
            ssim_partials(moments(mo[0], mo[1], mo[2], mo[3], mo[4], cx, cy, p), mo[0] - cx * p.defect, mo[1] - cy * p.defect, p, gs, gt,
                          a[k]);     // (m1 - cx, m2 - cy)
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kBPix; ++k) {
            const int i = tid + k * kThreads;
            if (i < kBMH * kBMW)
#pragma unroll
                for (int e = 0; e < 5; ++e) sh[e * kBMH * kBMW + i] = a[k][e];
        }
        __syncthreads();
        // transposed window: input column cx collects map columns cx + 10 - j
        for (int i = tid; i < kBMH * kBW; i += kThreads) {
            const int r = i / kBW, c = i % kBW;
#pragma unroll
            for (int e = 0; e < 5; ++e) {
                float s = 0.f;
#pragma unroll
                for (int j = 0; j < kTaps; ++j) s += taps.w[j] * sh[e * kBMH * kBMW + r * kBMW + c + (kTaps - 1) - j];
                st[e][r][c] = s;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kBH * kBW / kThreads; ++k) {
            const int i = tid + k * kThreads;
            const int r = i / kBW, c = i % kBW;
            if (ry0 + r >= p.H || rx0 + c >= p.W) continue;
            float t[5];
#pragma unroll
            for (int e = 0; e < 5; ++e) {
                float s = 0.f;
#pragma unroll
                for (int j = 0; j < kTaps; ++j) s += taps.w[j] * st[e][r + (kTaps - 1) - j][c];
                t[e] = s;
            }
            const float u = sx[r + kTaps - 1][c + kTaps - 1], v = sy[r + kTaps - 1][c + kTaps - 1];
            const size_t o = base + (size_t)(ry0 + r) * p.W + (rx0 + c);
            if (dx) dx[o] = t[0] + 2.f * u * t[2] + v * t[4];
            if (dy) dy[o] = t[1] + 2.f * v * t[3] + u * t[4];
        }
    }
}

int check_args(const float *x, const float *y, int32_t N, int32_t C, int32_t H, int32_t W, const float *taps, int32_t ws, const char *who) {
    VS_CHECK(x && y && taps, "%s: null pointer (x, y and taps are required)", who);
    VS_CHECK(N > 0 && C > 0, "%s: N = %d, C = %d must be positive", who, N, C);
    VS_CHECK(ws >= 1 && ws <= kTaps && (ws & 1), "%s: win_size = %d must be odd and at most %d", who, ws, kTaps);
    VS_CHECK(H >= ws && W >= ws, "%s: a %d x %d plane is smaller than the %d-tap window", who, H, W, ws);
    VS_CHECK((int64_t)N * C <= INT32_MAX && (int64_t)H * W <= INT32_MAX, "%s: too many planes or pixels", who);
    return 0;
}

void make_params(int32_t N, int32_t C, int32_t H, int32_t W, const float *taps, int32_t ws, float cov_norm, float c1, float c2,
                 int32_t flags, SsimTaps *t, SsimParams *p) {
    const int pad = (kTaps - ws) / 2;
    double sum = 0.0;
    for (int j = 0; j < kTaps; ++j) {
        t->w[j] = (j >= pad && j < pad + ws) ? taps[j - pad] : 0.f;
        sum += t->w[j];
    }
    const double T = (flags & VS_SSIM_UNIT_WINDOW) ? 1.0 : sum * sum;     // the separable window's total weight
    p->wsum = (float)T;
    p->defect = (float)(1.0 - T);
    p->H = H;
    p->W = W;
    p->Mh = H - ws + 1;
    p->Mw = W - ws + 1;
    p->off = -pad;
    p->P = N * C;
    p->cov_norm = cov_norm;
    p->c1 = c1;
    p->c2 = c2;
    p->inv_count = (float)(1.0 / ((double)p->Mh * p->Mw));
}

int forward_tiles(int32_t H, int32_t W, int32_t ws, int *tiles_x) {
    *tiles_x = vs::cdiv(W - ws + 1, kFW);
    return *tiles_x * vs::cdiv(H - ws + 1, kFH);
}

}  // namespace

extern "C" int64_t vs_ssim_workspace_bytes(int32_t N, int32_t C, int32_t H, int32_t W, int32_t win_size, int32_t flags) {
    if (N <= 0 || C <= 0 || win_size < 1 || win_size > kTaps || !(win_size & 1) || H < win_size || W < win_size) {
        vs::set_error("vs_ssim_workspace_bytes: bad shape N=%d C=%d H=%d W=%d win_size=%d", N, C, H, W, win_size);
        return -1;
    }
    int tx;
    return (int64_t)((flags & VS_SSIM_COMPONENTS) ? 4 : 1) * N * C * forward_tiles(H, W, win_size, &tx) * (int64_t)sizeof(float);
}

extern "C" int vs_ssim_forward(const float *x, const float *y, int32_t N, int32_t C, int32_t H, int32_t W, const float *taps, int32_t win_size,
                               float cov_norm, float c1, float c2, int32_t flags, float *workspace, float *out_plane, float *out_image,
                               vs_stream_t stream_) {
    if (check_args(x, y, N, C, H, W, taps, win_size, "vs_ssim_forward")) return -1;
    VS_CHECK(workspace, "vs_ssim_forward: null workspace (size: vs_ssim_workspace_bytes)");
    VS_CHECK(out_plane || out_image, "vs_ssim_forward: null out_plane and out_image");
    SsimTaps t;
    SsimParams p;
    make_params(N, C, H, W, taps, win_size, cov_norm, c1, c2, flags, &t, &p);
    const int components = (flags & VS_SSIM_COMPONENTS) ? 1 : 0;
    int tiles_x;
    const int ntiles = forward_tiles(H, W, win_size, &tiles_x);
    const hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(ssim_forward_kernel, dim3(ntiles, p.P < 65535 ? p.P : 65535), dim3(kThreads), 0, stream, x, y, t, p,
                       components, tiles_x, ntiles, workspace);
    VS_HIP(hipGetLastError());
    hipLaunchKernelGGL(ssim_reduce_kernel, dim3(N), dim3(kThreads), 0, stream, (const float *)workspace, N, C, ntiles, components ? 4 : 1,
                       1.0 / ((double)p.Mh * p.Mw), out_plane, out_image);
    VS_HIP(hipGetLastError());
    return 0;
}

extern "C" int vs_ssim_backward(const float *x, const float *y, int32_t N, int32_t C, int32_t H, int32_t W, const float *taps, int32_t win_size,
                                float cov_norm, float c1, float c2, int32_t flags, const float *g_ssim, const float *g_structure,
                                float *dx, float *dy,
                                vs_stream_t stream_) {
    if (check_args(x, y, N, C, H, W, taps, win_size, "vs_ssim_backward")) return -1;
    VS_CHECK(dx || dy, "vs_ssim_backward: null dx and dy");
    SsimTaps t;
    SsimParams p;
    make_params(N, C, H, W, taps, win_size, cov_norm, c1, c2, flags, &t, &p);
    const int tiles_x = vs::cdiv(W, kBW), ntiles = tiles_x * vs::cdiv(H, kBH);
    hipLaunchKernelGGL(ssim_backward_kernel, dim3(ntiles, p.P < 65535 ? p.P : 65535), dim3(kThreads), 0, (hipStream_t)stream_, x, y, t, p,
                       tiles_x, g_ssim, g_structure, dx, dy);
    VS_HIP(hipGetLastError());
    return 0;
}
