// Distillation point loss (training stage 1): Regr3D of src/loss/loss_conf_point.py:188-252 with normalize_pointcloud 'avg_dis'
// (src/geometry/ptc_geometry.py:270-328), forward and backward, f32.  Declared in include/vicasplat_distill.h (prefix vsd_).
//
//   select   one workgroup per (view, batch element): the order statistics that bracket the 0.01 and 0.99 quantiles of d = |gt|, by
//            radix selection on the bit pattern of d (non-negative floats order as unsigned integers): four 8-bit passes, all four
//            statistics together, histograms in LDS (integer atomics; a thread merges runs of equal digits first, so a distribution that
//            sits in one or two bins of the leading digit does not serialise on one LDS word).  d is recomputed in every pass (the pair's
//            points stay in L2) by dist3(), the one definition every kernel here uses: the mask of the later passes compares the same bits.
//   stats    streaming pass 1, grid (chunks, B): per-block counts of valid pixels, sums of valid |pr| and |gt|, sums of |pr_conf - gt_conf|.
//   factors  one workgroup: per-element factors, counts over the batch, the confidence term.
//   loss     streaming pass 2: per-block sums of gt_conf |gt / f_gt - pr / f_pr| over valid pixels and of the term the gradient of f_pr needs.
//   finish   one workgroup: the loss, and T_b per batch element.
//   backward one streaming pass over both views.
// Every sum is per-thread strided -> xor-shuffle tree -> LDS over the waves -> fixed-order sum over the chunks: no float atomics, the same
// inputs give the same bits.  Points are read as three dwords per lane (n is arbitrary, so a batch element's base is only 4-byte aligned).
#include "common.h"

#include "../../include/vicasplat_distill.h"

namespace {

constexpr int kSelThreads = 1024;
constexpr int kThreads = 256;
constexpr int kMaxChunks = 64;       // per batch element; one lane of the finishing wave per chunk
constexpr int kChunkPixels = 1024;   // pixels a streaming workgroup aims for
constexpr int kHead = 8;             // workspace words in front of the per-element arrays
constexpr int kP1 = 6, kP2 = 3;      // partial sums per workgroup of the two streaming passes
enum { W_STATUS = 0, W_C1 = 1, W_C2 = 2, W_CONF = 3, W_LOSS = 4 };

// ops.regr3d_workspace_view (vicasplat_amd/ops.py) mirrors kHead, the W_ words and the order thr | fp | fg below: change them together.
struct Layout {
    int64_t thr, fp, fg, gn, tb, p1, p2, words;
};

Layout layout(int B) {
    Layout l;
    l.thr = kHead;                      // [2][B][2]: (q01, q99) of (view, batch element)
    l.fp = l.thr + 4 * (int64_t)B;      // [B] factor of the prediction
    l.fg = l.fp + B;                    // [B] factor of the pseudo-GT
    l.gn = l.fg + B;                    // [B] 1 / (f_pr^2 (nnz + 1e-8)), 0 where the clip at 1e-8 is active
    l.tb = l.gn + B;                    // [B] sum_valid (gt_conf / count_v) e^ . pr
    l.p1 = l.tb + B;                    // [B][kMaxChunks][kP1]
    l.p2 = l.p1 + (int64_t)B * kMaxChunks * kP1;
    l.words = l.p2 + (int64_t)B * kMaxChunks * kP2;
    return l;
}

int chunks_of(int64_t n) {
    const int64_t c = vs::cdiv64(n, kChunkPixels);
    return (int)(c < 1 ? 1 : c > kMaxChunks ? kMaxChunks : c);
}

__device__ __forceinline__ float dist3(float x, float y, float z) {
    return __fsqrt_rn(__fmaf_rn(z, z, __fmaf_rn(y, y, __fmul_rn(x, x))));
}

// torch.lerp for f32 (ATen: the form that is exact at both ends)
__device__ __forceinline__ float lerp_torch(float a, float b, float w) {
    return w < 0.5f ? a + w * (b - a) : b - (b - a) * (1.f - w);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// K sums over a 256-thread workgroup, in a fixed order; thread k < K returns sum k, the other threads garbage.
template <int K>
__device__ __forceinline__ float block_sums(float (&v)[K], float (*sm)[K]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float s = wave_sum(v[k]);
        if (lane == 0) sm[w][k] = s;
    }
    __syncthreads();
    float r = 0.f;
    if (threadIdx.x < K) r = (sm[0][threadIdx.x] + sm[1][threadIdx.x]) + (sm[2][threadIdx.x] + sm[3][threadIdx.x]);
    return r;
}

__global__ void __launch_bounds__(kSelThreads) regr3d_select_kernel(const float *__restrict__ gt1, const float *__restrict__ gt2, int B, int n,
                                                                    float *__restrict__ ws, int64_t thr_off) {
    __shared__ unsigned hist[4][256];
    __shared__ unsigned prefix[4], rem[4];
    const int pair = blockIdx.x, v = pair / B, b = pair % B, tid = threadIdx.x;
    const float *pts = (v ? gt2 : gt1) + (size_t)b * n * 3;
    // ranks as torch.quantile forms them for an f32 input: q (n - 1) in f32
    const float r0 = __fmul_rn(0.01f, (float)(n - 1)), r1 = __fmul_rn(0.99f, (float)(n - 1));
    if (tid == 0) {
        rem[0] = (unsigned)floorf(r0);
        rem[1] = (unsigned)ceilf(r0);
        rem[2] = (unsigned)floorf(r1);
        rem[3] = (unsigned)ceilf(r1);
        for (int t = 0; t < 4; ++t) {
            if (rem[t] > (unsigned)(n - 1)) rem[t] = n - 1;      // cannot happen for q < 1; keeps every rank inside the data
            prefix[t] = 0;
        }
    }
    bool bad = false;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = tid; i < 4 * 256; i += kSelThreads) (&hist[0][0])[i] = 0;
        __syncthreads();
        unsigned pre[4];
        bool own[4];     // the first of the statistics that share a prefix counts for all of them
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            pre[t] = prefix[t];
            own[t] = true;
#pragma unroll
            for (int u = 0; u < t; ++u) own[t] = own[t] && pre[u] != pre[t];
        }
        int cb[4] = {-1, -1, -1, -1};
        unsigned cc[4] = {0, 0, 0, 0};
        for (int i = tid; i < n; i += kSelThreads) {
            const float *p = pts + (size_t)i * 3;
            const unsigned key = __float_as_uint(dist3(p[0], p[1], p[2]));
            bad = bad || key > 0x7f800000u;      // NaN, or a sign bit
            const unsigned high = shift == 24 ? 0u : key >> (shift + 8);
            const int bin = (key >> shift) & 255;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (own[t] && high == pre[t]) {
                    if (bin == cb[t]) {
                        ++cc[t];
                    } else {
                        if (cc[t]) atomicAdd(&hist[t][cb[t]], cc[t]);
                        cb[t] = bin;
                        cc[t] = 1;
                    }
                }
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (cc[t]) atomicAdd(&hist[t][cb[t]], cc[t]);
        __syncthreads();
        const int w = tid >> 6, lane = tid & 63;
        if (w < 4) {     // wave t finds the digit of statistic t: the bin in which the running count passes its rank
            const unsigned mine = w == 0 ? pre[0] : w == 1 ? pre[1] : w == 2 ? pre[2] : pre[3];
            int o = w;
#pragma unroll
            for (int u = 3; u >= 0; --u)
                if (u < w && pre[u] == mine) o = u;
            const unsigned h0 = hist[o][4 * lane], h1 = hist[o][4 * lane + 1], h2 = hist[o][4 * lane + 2], h3 = hist[o][4 * lane + 3];
            const unsigned s = h0 + h1 + h2 + h3;
            unsigned incl = s;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned up = __shfl_up(incl, d, 64);
                if (lane >= d) incl += up;
            }
            const unsigned r = rem[w];
            const unsigned long long over = __ballot(incl > r);
            const int first = over ? __ffsll((long long)over) - 1 : 63;
            if (lane == first) {
                unsigned below = incl - s;
                int bin = 4 * lane;
                if (below + h0 <= r) { below += h0; ++bin;
                    if (below + h1 <= r) { below += h1; ++bin;
                        if (below + h2 <= r) { below += h2; ++bin; } } }
                prefix[w] = (mine << 8) | (unsigned)bin;
                rem[w] = r - below;
            }
        }
        __syncthreads();
    }
    if (bad) ((int *)ws)[W_STATUS] = 1;
    if (tid == 0) {
        float *thr = ws + thr_off + 2 * (size_t)pair;
        thr[0] = lerp_torch(__uint_as_float(prefix[0]), __uint_as_float(prefix[1]), r0 - floorf(r0));
        thr[1] = lerp_torch(__uint_as_float(prefix[2]), __uint_as_float(prefix[3]), r1 - floorf(r1));
    }
}

struct Args {
    const float *gt[2], *pr[2], *cg[2], *pc[2];
    int B, n, chunks, normalize, has_conf;
    Layout l;
};

__device__ __forceinline__ void chunk_range(const Args &a, int &lo, int &hi) {
    const int len = (a.n + a.chunks - 1) / a.chunks;
    lo = blockIdx.x * len < a.n ? blockIdx.x * len : a.n;
    hi = a.n - lo < len ? a.n : lo + len;
}

__global__ void __launch_bounds__(kThreads) regr3d_stats_kernel(Args a, float *__restrict__ ws) {
    __shared__ float sm[4][kP1];
    const int b = blockIdx.y;
    int lo, hi;
    chunk_range(a, lo, hi);
    float acc[kP1] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // count 1, count 2 (exact: a chunk has far fewer than 2^24 pixels), |pr|, |gt|, conf 1, conf 2
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        const float q01 = ws[a.l.thr + 2 * ((size_t)v * a.B + b)], q99 = ws[a.l.thr + 2 * ((size_t)v * a.B + b) + 1];
        const size_t base = (size_t)b * a.n;
        for (int i = lo + threadIdx.x; i < hi; i += kThreads) {
            const float *g = a.gt[v] + (base + i) * 3;
            const float d = dist3(g[0], g[1], g[2]);
            if (d >= q01 && d <= q99) {
                acc[v] += 1.f;
                if (a.normalize) {
                    const float *p = a.pr[v] + (base + i) * 3;
                    acc[2] += dist3(p[0], p[1], p[2]);
                    acc[3] += d;
                }
            }
            if (a.has_conf) acc[4 + v] += fabsf(a.pc[v][base + i] - a.cg[v][base + i]);
        }
    }
    const float r = block_sums<kP1>(acc, sm);
    if (threadIdx.x < kP1) ws[a.l.p1 + ((size_t)b * kMaxChunks + blockIdx.x) * kP1 + threadIdx.x] = r;
}

// one workgroup of 1024: wave w takes the batch elements w, w + 16, ...; lane = chunk
template <int K>
__device__ __forceinline__ void chunk_sums(const float *part, int chunks, int lane, float (&out)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = wave_sum(lane < chunks ? part[(size_t)lane * K + k] : 0.f);
}

__global__ void __launch_bounds__(1024) regr3d_factors_kernel(Args a, float *__restrict__ ws) {
    __shared__ float tot[2][16];     // conf 1, conf 2 per wave
    __shared__ int cnt[2][16];       // count 1, count 2 per wave: integers, so the batch-wide counts are exact up to the 2^29 pixels admitted
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float t[2] = {0.f, 0.f};
    int c[2] = {0, 0};
    for (int b = w; b < a.B; b += 16) {
        float s[kP1];
        chunk_sums<kP1>(ws + a.l.p1 + (size_t)b * kMaxChunks * kP1, a.chunks, lane, s);
        c[0] += (int)s[0]; c[1] += (int)s[1];      // per element and view at most 2^24 pixels: s[0], s[1] are exact
        t[0] += s[4]; t[1] += s[5];
        if (lane == 0) {
            float fp = 1.f, fg = 1.f, gn = 0.f;
            if (a.normalize) {
                const float nnz = (float)((int)s[0] + (int)s[1]) + 1e-8f;
                const float rp = s[2] / nnz, rg = s[3] / nnz;
                fp = fmaxf(rp, 1e-8f);
                fg = fmaxf(rg, 1e-8f);
                gn = rp >= 1e-8f ? 1.f / (fp * fp * nnz) : 0.f;      // clip(min=1e-8) passes the gradient where raw >= min
            }
            ws[a.l.fp + b] = fp;
            ws[a.l.fg + b] = fg;
            ws[a.l.gn + b] = gn;
        }
    }
    if (lane == 0)
        for (int k = 0; k < 2; ++k) { tot[k][w] = t[k]; cnt[k][w] = c[k]; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float s[2] = {0.f, 0.f};
        int n[2] = {0, 0};
        for (int k = 0; k < 2; ++k)
            for (int j = 0; j < 16; ++j) { s[k] += tot[k][j]; n[k] += cnt[k][j]; }
        ws[W_C1] = (float)n[0];      // converted once, as the divisor of torch's mean is
        ws[W_C2] = (float)n[1];
        const float all = (float)a.B * (float)a.n;
        ws[W_CONF] = a.has_conf ? s[0] / all + s[1] / all : 0.f;
    }
}

__global__ void __launch_bounds__(kThreads) regr3d_loss_kernel(Args a, float *__restrict__ ws) {
    __shared__ float sm[4][kP2];
    const int b = blockIdx.y;
    int lo, hi;
    chunk_range(a, lo, hi);
    const float fp = ws[a.l.fp + b], fg = ws[a.l.fg + b];
    float acc[kP2] = {0.f, 0.f, 0.f};      // loss sum of view 1, of view 2, sum_valid (gt_conf / count_v) e^ . pr
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        const float q01 = ws[a.l.thr + 2 * ((size_t)v * a.B + b)], q99 = ws[a.l.thr + 2 * ((size_t)v * a.B + b) + 1];
        const float inv_cnt = 1.f / ws[W_C1 + v];
        const size_t base = (size_t)b * a.n;
        for (int i = lo + threadIdx.x; i < hi; i += kThreads) {
            const float *g = a.gt[v] + (base + i) * 3;
            const float gx = g[0], gy = g[1], gz = g[2];
            const float d = dist3(gx, gy, gz);
            if (d >= q01 && d <= q99) {
                const float *p = a.pr[v] + (base + i) * 3;
                const float px = p[0], py = p[1], pz = p[2], c = a.cg[v][base + i];
                float ex, ey, ez;
                if (a.normalize) { ex = gx / fg - px / fp; ey = gy / fg - py / fp; ez = gz / fg - pz / fp; }
                else { ex = gx - px; ey = gy - py; ez = gz - pz; }
                const float e = dist3(ex, ey, ez);
                acc[v] += c * e;
                if (a.normalize && e > 0.f) acc[2] += (c * inv_cnt) * ((ex * px + ey * py + ez * pz) / e);
            }
        }
    }
    const float r = block_sums<kP2>(acc, sm);
    if (threadIdx.x < kP2) ws[a.l.p2 + ((size_t)b * kMaxChunks + blockIdx.x) * kP2 + threadIdx.x] = r;
}

__global__ void __launch_bounds__(1024) regr3d_finish_kernel(Args a, float *__restrict__ ws, float *__restrict__ loss) {
    __shared__ float tot[2][16];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float t[2] = {0.f, 0.f};
    for (int b = w; b < a.B; b += 16) {
        float s[kP2];
        chunk_sums<kP2>(ws + a.l.p2 + (size_t)b * kMaxChunks * kP2, a.chunks, lane, s);
        t[0] += s[0]; t[1] += s[1];
        if (lane == 0) ws[a.l.tb + b] = s[2];
    }
    if (lane == 0) { tot[0][w] = t[0]; tot[1][w] = t[1]; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float s0 = 0.f, s1 = 0.f;
        for (int j = 0; j < 16; ++j) { s0 += tot[0][j]; s1 += tot[1][j]; }
        const float l = s0 / ws[W_C1] + s1 / ws[W_C2] + ws[W_CONF];
        ws[W_LOSS] = l;
        *loss = l;
    }
}

struct Grads {
    float *dp[2], *dc[2];
};

__global__ void __launch_bounds__(kThreads) regr3d_backward_kernel(Args a, Grads o, const float *__restrict__ ws, const float *__restrict__ grad_loss) {
    const int b = blockIdx.y;
    const float up = grad_loss[0];
    const float fp = ws[a.l.fp + b], fg = ws[a.l.fg + b];
    const float kn = a.normalize ? up * ws[a.l.tb + b] * ws[a.l.gn + b] : 0.f;      // dL/df_pr * df_pr/d|pr_j|, without the direction
    const float kc = up / ((float)a.B * (float)a.n);
    const size_t base = (size_t)b * a.n;
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        const float q01 = ws[a.l.thr + 2 * ((size_t)v * a.B + b)], q99 = ws[a.l.thr + 2 * ((size_t)v * a.B + b) + 1];
        const float kd = up / (ws[W_C1 + v] * fp);
        for (int i = blockIdx.x * kThreads + threadIdx.x; i < a.n; i += gridDim.x * kThreads) {
            const float *g = a.gt[v] + (base + i) * 3;
            const float gx = g[0], gy = g[1], gz = g[2];
            const float d = dist3(gx, gy, gz);
            float dx = 0.f, dy = 0.f, dz = 0.f;
            if (d >= q01 && d <= q99) {
                const float *p = a.pr[v] + (base + i) * 3;
                const float px = p[0], py = p[1], pz = p[2];
                float ex, ey, ez;
                if (a.normalize) { ex = gx / fg - px / fp; ey = gy / fg - py / fp; ez = gz / fg - pz / fp; }
                else { ex = gx - px; ey = gy - py; ez = gz - pz; }
                const float e = dist3(ex, ey, ez);
                if (e > 0.f) {      // |.| at 0: subgradient 0
                    const float s = -(kd * a.cg[v][base + i]) / e;
                    dx = s * ex; dy = s * ey; dz = s * ez;
                }
                if (a.normalize) {
                    const float r = dist3(px, py, pz);
                    if (r > 0.f) {
                        const float s = kn / r;
                        dx += s * px; dy += s * py; dz += s * pz;
                    }
                }
            }
            float *out = o.dp[v] + (base + i) * 3;
            out[0] = dx; out[1] = dy; out[2] = dz;
            if (a.has_conf) {
                const float t = a.pc[v][base + i] - a.cg[v][base + i];
                o.dc[v][base + i] = t > 0.f ? kc : t < 0.f ? -kc : t;      // t == 0: 0; NaN stays NaN
            }
        }
    }
}

int make_args(const char *who, const float *gt1, const float *gt2, const float *pr1, const float *pr2, const float *cg1, const float *cg2,
              const float *pc1, const float *pc2, int32_t B, int32_t H, int32_t W, int32_t normalize, const void *workspace,
              int64_t workspace_bytes, Args *a) {
    VS_CHECK(gt1 && gt2 && pr1 && pr2 && cg1 && cg2, "%s: null pointer (gt_pts, pr_pts and gt_conf of both views are required)", who);
    VS_CHECK(B > 0 && H > 0 && W > 0, "%s: B = %d, H = %d, W = %d must be positive", who, B, H, W);
    VS_CHECK((int64_t)H * W <= (1 << 24) && (int64_t)B * H * W <= INT32_MAX / 4,
             "%s: %d x %d pixels (at most 2^24 per view) in a batch of %d (at most 2^29 pixels in all) is too large", who, H, W, B);
    VS_CHECK(B <= 65535, "%s: B = %d exceeds 65535", who, B);
    VS_CHECK(workspace, "%s: null workspace (size: vsd_regr3d_workspace_bytes)", who);
    a->l = layout(B);
    VS_CHECK(workspace_bytes >= a->l.words * 4, "%s: workspace of %lld bytes, %lld needed", who, (long long)workspace_bytes,
             (long long)a->l.words * 4);
    VS_CHECK(((uintptr_t)workspace & 3) == 0, "%s: workspace is not 4-byte aligned", who);
    a->gt[0] = gt1; a->gt[1] = gt2; a->pr[0] = pr1; a->pr[1] = pr2; a->cg[0] = cg1; a->cg[1] = cg2; a->pc[0] = pc1; a->pc[1] = pc2;
    a->B = B;
    a->n = H * W;
    a->chunks = chunks_of(a->n);
    a->normalize = normalize != 0;
    a->has_conf = pc1 && pc2;      // the reference adds the confidence term only when both are given
    return 0;
}

}  // namespace

extern "C" int64_t vsd_regr3d_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    if (B <= 0 || H <= 0 || W <= 0 || B > 65535) {
        vs::set_error("vsd_regr3d_workspace_bytes: bad shape B=%d H=%d W=%d", B, H, W);
        return -1;
    }
    return layout(B).words * 4;
}

extern "C" int vsd_regr3d_forward(const float *gt_pts1, const float *gt_pts2, const float *pr_pts1, const float *pr_pts2,
                                  const float *gt_conf1, const float *gt_conf2, const float *pr_conf1, const float *pr_conf2, int32_t B,
                                  int32_t H, int32_t W, int32_t normalize_pts, void *workspace, int64_t workspace_bytes, float *loss,
                                  vs_stream_t stream_) {
    Args a;
    if (make_args("vsd_regr3d_forward", gt_pts1, gt_pts2, pr_pts1, pr_pts2, gt_conf1, gt_conf2, pr_conf1, pr_conf2, B, H, W, normalize_pts,
                  workspace, workspace_bytes, &a))
        return -1;
    VS_CHECK(loss, "vsd_regr3d_forward: null loss");
    const hipStream_t stream = (hipStream_t)stream_;
    float *ws = (float *)workspace;
    VS_HIP(hipMemsetAsync(ws, 0, kHead * 4, stream));
    hipLaunchKernelGGL(regr3d_select_kernel, dim3(2 * B), dim3(kSelThreads), 0, stream, gt_pts1, gt_pts2, B, a.n, ws, a.l.thr);
    VS_HIP(hipGetLastError());
    hipLaunchKernelGGL(regr3d_stats_kernel, dim3(a.chunks, B), dim3(kThreads), 0, stream, a, ws);
    VS_HIP(hipGetLastError());
    hipLaunchKernelGGL(regr3d_factors_kernel, dim3(1), dim3(1024), 0, stream, a, ws);
    VS_HIP(hipGetLastError());
    hipLaunchKernelGGL(regr3d_loss_kernel, dim3(a.chunks, B), dim3(kThreads), 0, stream, a, ws);
    VS_HIP(hipGetLastError());
    hipLaunchKernelGGL(regr3d_finish_kernel, dim3(1), dim3(1024), 0, stream, a, ws, loss);
    VS_HIP(hipGetLastError());
    int status = 0;
    VS_HIP(hipMemcpyAsync(&status, ws, sizeof(int), hipMemcpyDeviceToHost, stream));
    VS_HIP(hipStreamSynchronize(stream));
    if (status) {
        vs::set_error("vsd_regr3d_forward: a pseudo-GT point has a NaN (or negative) distance: its quantiles are undefined");
        return -3;
    }
    return 0;
}

extern "C" int vsd_regr3d_backward(const float *gt_pts1, const float *gt_pts2, const float *pr_pts1, const float *pr_pts2,
                                   const float *gt_conf1, const float *gt_conf2, const float *pr_conf1, const float *pr_conf2, int32_t B,
                                   int32_t H, int32_t W, int32_t normalize_pts, const float *grad_loss, const void *workspace,
                                   int64_t workspace_bytes, float *d_pr_pts1, float *d_pr_pts2, float *d_pr_conf1, float *d_pr_conf2,
                                   vs_stream_t stream_) {
    Args a;
    if (make_args("vsd_regr3d_backward", gt_pts1, gt_pts2, pr_pts1, pr_pts2, gt_conf1, gt_conf2, pr_conf1, pr_conf2, B, H, W, normalize_pts,
                  workspace, workspace_bytes, &a))
        return -1;
    VS_CHECK(grad_loss && d_pr_pts1 && d_pr_pts2, "vsd_regr3d_backward: null pointer (grad_loss and d_pr_pts of both views are required)");
    VS_CHECK(!a.has_conf || (d_pr_conf1 && d_pr_conf2), "vsd_regr3d_backward: pr_conf given, d_pr_conf null");
    Grads o;
    o.dp[0] = d_pr_pts1; o.dp[1] = d_pr_pts2; o.dc[0] = d_pr_conf1; o.dc[1] = d_pr_conf2;
    int gx = vs::cdiv(a.n, kThreads);
    const int cap = vs::cdiv(4096, B);      // ~4096 workgroups in all, grid-stride beyond
    if (gx > cap) gx = cap;
    hipLaunchKernelGGL(regr3d_backward_kernel, dim3(gx, B), dim3(kThreads), 0, (hipStream_t)stream_, a, o, (const float *)workspace, grad_loss);
    VS_HIP(hipGetLastError());
    return 0;
}
