// Visualisation of the validation step: the depth range of vis_depth_map (src/misc/utils.py:13-22), the colour-map lookup of
// apply_color_map_to_image (src/visualization/color_map.py) and the uint8 frames of render_video_generic
// (src/model/model_wrapper.py:805-813).  Declared in include/vicasplat_viz.h (prefix vsv_), which states the arithmetic.
//
//   range    init -> (pass, narrow) x 4.  A pass streams the values once (16 bytes per lane) and counts the 8-bit digit at `shift` of every
//            key whose higher digits equal a statistic's prefix: LDS histograms with integer atomics (a thread merges runs of equal digits
//            first, so a constant map does not serialise on one LDS word), then one integer atomic add per non-empty bin and workgroup into
//            the workspace's histograms.  Statistics that share a prefix share a histogram.  narrow (one workgroup, a wave per statistic)
//            finds the bin in which the running count passes the rank, extends the prefix, clears the histograms, and after the last pass
//            writes (near, far).  The first pass also counts positives and NaNs; narrow places the ranks of near with them.
//   max      the maximum of confidence_map as an integer atomic max on the same order-preserving keys (a NaN's key is the largest).
//   colour   one lane per 4 values (or per value): index, table lookup from LDS, three planes out.
//   frames   one lane per 4 output bytes (or per byte) of an rgb or gap row, or per 4 depth values, which write all three planes.
// Integer sums and maxima do not depend on the arrival order: the same inputs give the same bits.
#include "common.h"

#include "../../include/vicasplat_viz.h"

namespace {

constexpr int kThreads = VSV_THREADS;
constexpr int kVec = VSV_VEC;
constexpr int kMaxItems = INT32_MAX - kThreads;     // a grid's last workgroup may index past the items, never past 2^31 - 1
static_assert(kVec == 4, "a lane reads one float4");
// workspace words of vsv_depth_range
enum { W_HIST = 0, W_NPOS = 1024, W_NNAN = 1025, W_PREFIX = 1028, W_REM = 1032, W_WORDS = 1040 };

// Order-preserving key: IEEE order of the non-NaN values (-0 below +0) as unsigned order; every NaN is the largest key.
__device__ __forceinline__ unsigned key_of(float v) {
    const unsigned u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float value_of(unsigned key) {      // 0xffffffff comes back as a NaN
    return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

constexpr unsigned kKeyZero = 0x80000000u, kKeyInf = 0xff800000u;     // v > 0  <=>  kKeyZero < key <= kKeyInf

// torch.lerp for f32 (ATen: the form that is exact at both ends), every operation rounded on its own
__device__ __forceinline__ float lerp_torch(float a, float b, float w) {
    const float d = __fsub_rn(b, a);
    return w < 0.5f ? __fadd_rn(a, __fmul_rn(w, d)) : __fsub_rn(b, __fmul_rn(d, __fsub_rn(1.f, w)));
}

// The split of n values at a 4-byte aligned base: `head` single values up to the first 16-byte boundary, nvec float4, then a tail (< 4).
struct Span {
    int n, head, nvec;
};

Span span_of(const float *p, int64_t n) {
    Span s;
    s.n = (int)n;
    const int to_boundary = (int)(((16 - ((uintptr_t)p & 15)) & 15) / 4);
    s.head = to_boundary < s.n ? to_boundary : s.n;
    s.nvec = (s.n - s.head) / kVec;
    return s;
}

int blocks_of(const Span &s) {
    const int b = vs::cdiv(s.nvec, kThreads);
    return b < 1 ? 1 : b > VSV_MAX_BLOCKS ? VSV_MAX_BLOCKS : b;
}

// f(v) for every one of the span's values, each exactly once over the grid
template <class F>
__device__ __forceinline__ void for_each_value(const float *__restrict__ value, const Span s, F &&f) {
    const float4 *body = reinterpret_cast<const float4 *>(value + s.head);
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < s.nvec; i += gridDim.x * kThreads) {
        const float4 q = body[i];
        f(q.x);
        f(q.y);
        f(q.z);
        f(q.w);
    }
    if (blockIdx.x == 0) {
        const int tail0 = s.head + kVec * s.nvec, t = (int)threadIdx.x;
        if (t < s.head) f(value[t]);
        else if (t - s.head < s.n - tail0) f(value[tail0 + t - s.head]);
    }
}

__global__ void __launch_bounds__(kThreads) clear_kernel(uint4 *__restrict__ ws, int quads) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < quads) ws[i] = make_uint4(0u, 0u, 0u, 0u);
}

template <bool FIRST>
__global__ void __launch_bounds__(kThreads) range_pass_kernel(const float *__restrict__ value, Span s, unsigned *__restrict__ ws, int shift) {
    __shared__ unsigned hist[4][256];
    __shared__ unsigned counts[2];
    const int tid = threadIdx.x;
    for (int i = tid; i < 4 * 256; i += kThreads) (&hist[0][0])[i] = 0;
    if (tid < 2) counts[tid] = 0;
    unsigned pre[4];
    bool own[4];     // the first of the statistics that share a prefix counts for all of them
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        pre[t] = FIRST ? 0u : ws[W_PREFIX + t];
        own[t] = true;
#pragma unroll
        for (int u = 0; u < t; ++u) own[t] = own[t] && pre[u] != pre[t];
    }
    __syncthreads();
    int cb[4] = {-1, -1, -1, -1};
    unsigned cc[4] = {0, 0, 0, 0};
    unsigned npos = 0, nnan = 0;
    for_each_value(value, s, [&](float v) {
        const unsigned key = key_of(v);
        if (FIRST) {
            npos += key > kKeyZero && key <= kKeyInf;
            nnan += key == 0xffffffffu;
        }
        const unsigned high = FIRST ? 0u : key >> (shift + 8);
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
    });
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (cc[t]) atomicAdd(&hist[t][cb[t]], cc[t]);
    if (FIRST) {
        if (npos) atomicAdd(&counts[0], npos);
        if (nnan) atomicAdd(&counts[1], nnan);
    }
    __syncthreads();
    for (int i = tid; i < 4 * 256; i += kThreads) {
        const unsigned h = (&hist[0][0])[i];
        if (h) atomicAdd(&ws[W_HIST + i], h);
    }
    if (FIRST && tid < 2 && counts[tid]) atomicAdd(&ws[W_NPOS + tid], counts[tid]);
}

__global__ void __launch_bounds__(kThreads) range_narrow_kernel(unsigned *__restrict__ ws, int n, int shift, float *__restrict__ range,
                                                                float *__restrict__ order_stats) {
    __shared__ unsigned keys[4];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const unsigned m = ws[W_NPOS], nnan = ws[W_NNAN];
    // ranks as torch.quantile forms them for an f32 input: q (count - 1) in f32
    const float r_near = m ? __fmul_rn(0.01f, (float)(m - 1)) : 0.f, r_far = __fmul_rn(0.99f, (float)(n - 1));
    unsigned pre[4], rem;
    if (shift == 24) {
#pragma unroll
        for (int t = 0; t < 4; ++t) pre[t] = 0;
        if (w < 2) {      // the positives are the m keys above +0's and below the NaNs'; with none the rank 0 stands in and is not used
            const unsigned below = (unsigned)n - nnan - m, k = (unsigned)(w == 0 ? floorf(r_near) : ceilf(r_near));
            rem = m ? below + (k < m ? k : m - 1) : 0u;
        } else {
            const unsigned k = (unsigned)(w == 2 ? floorf(r_far) : ceilf(r_far));
            rem = k < (unsigned)n ? k : (unsigned)n - 1;
        }
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) pre[t] = ws[W_PREFIX + t];
        rem = ws[W_REM + w];
    }
    const unsigned mine = w == 0 ? pre[0] : w == 1 ? pre[1] : w == 2 ? pre[2] : pre[3];
    int o = w;
#pragma unroll
    for (int u = 3; u >= 0; --u)
        if (u < w && pre[u] == mine) o = u;
    // wave w finds the digit of statistic w: the bin in which the running count passes its rank
    const uint4 h = reinterpret_cast<const uint4 *>(ws + W_HIST + 256 * o)[lane];
    const unsigned sum = h.x + h.y + h.z + h.w;
    unsigned incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    const unsigned long long over = __ballot(incl > rem);
    const int first = over ? __ffsll((long long)over) - 1 : 63;
    unsigned new_pre = 0, new_rem = 0;
    if (lane == first) {
        unsigned below = incl - sum;
        int bin = 4 * lane;
        if (below + h.x <= rem) { below += h.x; ++bin;
            if (below + h.y <= rem) { below += h.y; ++bin;
                if (below + h.z <= rem) { below += h.z; ++bin; } } }
        new_pre = (mine << 8) | (unsigned)bin;
        new_rem = rem - below;
        keys[w] = new_pre;
    }
    __syncthreads();      // every wave has read the histograms and the old prefixes
    if (lane == first) {
        ws[W_PREFIX + w] = new_pre;
        ws[W_REM + w] = new_rem;
    }
    reinterpret_cast<uint4 *>(ws + W_HIST)[tid] = make_uint4(0u, 0u, 0u, 0u);
    if (shift == 0 && tid == 0) {
        const float a0 = m ? value_of(keys[0]) : 0.f, b0 = m ? value_of(keys[1]) : 0.f, a1 = value_of(keys[2]), b1 = value_of(keys[3]);
        range[0] = m ? logf(lerp_torch(a0, b0, __fsub_rn(r_near, floorf(r_near)))) : 0.f;
        range[1] = nnan ? __uint_as_float(0x7fc00000u) : logf(lerp_torch(a1, b1, __fsub_rn(r_far, floorf(r_far))));
        if (order_stats) {
            order_stats[0] = a0;
            order_stats[1] = b0;
            order_stats[2] = a1;
            order_stats[3] = b1;
        }
    }
}

__global__ void __launch_bounds__(kThreads) max_key_kernel(const float *__restrict__ value, Span s, unsigned *__restrict__ ws) {
    __shared__ unsigned best;
    if (threadIdx.x == 0) best = 0;
    __syncthreads();
    unsigned k = 0;
    for_each_value(value, s, [&](float v) {
        const unsigned key = key_of(v);
        k = key > k ? key : k;
    });
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned other = __shfl_xor(k, d, 64);
        k = other > k ? other : k;
    }
    if ((threadIdx.x & 63) == 0) atomicMax(&best, k);
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(ws, best);
}

// idx = min(trunc(clip(x, 0, 1) * 256), 255), or -1 for a NaN
__device__ __forceinline__ int index_of(float x) {
    if (x != x) return -1;
    const float c = x < 0.f ? 0.f : x > 1.f ? 1.f : x;
    const int i = (int)__fmul_rn(c, 256.f);
    return i > 255 ? 255 : i;
}

__device__ __forceinline__ float x_depth(float v, float near, float far_minus_near) {
    return __fsub_rn(1.f, __fdiv_rn(__fsub_rn(logf(v), near), far_minus_near));
}

// trunc(clip(c, 0, 1) * 255), 0 for a NaN
__device__ __forceinline__ unsigned byte_of(float c) {
    if (c != c) return 0u;
    const float k = c < 0.f ? 0.f : c > 1.f ? 1.f : c;
    return (unsigned)__fmul_rn(k, 255.f);
}

// the table as one word per entry: r | g << 8 | b << 16 of byte_of
__device__ __forceinline__ void stage_lut_bytes(const float *__restrict__ lut, unsigned *packed) {
    for (int i = threadIdx.x; i < 256; i += kThreads)
        packed[i] = byte_of(lut[3 * i]) | byte_of(lut[3 * i + 1]) << 8 | byte_of(lut[3 * i + 2]) << 16;
}

template <int PX>
struct Px;
template <>
struct Px<4> {
    using F = float4;
    using B = unsigned;       // four bytes
};
template <>
struct Px<1> {
    using F = float;
    using B = unsigned char;
};

__device__ __forceinline__ float lane_of(const float4 &q, int j) { return j == 0 ? q.x : j == 1 ? q.y : j == 2 ? q.z : q.w; }
__device__ __forceinline__ float lane_of(const float &q, int) { return q; }

// MODE: VSV_MODE_DEPTH reads (near, far) at `scale`, VSV_MODE_MAX the key of the maximum, VSV_MODE_UNIT nothing.  item = PX consecutive values of one image.
template <int PX, bool U8, int MODE>
__global__ void __launch_bounds__(kThreads) color_map_kernel(const float *__restrict__ value, int items, int hw, const void *__restrict__ scale,
                                                             const float *__restrict__ lut, void *__restrict__ out) {
    __shared__ float table[U8 ? 1 : 768];
    __shared__ unsigned packed[U8 ? 256 : 1];
    if (U8) stage_lut_bytes(lut, packed);
    else
        for (int i = threadIdx.x; i < 768; i += kThreads) table[i] = lut[i];
    __syncthreads();
    const int item = blockIdx.x * kThreads + threadIdx.x;
    if (item >= items) return;
    float near = 0.f, den;
    if (MODE == VSV_MODE_DEPTH) {
        near = static_cast<const float *>(scale)[0];
        den = __fsub_rn(static_cast<const float *>(scale)[1], near);
    } else {
        den = MODE == VSV_MODE_MAX ? value_of(*static_cast<const unsigned *>(scale)) : 1.f;
    }
    const int64_t p = (int64_t)item * PX;
    const int64_t img = p / hw, e = p - img * hw;
    const typename Px<PX>::F q = reinterpret_cast<const typename Px<PX>::F *>(value)[item];
    int idx[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        const float v = lane_of(q, j);
        idx[j] = index_of(MODE == VSV_MODE_DEPTH ? x_depth(v, near, den) : MODE == VSV_MODE_MAX ? __fdiv_rn(v, den) : v);
    }
    const int64_t base = img * 3 * hw + e;
    if (U8) {
        unsigned word[3] = {0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            const unsigned rgb = idx[j] < 0 ? 0u : packed[idx[j]];
#pragma unroll
            for (int c = 0; c < 3; ++c) word[c] |= ((rgb >> (8 * c)) & 255u) << (8 * j);
        }
        unsigned char *o = static_cast<unsigned char *>(out);
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<typename Px<PX>::B *>(o + base + (int64_t)c * hw) = (typename Px<PX>::B)word[c];
    } else {
        float *o = static_cast<float *>(out);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float r[PX];
#pragma unroll
            for (int j = 0; j < PX; ++j) r[j] = idx[j] < 0 ? 0.f : table[3 * idx[j] + c];
            if constexpr (PX == 4) *reinterpret_cast<float4 *>(o + base + (int64_t)c * hw) = make_float4(r[0], r[1], r[2], r[3]);
            else o[base + (int64_t)c * hw] = r[0];
        }
    }
}

// item = PX consecutive bytes of one row of an rgb or gap plane, or PX consecutive depth values (all three planes).  Per image the items
// are (3 H + 3 gap + H) rows of wq = W / PX.
template <int PX>
__global__ void __launch_bounds__(kThreads) frames_kernel(const float *__restrict__ rgb, const float *__restrict__ depth, int items, int H,
                                                          int W, int gap, const float *__restrict__ range, const float *__restrict__ lut,
                                                          unsigned char *__restrict__ frames) {
    __shared__ unsigned packed[256];
    stage_lut_bytes(lut, packed);
    __syncthreads();
    const int item = blockIdx.x * kThreads + threadIdx.x;
    if (item >= items) return;
    using F = typename Px<PX>::F;
    using B = typename Px<PX>::B;
    const int wq = W / PX, rows = 4 * H + 3 * gap, hf = 2 * H + gap;
    const int row_all = item / wq, xq = item - row_all * wq;
    const int img = row_all / rows, row = row_all - img * rows;
    const int64_t plane = (int64_t)hf * W;
    unsigned char *frame = frames + (int64_t)img * 3 * plane + (int64_t)xq * PX;
    if (row < 3 * H) {
        const int c = row / H, y = row - c * H;
        const F q = *reinterpret_cast<const F *>(rgb + (((int64_t)img * 3 + c) * H + y) * W + (int64_t)xq * PX);
        unsigned word = 0;
#pragma unroll
        for (int j = 0; j < PX; ++j) word |= byte_of(lane_of(q, j)) << (8 * j);
        *reinterpret_cast<B *>(frame + c * plane + (int64_t)y * W) = (B)word;
    } else if (row < 3 * H + 3 * gap) {
        const int g = row - 3 * H, c = g / gap, y = H + (g - c * gap);
        *reinterpret_cast<B *>(frame + c * plane + (int64_t)y * W) = (B)0xffffffffu;
    } else {
        const int y = row - 3 * H - 3 * gap;
        const float near = range[0], den = __fsub_rn(range[1], near);
        const F q = *reinterpret_cast<const F *>(depth + ((int64_t)img * H + y) * W + (int64_t)xq * PX);
        unsigned word[3] = {0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            const int idx = index_of(x_depth(lane_of(q, j), near, den));
            const unsigned c3 = idx < 0 ? 0u : packed[idx];
#pragma unroll
            for (int c = 0; c < 3; ++c) word[c] |= ((c3 >> (8 * c)) & 255u) << (8 * j);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<B *>(frame + c * plane + (int64_t)(H + gap + y) * W) = (B)word[c];
    }
}

bool aligned(const void *p, int a) { return ((uintptr_t)p & (uintptr_t)(a - 1)) == 0; }

template <int PX, bool U8>
void launch_color_map(int mode, const float *value, int items, int hw, const float *range, const void *ws, const float *lut, void *out,
                      hipStream_t st) {
    const dim3 grid(vs::cdiv(items, kThreads)), block(kThreads);
    if (mode == VSV_MODE_DEPTH)
        hipLaunchKernelGGL((color_map_kernel<PX, U8, VSV_MODE_DEPTH>), grid, block, 0, st, value, items, hw, (const void *)range, lut, out);
    else if (mode == VSV_MODE_MAX)
        hipLaunchKernelGGL((color_map_kernel<PX, U8, VSV_MODE_MAX>), grid, block, 0, st, value, items, hw, ws, lut, out);
    else
        hipLaunchKernelGGL((color_map_kernel<PX, U8, VSV_MODE_UNIT>), grid, block, 0, st, value, items, hw, ws, lut, out);
}

}  // namespace

extern "C" {

int64_t vsv_depth_range_workspace_bytes(int64_t n) {
    if (n < 0 || n > VSV_MAX_RANGE_N) {
        vs::set_error("vsv_depth_range_workspace_bytes: n = %lld outside [0, %d]", (long long)n, VSV_MAX_RANGE_N);
        return -1;
    }
    return (int64_t)W_WORDS * 4;
}

int vsv_depth_range(const float *value, int64_t n, float *range, float *order_stats, void *workspace, int64_t workspace_bytes,
                    vs_stream_t stream) {
    VS_CHECK(value && range, "vsv_depth_range: null pointer (value and range are required)");
    VS_CHECK(n >= 0, "vsv_depth_range: n = %lld is negative", (long long)n);
    VS_CHECK(n <= VSV_MAX_RANGE_N, "vsv_depth_range: n = %lld exceeds %d (the reference's slice of the positives is not built)", (long long)n,
             VSV_MAX_RANGE_N);
    VS_CHECK(workspace, "vsv_depth_range: null workspace (size: vsv_depth_range_workspace_bytes)");
    VS_CHECK(workspace_bytes >= (int64_t)W_WORDS * 4, "vsv_depth_range: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
             (long long)W_WORDS * 4);
    VS_CHECK(aligned(workspace, 16), "vsv_depth_range: workspace is not 16-byte aligned");
    VS_CHECK(aligned(value, 4) && aligned(range, 4) && aligned(order_stats, 4), "vsv_depth_range: value, range or order_stats is not 4-byte aligned");
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    unsigned *ws = static_cast<unsigned *>(workspace);
    const Span s = span_of(value, n);
    const dim3 grid(blocks_of(s)), block(kThreads);
    hipLaunchKernelGGL(clear_kernel, dim3(vs::cdiv(W_WORDS / 4, kThreads)), block, 0, st, reinterpret_cast<uint4 *>(ws), W_WORDS / 4);
    VS_HIP(hipGetLastError());
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (shift == 24) hipLaunchKernelGGL(range_pass_kernel<true>, grid, block, 0, st, value, s, ws, shift);
        else hipLaunchKernelGGL(range_pass_kernel<false>, grid, block, 0, st, value, s, ws, shift);
        VS_HIP(hipGetLastError());
        hipLaunchKernelGGL(range_narrow_kernel, dim3(1), block, 0, st, ws, s.n, shift, range, order_stats);
        VS_HIP(hipGetLastError());
    }
    return 0;
}

int64_t vsv_color_map_workspace_bytes(int32_t mode) {
    if (mode != VSV_MODE_DEPTH && mode != VSV_MODE_MAX && mode != VSV_MODE_UNIT) {
        vs::set_error("vsv_color_map_workspace_bytes: unknown mode %d", mode);
        return -1;
    }
    return mode == VSV_MODE_MAX ? 16 : 0;
}

int vsv_color_map(const float *value, int32_t M, int32_t H, int32_t W, int32_t mode, const float *range, const float *lut, void *out,
                  int32_t out_dtype, void *workspace, int64_t workspace_bytes, vs_stream_t stream) {
    VS_CHECK(mode == VSV_MODE_DEPTH || mode == VSV_MODE_MAX || mode == VSV_MODE_UNIT, "vsv_color_map: unknown mode %d", mode);
    VS_CHECK(out_dtype == VSV_OUT_F32 || out_dtype == VSV_OUT_U8, "vsv_color_map: unknown out_dtype %d", out_dtype);
    VS_CHECK(value && lut && out, "vsv_color_map: null pointer (value, lut and out are required)");
    VS_CHECK(mode != VSV_MODE_DEPTH || range, "vsv_color_map: null range in the depth mode");
    VS_CHECK(M >= 0 && H >= 0 && W >= 0, "vsv_color_map: M = %d, H = %d, W = %d must not be negative", M, H, W);
    const int64_t hw = (int64_t)H * W, n = hw * M;
    VS_CHECK(hw <= kMaxItems && n <= kMaxItems, "vsv_color_map: %lld values exceed %d", (long long)n, kMaxItems);
    VS_CHECK(aligned(value, 4) && aligned(lut, 4) && aligned(range, 4) && (out_dtype == VSV_OUT_U8 || aligned(out, 4)),
             "vsv_color_map: a pointer is not 4-byte aligned");
    if (mode == VSV_MODE_MAX) {
        VS_CHECK(workspace, "vsv_color_map: null workspace (size: vsv_color_map_workspace_bytes)");
        VS_CHECK(workspace_bytes >= 16, "vsv_color_map: workspace of %lld bytes, 16 needed", (long long)workspace_bytes);
        VS_CHECK(aligned(workspace, 16), "vsv_color_map: workspace is not 16-byte aligned");
    }
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (mode == VSV_MODE_MAX) {
        const Span s = span_of(value, n);
        hipLaunchKernelGGL(clear_kernel, dim3(1), dim3(kThreads), 0, st, static_cast<uint4 *>(workspace), 1);
        VS_HIP(hipGetLastError());
        hipLaunchKernelGGL(max_key_kernel, dim3(blocks_of(s)), dim3(kThreads), 0, st, value, s, static_cast<unsigned *>(workspace));
        VS_HIP(hipGetLastError());
    }
    const bool u8 = out_dtype == VSV_OUT_U8;
    const bool vec = hw % kVec == 0 && aligned(value, 16) && aligned(out, u8 ? 4 : 16);
    const int items = (int)(vec ? n / kVec : n);
    if (vec && u8) launch_color_map<4, true>(mode, value, items, (int)hw, range, workspace, lut, out, st);
    else if (vec) launch_color_map<4, false>(mode, value, items, (int)hw, range, workspace, lut, out, st);
    else if (u8) launch_color_map<1, true>(mode, value, items, (int)hw, range, workspace, lut, out, st);
    else launch_color_map<1, false>(mode, value, items, (int)hw, range, workspace, lut, out, st);
    VS_HIP(hipGetLastError());
    return 0;
}

int vsv_video_frames(const float *rgb, const float *depth, int32_t M, int32_t H, int32_t W, int32_t gap, const float *range,
                     const float *lut, uint8_t *frames, vs_stream_t stream) {
    VS_CHECK(rgb && depth && range && lut && frames, "vsv_video_frames: null pointer (rgb, depth, range, lut and frames are required)");
    VS_CHECK(M >= 0 && H >= 0 && W >= 0 && gap >= 0, "vsv_video_frames: M = %d, H = %d, W = %d, gap = %d must not be negative", M, H, W, gap);
    VS_CHECK(aligned(rgb, 4) && aligned(depth, 4) && aligned(range, 4) && aligned(lut, 4), "vsv_video_frames: a pointer is not 4-byte aligned");
    if (M == 0 || W == 0 || 2 * (int64_t)H + gap == 0) return 0;
    const bool vec = W % kVec == 0 && aligned(rgb, 16) && aligned(depth, 16) && aligned(frames, 4);
    // every factor is below 2^31: each product below fits int64 and is checked before the next is formed
    const int64_t rows = 4 * (int64_t)H + 3 * (int64_t)gap, planes_rows = 3 * (2 * (int64_t)H + gap);
    VS_CHECK(rows <= kMaxItems && (int64_t)M * rows <= kMaxItems && (int64_t)M * planes_rows <= kMaxItems,
             "vsv_video_frames: M = %d frames of %lld rows exceed %d", M, (long long)rows, kMaxItems);
    const int64_t items = (int64_t)M * rows * (vec ? W / kVec : W);
    VS_CHECK(items <= kMaxItems && (int64_t)M * planes_rows * W <= kMaxItems, "vsv_video_frames: %lld work items exceed %d",
             (long long)items, kMaxItems);
    const dim3 grid(vs::cdiv((int)items, kThreads)), block(kThreads);
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(frames_kernel<4>, grid, block, 0, st, rgb, depth, (int)items, H, W, gap, range, lut, frames);
    else hipLaunchKernelGGL(frames_kernel<1>, grid, block, 0, st, rgb, depth, (int)items, H, W, gap, range, lut, frames);
    VS_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
