// Vector drawing: antialiased lines and points (rings) over a batch of images, one layer per launch -- draw_lines / draw_points of
// src/visualization/drawing/ through render_over_image (rendering.py) with subdivision 8.  Declared in include/vicasplat_draw.h (prefix
// vsg_), where the semantics are written out.
//
//   grid = ceil(W / VSG_TILE_W) x ceil(H / VSG_TILE_H) x B workgroups of VSG_THREADS threads; a workgroup owns one tile and its one-pixel halo.
//   scan      VSG_SCAN_CHUNK records at a time, a thread per record: the thread forms the record's derived geometry (u, |D| + extra, w / 2)
//             once, in the reference's f32, and tests whether the record can reach tile + halo; the survivors are compacted into LDS in index
//             order (ballot + prefix count per wave, the waves' counts through LDS).  A round ends when the next chunk might not fit.
//   pass 0    a thread per sample of tile + halo walks the list from its top and stops at the first record that covers it; over several
//             rounds it keeps the largest index.  The RGBA of the samples goes to LDS.
//   mask      a thread per interior pixel compares its RGBA with its in-image neighbours; an unrefined pixel is blended and written here,
//             the refined ones are compacted into a list.
//   refine    a wave per refined pixel, the lane is the subsample (lane = 8 ky + kx); alpha is a ballot population count, the colour sum a
//             fixed xor butterfly.  With one round the list is still in LDS; with more the records are scanned again and the running top
//             index of every (pixel, subsample) sits in LDS between the rounds.
// No float atomics, no dependence on the batch: the same inputs give the same bits.
#include "common.h"

#include "../../include/vicasplat_draw.h"

#pragma clang fp contract(off)

#ifdef __FAST_MATH__
#error "draw.hip needs correctly rounded f32 division and square root: do not compile it with fast-math"
#endif

namespace {

constexpr int kWave = 64;
constexpr int kThreads = VSG_THREADS;
constexpr int kWaves = kThreads / kWave;
constexpr int kTW = VSG_TILE_W, kTH = VSG_TILE_H;
constexpr int kHW = kTW + 2, kHH = kTH + 2;      // tile + halo
constexpr int kHalo = kHW * kHH;
constexpr int kPix = kTW * kTH;
constexpr int kChunk = VSG_SCAN_CHUNK;
constexpr int kCap = VSG_LIST_CAP;
constexpr int kLines = 0, kPoints = 1;
static_assert(kChunk == kThreads, "a thread per record of a chunk");
static_assert(kHalo <= kThreads && kPix <= kThreads, "a thread per sample of tile + halo");
static_assert(kCap >= kChunk, "a whole chunk must fit into an empty list");
static_assert(kThreads % kWave == 0, "whole waves");

struct Shared {
    float4 ga[kCap];          // line: start x, start y, end x, end y       point: x, y, radius, inner radius
    float4 gb[kCap];          // line: ux, uy, |D| + extra, w / 2           point: unused
    int idx[kCap];            // the record's index within its image
    int rt[kPix][kWave];      // running top index of a refined pixel's subsamples, between rounds
    float c0[kHalo][4];       // pass-0 RGBA of tile + halo
    int masked[kPix];         // the refined pixels (their index in the tile)
    int wave_count[kWaves];
};

__device__ __forceinline__ bool is_nan(float v) { return v != v; }

// does list entry i cover the sample (px, py)?  The reference's f32, one rounding per operation (contraction is off in this file).
template <int KIND, int CAP>
__device__ __forceinline__ bool covers(const Shared &s, int i, float px, float py) {
    const float4 a = s.ga[i];
    if (KIND == kPoints) {
        const float dx = px - a.x, dy = py - a.y;
        const float d = sqrtf(dx * dx + dy * dy);
        return d >= a.w && d <= a.z;
    }
    const float4 b = s.gb[i];
    const float ix = px - a.x, iy = py - a.y;
    const float par = b.x * ix + b.y * iy;
    const float qx = ix - par * b.x, qy = iy - par * b.y;
    const float lo = CAP == VSG_CAP_SQUARE ? -b.w : 0.0f;
    bool in = par <= b.z && par > lo && sqrtf(qx * qx + qy * qy) < b.w;
    if (CAP == VSG_CAP_ROUND) {
        const float jx = px - a.z, jy = py - a.w;
        in = in || sqrtf(ix * ix + iy * iy) < b.w || sqrtf(jx * jx + jy * jy) < b.w;
    }
    return in;
}

// the largest index among the n list entries that cover the sample, or -1; the list is in index order, so the walk starts at its top and
// a lane stops testing at its first hit.  Every lane of the wave calls this (an inactive one tests nothing): the exit is wave-uniform.
template <int KIND, int CAP>
__device__ __forceinline__ int top_in_list(const Shared &s, int n, float px, float py, bool active) {
    int top = -1;
    for (int i = n - 1; i >= 0; --i) {
        const bool need = active && top < 0;
        if (__ballot(need) == 0) break;
        if (need && covers<KIND, CAP>(s, i, px, py)) top = s.idx[i];
    }
    return top;
}

// One round of the scan: records [cursor, end) of the image, a chunk at a time, until the next chunk might not fit; the survivors are
// appended to the list in index order.  Returns the list's length; `cursor` moves to the first record not looked at.  (fx0, fy0) is the
// corner of tile + halo.  All threads of the workgroup call it together.
template <int KIND, int CAP>
__device__ __forceinline__ int scan_round(Shared &s, const float *__restrict__ prims, int begin, int end, int &cursor, float fx0, float fy0) {
    constexpr int F = KIND == kLines ? VSG_LINE_FLOATS : VSG_POINT_FLOATS;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const float fx1 = fx0 + (float)kHW, fy1 = fy0 + (float)kHH;
    int n = 0;
    __syncthreads();      // everybody has finished with the previous round's list
    while (cursor < end && n <= kCap - kChunk) {
        const int i = cursor + tid;
        bool keep = false;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        if (i < end) {
            const float *r = prims + (size_t)i * F;
            if (KIND == kLines) {
                const float sx = r[0], sy = r[1], ex = r[2], ey = r[3], w = r[4];
                const float hw = 0.5f * w, extra = CAP == VSG_CAP_SQUARE ? hw : 0.0f;
                const float dx = ex - sx, dy = ey - sy;
                const float dn = sqrtf(dx * dx + dy * dy);
                const float ux = dx / dn, uy = dy / dn;
                a = make_float4(sx, sy, ex, ey);
                b = make_float4(ux, uy, dn + extra, hw);
                if (!(is_nan(sx) || is_nan(sy) || is_nan(ex) || is_nan(ey) || is_nan(w))) {
                    // conservative reach: w / 2 + extra around the segment (four times that when the direction is degenerate and u
                    // may have any length), plus a slack of 2^-16 of the magnitudes involved: the coverage test's own rounding is below
                    // 2^-20 of them.  Every comparison is written so that a NaN or an infinity keeps the record.
                    const bool directed = dn > 1e-10f;
                    float e = fabsf(hw) + fabsf(extra);
                    if (!directed) e = 4.0f * e;
                    const float mag = fabsf(sx) + fabsf(sy) + fabsf(ex) + fabsf(ey) + e + 32768.0f;
                    const float slack = mag * 0x1p-16f, m = e + slack;
                    keep = !(fmaxf(sx, ex) + m < fx0 || fminf(sx, ex) - m > fx1 || fmaxf(sy, ey) + m < fy0 || fminf(sy, ey) - m > fy1);
                    if (keep && directed && mag < 1e30f) {
                        // the oriented box: the centre of tile + halo against the segment, the tile's half diagonal added
                        const float R = 0.5f * sqrtf((float)(kHW * kHW + kHH * kHH)) + 0.25f;
                        const float cx = (fx0 + 0.5f * (float)kHW) - sx, cy = (fy0 + 0.5f * (float)kHH) - sy;
                        const float par = ux * cx + uy * cy, cross = ux * cy - uy * cx;
                        const float reach = m + R;
                        if (fabsf(cross) > reach || par < -reach || par > dn + reach) keep = false;
                    }
                }
            } else {
                const float cx = r[0], cy = r[1], rad = r[2], inner = r[3];
                a = make_float4(cx, cy, rad, inner);
                if (!(is_nan(cx) || is_nan(cy) || is_nan(rad) || is_nan(inner))) {
                    const float e = fabsf(rad);
                    const float mag = fabsf(cx) + fabsf(cy) + e + 32768.0f;
                    const float m = e + mag * 0x1p-16f;
                    keep = !(cx + m < fx0 || cx - m > fx1 || cy + m < fy0 || cy - m > fy1);
                }
            }
        }
        const unsigned long long vote = __ballot(keep);
        if (lane == 0) s.wave_count[wave] = __popcll(vote);
        __syncthreads();
        int base = n, total = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const int c = s.wave_count[w];
            if (w < wave) base += c;
            total += c;
        }
        if (keep) {
            const int slot = base + __popcll(vote & ((1ull << lane) - 1ull));
            s.ga[slot] = a;
            if (KIND == kLines) s.gb[slot] = b;
            s.idx[slot] = i - begin;
        }
        n += total;
        cursor += kChunk;
        __syncthreads();      // the list is complete up to n; wave_count may be written again
    }
    return n;
}

__device__ __forceinline__ float blend(float image, float colour, float alpha) { return image * (1.0f - alpha) + colour * alpha; }

template <int KIND, int CAP>
__global__ void __launch_bounds__(kThreads) draw_kernel(const float *image, float *out, int H, int W, const float *__restrict__ prims,
                                                       int n_prims, const int *__restrict__ offsets, int num_passes) {
    constexpr int F = KIND == kLines ? VSG_LINE_FLOATS : VSG_POINT_FLOATS;
    constexpr int kColour = F - 3;
    __shared__ Shared s;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int bimg = blockIdx.z, x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    const size_t plane = (size_t)H * W;
    const float *img = image + (size_t)bimg * 3 * plane;
    float *dst = out + (size_t)bimg * 3 * plane;
    // the image's records, clamped so that no offset leads outside the array
    const int begin = min(max(offsets[bimg], 0), n_prims), end = min(max(offsets[bimg + 1], begin), n_prims);

    // this thread's interior pixel
    const int px_i = tid % kTW, py_i = tid / kTW, x = x0 + px_i, y = y0 + py_i;
    const bool pixel = tid < kPix && x < W && y < H;
    if (begin == end) {      // nothing to draw: the image goes through
        if (pixel)
            for (int c = 0; c < 3; ++c) dst[c * plane + (size_t)y * W + x] = img[c * plane + (size_t)y * W + x];
        return;
    }
    const float *mine = prims + (size_t)begin * F;      // the record array of this image

    // ---- pass 0 over tile + halo
    const int hx = tid % kHW, hy = tid / kHW, sxp = x0 - 1 + hx, syp = y0 - 1 + hy;
    const bool sample = tid < kHalo && sxp >= 0 && sxp < W && syp >= 0 && syp < H;
    const float fx0 = (float)(x0 - 1), fy0 = (float)(y0 - 1);
    int cursor = begin, rounds = 0, n = 0, top0 = -1;
    do {
        n = scan_round<KIND, CAP>(s, prims, begin, end, cursor, fx0, fy0);
        top0 = max(top0, top_in_list<KIND, CAP>(s, n, (float)sxp + 0.5f, (float)syp + 0.5f, sample));
        ++rounds;
    } while (cursor < end);
    if (sample) {
        const float *col = mine + (size_t)max(top0, 0) * F + kColour;
        s.c0[tid][0] = col[0];
        s.c0[tid][1] = col[1];
        s.c0[tid][2] = col[2];
        s.c0[tid][3] = top0 >= 0 ? 1.0f : 0.0f;
    }
    __syncthreads();

    // ---- the refine mask; an unrefined pixel is finished here
    bool refine = false;
    if (pixel) {
        const int h = (py_i + 1) * kHW + px_i + 1;
        const float r = s.c0[h][0], g = s.c0[h][1], b = s.c0[h][2], a = s.c0[h][3];
        if (num_passes > 0) {
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    if (dx == 0 && dy == 0) continue;
                    const int nx = x + dx, ny = y + dy;
                    if (nx < 0 || nx >= W || ny < 0 || ny >= H) continue;      // no neighbour outside the image
                    const float *q = s.c0[h + dy * kHW + dx];
                    refine = refine || q[0] != r || q[1] != g || q[2] != b || q[3] != a;
                }
        }
        if (!refine) {
            const size_t at = (size_t)y * W + x;
            dst[at] = blend(img[at], r, a);
            dst[plane + at] = blend(img[plane + at], g, a);
            dst[2 * plane + at] = blend(img[2 * plane + at], b, a);
        }
    }
    const unsigned long long vote = __ballot(refine);
    if (lane == 0) s.wave_count[wave] = __popcll(vote);
    __syncthreads();
    int base = 0, nmask = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const int c = s.wave_count[w];
        if (w < wave) base += c;
        nmask += c;
    }
    if (refine) s.masked[base + __popcll(vote & ((1ull << lane) - 1ull))] = tid;
    if (nmask == 0) return;      // uniform over the workgroup
    __syncthreads();

    // ---- refinement: a wave per refined pixel, the lane is the subsample
    const bool single = rounds == 1;      // the list of the only round is still in LDS
    const float ox = ((float)(lane & 7) + 0.5f) / 8.0f - 0.5f, oy = ((float)(lane >> 3) + 0.5f) / 8.0f - 0.5f;
    bool first = true;
    cursor = begin;
    for (;;) {
        if (!single) n = scan_round<KIND, CAP>(s, prims, begin, end, cursor, fx0, fy0);
        const bool last = single || cursor >= end;
        for (int j = wave; j < nmask; j += kWaves) {
            const int t = s.masked[j];
            const int qx = x0 + t % kTW, qy = y0 + t / kTW;
            int top = top_in_list<KIND, CAP>(s, n, ((float)qx + 0.5f) + ox, ((float)qy + 0.5f) + oy, true);
            if (!first) top = max(top, s.rt[j][lane]);
            if (!last) {
                s.rt[j][lane] = top;      // read back by this same lane of this same wave in the next round
                continue;
            }
            const bool hit = top >= 0;
            const int count = __popcll(__ballot(hit));
            float cr = 0.0f, cg = 0.0f, cb = 0.0f;      // c_i a_i: the colour under a covered subsample, 0 under an uncovered one
            if (hit) {
                const float *col = mine + (size_t)top * F + kColour;
                cr = col[0];
                cg = col[1];
                cb = col[2];
            }
#pragma unroll
            for (int d = 1; d < kWave; d <<= 1) {
                cr += __shfl_xor(cr, d, kWave);
                cg += __shfl_xor(cg, d, kWave);
                cb += __shfl_xor(cb, d, kWave);
            }
            if (lane < 3) {
                const float sum = lane == 0 ? cr : lane == 1 ? cg : cb;
                const float colour = sum / ((float)count + 1e-10f), alpha = (float)count / 64.0f;
                const size_t at = lane * plane + (size_t)qy * W + qx;
                dst[at] = blend(img[at], colour, alpha);
            }
        }
        if (last) break;
        first = false;
    }
}

int check_common(const char *who, const void *image, const void *out, int B, int H, int W, const void *prims, int n_prims, const void *offsets,
                 int num_passes) {
    VS_CHECK(B >= 0 && H >= 0 && W >= 0 && n_prims >= 0, "%s: B = %d, H = %d, W = %d, n_prims = %d: none may be negative", who, B, H, W, n_prims);
    VS_CHECK(H <= VSG_MAX_SIDE && W <= VSG_MAX_SIDE, "%s: H = %d, W = %d exceed %d (above it a sample coordinate is not exact in f32)", who, H, W,
             VSG_MAX_SIDE);
    VS_CHECK(B <= VSG_MAX_BATCH, "%s: B = %d images exceed the grid limit %d", who, B, VSG_MAX_BATCH);
    VS_CHECK(n_prims <= (1 << 28) - 1, "%s: n_prims = %d exceeds 2^28 - 1", who, n_prims);
    VS_CHECK(num_passes == 0 || num_passes == 1, "%s: num_passes = %d is neither 0 nor 1 (deeper refinement is not built)", who, num_passes);
    if ((int64_t)B * H * W == 0) return 1;      // nothing to do
    VS_CHECK(image && out && offsets, "%s: null pointer (image, out and prim_offsets are required)", who);
    VS_CHECK(prims || n_prims == 0, "%s: null pointer (the record array is required when n_prims > 0)", who);
    if (image != out) {
        const uintptr_t a = (uintptr_t)image, b = (uintptr_t)out, bytes = (uintptr_t)B * 3 * H * W * sizeof(float);
        VS_CHECK(a + bytes <= b || b + bytes <= a, "%s: out overlaps image without being equal to it", who);
    }
    return 0;
}

template <int KIND, int CAP>
int launch(const float *image, float *out, int B, int H, int W, const float *prims, int n_prims, const int32_t *offsets, int num_passes,
           hipStream_t stream) {
    const dim3 grid((unsigned)vs::cdiv(W, kTW), (unsigned)vs::cdiv(H, kTH), (unsigned)B);
    hipLaunchKernelGGL((draw_kernel<KIND, CAP>), grid, dim3(kThreads), 0, stream, image, out, H, W, prims, n_prims, offsets, num_passes);
    VS_HIP(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" int vsg_draw_lines(const float *image, float *out, int32_t B, int32_t H, int32_t W, const float *lines, int32_t n_prims,
                              const int32_t *prim_offsets, int32_t cap, int32_t num_passes, vs_stream_t stream_) {
    const char *who = "vsg_draw_lines";
    VS_CHECK(cap == VSG_CAP_BUTT || cap == VSG_CAP_ROUND || cap == VSG_CAP_SQUARE, "%s: cap %d is none of %d (butt), %d (round), %d (square)", who,
             cap, VSG_CAP_BUTT, VSG_CAP_ROUND, VSG_CAP_SQUARE);
    const int rc = check_common(who, image, out, B, H, W, lines, n_prims, prim_offsets, num_passes);
    if (rc != 0) return rc < 0 ? rc : 0;
    const hipStream_t stream = (hipStream_t)stream_;
    if (cap == VSG_CAP_BUTT) return launch<kLines, VSG_CAP_BUTT>(image, out, B, H, W, lines, n_prims, prim_offsets, num_passes, stream);
    if (cap == VSG_CAP_ROUND) return launch<kLines, VSG_CAP_ROUND>(image, out, B, H, W, lines, n_prims, prim_offsets, num_passes, stream);
    return launch<kLines, VSG_CAP_SQUARE>(image, out, B, H, W, lines, n_prims, prim_offsets, num_passes, stream);
}

extern "C" int vsg_draw_points(const float *image, float *out, int32_t B, int32_t H, int32_t W, const float *points, int32_t n_prims,
                               const int32_t *prim_offsets, int32_t num_passes, vs_stream_t stream_) {
    const int rc = check_common("vsg_draw_points", image, out, B, H, W, points, n_prims, prim_offsets, num_passes);
    if (rc != 0) return rc < 0 ? rc : 0;
    return launch<kPoints, 0>(image, out, B, H, W, points, n_prims, prim_offsets, num_passes, (hipStream_t)stream_);
}
