// The crop shim of the dataset loaders: PIL's 8-bit Lanczos reduction, a crop window and the optional left-right mirror in one launch.
// Declared in include/vicasplat_data.h (prefix vsp_), where the algorithm is written out.
//
//   one workgroup of 256 lanes per frame, band of R output rows and tile of kTileW output columns.
//   rows     the source rows the band's vertical taps read, [row0, row0 + rows): from the vertical table, clamped to the source and to the
//            capacity the host sized the LDS tile for (rows_cap, a bound on any band of the true table; a foreign table gives wrong bytes,
//            never an access outside the tile or the source)
//   pass 1   the horizontal pass of those rows, restricted to the tile's columns, into an 8-bit LDS tile [rows][3][kTileW]: one lane per
//            (row, column), three channels each; a mirrored frame reads the source column w_in - 1 - x
//   pass 2   the vertical pass from the tile: one lane per (row, channel, four columns): a dword of LDS per tap, a float4 store where the
//            address allows it
//   A pass whose table is absent (in == out) copies.  Integer arithmetic throughout; the float form of a byte is float(u) / 255 and the
//   normalised form (float(u) / 255 - mean) / std, each operation rounded once (no contraction, no reciprocal).
// No atomics, no workspace: the same inputs give the same bits, alone or inside a batch.
#include "common.h"

#include "../../include/vicasplat_data.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kTileW = 128;            // output columns per workgroup: a tile row is 128 B per channel
constexpr int kBandRows = 16;          // output rows per workgroup, halved while the LDS tile would not fit
constexpr int kMaxRows = 128;          // source rows an LDS tile holds at most: 128 x 3 x 128 B = 48 KiB
constexpr int kPrecisionBits = 22;

struct Params {
    const void *src;
    const int32_t *bounds_x, *k_x, *bounds_y, *k_y;      // null: the pass is skipped
    const uint8_t *mirror;
    float *out;
    int h_in, w_in, kx, ky, row, col, h_out, w_out;
    int band, rows_cap, tiles_x, bands;
    int normalize;
    float mean[3], std[3];
};

__device__ __forceinline__ int clip8(int acc) {
    const int v = acc >> kPrecisionBits;      // arithmetic
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// the reference's (image * 255).clip(0, 255).type(uint8); a NaN fails the first comparison and becomes 0
__device__ __forceinline__ int quantise(float v) {
    const float s = v * 255.0f;
    return s > 0.0f ? (s < 255.0f ? (int)s : 255) : 0;
}

template <int LAYOUT>
__device__ __forceinline__ void load_pixel(const void *frame, int h_in, int w_in, int y, int x, int (&p)[3]) {
    const size_t plane = (size_t)h_in * w_in, at = (size_t)y * w_in + x;
    if (LAYOUT == VSP_LAYOUT_U8_HWC) {
        const uint8_t *s = (const uint8_t *)frame + 3 * at;
        p[0] = s[0];
        p[1] = s[1];
        p[2] = s[2];
    } else if (LAYOUT == VSP_LAYOUT_U8_CHW) {
        const uint8_t *s = (const uint8_t *)frame + at;
        p[0] = s[0];
        p[1] = s[plane];
        p[2] = s[2 * plane];
    } else {
        const float *s = (const float *)frame + at;
        p[0] = quantise(s[0]);
        p[1] = quantise(s[plane]);
        p[2] = quantise(s[2 * plane]);
    }
}

template <int LAYOUT>
__global__ void __launch_bounds__(kThreads) rescale_crop_kernel(const Params P) {
    extern __shared__ __align__(16) uint8_t tile[];      // [rows][3][kTileW]
    const int tid = threadIdx.x;
    int b = blockIdx.x;
    const int tx = b % P.tiles_x;
    b /= P.tiles_x;
    const int band = b % P.bands, n = b / P.bands;
    const int x0 = tx * kTileW, tw = min(kTileW, P.w_out - x0);
    const int y0 = band * P.band, th = min(P.band, P.h_out - y0);
    const size_t frame_elems = (size_t)3 * P.h_in * P.w_in;
    const void *frame = LAYOUT == VSP_LAYOUT_F32_CHW ? (const void *)((const float *)P.src + (size_t)n * frame_elems)
                                                     : (const void *)((const uint8_t *)P.src + (size_t)n * frame_elems);
    const bool flip = P.mirror != nullptr && P.mirror[n] != 0;

    // ---- the source rows of this band (uniform: every lane reads the same table entries)
    int row0, rows;
    if (P.k_y) {
        int lo = P.h_in, hi = 0;
        for (int y = 0; y < th; ++y) {
            const int ys = P.row + y0 + y;
            const int ymin = min(max(P.bounds_y[2 * ys], 0), P.h_in);
            const int cnt = min(max(P.bounds_y[2 * ys + 1], 0), min(P.ky, P.h_in - ymin));
            lo = min(lo, ymin);
            hi = max(hi, ymin + cnt);
        }
        row0 = lo;
        rows = min(max(hi - lo, 0), P.rows_cap);
    } else {
        row0 = P.row + y0;      // h_scaled == h_in: the window lies inside the source (checked on the host)
        rows = th;              // <= band <= rows_cap
    }

    // ---- pass 1: horizontal, into the tile
    // (a lane keeps its column: kThreads is a multiple of kTileW, so the column's window and taps are read once)
    static_assert(kThreads % kTileW == 0, "a lane's column must not change between its rows");
    const int x = tid % kTileW, xs = P.col + x0 + x;
    int xmin = 0, cnt = 0;
    const int32_t *k = nullptr;
    if (P.k_x && x < tw) {
        xmin = min(max(P.bounds_x[2 * xs], 0), P.w_in);
        cnt = min(max(P.bounds_x[2 * xs + 1], 0), min(P.kx, P.w_in - xmin));
        k = P.k_x + (size_t)xs * P.kx;
    }
    for (int r = tid / kTileW; r < rows; r += kThreads / kTileW) {
        if (x >= tw) break;
        int v[3];
        if (P.k_x) {
            int acc[3] = {1 << (kPrecisionBits - 1), 1 << (kPrecisionBits - 1), 1 << (kPrecisionBits - 1)};
            for (int t = 0; t < cnt; ++t) {
                const int sx = flip ? P.w_in - 1 - (xmin + t) : xmin + t;
                int p[3];
                load_pixel<LAYOUT>(frame, P.h_in, P.w_in, row0 + r, sx, p);
                const int kt = k[t];
                acc[0] += kt * p[0];
                acc[1] += kt * p[1];
                acc[2] += kt * p[2];
            }
            v[0] = clip8(acc[0]);
            v[1] = clip8(acc[1]);
            v[2] = clip8(acc[2]);
        } else {
            load_pixel<LAYOUT>(frame, P.h_in, P.w_in, row0 + r, flip ? P.w_in - 1 - xs : xs, v);
        }
        uint8_t *o = tile + (size_t)r * 3 * kTileW + x;
        o[0] = (uint8_t)v[0];
        o[kTileW] = (uint8_t)v[1];
        o[2 * kTileW] = (uint8_t)v[2];
    }
    __syncthreads();

    // ---- pass 2: vertical, four columns per lane
    constexpr int kQuads = kTileW / 4;
    for (int i = tid; i < th * 3 * kQuads; i += kThreads) {
        const int q = i % kQuads, c = (i / kQuads) % 3, y = i / (3 * kQuads);
        const int x = 4 * q;
        if (x >= tw) continue;
        int u[4];
        if (P.k_y) {
            const int ys = P.row + y0 + y;
            const int ymin = min(max(P.bounds_y[2 * ys], 0), P.h_in);
            const int cnt = min(max(P.bounds_y[2 * ys + 1], 0), min(P.ky, P.h_in - ymin));
            const int32_t *k = P.k_y + (size_t)ys * P.ky;
            int acc[4] = {1 << (kPrecisionBits - 1), 1 << (kPrecisionBits - 1), 1 << (kPrecisionBits - 1), 1 << (kPrecisionBits - 1)};
            for (int t = 0; t < cnt; ++t) {
                const int r = ymin + t - row0;
                if (r < 0 || r >= rows) continue;      // never with the table of these sizes
                const uint32_t w = *(const uint32_t *)(tile + ((size_t)r * 3 + c) * kTileW + x);
                const int kt = k[t];
                acc[0] += kt * (int)(w & 255u);
                acc[1] += kt * (int)((w >> 8) & 255u);
                acc[2] += kt * (int)((w >> 16) & 255u);
                acc[3] += kt * (int)(w >> 24);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) u[j] = clip8(acc[j]);
        } else {
            const uint32_t w = *(const uint32_t *)(tile + ((size_t)y * 3 + c) * kTileW + x);
            u[0] = (int)(w & 255u);
            u[1] = (int)((w >> 8) & 255u);
            u[2] = (int)((w >> 16) & 255u);
            u[3] = (int)(w >> 24);
        }
        float f[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f[j] = (float)u[j] / 255.0f;
            if (P.normalize) f[j] = (f[j] - P.mean[c]) / P.std[c];
        }
        float *o = P.out + (((size_t)n * 3 + c) * P.h_out + (y0 + y)) * P.w_out + x0 + x;
        if (x + 4 <= tw && ((uintptr_t)o & 15u) == 0) {
            *(float4 *)o = make_float4(f[0], f[1], f[2], f[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x + j < tw) o[j] = f[j];
        }
    }
}

// an upper bound on the source rows any band of `band` output rows reads: the first row's xmin is at least center_a - support - 0.5, the
// last row's xmax at most center_b + support + 0.5, and center_b - center_a = (band - 1) scale
int rows_bound(int band, int in, int out) {
    if (in == out) return band;
    const double scale = (double)in / out, support = 3.0 * (scale > 1.0 ? scale : 1.0);
    return (int)((band - 1) * scale + 2.0 * support) + 3;
}

}  // namespace

extern "C" int vsp_rescale_crop(const void *src, int32_t layout, int32_t N, int32_t h_in, int32_t w_in, const int32_t *bounds_x,
                                const int32_t *k_x, int32_t w_scaled, int32_t kx, const int32_t *bounds_y, const int32_t *k_y, int32_t h_scaled,
                                int32_t ky, int32_t row, int32_t col, int32_t h_out, int32_t w_out, const uint8_t *mirror, const float *mean,
                                const float *std, float *out, vs_stream_t stream_) {
    const char *who = "vsp_rescale_crop";
    VS_CHECK(src && out, "%s: null pointer (src and out are required)", who);
    VS_CHECK(layout == VSP_LAYOUT_U8_HWC || layout == VSP_LAYOUT_U8_CHW || layout == VSP_LAYOUT_F32_CHW,
             "%s: layout %d is none of %d (uint8 HWC), %d (uint8 CHW), %d (f32 CHW)", who, layout, VSP_LAYOUT_U8_HWC, VSP_LAYOUT_U8_CHW,
             VSP_LAYOUT_F32_CHW);
    VS_CHECK(N >= 0 && h_in >= 1 && w_in >= 1 && h_scaled >= 1 && w_scaled >= 1 && h_out >= 1 && w_out >= 1,
             "%s: N = %d, source %d x %d, scaled %d x %d, output %d x %d: N must not be negative, every size must be at least 1", who, N, h_in,
             w_in, h_scaled, w_scaled, h_out, w_out);
    VS_CHECK(h_scaled <= h_in && w_scaled <= w_in, "%s: scaled %d x %d exceeds the source %d x %d: enlarging is not built", who, h_scaled,
             w_scaled, h_in, w_in);
    VS_CHECK(row >= 0 && col >= 0 && (int64_t)row + h_out <= h_scaled && (int64_t)col + w_out <= w_scaled,
             "%s: crop window (row %d, col %d, %d x %d) lies outside the scaled image %d x %d", who, row, col, h_out, w_out, h_scaled, w_scaled);
    const bool pass_x = w_scaled != w_in, pass_y = h_scaled != h_in;
    VS_CHECK(!pass_x || (bounds_x && k_x), "%s: null horizontal table (bounds_x and k_x are required when w_scaled != w_in)", who);
    VS_CHECK(!pass_y || (bounds_y && k_y), "%s: null vertical table (bounds_y and k_y are required when h_scaled != h_in)", who);
    VS_CHECK(!pass_x || (kx >= 1 && kx <= VSP_MAX_TAPS), "%s: kx = %d is outside [1, %d]", who, kx, VSP_MAX_TAPS);
    VS_CHECK(!pass_y || (ky >= 1 && ky <= VSP_MAX_TAPS), "%s: ky = %d is outside [1, %d]", who, ky, VSP_MAX_TAPS);
    VS_CHECK((mean == nullptr) == (std == nullptr), "%s: mean and std are given together or not at all", who);
    int band = kBandRows;
    while (band > 1 && rows_bound(band, h_in, h_scaled) > kMaxRows) band /= 2;
    const int rows_cap = rows_bound(band, h_in, h_scaled);
    VS_CHECK(rows_cap <= kMaxRows, "%s: a single output row reads %d source rows (%d -> %d), more than the %d an LDS tile holds", who, rows_cap,
             h_in, h_scaled, kMaxRows);
    const int tiles_x = vs::cdiv(w_out, kTileW), bands = vs::cdiv(h_out, band);
    const int64_t blocks = (int64_t)N * tiles_x * bands;
    VS_CHECK(blocks <= INT32_MAX, "%s: %lld workgroups (N = %d, output %d x %d) exceed 2^31 - 1", who, (long long)blocks, N, h_out, w_out);
    if (N == 0) return 0;

    Params P;
    P.src = src;
    P.bounds_x = pass_x ? bounds_x : nullptr;
    P.k_x = pass_x ? k_x : nullptr;
    P.bounds_y = pass_y ? bounds_y : nullptr;
    P.k_y = pass_y ? k_y : nullptr;
    P.mirror = mirror;
    P.out = out;
    P.h_in = h_in;
    P.w_in = w_in;
    P.kx = kx;
    P.ky = ky;
    P.row = row;
    P.col = col;
    P.h_out = h_out;
    P.w_out = w_out;
    P.band = band;
    P.rows_cap = rows_cap;
    P.tiles_x = tiles_x;
    P.bands = bands;
    P.normalize = mean != nullptr;
    for (int c = 0; c < 3; ++c) {
        P.mean[c] = mean ? mean[c] : 0.0f;
        P.std[c] = std ? std[c] : 1.0f;
    }
    const hipStream_t stream = (hipStream_t)stream_;
    const size_t lds = (size_t)rows_cap * 3 * kTileW;
    const dim3 grid((unsigned)blocks), block(kThreads);
    if (layout == VSP_LAYOUT_U8_HWC)
        hipLaunchKernelGGL(rescale_crop_kernel<VSP_LAYOUT_U8_HWC>, grid, block, lds, stream, P);
    else if (layout == VSP_LAYOUT_U8_CHW)
        hipLaunchKernelGGL(rescale_crop_kernel<VSP_LAYOUT_U8_CHW>, grid, block, lds, stream, P);
    else
        hipLaunchKernelGGL(rescale_crop_kernel<VSP_LAYOUT_F32_CHW>, grid, block, lds, stream, P);
    VS_HIP(hipGetLastError());
    return 0;
}
