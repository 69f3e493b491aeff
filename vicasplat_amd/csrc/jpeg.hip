// The baseline JPEG decoder: compressed frames -> uint8 [N, h, w, 3], byte for byte libjpeg-turbo's default decode.
// Declared in include/vicasplat_jpeg.h (prefix vsj_), where the formats, the arithmetic and the status bits are written out; the serial
// parts (descriptor checks, bit reader, Huffman decode, inverse DCT) are csrc/jpeg_decode.h, shared with the host program of the tests.
//
//   entropy_kernel   one wave per (frame, 64 restart segments), one lane per segment; the frame's DC / AC tables in LDS.  Coefficients go
//                    to the (zeroed) workspace as int16 in natural order; every segment writes its own status word.
//   idct_kernel      one lane per 8 x 8 block: dequantise, islow inverse DCT, clamp; 8-byte stores into the component's padded plane.
//   colour_kernel    one lane per four output pixels of a row: chroma upsampling on the true subsampled size, YCbCr -> RGB, three dword
//                    stores where the address allows them.
//   status_kernel    one wave per frame: the OR of its segments' words.
// No atomics and no host synchronisation; the descriptors are checked on the device (frame_geometry) before any index is formed from them.
#include "common.h"

#include "jpeg_decode.h"

namespace {

constexpr int kEntropyThreads = 64;      // one wave: lanes of a frame share its tables (and fill the 64 zig-zag entries)
constexpr int kThreads = 256;

struct Args {
    const int32_t *frames, *segs;
    const uint16_t *quant;
    const uint8_t *huff, *bytes;
    int16_t *coef;
    uint8_t *samples;
    int32_t *seg_status;
    uint8_t *out;
    int32_t *status;
    int N, h, w, segments, n_quant, n_huff, nbytes;
    int64_t blocks;
    int chunks;      // entropy workgroups per frame, idct / colour tiles per frame: the divisor of the kernel's own grid
};

__device__ __forceinline__ bool geometry(const Args &A, int n, vsj::Geom &g) {
    return vsj::frame_geometry(A.frames + (size_t)n * VSJ_FRAME_WORDS, A.h, A.w, A.segments, A.blocks, A.n_quant, A.n_huff, g);
}

__global__ void __launch_bounds__(kEntropyThreads) entropy_kernel(const Args A) {
    __shared__ __align__(16) uint8_t tabs[6 * VSJ_HUFF_BYTES];
    __shared__ uint8_t zz[64];
    const int n = blockIdx.x / A.chunks, chunk = blockIdx.x % A.chunks, tid = threadIdx.x;
    vsj::Geom g;
    if (!geometry(A, n, g) || chunk * kEntropyThreads >= g.nseg) return;      // uniform
    static_assert(VSJ_HUFF_BYTES % 16 == 0, "tables are copied 16 bytes at a time");
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (c >= g.ncomp) break;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const uint4 *src = (const uint4 *)(A.huff + (size_t)(k ? g.ac[c] : g.dc[c]) * VSJ_HUFF_BYTES);
            uint4 *dst = (uint4 *)(tabs + (3 * k + c) * VSJ_HUFF_BYTES);
            for (int i = tid; i < VSJ_HUFF_BYTES / 16; i += kEntropyThreads) dst[i] = src[i];
        }
    }
    zz[tid] = (uint8_t)vsj::zigzag_to_natural(tid);
    __syncthreads();
    const int s = chunk * kEntropyThreads + tid;
    if (s >= g.nseg) return;
    const int32_t *seg = A.segs + (size_t)(g.seg0 + s) * VSJ_SEG_WORDS;
    const int begin = seg[0], end = seg[1], first = seg[2], count = seg[3];
    int err = VSJ_STATUS_DESC;
    if (begin >= 0 && begin <= end && end <= A.nbytes && first >= 0 && count >= 0 && (int64_t)first + count <= (int64_t)g.mcus_x * g.mcus_y) {
        err = vsj::decode_segment(g, A.bytes, begin, end, first, count, tabs, zz, A.coef + (size_t)g.block0 * 64);
    }
    A.seg_status[g.seg0 + s] = err;
}

__global__ void __launch_bounds__(kThreads) idct_kernel(const Args A) {
    const int n = blockIdx.x / A.chunks, tile = blockIdx.x % A.chunks;
    vsj::Geom g;
    if (!geometry(A, n, g)) return;
    const int j = tile * kThreads + threadIdx.x;
    if (j >= g.base[3]) return;
    const int c = j < g.base[1] ? 0 : (j < g.base[2] ? 1 : 2);
    const int jj = j - g.base[c], by = jj / g.bw[c], bx = jj % g.bw[c];
    uint32_t px[16];
    vsj::idct_islow((const int16_t *)__builtin_assume_aligned(A.coef + ((size_t)g.block0 + j) * 64, 16), A.quant + (size_t)g.qt[c] * 64, px);
    const size_t stride = (size_t)g.bw[c] * 8;
    uint8_t *plane = A.samples + ((size_t)g.block0 + g.base[c]) * 64 + (size_t)by * 8 * stride + (size_t)bx * 8;
#pragma unroll
    for (int r = 0; r < 8; ++r) *(uint2 *)(plane + r * stride) = make_uint2(px[2 * r], px[2 * r + 1]);
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// the chroma samples under the four output pixels 4 q .. 4 q + 3 of row y, from one chroma plane of row stride `stride`
__device__ __forceinline__ void chroma4(const uint8_t *plane, size_t stride, const vsj::Geom &g, int h, int w, int y, int q, int (&o)[4]) {
    if (g.hs == 1) {      // 1 x 1: the plane has the luma's size
        const uint32_t v = *(const uint32_t *)(plane + (size_t)y * stride + 4 * q);
        o[0] = v & 255u, o[1] = (v >> 8) & 255u, o[2] = (v >> 16) & 255u, o[3] = v >> 24;
        return;
    }
    const int wc = (w + 1) / 2, hc = g.vs == 2 ? (h + 1) / 2 : h;      // the true subsampled size, not the padded plane's
    const int r = g.vs == 2 ? y >> 1 : y;
    const uint8_t *row = plane + (size_t)r * stride;
    if (wc <= 2) {
        o[0] = o[1] = row[min(2 * q, wc - 1)];
        o[2] = o[3] = row[min(2 * q + 1, wc - 1)];
        return;
    }
    int s[4];
    if (g.vs == 2) {
        const uint8_t *near = plane + (size_t)min(max((y & 1) ? r + 1 : r - 1, 0), hc - 1) * stride;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = min(max(2 * q - 1 + j, 0), wc - 1);
            s[j] = 3 * row[x] + near[x];
        }
        o[0] = (3 * s[1] + s[0] + 8) >> 4;
        o[1] = (3 * s[1] + s[2] + 7) >> 4;
        o[2] = (3 * s[2] + s[1] + 8) >> 4;
        o[3] = (3 * s[2] + s[3] + 7) >> 4;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = row[min(max(2 * q - 1 + j, 0), wc - 1)];
        o[0] = (3 * s[1] + s[0] + 1) >> 2;
        o[1] = (3 * s[1] + s[2] + 2) >> 2;
        o[2] = (3 * s[2] + s[1] + 1) >> 2;
        o[3] = (3 * s[2] + s[3] + 2) >> 2;
    }
}

__global__ void __launch_bounds__(kThreads) colour_kernel(const Args A) {
    const int n = blockIdx.x / A.chunks, tile = blockIdx.x % A.chunks;
    vsj::Geom g;
    if (!geometry(A, n, g)) return;
    const int quads = (A.w + 3) / 4;
    const int64_t i = (int64_t)tile * kThreads + threadIdx.x;
    if (i >= (int64_t)quads * A.h) return;
    const int y = (int)(i / quads), q = (int)(i % quads), x = 4 * q;
    const uint8_t *planes = A.samples + (size_t)g.block0 * 64;
    // (every plane is padded to whole blocks: the dword at column 4 q of a row lies inside it)
    const uint32_t yy = *(const uint32_t *)(planes + (size_t)y * g.bw[0] * 8 + x);
    uint32_t rgb[3] = {0, 0, 0};      // 12 bytes: R G B R | G B R G | B R G B
    int cb[4], cr[4];
    if (g.ncomp == 3) {
        chroma4(planes + (size_t)g.base[1] * 64, (size_t)g.bw[1] * 8, g, A.h, A.w, y, q, cb);
        chroma4(planes + (size_t)g.base[2] * 64, (size_t)g.bw[2] * 8, g, A.h, A.w, y, q, cr);
    }
    uint8_t px[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int lum = (int)((yy >> (8 * j)) & 255u);
        int R = lum, G = lum, B = lum;
        if (g.ncomp == 3) {
            const int b = cb[j] - 128, r = cr[j] - 128;
            R = clamp255(lum + ((91881 * r + 32768) >> 16));
            G = clamp255(lum + ((-22554 * b - 46802 * r + 32768) >> 16));
            B = clamp255(lum + ((116130 * b + 32768) >> 16));
        }
        px[3 * j] = (uint8_t)R;
        px[3 * j + 1] = (uint8_t)G;
        px[3 * j + 2] = (uint8_t)B;
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) rgb[k / 4] |= (uint32_t)px[k] << (8 * (k % 4));
    uint8_t *o = A.out + (((size_t)n * A.h + y) * A.w + x) * 3;
    if (x + 4 <= A.w && ((uintptr_t)o & 3u) == 0) {
        uint32_t *o4 = (uint32_t *)o;
        o4[0] = rgb[0];
        o4[1] = rgb[1];
        o4[2] = rgb[2];
    } else {
        for (int k = 0; k < 12; ++k)
            if (x + k / 3 < A.w) o[k] = px[k];
    }
}

__global__ void __launch_bounds__(64) status_kernel(const Args A) {
    const int n = blockIdx.x;
    vsj::Geom g;
    int v = 0;
    if (!geometry(A, n, g)) {
        v = VSJ_STATUS_DESC;
    } else {
        for (int s = threadIdx.x; s < g.nseg; s += 64) v |= A.seg_status[g.seg0 + s];
    }
    for (int d = 32; d >= 1; d >>= 1) v |= __shfl_xor(v, d, 64);
    if (threadIdx.x == 0) A.status[n] = v;
}

int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

}  // namespace

extern "C" int64_t vsj_workspace_bytes(int64_t blocks, int32_t segments) {
    VS_CHECK(blocks >= 0 && blocks <= INT32_MAX && segments >= 0, "vsj_workspace_bytes: blocks = %lld, segments = %d: neither may be negative, blocks at most 2^31 - 1",
             (long long)blocks, segments);
    return blocks * (128 + 64) + align16((int64_t)segments * 4);
}

extern "C" int vsj_decode(const void *packed, int64_t packed_bytes, int32_t N, int32_t h, int32_t w, int32_t segments, int32_t max_frame_segments,
                          int32_t n_quant, int32_t n_huff, int64_t blocks, void *workspace, int64_t workspace_bytes, uint8_t *out,
                          int32_t *status, vs_stream_t stream_) {
    const char *who = "vsj_decode";
    VS_CHECK(packed && workspace && out && status, "%s: null pointer (packed, workspace, out and status are required)", who);
    VS_CHECK(N >= 0 && h >= 1 && w >= 1 && segments >= 1 && max_frame_segments >= 1 && n_quant >= 1 && n_huff >= 1 && blocks >= 1,
             "%s: N = %d, frame %d x %d, segments = %d, max_frame_segments = %d, n_quant = %d, n_huff = %d, blocks = %lld: N must not be negative, "
             "every other size must be at least 1", who, N, h, w, segments, max_frame_segments, n_quant, n_huff, (long long)blocks);
    VS_CHECK(blocks <= INT32_MAX, "%s: %lld blocks exceed 2^31 - 1", who, (long long)blocks);
    const int64_t at_segs = (int64_t)N * VSJ_FRAME_WORDS * 4, at_quant = at_segs + (int64_t)segments * VSJ_SEG_WORDS * 4;
    const int64_t at_huff = at_quant + (int64_t)n_quant * 128, at_bytes = at_huff + (int64_t)n_huff * VSJ_HUFF_BYTES;
    VS_CHECK(at_bytes <= packed_bytes, "%s: the sections (%d frames, %d segments, %d + %d tables) take %lld bytes, the packed buffer has %lld", who, N,
             segments, n_quant, n_huff, (long long)at_bytes, (long long)packed_bytes);
    VS_CHECK(packed_bytes - at_bytes <= INT32_MAX, "%s: %lld compressed bytes exceed 2^31 - 1", who, (long long)(packed_bytes - at_bytes));
    const int64_t need = (int64_t)blocks * (128 + 64) + align16((int64_t)segments * 4);
    VS_CHECK(workspace_bytes >= need, "%s: the workspace has %lld bytes, %lld blocks and %d segments need %lld (vsj_workspace_bytes)", who,
             (long long)workspace_bytes, (long long)blocks, segments, (long long)need);
    VS_CHECK(((uintptr_t)packed & 15u) == 0 && ((uintptr_t)workspace & 15u) == 0 && ((uintptr_t)status & 3u) == 0,
             "%s: packed and workspace must be 16-byte aligned, status 4-byte aligned", who);
    const int64_t worst = 12 * (int64_t)vs::cdiv(w, 16) * vs::cdiv(h, 16);      // blocks of a frame at most: 4:4:4 on 16 x 16 MCUs bounds every sampling
    const int chunks_e = vs::cdiv(max_frame_segments, kEntropyThreads);
    const int64_t tiles_i = vs::cdiv64(worst, kThreads), tiles_c = vs::cdiv64((int64_t)vs::cdiv(w, 4) * h, kThreads);
    VS_CHECK((int64_t)N * chunks_e <= INT32_MAX && N * tiles_i <= INT32_MAX && N * tiles_c <= INT32_MAX,
             "%s: N = %d frames of %d x %d with up to %d segments exceed 2^31 - 1 workgroups", who, N, h, w, max_frame_segments);
    if (N == 0) return 0;

    const uint8_t *base = (const uint8_t *)packed;
    Args A;
    A.frames = (const int32_t *)base;
    A.segs = (const int32_t *)(base + at_segs);
    A.quant = (const uint16_t *)(base + at_quant);
    A.huff = base + at_huff;
    A.bytes = base + at_bytes;
    A.coef = (int16_t *)workspace;
    A.samples = (uint8_t *)workspace + blocks * 128;
    A.seg_status = (int32_t *)((uint8_t *)workspace + blocks * (128 + 64));
    A.out = out;
    A.status = status;
    A.N = N;
    A.h = h;
    A.w = w;
    A.segments = segments;
    A.n_quant = n_quant;
    A.n_huff = n_huff;
    A.nbytes = (int)(packed_bytes - at_bytes);
    A.blocks = blocks;
    const hipStream_t stream = (hipStream_t)stream_;
    VS_HIP(hipMemsetAsync(workspace, 0, (size_t)blocks * 128, stream));      // coefficients an end-of-block leaves out are zero
    A.chunks = chunks_e;
    hipLaunchKernelGGL(entropy_kernel, dim3((unsigned)(N * chunks_e)), dim3(kEntropyThreads), 0, stream, A);
    A.chunks = (int)tiles_i;
    hipLaunchKernelGGL(idct_kernel, dim3((unsigned)(N * tiles_i)), dim3(kThreads), 0, stream, A);
    A.chunks = (int)tiles_c;
    hipLaunchKernelGGL(colour_kernel, dim3((unsigned)(N * tiles_c)), dim3(kThreads), 0, stream, A);
    hipLaunchKernelGGL(status_kernel, dim3((unsigned)N), dim3(64), 0, stream, A);
    VS_HIP(hipGetLastError());
    return 0;
}
