// The PNG encoder: device images -> complete PNG files in device memory, one per image.
// Declared in include/vicasplat_png.h (prefix vse_), where the stream is written out; the serial parts (filters, tokens, code construction,
// block decision, bit writer, checksums) are csrc/png_deflate.h, shared with the host program of the tests.
//
//   filter_kernel    one wave per (image, row): the row quantised on the fly, the five filters' costs by a wave reduction, the chosen row to
//                    the workspace.
//   segment_kernel   two waves per (image, segment), the coder's tables in LDS (6 KB: sixteen segments a CU; staging the segment's 16 KB
//                    there as well was measured 1.7 x slower, the serial coder living on how many segments run at once).  One lane runs the serial coder
//                    (tokens, tree, block decision, the bits); every lane sorts the symbols by frequency for it; wave 1 takes the segment's
//                    Adler sums beside the token count and the chunk's CRC-32 after the bits, a stretch per lane, combined in order.
//   layout_kernel    one lane per image: the chunks' offsets, the Adler-32 of the whole stream, the file's length.
//   gather_kernel    one workgroup per (image, segment): the chunk (length, type, data, CRC) to its place; the first also writes the
//                    signature and IHDR, the last the Adler-32 and IEND.
// No atomics and no host synchronisation; every store is an ordinary vector store.
#include "common.h"

#include "png_deflate.h"

namespace {

constexpr int kWave = 64;
constexpr int kGather = 256;

struct Args {
    const void *images;
    uint8_t *filt, *segdata, *out;
    uint4 *meta;           // per segment: deflate bytes, the CRC-32 of type and data, Adler sums sa and sb
    int32_t *offs;         // per segment: the chunk's offset in its file
    uint32_t *adler;       // per image
    int32_t *lengths;
    vse::Shape s;
    int n, layout, mode;
    int64_t fstride, cap, out_stride;
};

__device__ __forceinline__ int sample(const Args &A, int i, int y, int j) {      // byte j of row y of image i, quantised
    const int x = j / A.s.c, ch = j - x * A.s.c;
    if (A.layout == VSP_LAYOUT_U8_HWC) return ((const uint8_t *)A.images)[((size_t)i * A.s.h + y) * ((size_t)A.s.w * A.s.c) + j];
    const size_t at = (((size_t)i * A.s.c + ch) * A.s.h + y) * A.s.w + x;
    return A.layout == VSP_LAYOUT_U8_CHW ? ((const uint8_t *)A.images)[at] : vse::quantise(((const float *)A.images)[at]);
}

__global__ void __launch_bounds__(kWave) filter_kernel(const Args A) {
    const int i = blockIdx.x / A.s.h, y = blockIdx.x % A.s.h, lane = threadIdx.x;
    const int nb = A.s.rb - 1, c = A.s.c;
    int type = A.mode;
    if (A.mode == VSE_FILTER_ADAPTIVE) {
        uint32_t cost[5] = {0, 0, 0, 0, 0};
        for (int j = lane; j < nb; j += kWave) {
            const int x = sample(A, i, y, j), a = j >= c ? sample(A, i, y, j - c) : 0;
            const int b = y > 0 ? sample(A, i, y - 1, j) : 0, cc = (y > 0 && j >= c) ? sample(A, i, y - 1, j - c) : 0;
#pragma unroll
            for (int t = 0; t < 5; ++t) cost[t] += (uint32_t)vse::signed_cost(vse::filter_value(t, x, a, b, cc));
        }
#pragma unroll
        for (int t = 0; t < 5; ++t)
            for (int d = 32; d >= 1; d >>= 1) cost[t] += __shfl_xor(cost[t], d, kWave);
        type = vse::best_filter(cost);
    }
    uint8_t *row = A.filt + (size_t)i * A.fstride + (size_t)y * A.s.rb;
    if (lane == 0) row[0] = (uint8_t)type;
    for (int j = lane; j < nb; j += kWave) {
        const int x = sample(A, i, y, j), a = j >= c ? sample(A, i, y, j - c) : 0;
        const int b = y > 0 ? sample(A, i, y - 1, j) : 0, cc = (y > 0 && j >= c) ? sample(A, i, y - 1, j - c) : 0;
        row[1 + j] = vse::filter_value(type, x, a, b, cc);
    }
}

__global__ void __launch_bounds__(2 * kWave) segment_kernel(const Args A) {
    __shared__ vse::Work work;
    __shared__ vse::CountTokens counts;
    __shared__ uint32_t sums[2];
    __shared__ int bytes;
    const int i = blockIdx.x / A.s.S, seg = blockIdx.x % A.s.S, tid = threadIdx.x, lane = tid - kWave;
    const int L = vse::segment_rows(A.s, seg) * A.s.rb;
    const uint8_t *src = A.filt + (size_t)i * A.fstride + (size_t)seg * A.s.R * A.s.rb;
    uint8_t *dst = A.segdata + ((size_t)i * A.s.S + seg) * A.cap;
    if (tid == 0) {
        counts = vse::count_segment(src, L, work);
    } else if (tid >= kWave) {
        const int per = (L + kWave - 1) / kWave;
        const int lo = min(lane * per, L), hi = min(lo + per, L);
        uint32_t sa, sb;
        vse::adler_sums(src + lo, hi - lo, sa, sb);
        // the stretches in order: lane k's sums appended to those of the lanes below it
        uint32_t a = 0, b = 0;
        for (int k = 0; k < kWave; ++k) {
            const uint32_t ka = __shfl(sa, k, kWave), kb = __shfl(sb, k, kWave);
            const int klo = min(k * per, L), klen = min(klo + per, L) - klo;
            vse::adler_append(a, b, ka, kb, klen);
        }
        if (lane == 0) sums[0] = a, sums[1] = b;
    }
    __syncthreads();
    // vse::sort_symbols with every lane: a used symbol's place is the number of used symbols before it in (frequency, symbol) order
    for (int s = tid; s < 286; s += 2 * kWave) {
        const uint32_t f = work.freq[s];
        if (f == 0) continue;
        int rank = 0;
        for (int u = 0; u < 286; ++u) {
            const uint32_t fu = work.freq[u];
            rank += (fu != 0 && (fu < f || (fu == f && u < s))) ? 1 : 0;
        }
        work.order[rank] = (uint16_t)s;
    }
    __syncthreads();
    if (tid == 0) {
        int used = 0;
        for (int s = 0; s < 286; ++s) used += work.freq[s] != 0 ? 1 : 0;
        bytes = vse::finish_segment(src, L, seg == A.s.S - 1, dst, work, counts, used);
    }
    __syncthreads();
    if (tid >= kWave) {      // the chunk's CRC-32 so far (type, the zlib header in the first chunk, the data): a stretch per lane, combined in order
        const int len = bytes, per = (len + kWave - 1) / kWave;
        const int lo = min(lane * per, len), hi = min(lo + per, len);
        const uint32_t mine = ~vse::crc_bytes(0xFFFFFFFFu, dst + lo, hi - lo), shift = vse::crc_x8n((uint32_t)(hi - lo));
        uint32_t crc = 0xFFFFFFFFu;
        crc = vse::crc_update(crc, 'I'), crc = vse::crc_update(crc, 'D'), crc = vse::crc_update(crc, 'A'), crc = vse::crc_update(crc, 'T');
        if (seg == 0) crc = vse::crc_update(crc, 0x78), crc = vse::crc_update(crc, 0x01);
        crc = ~crc;
        for (int k = 0; k < kWave; ++k) crc = vse::crc_mul(__shfl(shift, k, kWave), crc) ^ __shfl(mine, k, kWave);
        if (lane == 0) A.meta[(size_t)i * A.s.S + seg] = make_uint4((uint32_t)len, crc, sums[0], sums[1]);
    }
}

__global__ void __launch_bounds__(kWave) layout_kernel(const Args A) {
    const int i = blockIdx.x * kWave + threadIdx.x;
    if (i >= A.n) return;
    uint32_t a = 1, b = 0;
    int64_t at = vse::kPrefixBytes;
    for (int seg = 0; seg < A.s.S; ++seg) {
        const uint4 m = A.meta[(size_t)i * A.s.S + seg];
        A.offs[(size_t)i * A.s.S + seg] = (int32_t)at;
        at += 12 + (int64_t)m.x + (seg == 0 ? 2 : 0) + (seg == A.s.S - 1 ? 4 : 0);
        vse::adler_append(a, b, m.z, m.w, vse::segment_rows(A.s, seg) * A.s.rb);
    }
    A.adler[i] = (b << 16) | a;
    A.lengths[i] = (int32_t)(at + vse::kIendBytes);
}

__global__ void __launch_bounds__(kGather) gather_kernel(const Args A) {
    const int i = blockIdx.x / A.s.S, seg = blockIdx.x % A.s.S, tid = threadIdx.x;
    const bool first = seg == 0, last = seg == A.s.S - 1;
    const uint4 m = A.meta[(size_t)i * A.s.S + seg];
    const int len = (int)m.x, head = first ? 2 : 0;
    uint8_t *file = A.out + (size_t)i * A.out_stride;
    uint8_t *chunk = file + A.offs[(size_t)i * A.s.S + seg];
    const uint8_t *src = A.segdata + ((size_t)i * A.s.S + seg) * A.cap;
    for (int k = tid; k < len; k += kGather) chunk[8 + head + k] = src[k];
    if (first && tid == kWave) {
        uint8_t p[vse::kPrefixBytes];
        vse::file_prefix(A.s, p);
        for (int k = 0; k < vse::kPrefixBytes; ++k) file[k] = p[k];
    }
    if (tid == 0) {
        const uint32_t adler = A.adler[i];
        const int dlen = len + head + (last ? 4 : 0);
        vse::put_be32(chunk, (uint32_t)dlen);
        chunk[4] = 'I', chunk[5] = 'D', chunk[6] = 'A', chunk[7] = 'T';
        if (first) chunk[8] = 0x78, chunk[9] = 0x01;
        uint32_t crc = ~m.y;
        uint8_t *tail = chunk + 8 + head + len;
        if (last) {
            vse::put_be32(tail, adler);
            for (int k = 0; k < 4; ++k) crc = vse::crc_update(crc, (uint8_t)(adler >> (24 - 8 * k)));
            tail += 4;
        }
        vse::put_be32(tail, ~crc);
        if (last)
            for (int k = 0; k < vse::kIendBytes; ++k) tail[4 + k] = vse::iend_byte(k);
    }
}

int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// the shape or a message: false for what the encoder refuses
bool checked_shape(const char *who, int h, int w, int c, vse::Shape &s) {
    if (h < 1 || w < 1) {
        vs::set_error("%s: image %d x %d: both sizes must be at least 1", who, h, w);
        return false;
    }
    if (!(c == 1 || c == 3 || c == 4)) {
        vs::set_error("%s: c = %d: 1 (grey), 3 (RGB) or 4 (RGBA) channels", who, c);
        return false;
    }
    if (!vse::make_shape(h, w, c, s)) {
        vs::set_error("%s: image %d x %d x %d: a row of %lld bytes or %d rows exceed 65535", who, h, w, c, 1 + (long long)w * c, h);
        return false;
    }
    return true;
}

struct Layout {
    int64_t fstride, cap, at_seg, at_meta, at_offs, at_adler, total;
};

Layout workspace_layout(const vse::Shape &s, int64_t n) {
    Layout l;
    l.fstride = align16((int64_t)s.h * s.rb);
    l.cap = vse::segment_capacity(s);
    l.at_seg = n * l.fstride;
    l.at_meta = l.at_seg + n * s.S * l.cap;
    l.at_offs = l.at_meta + n * s.S * 16;
    l.at_adler = l.at_offs + align16(n * s.S * 4);
    l.total = l.at_adler + align16(n * 4);
    return l;
}

}  // namespace

extern "C" int64_t vse_png_bound(int32_t h, int32_t w, int32_t c) {
    vse::Shape s;
    if (!checked_shape("vse_png_bound", h, w, c, s)) return -1;
    return vse::file_bound(s);
}

extern "C" int64_t vse_png_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t c) {
    const char *who = "vse_png_workspace_bytes";
    vse::Shape s;
    if (!checked_shape(who, h, w, c, s)) return -1;
    VS_CHECK(n >= 0, "%s: n = %d must not be negative", who, n);
    VS_CHECK((int64_t)n * vse::file_bound(s) < (1ll << 31), "%s: %d files of up to %lld bytes reach 2^31", who, n, (long long)vse::file_bound(s));
    return workspace_layout(s, n).total;
}

extern "C" int vse_png_encode(const void *images, int32_t layout, int32_t n, int32_t h, int32_t w, int32_t c, int32_t filter_mode, void *workspace,
                              int64_t workspace_bytes, uint8_t *out, int64_t out_stride, int32_t *lengths, vs_stream_t stream_) {
    const char *who = "vse_png_encode";
    VS_CHECK(images && workspace && out && lengths, "%s: null pointer (images, workspace, out and lengths are required)", who);
    VS_CHECK(layout == VSP_LAYOUT_U8_HWC || layout == VSP_LAYOUT_U8_CHW || layout == VSP_LAYOUT_F32_CHW, "%s: unknown layout %d", who, layout);
    VS_CHECK(filter_mode >= VSE_FILTER_NONE && filter_mode <= VSE_FILTER_ADAPTIVE, "%s: unknown filter mode %d (0 .. 4 or VSE_FILTER_ADAPTIVE)", who,
             filter_mode);
    vse::Shape s;
    if (!checked_shape(who, h, w, c, s)) return -1;
    VS_CHECK(n >= 0, "%s: n = %d must not be negative", who, n);
    const int64_t bound = vse::file_bound(s);
    VS_CHECK((int64_t)n * bound < (1ll << 31), "%s: %d files of up to %lld bytes reach 2^31", who, n, (long long)bound);
    VS_CHECK(out_stride >= bound, "%s: out_stride = %lld is below the bound of %lld bytes (vse_png_bound)", who, (long long)out_stride, (long long)bound);
    const Layout l = workspace_layout(s, n);
    VS_CHECK(workspace_bytes >= l.total, "%s: the workspace has %lld bytes, %d images of %d x %d x %d need %lld (vse_png_workspace_bytes)", who,
             (long long)workspace_bytes, n, h, w, c, (long long)l.total);
    VS_CHECK(((uintptr_t)workspace & 15u) == 0 && ((uintptr_t)lengths & 3u) == 0 && (layout != VSP_LAYOUT_F32_CHW || ((uintptr_t)images & 3u) == 0),
             "%s: the workspace must be 16-byte aligned, lengths and f32 images 4-byte aligned", who);
    if (n == 0) return 0;

    Args A;
    uint8_t *base = (uint8_t *)workspace;
    A.images = images;
    A.filt = base;
    A.segdata = base + l.at_seg;
    A.meta = (uint4 *)(base + l.at_meta);
    A.offs = (int32_t *)(base + l.at_offs);
    A.adler = (uint32_t *)(base + l.at_adler);
    A.out = out;
    A.lengths = lengths;
    A.s = s;
    A.n = n;
    A.layout = layout;
    A.mode = filter_mode;
    A.fstride = l.fstride;
    A.cap = l.cap;
    A.out_stride = out_stride;
    const hipStream_t stream = (hipStream_t)stream_;
    // (n bound < 2^31 and bound > h, S: the grids below are below 2^31 workgroups)
    hipLaunchKernelGGL(filter_kernel, dim3((unsigned)(n * h)), dim3(kWave), 0, stream, A);
    hipLaunchKernelGGL(segment_kernel, dim3((unsigned)(n * s.S)), dim3(2 * kWave), 0, stream, A);
    hipLaunchKernelGGL(layout_kernel, dim3((unsigned)vs::cdiv(n, kWave)), dim3(kWave), 0, stream, A);
    hipLaunchKernelGGL(gather_kernel, dim3((unsigned)(n * s.S)), dim3(kGather), 0, stream, A);
    VS_HIP(hipGetLastError());
    return 0;
}
