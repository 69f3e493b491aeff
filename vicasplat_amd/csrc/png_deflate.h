// The PNG encoder's serial parts, for the device and for the host: the shape rules, the quantisation, the filter predictors, the tokens of
// one segment, the code-length construction, the block-size decision, the bit writer, Adler-32 and CRC-32, and the fixed bytes of a file.
// csrc/png.hip builds its kernels from these functions; tests/png_probe.cpp compiles the same text with the host compiler under the address
// and undefined-behaviour sanitizers.  include/vicasplat_png.h states the stream; nothing here depends on HIP.
#pragma once
#include <cstdint>
#include <cstring>

#include "../../include/vicasplat_png.h"

#if defined(__HIPCC__)
#define VSE_HD __host__ __device__ __forceinline__
#else
#define VSE_HD inline
#endif

namespace vse {

constexpr int kLitLen = 288;          // literal/length symbols of the fixed code (286 can occur)
constexpr int kClen = 19;
constexpr uint32_t kAdlerMod = 65521;

// ---- the shape ----------------------------------------------------------------------------------------------------------------------------
struct Shape {
    int h, w, c, rb;      // rb: bytes of a filtered row
    int R, S;             // rows per segment, segments
};

VSE_HD bool make_shape(int h, int w, int c, Shape &s) {
    if (h < 1 || w < 1 || !(c == 1 || c == 3 || c == 4) || h > VSE_MAX_ROWS) return false;
    const int64_t rb = 1 + (int64_t)w * c;
    if (rb > VSE_MAX_ROW_BYTES) return false;
    s.h = h, s.w = w, s.c = c, s.rb = (int)rb;
    const int r = VSE_SEGMENT_BYTES / s.rb;
    s.R = r < 1 ? 1 : (r > h ? h : r);
    s.S = (h + s.R - 1) / s.R;
    return true;
}

VSE_HD int segment_rows(const Shape &s, int seg) {
    const int left = s.h - seg * s.R;
    return left < s.R ? left : s.R;
}

VSE_HD int64_t segment_capacity(const Shape &s) { return (((int64_t)s.R * s.rb + 10) + 15) & ~(int64_t)15; }      // deflate data of one segment at most, padded
VSE_HD int64_t file_bound(const Shape &s) { return 51 + (int64_t)s.h * s.rb + 22 * (int64_t)s.S; }

// ---- pixels and filters -------------------------------------------------------------------------------------------------------------------
VSE_HD uint8_t quantise(float x) {
    float v = x > 0.0f ? x : 0.0f;      // a NaN compares false: 0
    v = v < 1.0f ? v : 1.0f;
    return (uint8_t)(int)(v * 255.0f);
}

VSE_HD int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

VSE_HD uint8_t filter_value(int type, int x, int a, int b, int c) {
    const int pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : paeth(a, b, c);
    return (uint8_t)(x - pred);
}

VSE_HD int signed_cost(uint8_t v) { return v < 128 ? v : 256 - v; }

// the filter type of a row from the five costs: the smallest, the lowest type on a tie
VSE_HD int best_filter(const uint32_t (&cost)[5]) {
    int best = 0;
    for (int t = 1; t < 5; ++t)
        if (cost[t] < cost[best]) best = t;
    return best;
}

// ---- checksums ----------------------------------------------------------------------------------------------------------------------------
VSE_HD uint32_t crc_update(uint32_t crc, uint8_t byte) {      // the running (not yet inverted) CRC-32, four bits at a time
    constexpr uint32_t t[16] = {0x00000000u, 0x1DB71064u, 0x3B6E20C8u, 0x26D930ACu, 0x76DC4190u, 0x6B6B51F4u, 0x4DB26158u, 0x5005713Cu,
                                0xEDB88320u, 0xF00F9344u, 0xD6D6A3E8u, 0xCB61B38Cu, 0x9B64C2B0u, 0x86D3D2D4u, 0xA00AE278u, 0xBDBDF21Cu};
    crc ^= byte;
    crc = (crc >> 4) ^ t[crc & 15u];
    crc = (crc >> 4) ^ t[crc & 15u];
    return crc;
}

VSE_HD uint32_t crc_bytes(uint32_t crc, const uint8_t *p, int n) {
    for (int i = 0; i < n; ++i) crc = crc_update(crc, p[i]);
    return crc;
}

// CRC-32 values are polynomials over GF(2) modulo the CRC polynomial, bit 31 the coefficient of x^0 (the reflected form).  crc_mul: their
// product; crc_x8n: x^(8 n); crc_combine: the CRC-32 of A followed by B from the (finished) CRC-32 of A, that of B and B's length --
// crc(A B) = crc(A) x^(8 |B|) + crc(B), the identity zlib's crc32_combine rests on.  The kernels sum a chunk's CRC stretch by stretch with it.
VSE_HD uint32_t crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}

VSE_HD uint32_t crc_x8n(uint32_t n) {
    uint32_t p = 1u << 31, sq = 1u << 23;      // 1 and x^8
    for (; n; n >>= 1) {
        if (n & 1u) p = crc_mul(sq, p);
        sq = crc_mul(sq, sq);
    }
    return p;
}

VSE_HD uint32_t crc_combine(uint32_t crc_a, uint32_t crc_b, uint32_t len_b) { return crc_mul(crc_x8n(len_b), crc_a) ^ crc_b; }

// The Adler sums of `len` bytes started from (0, 0): sa = sum d[i], sb = sum (len - i) d[i], both modulo 65521.
VSE_HD void adler_sums(const uint8_t *p, int len, uint32_t &sa, uint32_t &sb) {
    uint32_t a = 0, b = 0;
    int i = 0;
    while (i < len) {
        const int end = len - i > 5000 ? i + 5000 : len;      // 5000 * 255 * 5001 / 2 + 65520 * 5001 < 2^32
        for (; i < end; ++i) {
            a += p[i];
            b += a;
        }
        a %= kAdlerMod;
        b %= kAdlerMod;
    }
    sa = a, sb = b;
}

// (A, B) of a stream extended by a piece of `len` bytes whose sums are (sa, sb)
VSE_HD void adler_append(uint32_t &A, uint32_t &B, uint32_t sa, uint32_t sb, int len) {
    B = (uint32_t)((B + (uint64_t)len * A + sb) % kAdlerMod);
    A = (A + sa) % kAdlerMod;
}

VSE_HD void put_be32(uint8_t *p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v;
}

// The 33 bytes every file starts with (signature and IHDR) and the 12 it ends with (IEND).
constexpr int kPrefixBytes = 33, kIendBytes = 12;

VSE_HD void file_prefix(const Shape &s, uint8_t (&p)[kPrefixBytes]) {
    constexpr uint8_t sig[8] = {0x89, 0x50, 0x4E, 0x47, 0x0D, 0x0A, 0x1A, 0x0A};
    for (int i = 0; i < 8; ++i) p[i] = sig[i];
    put_be32(p + 8, 13);
    p[12] = 'I', p[13] = 'H', p[14] = 'D', p[15] = 'R';
    put_be32(p + 16, (uint32_t)s.w);
    put_be32(p + 20, (uint32_t)s.h);
    p[24] = 8;
    p[25] = s.c == 1 ? 0 : (s.c == 3 ? 2 : 6);
    p[26] = p[27] = p[28] = 0;
    put_be32(p + 29, ~crc_bytes(0xFFFFFFFFu, p + 12, 17));
}

VSE_HD uint8_t iend_byte(int i) {
    constexpr uint8_t iend[kIendBytes] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
    return iend[i];
}

// ---- the bit writer -----------------------------------------------------------------------------------------------------------------------
struct BitWriter {
    uint8_t *out;
    int pos;             // bytes written
    uint64_t acc;
    int n;               // bits waiting in acc, fewer than 8 between calls

    VSE_HD void put(uint32_t bits, int count) {      // count <= 32, least significant bit first
        acc |= (uint64_t)bits << n;
        n += count;
        while (n >= 8) {
            out[pos++] = (uint8_t)acc;
            acc >>= 8;
            n -= 8;
        }
    }
    VSE_HD void align() {
        if (n > 0) {
            out[pos++] = (uint8_t)acc;
            acc = 0, n = 0;
        }
    }
};

// ---- tokens -------------------------------------------------------------------------------------------------------------------------------
// Calls f.literal(byte) and f.match(length) for the tokens of the L bytes of a segment, in order.
template <class F>
VSE_HD void for_each_token(const uint8_t *seg, int L, F &f) {
    int i = 0;
    while (i < L) {
        const uint8_t v = seg[i];
        int j = i + 1;
        while (j < L && seg[j] == v) ++j;
        f.literal(v);
        int rest = j - i - 1;
        while (rest >= 258) {
            f.match(258);
            rest -= 258;
        }
        if (rest >= 3) {
            f.match(rest);
        } else {
            for (int k = 0; k < rest; ++k) f.literal(v);
        }
        i = j;
    }
}

// the length symbol (257 ..) of a match length 3 .. 258, its extra bits and their count
VSE_HD int length_symbol(int len, int &extra, int &nextra) {
    constexpr uint16_t base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    constexpr uint8_t bits[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    int k = 28;
    while (base[k] > len) --k;
    extra = len - base[k];
    nextra = bits[k];
    return 257 + k;
}

// ---- code lengths -------------------------------------------------------------------------------------------------------------------------
// Everything one segment's coding needs besides its bytes: in LDS on the device, one per workgroup.
struct Work {
    uint32_t freq[kLitLen];          // literal/length frequencies
    uint32_t weight[kLitLen];        // the merged nodes of the tree under construction
    uint16_t order[kLitLen];         // used symbols by (frequency, symbol)
    uint16_t parent[2 * kLitLen];
    uint8_t depth[2 * kLitLen];
    uint8_t len[kLitLen + 1];        // literal/length lengths, then the distance length: the code-length sequence reads them as one
    uint16_t code[kLitLen];          // the codes, bit-reversed: ready for the writer
    uint16_t seq[kLitLen + 1];       // the code-length sequence: symbol | (extra << 8)
    uint32_t cfreq[kClen];
    uint8_t clen[kClen];
    uint16_t ccode[kClen];
};

// The used symbols (frequency > 0) of `nsym` in ascending order of (frequency, symbol) into w.order; returns their number.  (The kernel sorts
// the literal/length alphabet with all its lanes instead: the keys are distinct, so the order is the same.)
VSE_HD int sort_symbols(const uint32_t *freq, int nsym, Work &w) {
    int used = 0;
    for (int s = 0; s < nsym; ++s) {
        if (freq[s] == 0) continue;
        int k = used++;      // insertion; the symbols arrive in ascending order, so equal frequencies keep it
        while (k > 0 && freq[w.order[k - 1]] > freq[s]) {
            w.order[k] = w.order[k - 1];
            --k;
        }
        w.order[k] = (uint16_t)s;
    }
    return used;
}

// The lengths of `nsym` symbols from their frequencies under the limit `limit` (include/vicasplat_png.h, DYNAMIC CODES 2. to 4.), the `used`
// symbols of step 1. being in w.order.
VSE_HD void code_lengths_sorted(const uint32_t *freq, int nsym, int used, int limit, uint8_t *len, Work &w) {
    for (int s = 0; s < nsym; ++s) len[s] = 0;
    if (used == 0) return;
    if (used == 1) {
        len[w.order[0]] = 1;
        return;
    }
    // nodes 0 .. used - 1 are the leaves in order, used .. 2 used - 2 the merged nodes in the order of their making
    int leaf = 0, node = 0, made = 0;
    while (made < used - 1) {
        uint32_t sum = 0;
        for (int pick = 0; pick < 2; ++pick) {
            const bool take_leaf = leaf < used && (node >= made || freq[w.order[leaf]] <= w.weight[node]);
            if (take_leaf) {
                sum += freq[w.order[leaf]];
                w.parent[leaf++] = (uint16_t)(used + made);
            } else {
                sum += w.weight[node];
                w.parent[used + node++] = (uint16_t)(used + made);
            }
        }
        w.weight[made++] = sum;
    }
    uint32_t n[32];
    for (int d = 0; d < 32; ++d) n[d] = 0;
    const int root = 2 * used - 2;
    w.depth[root] = 0;
    for (int i = root - 1; i >= 0; --i) {
        int d = w.depth[w.parent[i]] + 1;
        if (d > 31) d = 31;      // (past the limit anyway: step 3 folds it)
        w.depth[i] = (uint8_t)d;
        if (i < used) n[d] += 1;
    }
    for (int d = limit + 1; d < 32; ++d) n[limit] += n[d];
    uint32_t kraft = 0;
    for (int d = 1; d <= limit; ++d) kraft += n[d] << (limit - d);
    while (kraft > (1u << limit)) {
        n[limit] -= 1;
        for (int d = limit - 1; d >= 1; --d) {
            if (n[d]) {
                n[d] -= 1;
                n[d + 1] += 2;
                break;
            }
        }
        kraft -= 1;
    }
    int at = 0;
    for (int d = limit; d >= 1; --d)
        for (uint32_t k = 0; k < n[d]; ++k) len[w.order[at++]] = (uint8_t)d;
}

VSE_HD void code_lengths(const uint32_t *freq, int nsym, int limit, uint8_t *len, Work &w) {
    code_lengths_sorted(freq, nsym, sort_symbols(freq, nsym, w), limit, len, w);
}

// the canonical codes of RFC 1951 3.2.2, each reversed over its length
VSE_HD void canonical_codes(const uint8_t *len, int nsym, uint16_t *code) {
    uint32_t count[16], next[16];
    for (int d = 0; d < 16; ++d) count[d] = 0;
    for (int s = 0; s < nsym; ++s) count[len[s]] += 1;
    count[0] = 0;
    uint32_t c = 0;
    next[0] = 0;
    for (int d = 1; d < 16; ++d) {
        c = (c + count[d - 1]) << 1;
        next[d] = c;
    }
    for (int s = 0; s < nsym; ++s) {
        const int l = len[s];
        uint32_t v = l ? next[l]++ : 0, r = 0;
        for (int k = 0; k < l; ++k) r |= ((v >> k) & 1u) << (l - 1 - k);
        code[s] = (uint16_t)r;
    }
}

VSE_HD void fixed_lengths(uint8_t *len) {
    for (int s = 0; s < kLitLen; ++s) len[s] = s < 144 ? 8 : (s < 256 ? 9 : (s < 280 ? 7 : 8));
}

struct CountTokens {
    uint32_t *freq;
    uint32_t matches, extra_bits;
    VSE_HD void literal(uint8_t v) { freq[v] += 1; }
    VSE_HD void match(int l) {
        int e, ne;
        freq[length_symbol(l, e, ne)] += 1;
        matches += 1;
        extra_bits += (uint32_t)ne;
    }
};

struct EmitTokens {
    BitWriter *bw;
    const uint16_t *code;
    const uint8_t *len;
    uint32_t dist_code;
    int dist_len;
    VSE_HD void literal(uint8_t v) { bw->put(code[v], len[v]); }
    VSE_HD void match(int l) {
        int e, ne;
        const int s = length_symbol(l, e, ne);
        bw->put(code[s], len[s]);
        if (ne) bw->put((uint32_t)e, ne);
        bw->put(dist_code, dist_len);
    }
};

// The code-length sequence of the `count` lengths in len[] (the literal/length lengths and the distance length behind them) into w.seq and
// w.cfreq; returns its number of entries.
VSE_HD int code_length_sequence(const uint8_t *len, int count, Work &w) {
    for (int s = 0; s < kClen; ++s) w.cfreq[s] = 0;
    int m = 0, i = 0;
    while (i < count) {
        const int v = len[i];
        int j = i + 1;
        while (j < count && len[j] == v) ++j;
        int r = j - i;
        i = j;
        if (v == 0) {
            while (r >= 138) {
                w.seq[m++] = (uint16_t)(18 | ((138 - 11) << 8));
                w.cfreq[18] += 1;
                r -= 138;
            }
            if (r >= 11) {
                w.seq[m++] = (uint16_t)(18 | ((r - 11) << 8));
                w.cfreq[18] += 1;
            } else if (r >= 3) {
                w.seq[m++] = (uint16_t)(17 | ((r - 3) << 8));
                w.cfreq[17] += 1;
            } else {
                for (int k = 0; k < r; ++k) w.seq[m++] = 0;
                w.cfreq[0] += (uint32_t)r;
            }
        } else {
            w.seq[m++] = (uint16_t)v;
            w.cfreq[v] += 1;
            r -= 1;
            while (r >= 6) {
                w.seq[m++] = (uint16_t)(16 | (3 << 8));
                w.cfreq[16] += 1;
                r -= 6;
            }
            if (r >= 3) {
                w.seq[m++] = (uint16_t)(16 | ((r - 3) << 8));
                w.cfreq[16] += 1;
            } else {
                for (int k = 0; k < r; ++k) w.seq[m++] = (uint16_t)v;
                w.cfreq[v] += (uint32_t)r;
            }
        }
    }
    return m;
}

// ---- one segment --------------------------------------------------------------------------------------------------------------------------
enum Form { kStored = 0, kFixed = 1, kDynamic = 2 };

// The first step of a segment's coding: the token frequencies into w.freq.
VSE_HD CountTokens count_segment(const uint8_t *seg, int L, Work &w) {
    for (int s = 0; s < kLitLen; ++s) w.freq[s] = 0;
    CountTokens ct{w.freq, 0, 0};
    for_each_token(seg, L, ct);
    w.freq[256] = 1;
    return ct;
}

// The rest: the deflate data of the L bytes (1 .. 65535) of one segment into `out` (L + 10 bytes at most) -- its block in the smallest form,
// then the empty stored block unless the segment is the file's last -- from count_segment's result and the `used` literal/length symbols
// sorted into w.order (sort_symbols).  Returns the number of bytes; *form_out, when given, the form it took.
VSE_HD int finish_segment(const uint8_t *seg, int L, bool last, uint8_t *out, Work &w, const CountTokens &ct, int used, int *form_out = nullptr) {
    constexpr uint8_t clen_order[kClen] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

    // the fixed form's bits
    uint64_t fixed_bits = 3 + (uint64_t)ct.extra_bits + 5ull * ct.matches;
    for (int s = 0; s < 286; ++s) fixed_bits += (uint64_t)w.freq[s] * (s < 144 ? 8 : (s < 256 ? 9 : (s < 280 ? 7 : 8)));

    // the dynamic form's codes and bits
    code_lengths_sorted(w.freq, 286, used, 15, w.len, w);
    int nlit = 286;
    while (w.len[nlit - 1] == 0) --nlit;      // symbol 256 is used: nlit >= 257
    w.len[nlit] = ct.matches ? 1 : 0;         // the one distance code
    const int m = code_length_sequence(w.len, nlit + 1, w);
    code_lengths(w.cfreq, kClen, 7, w.clen, w);
    int nclen = kClen;
    while (nclen > 4 && w.clen[clen_order[nclen - 1]] == 0) --nclen;
    uint64_t dyn_bits = 3 + 14 + 3ull * nclen + (uint64_t)ct.extra_bits + (uint64_t)ct.matches;
    for (int s = 0; s < kClen; ++s) dyn_bits += (uint64_t)w.cfreq[s] * w.clen[s];
    dyn_bits += 2ull * w.cfreq[16] + 3ull * w.cfreq[17] + 7ull * w.cfreq[18];
    for (int s = 0; s < nlit; ++s) dyn_bits += (uint64_t)w.freq[s] * w.len[s];
    const uint64_t stored_bits = 40 + 8ull * (uint64_t)L;

    const Form form = (stored_bits <= fixed_bits && stored_bits <= dyn_bits) ? kStored : (fixed_bits <= dyn_bits ? kFixed : kDynamic);
    if (form_out) *form_out = (int)form;
    BitWriter bw{out, 0, 0, 0};
    bw.put((last ? 1u : 0u) | ((uint32_t)form << 1), 3);
    if (form == kStored) {
        bw.align();
        bw.put((uint32_t)L, 16);
        bw.put((uint32_t)L ^ 0xFFFFu, 16);
        for (int i = 0; i < L; ++i) out[bw.pos + i] = seg[i];
        bw.pos += L;
    } else {
        uint32_t dist_code = 0;
        int dist_len = 5;
        if (form == kFixed) {
            fixed_lengths(w.len);
            canonical_codes(w.len, kLitLen, w.code);
        } else {
            canonical_codes(w.clen, kClen, w.ccode);
            bw.put((uint32_t)(nlit - 257), 5);
            bw.put(0, 5);
            bw.put((uint32_t)(nclen - 4), 4);
            for (int k = 0; k < nclen; ++k) bw.put(w.clen[clen_order[k]], 3);
            for (int k = 0; k < m; ++k) {
                const int s = w.seq[k] & 255, e = w.seq[k] >> 8;
                bw.put(w.ccode[s], w.clen[s]);
                if (s >= 16) bw.put((uint32_t)e, s == 16 ? 2 : (s == 17 ? 3 : 7));
            }
            canonical_codes(w.len, nlit, w.code);
            dist_len = 1;
        }
        EmitTokens et{&bw, w.code, w.len, dist_code, dist_len};
        for_each_token(seg, L, et);
        bw.put(w.code[256], w.len[256]);
    }
    if (last) {
        bw.align();
    } else {
        bw.put(0, 3);
        bw.align();
        bw.put(0xFFFF0000u, 32);
    }
    return bw.pos;
}

VSE_HD int encode_segment(const uint8_t *seg, int L, bool last, uint8_t *out, Work &w, int *form_out = nullptr) {
    const CountTokens ct = count_segment(seg, L, w);
    return finish_segment(seg, L, last, out, w, ct, sort_symbols(w.freq, 286, w), form_out);
}

}  // namespace vse
