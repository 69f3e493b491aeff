// The baseline JPEG decoder's serial parts, for the device and for the host: descriptor checks, the bit reader, the Huffman decode of one
// restart segment and the islow inverse DCT.  csrc/jpeg.hip builds its kernels from these functions; tests/jpeg_probe.cpp compiles the same
// text with the host compiler under the address and undefined-behaviour sanitizers.  include/vicasplat_jpeg.h states the formats, the
// arithmetic and the status bits; nothing here depends on HIP.
#pragma once
#include <cstdint>
#include <cstring>

#include "../../include/vicasplat_jpeg.h"

#if defined(__HIPCC__)
#define VSJ_HD __host__ __device__ __forceinline__
#define VSJ_UNROLL _Pragma("unroll")
#else
#define VSJ_HD inline
#define VSJ_UNROLL
#endif

namespace vsj {

// One frame's geometry, derived from its descriptor words and checked against the call's sizes (frame_geometry).
struct Geom {
    int ncomp, hs, vs;             // components; luma sampling factors (chroma is 1 x 1)
    int mcus_x, mcus_y;            // MCUs per row and per column
    int seg0, nseg;                // the frame's restart segments in the segment table
    int64_t block0;                // the frame's first 8 x 8 block in the workspace
    int bw[3], bh[3];              // blocks per row / column of each component's padded plane
    int base[4];                   // first block of each component inside the frame; base[ncomp ..] = blocks of the frame
    int qt[3], dc[3], ac[3];       // table indices per component
};

VSJ_HD int cdiv(int a, int b) { return (a + b - 1) / b; }

// The geometry of the frame whose descriptor is `d` (VSJ_FRAME_WORDS words), or false when the descriptor does not belong to the call's
// sizes: every index a kernel derives from a Geom that passed lies inside the buffers of the call.
VSJ_HD bool frame_geometry(const int32_t *d, int h, int w, int segments, int64_t blocks, int n_quant, int n_huff, Geom &g) {
    g.ncomp = d[VSJ_F_NCOMP];
    g.hs = d[VSJ_F_HS];
    g.vs = d[VSJ_F_VS];
    if (!(g.ncomp == 1 || g.ncomp == 3) || !(g.hs == 1 || g.hs == 2) || !(g.vs == 1 || g.vs == 2)) return false;
    if ((g.vs == 2 && g.hs != 2) || (g.ncomp == 1 && g.hs != 1)) return false;
    g.mcus_x = d[VSJ_F_MCUS_X];
    g.mcus_y = d[VSJ_F_MCUS_Y];
    if (g.mcus_x != cdiv(w, 8 * g.hs) || g.mcus_y != cdiv(h, 8 * g.vs)) return false;
    g.seg0 = d[VSJ_F_SEG0];
    g.nseg = d[VSJ_F_NSEG];
    if (g.seg0 < 0 || g.nseg < 0 || (int64_t)g.seg0 + g.nseg > segments) return false;
    const int64_t mcus = (int64_t)g.mcus_x * g.mcus_y;
    int64_t at = 0;
    for (int c = 0; c < 3; ++c) {
        const bool live = c < g.ncomp;
        g.bw[c] = live ? g.mcus_x * (c == 0 ? g.hs : 1) : 0;
        g.bh[c] = live ? g.mcus_y * (c == 0 ? g.vs : 1) : 0;
        if (at > INT32_MAX) return false;
        g.base[c] = (int)at;
        if (live) at += mcus * (c == 0 ? g.hs * g.vs : 1);
        g.qt[c] = d[VSJ_F_QUANT + c];
        g.dc[c] = d[VSJ_F_DC + c];
        g.ac[c] = d[VSJ_F_AC + c];
        if (live && (g.qt[c] < 0 || g.qt[c] >= n_quant || g.dc[c] < 0 || g.dc[c] >= n_huff || g.ac[c] < 0 || g.ac[c] >= n_huff)) return false;
    }
    if (at > INT32_MAX) return false;
    g.base[3] = (int)at;
    g.block0 = d[VSJ_F_BLOCK0];
    return g.block0 >= 0 && g.block0 + at <= blocks;
}

// ---- the bit reader: bytes [pos, end) of `data`, stuffing removed, zeros past the end -----------------------------------------------------
struct BitReader {
    const uint8_t *data;
    int pos, end;
    uint64_t acc;      // the next bits, from bit 63 down
    int nbits;         // valid bits in acc
    int pad;           // zero bytes made up: past the end, or from an FF that no 00 follows
    int err;           // VSJ_STATUS_* bits
    uint32_t w[4];     // the bytes [pos, pos + 4 have) read ahead, w[0] first (only ever indexed by constants: registers on the device)
    int have;
};

VSJ_HD void reader_init(BitReader &br, const uint8_t *data, int begin, int end) {
    br.data = data;
    br.pos = begin;
    br.end = end > begin ? end : begin;
    br.acc = 0;
    br.nbits = 0;
    br.pad = 0;
    br.err = 0;
    br.have = 0;
    br.w[0] = br.w[1] = br.w[2] = br.w[3] = 0;
}

VSJ_HD uint32_t bswap32(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24); }

// one byte of the range behind the accumulator (nbits <= 56), the 00 after an FF dropped; a zero once the range or its data has ended
VSJ_HD void append_byte(BitReader &br) {
    uint32_t b = 0;
    if (br.pos < br.end && !(br.err & VSJ_STATUS_MARKER)) {
        b = br.data[br.pos++];
        if (b == 0xFF) {
            if (br.pos < br.end && br.data[br.pos] == 0) {
                ++br.pos;
            } else {      // a marker, or the range ends inside the pair: nothing after it is entropy-coded data
                br.err |= VSJ_STATUS_MARKER;
                b = 0;
                ++br.pad;
            }
        }
    } else {
        ++br.pad;
    }
    br.acc |= (uint64_t)b << (56 - br.nbits);
    br.nbits += 8;
}

// At least 33 valid bits afterwards: a code (<= 16 bits) and its value bits (<= 15) need no second call.  Sixteen bytes are read at a
// time while the range has them, and go into the accumulator four at a time; four bytes with an FF among them, and the range's last
// fifteen, go one by one.
VSJ_HD void refill(BitReader &br) {
    while (br.nbits <= 32) {
        if (br.have == 0 && br.pos + 16 <= br.end) {
            memcpy(br.w, br.data + br.pos, 16);
            br.have = 4;
        }
        if (br.have > 0) {
            const uint32_t v = br.w[0];
            if ((((~v) - 0x01010101u) & v & 0x80808080u) == 0) {      // none of the four bytes is FF
                br.acc |= (uint64_t)bswap32(v) << (32 - br.nbits);
                br.nbits += 32;
                br.pos += 4;
                br.w[0] = br.w[1];
                br.w[1] = br.w[2];
                br.w[2] = br.w[3];
                --br.have;
                continue;
            }
            br.have = 0;
        }
        while (br.nbits <= 56) append_byte(br);
    }
}

VSJ_HD void consume(BitReader &br, int n) {
    br.acc <<= n;
    br.nbits -= n;
}

// One symbol of the table at `tab` (VSJ_HUFF_BYTES bytes, the layout of include/vicasplat_jpeg.h), or -1 with VSJ_STATUS_CODE set.
VSJ_HD int decode_symbol(BitReader &br, const uint8_t *tab) {
    refill(br);
    const uint32_t top = (uint32_t)(br.acc >> 48);
    const uint32_t e = ((const uint16_t *)tab)[top >> (16 - VSJ_LOOK_BITS)];
    if (e) {
        consume(br, (int)(e >> 8));
        return (int)(e & 255u);
    }
    const int32_t *maxcode = (const int32_t *)(tab + VSJ_HUFF_MAXCODE);
    const int32_t *valoff = (const int32_t *)(tab + VSJ_HUFF_VALOFF);
    for (int l = VSJ_LOOK_BITS + 1; l <= 16; ++l) {
        const int code = (int)(top >> (16 - l));
        if (code <= maxcode[l]) {
            consume(br, l);
            return tab[VSJ_HUFF_VALS + ((code + valoff[l]) & 255)];
        }
    }
    br.err |= VSJ_STATUS_CODE;
    return -1;
}

// the s value bits that follow a symbol, sign-extended as the standard's EXTEND does; s in [0, 15]
VSJ_HD int receive_extend(BitReader &br, int s) {
    if (s == 0) return 0;
    const int v = (int)(br.acc >> (64 - s));
    consume(br, s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

VSJ_HD int zigzag_to_natural(int k) {
    constexpr uint8_t zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return zz[k & 63];
}

// One 8 x 8 block into `coef` (64 int16 in natural order, zero on entry).  false: the block is damaged (br.err says how).
VSJ_HD bool decode_block(BitReader &br, const uint8_t *dc_tab, const uint8_t *ac_tab, const uint8_t *zz, int &pred, int16_t *coef) {
    const int s = decode_symbol(br, dc_tab);
    if (s < 0) return false;
    pred = (int16_t)(uint16_t)(pred + receive_extend(br, s & 15));
    coef[0] = (int16_t)pred;
    int k = 1;
    while (k < 64) {
        const int rs = decode_symbol(br, ac_tab);
        if (rs < 0) return false;
        const int r = rs >> 4, size = rs & 15;
        if (size == 0) {
            if (r != 15) break;      // end of block
            k += 16;
            continue;
        }
        k += r;
        if (k > 63) {
            br.err |= VSJ_STATUS_INDEX;
            return false;
        }
        coef[zz[k]] = (int16_t)receive_extend(br, size);
        ++k;
    }
    if (k > 64) {      // a run of sixteen zeros that passes the block's end
        br.err |= VSJ_STATUS_INDEX;
        return false;
    }
    return true;
}

// One restart segment: the MCUs [first_mcu, first_mcu + n_mcu) of the frame, from the bytes [begin, end) of `bytes`, into the frame's
// coefficient blocks at `coef` (g.base[ncomp] blocks of 64, zero on entry).  tabs: six tables of VSJ_HUFF_BYTES bytes, the DC table of
// component c at index c and its AC table at 3 + c (one array, so that the device keeps it in LDS); zz: zigzag_to_natural of 0 .. 63.
// The caller has checked 0 <= first_mcu, 0 <= n_mcu, first_mcu + n_mcu <= mcus_x * mcus_y and 0 <= begin <= end <= the length of `bytes`.
// Returns the VSJ_STATUS_* bits of the segment; decoding stops at the first damaged block, the rest of the segment stays zero.
VSJ_HD int decode_segment(const Geom &g, const uint8_t *bytes, int begin, int end, int first_mcu, int n_mcu, const uint8_t *tabs,
                          const uint8_t *zz, int16_t *coef) {
    BitReader br;
    reader_init(br, bytes, begin, end);
    // (no array of the geometry is indexed by a variable here: everything stays in registers on the device)
    const int hs = g.hs, vs = g.vs, mcus_x = g.mcus_x, bw0 = g.bw[0], base1 = g.base[1], base2 = g.base[2];
    const bool colour = g.ncomp == 3;
    const uint8_t *dc1 = tabs + VSJ_HUFF_BYTES, *dc2 = tabs + 2 * VSJ_HUFF_BYTES, *ac0 = tabs + 3 * VSJ_HUFF_BYTES;
    const uint8_t *ac1 = tabs + 4 * VSJ_HUFF_BYTES, *ac2 = tabs + 5 * VSJ_HUFF_BYTES;
    int pred0 = 0, pred1 = 0, pred2 = 0;
    bool ok = true;
    int mx = first_mcu % mcus_x, my = first_mcu / mcus_x;
    for (int m = 0; m < n_mcu && ok; ++m) {
        for (int v = 0; v < vs && ok; ++v)
            for (int u = 0; u < hs && ok; ++u)
                ok = decode_block(br, tabs, ac0, zz, pred0, coef + ((int64_t)(my * vs + v) * bw0 + (mx * hs + u)) * 64);
        if (colour && ok) {
            const int64_t at = (int64_t)my * mcus_x + mx;
            ok = decode_block(br, dc1, ac1, zz, pred1, coef + (base1 + at) * 64);
            if (ok) ok = decode_block(br, dc2, ac2, zz, pred2, coef + (base2 + at) * 64);
        }
        if (++mx == mcus_x) {
            mx = 0;
            ++my;
        }
    }
    if (ok) {
        const int left = br.nbits - 8 * br.pad;      // true bits read and not used
        if (left < 0)
            br.err |= VSJ_STATUS_SHORT;
        else if (br.pos < br.end || left >= 8)
            br.err |= VSJ_STATUS_LEFTOVER;
    }
    return br.err;
}

// ---- libjpeg's "islow" inverse DCT ---------------------------------------------------------------------------------------------------------
VSJ_HD int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one 8-point pass: in[0..7] -> out[0..7], descaled by n bits
VSJ_HD void idct_1d(const int (&c)[8], int (&o)[8], int n) {
    int z1 = (c[2] + c[6]) * 4433;
    const int tmp2 = z1 - c[6] * 15137, tmp3 = z1 + c[2] * 6270;
    const int tmp0 = (int)((uint32_t)(c[0] + c[4]) << 13), tmp1 = (int)((uint32_t)(c[0] - c[4]) << 13);
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    int t0 = c[7], t1 = c[5], t2 = c[3], t3 = c[1];
    z1 = t0 + t3;
    int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const int z5 = (z3 + z4) * 9633;
    t0 *= 2446;
    t1 *= 16819;
    t2 *= 25172;
    t3 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    t0 += z1 + z3;
    t1 += z2 + z4;
    t2 += z2 + z3;
    t3 += z1 + z4;
    o[0] = descale(tmp10 + t3, n);
    o[7] = descale(tmp10 - t3, n);
    o[1] = descale(tmp11 + t2, n);
    o[6] = descale(tmp11 - t2, n);
    o[2] = descale(tmp12 + t1, n);
    o[5] = descale(tmp12 - t1, n);
    o[3] = descale(tmp13 + t0, n);
    o[4] = descale(tmp13 - t0, n);
}

// coef: 64 int16 in natural order, 16-byte aligned; q: 64 quantisation values in natural order; out: the 8 x 8 samples, row r in
// out[2 r] (columns 0..3, column 0 in the low byte) and out[2 r + 1] (columns 4..7).  A sample outside [0, 255] is clamped.
// The sums are int32, which every block of a stream an encoder wrote fits; a damaged block's samples are unspecified.
VSJ_HD void idct_islow(const int16_t *coef, const uint16_t *q, uint32_t (&out)[16]) {
    int ws[64];
VSJ_UNROLL
    for (int x = 0; x < 8; ++x) {
        int c[8], o[8];
VSJ_UNROLL
        for (int y = 0; y < 8; ++y) c[y] = (int)coef[8 * y + x] * (int)q[8 * y + x];
        idct_1d(c, o, 11);
VSJ_UNROLL
        for (int y = 0; y < 8; ++y) ws[8 * y + x] = o[y];
    }
VSJ_UNROLL
    for (int y = 0; y < 8; ++y) {
        int c[8], o[8];
VSJ_UNROLL
        for (int x = 0; x < 8; ++x) c[x] = ws[8 * y + x];
        idct_1d(c, o, 18);
        uint32_t lo = 0, hi = 0;
VSJ_UNROLL
        for (int x = 0; x < 4; ++x) {
            const int a = o[x] + 128, b = o[x + 4] + 128;
            lo |= (uint32_t)(a < 0 ? 0 : (a > 255 ? 255 : a)) << (8 * x);
            hi |= (uint32_t)(b < 0 ? 0 : (b > 255 ? 255 : b)) << (8 * x);
        }
        out[2 * y] = lo;
        out[2 * y + 1] = hi;
    }
}

}  // namespace vsj
