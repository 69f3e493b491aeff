// A host program around vicasplat_amd/csrc/jpeg_decode.h: the entropy decoder and the inverse DCT of the JPEG kernels, compiled with the
// host compiler under -fsanitize=address,undefined by tests/test_jpeg_cpu.py and run on the CPU only.
//
// stdin, binary, any number of jobs: eight int32 (h, w, segments, n_quant, n_huff, blocks, packed_bytes, nbytes: the compressed bytes
// without the buffer's padding), then the packed buffer of a one-frame call as include/vicasplat_jpeg.h lays it out.  Every section is
// copied into a heap block of exactly its own size, so that a read or write one byte outside it is reported.  stdout per job: int32 status (the OR of the segments' words, VSJ_STATUS_DESC for a
// descriptor that does not belong), then blocks * 64 int16 coefficients, then -- status 0 only -- blocks * 64 samples of the inverse DCT.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../vicasplat_amd/csrc/jpeg_decode.h"

static bool read_exact(void *dst, size_t n) { return n == 0 || fread(dst, 1, n, stdin) == n; }

template <class T>
static T *exact_copy(const uint8_t *src, size_t count) {
    T *p = (T *)malloc(count * sizeof(T) + (count == 0));
    if (count) memcpy(p, src, count * sizeof(T));
    return p;
}

int main() {
    int32_t head[8];
    while (read_exact(head, sizeof head)) {
        const int h = head[0], w = head[1], segments = head[2], n_quant = head[3], n_huff = head[4], blocks = head[5], packed_bytes = head[6];
        std::vector<uint8_t> packed((size_t)packed_bytes);
        if (!read_exact(packed.data(), packed.size())) return 2;
        const size_t at_segs = (size_t)VSJ_FRAME_WORDS * 4, at_quant = at_segs + (size_t)segments * VSJ_SEG_WORDS * 4;
        const size_t at_huff = at_quant + (size_t)n_quant * 128, at_bytes = at_huff + (size_t)n_huff * VSJ_HUFF_BYTES;
        if (at_bytes > packed.size()) return 3;
        const int nbytes = head[7];
        if (nbytes < 0 || at_bytes + (size_t)nbytes > packed.size()) return 4;
        int32_t *frame = exact_copy<int32_t>(packed.data(), VSJ_FRAME_WORDS);
        int32_t *segs = exact_copy<int32_t>(packed.data() + at_segs, (size_t)segments * VSJ_SEG_WORDS);
        uint16_t *quant = exact_copy<uint16_t>(packed.data() + at_quant, (size_t)n_quant * 64);
        uint8_t *huff = exact_copy<uint8_t>(packed.data() + at_huff, (size_t)n_huff * VSJ_HUFF_BYTES);
        uint8_t *bytes = exact_copy<uint8_t>(packed.data() + at_bytes, (size_t)nbytes);
        int16_t *coef = (int16_t *)aligned_alloc(16, (size_t)blocks * 128 + 16 * (blocks == 0));
        memset(coef, 0, (size_t)blocks * 128);

        vsj::Geom g;
        int32_t status = 0;
        if (!vsj::frame_geometry(frame, h, w, segments, blocks, n_quant, n_huff, g)) {
            status = VSJ_STATUS_DESC;
        } else {
            std::vector<uint8_t> tabs(6 * VSJ_HUFF_BYTES);      // as the kernel stages them in LDS
            for (int c = 0; c < g.ncomp; ++c) {
                memcpy(tabs.data() + (size_t)c * VSJ_HUFF_BYTES, huff + (size_t)g.dc[c] * VSJ_HUFF_BYTES, VSJ_HUFF_BYTES);
                memcpy(tabs.data() + (size_t)(3 + c) * VSJ_HUFF_BYTES, huff + (size_t)g.ac[c] * VSJ_HUFF_BYTES, VSJ_HUFF_BYTES);
            }
            uint8_t zz[64];
            for (int k = 0; k < 64; ++k) zz[k] = (uint8_t)vsj::zigzag_to_natural(k);
            for (int s = 0; s < g.nseg; ++s) {
                const int32_t *seg = segs + (size_t)(g.seg0 + s) * VSJ_SEG_WORDS;
                const int begin = seg[0], end = seg[1], first = seg[2], count = seg[3];
                if (begin >= 0 && begin <= end && end <= nbytes && first >= 0 && count >= 0 && (int64_t)first + count <= (int64_t)g.mcus_x * g.mcus_y)
                    status |= vsj::decode_segment(g, bytes, begin, end, first, count, tabs.data(), zz, coef + (size_t)g.block0 * 64);
                else
                    status |= VSJ_STATUS_DESC;
            }
        }
        fwrite(&status, 4, 1, stdout);
        fwrite(coef, 128, (size_t)blocks, stdout);
        if (status == 0) {
            for (int j = 0; j < g.base[3]; ++j) {
                const int c = j < g.base[1] ? 0 : (j < g.base[2] ? 1 : 2);
                uint32_t px[16];
                vsj::idct_islow(coef + ((size_t)g.block0 + j) * 64, quant + (size_t)g.qt[c] * 64, px);
                fwrite(px, 4, 16, stdout);
            }
        }
        free(frame);
        free(segs);
        free(quant);
        free(huff);
        free(bytes);
        free(coef);
    }
    return 0;
}
