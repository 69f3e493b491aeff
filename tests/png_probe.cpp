// A host program around vicasplat_amd/csrc/png_deflate.h: the PNG encoder's serial code (filters, tokens, code construction, block decision,
// bit writer, checksums, file framing), compiled with the host compiler under -fsanitize=address,undefined by tests/test_png_cpu.py and run
// on the CPU only.  It walks an image the way the kernels of csrc/png.hip do: row by row, segment by segment, chunk by chunk.
//
// stdin, binary, any number of jobs: four int32 (h, w, c, filter mode), then the h * w * c pixel bytes (HWC).  Every buffer is a heap block
// of exactly the size the header promises, so that a read or write one byte outside it is reported.  stdout per job: int32 length (-1 for a
// refused shape), then the file's bytes.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../vicasplat_amd/csrc/png_deflate.h"

static bool read_exact(void *dst, size_t n) { return n == 0 || fread(dst, 1, n, stdin) == n; }

int main() {
    int32_t head[4];
    while (read_exact(head, sizeof head)) {
        const int h = head[0], w = head[1], c = head[2], mode = head[3];
        vse::Shape s;
        if (!vse::make_shape(h, w, c, s)) {
            const int32_t refused = -1;
            fwrite(&refused, 4, 1, stdout);
            continue;
        }
        const size_t nb = (size_t)w * c;
        uint8_t *px = (uint8_t *)malloc((size_t)h * nb);
        if (!read_exact(px, (size_t)h * nb)) return 2;

        // the filtered stream
        uint8_t *filt = (uint8_t *)malloc((size_t)h * s.rb);
        for (int y = 0; y < h; ++y) {
            auto at = [&](int yy, long j) { return (yy < 0 || j < 0) ? 0 : (int)px[(size_t)yy * nb + (size_t)j]; };
            int type = mode;
            if (mode == VSE_FILTER_ADAPTIVE) {
                uint32_t cost[5] = {0, 0, 0, 0, 0};
                for (long j = 0; j < (long)nb; ++j)
                    for (int t = 0; t < 5; ++t)
                        cost[t] += (uint32_t)vse::signed_cost(vse::filter_value(t, at(y, j), at(y, j - c), at(y - 1, j), j >= c ? at(y - 1, j - c) : 0));
                type = vse::best_filter(cost);
            }
            uint8_t *row = filt + (size_t)y * s.rb;
            row[0] = (uint8_t)type;
            for (long j = 0; j < (long)nb; ++j)
                row[1 + j] = vse::filter_value(type, at(y, j), at(y, j - c), at(y - 1, j), j >= c ? at(y - 1, j - c) : 0);
        }

        // the file, into a block of exactly the bound
        const int64_t bound = vse::file_bound(s);
        uint8_t *file = (uint8_t *)malloc((size_t)bound);
        uint8_t prefix[vse::kPrefixBytes];
        vse::file_prefix(s, prefix);
        memcpy(file, prefix, vse::kPrefixBytes);
        int64_t pos = vse::kPrefixBytes;
        uint32_t A = 1, B = 0;
        vse::Work *work = (vse::Work *)malloc(sizeof(vse::Work));
        for (int seg = 0; seg < s.S; ++seg) {
            const int L = vse::segment_rows(s, seg) * s.rb;
            const bool first = seg == 0, last = seg == s.S - 1;
            uint8_t *piece = (uint8_t *)malloc((size_t)L);          // the segment alone: the coder may not read past it
            memcpy(piece, filt + (size_t)seg * s.R * s.rb, (size_t)L);
            uint8_t *data = (uint8_t *)malloc((size_t)L + 10);
            const int len = vse::encode_segment(piece, L, last, data, *work);
            // its Adler sums in 64 stretches, as the kernel takes them
            uint32_t a = 0, b = 0;
            const int per = (L + 63) / 64;
            for (int k = 0; k < 64; ++k) {
                const int lo = k * per < L ? k * per : L, hi = lo + per < L ? lo + per : L;
                uint32_t sa, sb;
                vse::adler_sums(piece + lo, hi - lo, sa, sb);
                vse::adler_append(a, b, sa, sb, hi - lo);
            }
            vse::adler_append(A, B, a, b, L);
            uint8_t *chunk = file + pos;
            const int head_bytes = first ? 2 : 0, dlen = len + head_bytes + (last ? 4 : 0);
            vse::put_be32(chunk, (uint32_t)dlen);
            memcpy(chunk + 4, "IDAT", 4);
            if (first) chunk[8] = 0x78, chunk[9] = 0x01;
            memcpy(chunk + 8 + head_bytes, data, (size_t)len);
            if (last) vse::put_be32(chunk + 8 + head_bytes + len, (B << 16) | A);
            // the chunk's CRC-32 as the kernels take it: type and zlib header, then the data in 64 stretches combined in order, then the Adler-32
            uint32_t crc = ~vse::crc_bytes(0xFFFFFFFFu, chunk + 4, 4 + head_bytes);
            const int cper = (len + 63) / 64;
            for (int k = 0; k < 64; ++k) {
                const int lo = k * cper < len ? k * cper : len, hi = lo + cper < len ? lo + cper : len;
                crc = vse::crc_combine(crc, ~vse::crc_bytes(0xFFFFFFFFu, data + lo, hi - lo), (uint32_t)(hi - lo));
            }
            if (last) crc = ~vse::crc_bytes(~crc, chunk + 8 + head_bytes + len, 4);
            vse::put_be32(chunk + 8 + dlen, crc);
            pos += 12 + dlen;
            free(piece);
            free(data);
        }
        for (int k = 0; k < vse::kIendBytes; ++k) file[pos++] = vse::iend_byte(k);
        const int32_t length = (int32_t)pos;
        fwrite(&length, 4, 1, stdout);
        fwrite(file, 1, (size_t)pos, stdout);
        free(work);
        free(file);
        free(filt);
        free(px);
    }
    return 0;
}
