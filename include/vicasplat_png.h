/* vicasplat_png.h -- the PNG entries of libvicasplat_hip.so (csrc/png.hip, csrc/png_deflate.h): an encoder that turns device images into
 * complete PNG files on the device, so that the compressed file crosses to the host and not the raw frame.
 *
 * A header of the same library beside the others: their entries and the ABI version are unchanged by it.  Its entries carry the prefix
 * vse_; they report errors as the entries of vicasplat_hip.h do (a negative return and a message behind the library's error call, before
 * any HIP call) and take the same stream type last.
 *
 * An encoder chooses its own stream.  This one is cut so that rows, segments and files are independent pieces of work, and it is stated
 * here completely: tests/png_ref.py restates it from this comment and the kernels' files equal the restatement's byte for byte.
 *
 * IMAGE      8 bits, C = 1, 3 or 4 channels (PNG colour types 0, 2, 6), H x W.  A row takes rb = 1 + W C bytes.  rb > 65535, H > 65535 and
 *            a batch whose n * vse_png_bound reaches 2^31 are refused.
 * FLOAT      an f32 sample x becomes uint8(trunc(min(max(x, 0), 1) * 255)), the product in f32; -0 gives 0, +inf 255, -inf 0 and a NaN
 *            BECOMES 0 (the reference's cast of a NaN is undefined).
 * FILE       the 8 signature bytes 89 50 4E 47 0D 0A 1A 0A; IHDR (width, height big-endian, depth 8, colour type, compression 0,
 *            filter method 0, no interlace); one IDAT chunk per segment, in order; IEND.  A chunk is its data's length (4 bytes, big-endian),
 *            its type, its data and the CRC-32 (polynomial EDB88320, reflected, initial value and final xor FFFFFFFF, big-endian) of type
 *            and data.  The first IDAT's data begins with the zlib header 78 01; the last IDAT's data ends with the big-endian Adler-32 of
 *            the whole filtered stream.
 * FILTERED   every row is a filter-type byte and W C filtered bytes, modulo 256, with a = the byte C positions to the left (0 in the
 *  STREAM    first pixel), b = the byte above (0 in row 0) and c = the byte above a:  0 x;  1 x - a;  2 x - b;  3 x - floor((a + b) / 2);
 *            4 x - paeth, where p = a + b - c, pa = |p - a|, pb = |p - b|, pc = |p - c| and paeth = a if pa <= pb and pa <= pc, else b if
 *            pb <= pc, else c.  filter_mode 0..4 uses that type on every row; VSE_FILTER_ADAPTIVE takes per row the type whose filtered
 *            bytes, read as signed (v < 128 ? v : 256 - v), have the smallest sum, the lowest type on a tie.
 * SEGMENTS   R = clamp(floor(16384 / rb), 1, H) consecutive rows each (the last one may be shorter), S = ceil(H / R) of them.  A segment
 *            has L <= max(16384, rb) <= 65535 bytes, and its deflate data starts and ends on a byte boundary of the zlib stream.
 * TOKENS     the segment's bytes are cut into maximal runs of equal bytes (a run never leaves the segment).  A run of n bytes is one
 *            literal, then its n - 1 repeats as matches of distance 1: pieces of 258 while at least 258 remain, then the rest r as one
 *            match if r >= 3 and as r literals if r < 3.  No other distance is used.
 * CODING     one block per segment, the smallest of three forms by their exact bit counts, the stored form on a tie with either other,
 *            the fixed one on a tie with the dynamic one:
 *              stored   3 header bits, padding to the byte, LEN, NLEN (little-endian), the L bytes: 40 + 8 L bits;
 *              fixed    3 + the tokens in the fixed code of RFC 1951 + the end-of-block symbol (7 bits);
 *              dynamic  3 + 14 + 3 (HCLEN + 4) + the code-length sequence + the tokens + the end-of-block symbol.
 *            BFINAL is 1 in the last segment's block and 0 elsewhere.  A match of length l is the length symbol and extra bits of RFC 1951
 *            (258 is symbol 285) followed by distance symbol 0, which has no extra bits.  Huffman codes enter the stream from their most
 *            significant bit, every other field from its least significant bit; bits fill each byte from bit 0.
 *            After its block every segment but the last writes an empty stored block: the bits 000, padding to the byte, 00 00 FF FF.  The
 *            last segment pads to the byte with zero bits.
 * DYNAMIC    frequencies: every literal and length symbol of the tokens, 1 for symbol 256; distance symbol 0 once per match.
 *  CODES     Lengths of an alphabet from its frequencies, with the limit M (15 for both alphabets, 7 for the code-length alphabet):
 *              1. the used symbols (frequency > 0) in ascending order of (frequency, symbol).  None: all lengths 0.  One: length 1.
 *              2. a Huffman tree by the two-queue method: the leaves in that order in one queue, the merged nodes in the order of
 *                 their making in the other; each step removes the two lightest heads, a leaf before a merged node of the same weight,
 *                 and appends their sum.  n[d] = the number of leaves at depth d.
 *              3. the limit: n[M] += the sum of n[d] over d > M; K = the sum of n[d] * 2^(M - d) over d = 1..M; while K > 2^M: n[M] -= 1,
 *                 the largest d < M with n[d] > 0 gets n[d] -= 1 and n[d + 1] += 2, K -= 1.
 *              4. the symbols in the order of 1. take the lengths from the longest down: the first n[M] get M, the next n[M - 1] get
 *                 M - 1, and so on.  Codes are the canonical ones of RFC 1951 3.2.2.
 *            HLIT = (the last used literal/length symbol + 1) - 257.  HDIST = 0: the one distance code has length 1 when the segment has
 *            a match and 0 when it has none.  The code-length sequence is the HLIT + 257 literal/length lengths followed by the one
 *            distance length, taken as ONE sequence and cut into maximal runs of equal values.  A run of r zeros: symbol 18 with 138
 *            while r >= 138, then 18 with r if r >= 11, 17 with r if 3 <= r <= 10, r symbols 0 if r < 3.  A run of r values v > 0: the
 *            symbol v, then for the r - 1 others symbol 16 with 6 while at least 6 remain, then 16 with the rest t if t >= 3 and t
 *            symbols v if t < 3.  The code-length alphabet's lengths come from the frequencies of these symbols (limit 7) and are sent in
 *            the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15 up to the last non-zero one, at least four (HCLEN).  Extra bits: 2
 *            for 16 (count - 3), 3 for 17 (count - 3), 7 for 18 (count - 11).
 *
 * vse_png_bound: an upper bound on one file's bytes, 51 + H rb + 22 S: signature, IHDR and IEND (45), the zlib header and the Adler-32 (6),
 *   the filtered bytes, and per segment 12 bytes of chunk framing, 5 of a stored block's header and 5 of the empty stored block.  Negative
 *   with a message for a shape the encoder refuses.
 * vse_png_workspace_bytes: the workspace vse_png_encode needs for n images of that shape (the filtered streams, every segment's deflate
 *   data at its worst-case size, and four words per segment); negative with a message as above or when n is negative.
 * vse_png_encode: out [n, out_stride] bytes, file i from out + i * out_stride on, lengths [n] int32 its size.  out_stride >= the bound.
 *   images: n contiguous images in the form `layout` names, the codes of vicasplat_data.h: VSP_LAYOUT_U8_HWC uint8 [n, H, W, C],
 *   VSP_LAYOUT_U8_CHW uint8 [n, C, H, W], VSP_LAYOUT_F32_CHW f32 [n, C, H, W] quantised as above (4-byte aligned).
 *   workspace: at least vse_png_workspace_bytes(n, h, w, c) bytes, 16-byte aligned, overwritten.  lengths: 4-byte aligned; out: any address.
 *   Asynchronous on `stream`, no host synchronisation, no atomics, ordinary vector stores only: the call can be captured into a graph, the
 *   same input gives the same bytes, and a file's bytes do not depend on the batch it is in.  Nothing is written outside
 *   out[i, :bound], lengths[i] and the workspace; the bytes of out[i] past lengths[i] are left as they were.  n = 0 is a no-op.
 *   A null pointer, a misaligned or too-small workspace, misaligned images or lengths, an unknown layout, c or filter mode, a refused
 *   shape, out_stride below the bound or n < 0 return a negative code and a message before any HIP call.
 */
#ifndef VICASPLAT_PNG_H
#define VICASPLAT_PNG_H
#include "vicasplat_data.h"

#define VSE_FILTER_NONE 0
#define VSE_FILTER_SUB 1
#define VSE_FILTER_UP 2
#define VSE_FILTER_AVERAGE 3
#define VSE_FILTER_PAETH 4
#define VSE_FILTER_ADAPTIVE 5
#define VSE_SEGMENT_BYTES 16384
#define VSE_MAX_ROW_BYTES 65535
#define VSE_MAX_ROWS 65535

#ifdef __cplusplus
extern "C" {
#endif

int64_t vse_png_bound(int32_t h, int32_t w, int32_t c);
int64_t vse_png_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t c);
int vse_png_encode(const void *images, int32_t layout, int32_t n, int32_t h, int32_t w, int32_t c, int32_t filter_mode, void *workspace,
                   int64_t workspace_bytes, uint8_t *out, int64_t out_stride, int32_t *lengths, vs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VICASPLAT_PNG_H */
