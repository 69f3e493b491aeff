/* vicasplat_jpeg.h -- the JPEG entries of libvicasplat_hip.so (csrc/jpeg.hip, csrc/jpeg_decode.h): a baseline decoder whose pixels equal
 * libjpeg-turbo's default decode (what PIL's Image.open gives) byte for byte.
 *
 * A header of the same library beside the eight of vicasplat_hip.h's family: their entries and the ABI version are unchanged by it.  Its
 * entries carry the prefix vsj_; they report errors as the entries of vicasplat_hip.h do (a negative return and a message behind the
 * library's error call, before any HIP call) and take the same stream type last.
 *
 * Streams: 8-bit baseline sequential Huffman JPEG (SOF0, SOF1 at 8 bits), one interleaved scan, 1 component (grayscale) or 3 components
 * YCbCr with chroma sampled 1 x 1 and luma 1 x 1, 2 x 1 or 2 x 2, any restart interval.  The host (vicasplat_amd/dataset/jpeg.py) walks the
 * markers, refuses everything else, and describes each frame to the device in ONE packed buffer:
 *
 *   frames    [N, VSJ_FRAME_WORDS] int32, the words VSJ_F_*: components; luma sampling hs, vs; MCUs per row and column (ceil(w / 8 hs),
 *             ceil(h / 8 vs)); first entry and count of the frame's restart segments in `segs`; the frame's first 8 x 8 block in the
 *             workspace; per component the index of its quantisation table, its DC and its AC Huffman table.  The other words are 0.
 *             A frame's blocks: component 0 first, then 1 and 2; a component's plane is padded to whole MCUs and its blocks lie row-major,
 *             (mcus_x hs) x (mcus_y vs) for luma, mcus_x x mcus_y for chroma.
 *   segs      [segments, VSJ_SEG_WORDS] int32: first byte and end (one past the last byte) of the segment's entropy-coded data as offsets
 *             into `bytes`, markers and fill bytes excluded; its first MCU; its number of MCUs.
 *   quant     [n_quant, 64] uint16, natural (row-major) order.
 *   huff      [n_huff, VSJ_HUFF_BYTES] bytes, one decode table each: look [2^VSJ_LOOK_BITS] uint16 indexed by the next VSJ_LOOK_BITS bits,
 *             (length << 8) | symbol of the code that starts there, 0 when that code is longer; at VSJ_HUFF_MAXCODE maxcode [18] int32,
 *             the largest code of each length 1..16 (-1: none; entries 0 and 17 are -1); at VSJ_HUFF_VALOFF valoff [18] int32, the index of
 *             a length's first symbol minus its first code; at VSJ_HUFF_VALS the 256 symbols in code order.
 *   bytes     the compressed bytes of all frames, to the end of the buffer.
 *   The sections follow each other without gaps in that order; every one starts on a multiple of 16 bytes.
 *
 * Decoding, three kernels and one reduction behind vsj_decode:
 *   entropy   one lane per (frame, restart segment), the frame's tables in LDS.  The bit reader drops the 00 after an FF and reads zeros
 *             past the segment's end.  DC: a category s, then s bits v; the difference is v if v >= 1 << (s - 1), else v - (1 << s) + 1;
 *             the predictor starts at 0 in every segment.  AC: rs = (r << 4) | s; s = 0 with r = 15 skips 16 positions, s = 0 otherwise
 *             ends the block; else k += r and the value goes to zig-zag position k.  Coefficients are int16 in natural order.
 *   idct      one lane per block: coef * q in int32, then libjpeg's "islow" inverse DCT (jidctint.c): CONST_BITS 13, PASS1_BITS 2,
 *             columns first (descale by 11 bits, rounding), then rows (18 bits), sample = clamp(v + 128, 0, 255).
 *   colour    chroma upsampled on its true size W' = ceil(w / 2), H' = ceil(h / 2) (jdsample.c, "fancy"), edges replicated:
 *             2 x 1: out[2i] = (3 in[i] + in[i-1] + 1) >> 2, out[2i+1] = (3 in[i] + in[i+1] + 2) >> 2;
 *             2 x 2: s = 3 row[r] + row[r-1] for the output row 2r, 3 row[r] + row[r+1] for 2r + 1, then
 *                    out[2i] = (3 s[i] + s[i-1] + 8) >> 4, out[2i+1] = (3 s[i] + s[i+1] + 7) >> 4;
 *             W' <= 2: plain replication, as the library does.  Then jdcolor.c with cb, cr minus 128:
 *             R = clamp(Y + ((91881 cr + 32768) >> 16)), G = clamp(Y + ((-22554 cb - 46802 cr + 32768) >> 16)),
 *             B = clamp(Y + ((116130 cb + 32768) >> 16)).  A grayscale frame stores R = G = B = Y.
 *   status    per frame, the OR of its segments' VSJ_STATUS_* bits: INDEX a coefficient position past 63; CODE bits that are no code of
 *             the table; SHORT the segment ended before its last MCU; LEFTOVER a whole byte or more of the segment was not used; MARKER an
 *             FF inside the segment that no 00 follows; DESC the descriptor does not belong to the call's sizes (nothing of that frame is
 *             read or written).  A segment stops at its first damaged block; its remaining coefficients are zero.
 *
 * vsj_workspace_bytes: the workspace vsj_decode needs for `blocks` 8 x 8 blocks and `segments` restart segments in all (coefficients,
 *   sample planes and one status word per segment); negative with a message when an argument is negative.
 * vsj_decode: out [N, h, w, 3] uint8 packed -- VSP_LAYOUT_U8_HWC of vicasplat_data.h -- and status [N] int32 (0 = clean).
 *   packed, packed_bytes: the buffer above ON THE DEVICE, 16-byte aligned; segments, n_quant, n_huff: the lengths of its sections;
 *   max_frame_segments: an upper bound on any frame's segment count (it sizes the entropy grid); blocks: the blocks of all frames.
 *   workspace: at least vsj_workspace_bytes(blocks, segments) bytes, 16-byte aligned, overwritten.
 *   Asynchronous on `stream`, no host synchronisation, no atomics, status written with ordinary stores: the call can be captured into a graph,
 *   the same input gives the same bits, and a frame's bytes do not depend on the batch it is in.  N = 0 is a no-op.
 *   Memory: a segment is never read outside its byte range, a frame is never written outside its own blocks, pixels and status word,
 *   whatever the bytes say; every descriptor index is checked on the device against the sizes given here, so that a descriptor that does
 *   not belong gives VSJ_STATUS_DESC and no access outside the buffers.  Pixels of a frame with a non-zero status are unspecified.
 *   A null pointer, a size below 1 (N below 0), sections longer than packed_bytes, more than 2^31 - 1 compressed bytes, blocks or
 *   workgroups, a workspace that is too small or a misaligned buffer return a negative code and a message before any HIP call.
 */
#ifndef VICASPLAT_JPEG_H
#define VICASPLAT_JPEG_H
#include "vicasplat_hip.h"

#define VSJ_FRAME_WORDS 24
#define VSJ_F_NCOMP 0
#define VSJ_F_HS 1
#define VSJ_F_VS 2
#define VSJ_F_MCUS_X 3
#define VSJ_F_MCUS_Y 4
#define VSJ_F_SEG0 5
#define VSJ_F_NSEG 6
#define VSJ_F_BLOCK0 7
#define VSJ_F_QUANT 8
#define VSJ_F_DC 11
#define VSJ_F_AC 14
#define VSJ_SEG_WORDS 4
#define VSJ_LOOK_BITS 9
#define VSJ_HUFF_MAXCODE 1024
#define VSJ_HUFF_VALOFF 1096
#define VSJ_HUFF_VALS 1168
#define VSJ_HUFF_BYTES 1424
#define VSJ_STATUS_INDEX 1
#define VSJ_STATUS_CODE 2
#define VSJ_STATUS_SHORT 4
#define VSJ_STATUS_LEFTOVER 8
#define VSJ_STATUS_MARKER 16
#define VSJ_STATUS_DESC 32

#ifdef __cplusplus
extern "C" {
#endif

int64_t vsj_workspace_bytes(int64_t blocks, int32_t segments);
int vsj_decode(const void *packed, int64_t packed_bytes, int32_t N, int32_t h, int32_t w, int32_t segments, int32_t max_frame_segments,
               int32_t n_quant, int32_t n_huff, int64_t blocks, void *workspace, int64_t workspace_bytes, uint8_t *out, int32_t *status,
               vs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VICASPLAT_JPEG_H */
