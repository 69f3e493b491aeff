/* vicasplat_draw.h -- the vector-drawing entries of libvicasplat_hip.so (csrc/draw.hip): antialiased lines and points (rings) drawn over
 * a batch of images, one layer per call.
 *
 * A further public header of the same library: vicasplat_hip.h and its ABI version are unchanged by it, and so are the other headers.  Its
 * entries carry the prefix vsg_; they report errors as the entries of vicasplat_hip.h do (a negative return and a message behind the
 * library's error call) and take the same stream type.  Both entries are asynchronous on `stream`, synchronise nothing with the host,
 * take no workspace and can be captured into a graph.  There are no float atomics: the same inputs give the same bits, and an image's
 * result does not depend on the batch it is in.
 *
 * draw_lines (src/visualization/drawing/lines.py), draw_points (points.py) and render_over_image / run_msaa_pass / detect_msaa_pixels /
 * reduce_straight_alpha (rendering.py) with subdivision 8, in f32.
 *
 * Both entries: image [B, 3, H, W] f32 and out of the same shape, contiguous; out == image is allowed (a pixel depends on no other pixel
 * of the image), any other overlap of the two is refused.  The primitives are given IN PIXEL SPACE (the world -> pixel conversion is the
 * caller's): one device array of `n_prims` records, and prim_offsets [B + 1] int32 on the device, which gives image b the records
 * [off[b], off[b + 1]) -- read on the device and clamped there to 0 <= off[b] <= off[b + 1] <= n_prims, so that no offset can lead
 * outside the array.  A record's position in its image's range is its index.
 *   line record  VSG_LINE_FLOATS  f32: start x, start y, end x, end y, width, r, g, b
 *   point record VSG_POINT_FLOATS f32: x, y, radius, inner radius, r, g, b
 *
 * Coverage of a sample p = (x, y), every operation rounded once to f32 in the order written, nothing contracted into an fma, division and
 * square root correctly rounded (csrc/draw.hip is compiled as csrc/overlap.hip is):
 *   line body   D = end - start, n = sqrt(Dx Dx + Dy Dy), u = D / n, i = p - start, par = ux ix + uy iy, q = i - par u;
 *               inside when par <= n + extra and par > -extra and sqrt(qx qx + qy qy) < w / 2, with extra = w / 2 for VSG_CAP_SQUARE
 *               and 0 otherwise.
 *   round cap   VSG_CAP_ROUND: also inside when |p - start| < w / 2 or |p - end| < w / 2 (|v| = sqrt(vx vx + vy vy)).
 *   zero length n = 0 makes u NaN: the body covers nothing (a comparison with a NaN is false), the round caps still do.
 *   point       d = |p - c|; inside when inner <= d and d <= radius, both ends inclusive.
 *   NaN         a record with a NaN among its geometry (everything but the colour) covers nothing.  ONE STATED DEVIATION: in the
 *               reference a round-capped line whose end alone is NaN still draws the cap at its start.
 *   Infinite coordinates, widths and radii are legal and follow IEEE (an infinite width covers every sample the body's `par` test admits).
 * A sample takes the colour of the HIGHEST-INDEXED record of its image that covers it, and alpha 1; an uncovered sample has alpha 0 and
 * (as the reference's argmax over nothing gives) the colour of record 0.
 *   pass 0      samples the pixel centres (x + 0.5, y + 0.5).
 *   num_passes = 1: a pixel is refined when its pass-0 RGBA differs (!=, any channel) from that of any of its up to eight neighbours INSIDE
 *               the image; there are no neighbours outside, so a record that covers the whole image refines nothing.  A refined pixel
 *               samples centre + ((k + 0.5) / 8 - 0.5) for k = 0 .. 7 in x and in y (all exact in f32 for H, W <= VSG_MAX_SIDE) and gets
 *               colour = sum(c_i a_i) / (sum(a_i) + 1e-10f), alpha = sum(a_i) / 64.  sum(a_i) is an integer count; the colour sum is a
 *               fixed butterfly over the 64 lanes of a wave (lane = 8 ky + kx; partner distances 1, 2, 4, 8, 16, 32 in that order).
 *   blend       out = image (1 - alpha) + colour alpha, two products and one sum.
 * Non-finite colours are unspecified.  An image with no records is copied through (STATED DEVIATION: the reference raises on the argmax
 * of an empty list).
 *
 * Kernel: one workgroup of VSG_THREADS threads per tile of VSG_TILE_W x VSG_TILE_H pixels, plus a one-pixel halo for the neighbour test.
 * It scans its image's records VSG_SCAN_CHUNK at a time and compacts into LDS, in index order (wave ballot + prefix count), those that can
 * reach the tile plus halo: the record's bounding box, expanded by w / 2 + extra (or the radius) and a slack far above the f32 rounding of
 * the coverage test, must meet it, and for a line of finite, non-degenerate direction so must the oriented box around the segment.  The
 * test only ever keeps too much (NaN and infinite extents compare false and are kept), so it cannot change a result.  The list holds
 * VSG_LIST_CAP records; a longer one is processed in several rounds, with the running topmost index per sample kept in registers (pass 0)
 * or in LDS (subsamples).  Pass 0 is evaluated for tile + halo, the refine mask formed for the interior, and the masked pixels are handed
 * to the waves one pixel per wave: the lane is the subsample, alpha a ballot population count.
 *
 * Refused with a negative code and a message before any HIP call: a null image, out or prim_offsets with B H W > 0, a null record array
 * with n_prims > 0, a negative B, H, W or n_prims, H or W above VSG_MAX_SIDE, B above VSG_MAX_BATCH (the grid's z extent), an unknown cap,
 * num_passes outside {0, 1}, n_prims above 2^31 / 8, out overlapping image without being equal to it.  B H W = 0 is a no-op.
 */
#ifndef VICASPLAT_DRAW_H
#define VICASPLAT_DRAW_H
#include "vicasplat_hip.h"

#define VSG_THREADS 256
#define VSG_TILE_W 16
#define VSG_TILE_H 8
#define VSG_SCAN_CHUNK 256
#define VSG_LIST_CAP 512
#define VSG_MAX_SIDE 16384
#define VSG_MAX_BATCH 65535
#define VSG_LINE_FLOATS 8
#define VSG_POINT_FLOATS 7
#define VSG_CAP_BUTT 0
#define VSG_CAP_ROUND 1
#define VSG_CAP_SQUARE 2

#ifdef __cplusplus
extern "C" {
#endif

int vsg_draw_lines(const float *image, float *out, int32_t B, int32_t H, int32_t W, const float *lines, int32_t n_prims,
                   const int32_t *prim_offsets, int32_t cap, int32_t num_passes, vs_stream_t stream);
int vsg_draw_points(const float *image, float *out, int32_t B, int32_t H, int32_t W, const float *points, int32_t n_prims,
                    const int32_t *prim_offsets, int32_t num_passes, vs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VICASPLAT_DRAW_H */
