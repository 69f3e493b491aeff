/* vicasplat_data.h -- the data-side entries of libvicasplat_hip.so (csrc/preprocess.hip): the crop shim of the dataset loaders.
 *
 * A sixth public header of the same library: vicasplat_hip.h and its ABI version are unchanged by it, and so are the other four.  Its
 * entries carry the prefix vsp_; they report errors as the entries of vicasplat_hip.h do (a negative return and a message behind the
 * library's error call) and take the same stream type.
 *
 * rescale_and_crop (src/dataset/shims/crop_shim.py:11-75) with the mirror of reflect_views (augmentation_shim.py:16-21) folded in: per
 * frame, the source quantised to 8 bits, PIL's 8-bit Lanczos reduction (Image.resize(..., Image.LANCZOS), reducing only) to
 * h_scaled x w_scaled, a crop window, and the division by 255 -- byte for byte what the reference computes on the host.
 *
 * PIL's resample, one axis, `in` -> `out` samples, out <= in:
 *   scale = in / out, filterscale = max(scale, 1), support = 3 filterscale, ksize = ceil(support) * 2 + 1;
 *   for the output index xx: center = (xx + 0.5) scale, xmin = max(int(center - support + 0.5), 0),
 *   xmax = min(int(center + support + 0.5), in), n = xmax - xmin, w[x] = L((x + xmin - center + 0.5) * (1 / filterscale)) for x < n,
 *   L(t) = sinc(t) sinc(t / 3) on -3 <= t < 3 and 0 elsewhere, in float64, divided by their sum in index order;
 *   k[x] = int(w[x] * 2^22 +- 0.5) (half away from zero); the sample is clamp((2^21 + sum_x k[x] p[xmin + x]) >> 22, 0, 255).
 *   The horizontal pass comes first and rounds to bytes; the vertical pass reads those bytes.  A pass whose in == out is skipped.
 * The tables are built on the host (vicasplat_amd/dataset/shims/crop_shim.py resample_tables, with the C library's sin that PIL calls)
 * and handed over as device arrays: bounds [out, 2] int32 = (xmin, n) and k [out, ksize] int32, the taps past n zero.  The builder
 * guarantees 255 sum|k| + 2^21 < 2^31 per row: the sums are int32.  The kernel clamps what it reads from the tables to the source and
 * to ksize, so that a table that does not belong to the sizes gives wrong bytes and no access outside the buffers.
 *
 * vsp_rescale_crop: out [N, 3, h_out, w_out] f32 planar = float32(u) / 255, or (float32(u) / 255 - mean[c]) / std[c] when mean and std
 *   are given (a true IEEE subtraction and division: bit-equal to the reference's normalize_image on the raw form).
 *   src: N frames of h_in x w_in x 3, contiguous, in the form `layout` names:
 *     VSP_LAYOUT_U8_HWC (0) uint8 packed [N, h_in, w_in, 3], as a decoder delivers it;
 *     VSP_LAYOUT_U8_CHW (1) uint8 planar [N, 3, h_in, w_in];
 *     VSP_LAYOUT_F32_CHW (2) f32 planar [N, 3, h_in, w_in] in [0, 1], quantised as the reference does it: an f32 product with 255,
 *       clamped to [0, 255], truncated.  NaN BECOMES 0 (the reference's cast of a NaN is undefined).
 *   bounds_x, k_x, w_scaled, kx: the horizontal table of w_in -> w_scaled ([w_scaled, 2] and [w_scaled, kx]); w_scaled == w_in skips the
 *     pass, and the three other arguments are then not read.  bounds_y, k_y, h_scaled, ky: the same for the rows.
 *   row, col: the crop window's corner in the scaled image; only its h_out rows and w_out columns are computed.
 *   mirror: uint8 [N] on the device or null; a frame whose flag is not 0 is mirrored left-right BEFORE the resample and the crop (the
 *     source column w_in - 1 - x is read for x), which is the reference's order.
 *   mean, std: both null, or both HOST arrays of 3 floats, read before the launch.
 *   Asynchronous on `stream`, no host synchronisation, no workspace, no atomics: it can be captured into a graph, the same inputs give the
 *   same bits, and a frame's result does not depend on the batch it is in.  N = 0 is a no-op.  A null src or out, a null table of a pass
 *   that is not skipped, mean without std, an unknown layout, a size below 1, w_scaled > w_in or h_scaled > h_in (enlarging is not
 *   built), a crop window outside the scaled image, kx or ky outside [1, VSP_MAX_TAPS], or more than 2^31 - 1 workgroups return a negative
 *   code and a message before any HIP call.
 */
#ifndef VICASPLAT_DATA_H
#define VICASPLAT_DATA_H
#include "vicasplat_hip.h"

#define VSP_LAYOUT_U8_HWC 0
#define VSP_LAYOUT_U8_CHW 1
#define VSP_LAYOUT_F32_CHW 2
#define VSP_MAX_TAPS 128

#ifdef __cplusplus
extern "C" {
#endif

int vsp_rescale_crop(const void *src, int32_t layout, int32_t N, int32_t h_in, int32_t w_in, const int32_t *bounds_x, const int32_t *k_x,
                     int32_t w_scaled, int32_t kx, const int32_t *bounds_y, const int32_t *k_y, int32_t h_scaled, int32_t ky, int32_t row,
                     int32_t col, int32_t h_out, int32_t w_out, const uint8_t *mirror, const float *mean, const float *std, float *out,
                     vs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VICASPLAT_DATA_H */
