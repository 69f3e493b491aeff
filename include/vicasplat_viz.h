/* vicasplat_viz.h -- the visualisation entries of libvicasplat_hip.so (csrc/viz.hip): the depth colour maps and the video frames of the
 * validation step.
 *
 * A seventh public header of the same library: vicasplat_hip.h and its ABI version are unchanged by it, and so are the other five.  Its
 * entries carry the prefix vsv_; they report errors as the entries of vicasplat_hip.h do (a negative return and a message behind the
 * library's error call) and take the same stream type.  Every entry is asynchronous on `stream`, synchronises nothing with the host, takes
 * its workspace from the caller and can be captured into a graph.  There are no float atomics: the same inputs give the same bits.
 *
 * vis_depth_map (src/misc/utils.py:13-22), confidence_map (:25-35), apply_color_map_to_image (src/visualization/color_map.py:9-27) and
 * the frame packing of render_video_generic (src/model/model_wrapper.py:805-813).
 *
 * vsv_depth_range: range[0] = near, range[1] = far of n contiguous f32 values, n <= VSV_MAX_RANGE_N (the reference slices
 *   [:16_000_000]; a larger n is refused: the ordered compaction the slice of the positives would need is not built).
 *     far  = log(Q_0.99(all n values)); near = log(Q_0.01(the values > 0)), and near = 0 when no value is > 0.
 *     Q_q over m values is torch.quantile for an f32 input: rank r = f32(q) * f32(m - 1) formed in f32, the order statistics a at
 *     floor(r) and b at ceil(r), exact, and torch.lerp with w = r - floor(r): a + w (b - a) for w < 0.5, else b - (b - a) (1 - w).
 *     A NaN among the values makes far NaN and does not touch near.  Negative values and infinities take part in far by IEEE order
 *     (-0 sorts below +0; both quantiles then compare equal).  log is the f32 library logarithm; log of a negative quantile is NaN.
 *   The selection is a radix selection on order-preserving 32-bit keys, four 8-bit passes over the data.  In each pass a workgroup
 *   counts in LDS with integer atomics and adds its counts to one histogram per statistic in the workspace with integer atomics
 *   (integer sums do not depend on the arrival order); a one-workgroup kernel between the passes narrows the four ranks.  The first pass
 *   also counts the positives and the NaNs, which place the ranks of near among all n keys (the positives are the keys above +0's).
 *   order_stats: null, or [4] f32 = (a, b) of near, then (a, b) of far; the pair of near is (0, 0) when no value is > 0.
 *   workspace: vsv_depth_range_workspace_bytes(n) bytes, 16-byte aligned, contents arbitrary on entry.
 *   Values are read 16 bytes per lane from the first 16-byte boundary of `value` on; the elements before it and the tail are read singly.
 *   Launch geometry: workgroups of VSV_THREADS threads, VSV_VEC values per thread and round, at most VSV_MAX_BLOCKS workgroups.
 *
 * vsv_color_map: value [M, H, W] f32 -> out [M, 3, H, W], f32 (VSV_OUT_F32) or uint8 (VSV_OUT_U8), through lut [256, 3] f32.
 *     VSV_MODE_DEPTH: x = 1 - (log v - near) / (far - near), (near, far) = range[0..1] read on the device.
 *     VSV_MODE_MAX:   x = v / max(v) over all M H W values; the max propagates a NaN as torch.max does; range is not read.
 *     VSV_MODE_UNIT:  x = v (apply_color_map itself); range is not read.
 *     All in f32, IEEE results stand (v = 0 gives x = +inf, clipped to 1, when far > near; far == near gives NaN).
 *     idx = min(trunc(clip(x, 0, 1) * 256), 255); f32 out = lut[idx], and (0, 0, 0) for a NaN x (matplotlib's Colormap.__call__: a
 *     pure lookup); uint8 out = trunc(clip(lut[idx], 0, 1) * 255), and 0 for a NaN x or a NaN table entry.
 *   The table is staged in LDS.  With H W a multiple of 4 and value and out 16-byte aligned a lane loads 16 bytes and stores 16 bytes
 *   (f32) or 4 bytes (uint8) per plane; otherwise every element goes singly.
 *   workspace: vsv_color_map_workspace_bytes(mode) bytes (0 for the other modes than VSV_MODE_MAX: it may then be null), 16-byte aligned.
 *
 * vsv_video_frames: frames [M, 3, 2 H + gap, W] uint8 in one launch from rgb [M, 3, H, W] f32 and depth [M, H, W] f32:
 *     rows 0 .. H - 1: trunc(clip(rgb, 0, 1) * 255); the next gap rows: 255; the last H rows: the uint8 colour of VSV_MODE_DEPTH.
 *     This is vcat(rgb, vis_depth_map(depth)) with a white gap, then (video.clip(0, 1) * 255).type(torch.uint8).
 *     A NaN (rgb, x or table entry) GIVES 0: a stated choice, torch's cast of a NaN is platform-defined.
 *   With W a multiple of 4 and all three pointers 16-byte aligned (frames: 4-byte) a lane handles four pixels, else one.
 *
 * Every entry returns a negative code and a message before any HIP call on a null pointer, a negative size, an unknown mode or dtype, a
 * workspace that is null, short or misaligned, n > VSV_MAX_RANGE_N, or more than 2^31 - 1 - VSV_THREADS work items.  A zero-size call is a no-op.
 */
#ifndef VICASPLAT_VIZ_H
#define VICASPLAT_VIZ_H
#include "vicasplat_hip.h"

#define VSV_THREADS 256
#define VSV_VEC 4
#define VSV_MAX_BLOCKS 1024
#define VSV_MAX_RANGE_N 16000000
#define VSV_MODE_DEPTH 0
#define VSV_MODE_MAX 1
#define VSV_MODE_UNIT 2
#define VSV_OUT_F32 0
#define VSV_OUT_U8 1

#ifdef __cplusplus
extern "C" {
#endif

int64_t vsv_depth_range_workspace_bytes(int64_t n);
int vsv_depth_range(const float *value, int64_t n, float *range, float *order_stats, void *workspace, int64_t workspace_bytes,
                    vs_stream_t stream);
int64_t vsv_color_map_workspace_bytes(int32_t mode);
int vsv_color_map(const float *value, int32_t M, int32_t H, int32_t W, int32_t mode, const float *range, const float *lut, void *out,
                  int32_t out_dtype, void *workspace, int64_t workspace_bytes, vs_stream_t stream);
int vsv_video_frames(const float *rgb, const float *depth, int32_t M, int32_t H, int32_t W, int32_t gap, const float *range,
                     const float *lut, uint8_t *frames, vs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VICASPLAT_VIZ_H */
