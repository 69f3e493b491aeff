/* vicasplat_distill.h -- the distillation entries of libvicasplat_hip.so (csrc/distill.hip): the point loss of training stage 1.
 *
 * A second public header of the same library: vicasplat_hip.h and its ABI version are unchanged by it.  Its entries carry the prefix
 * vsd_; they report errors as the entries of vicasplat_hip.h do (a negative return and a message behind the library's error call) and
 * take the same stream type.
 *
 * Regr3D (src/loss/loss_conf_point.py:188-252 with normalize_pointcloud 'avg_dis', src/geometry/ptc_geometry.py:270-328), all f32:
 *   gt_pts1/2, pr_pts1/2: [B, H, W, 3]; gt_conf1/2, pr_conf1/2: [B, H, W]; contiguous device memory; n = H * W is arbitrary.
 *   d_v = |gt_v| per pixel; (q01, q99)_v per batch element = torch.quantile(d_v, (0.01, 0.99)) with the default linear interpolation in
 *   f32 arithmetic (rank = q (n - 1), floor, frac, torch's lerp), found by radix selection on the bit patterns, never by sorting;
 *   valid_v = (d_v >= q01_v) & (d_v <= q99_v).
 *   normalize_pts != 0: prediction and pseudo-GT are each divided by their own per-batch-element factor
 *     max(sum_valid |p| over both views / (nnz1 + nnz2 + 1e-8), 1e-8).
 *   loss = sum_valid1 gt_conf1 |gt1 - pr1| / count(valid1) + the same for view 2 (counts over the whole batch)
 *          + mean |pr_conf1 - gt_conf1| + mean |pr_conf2 - gt_conf2| over all pixels when BOTH pr_conf pointers are given.
 *   Every reduction has two stages in a fixed order and there are no float atomics: the same inputs give the same bits.
 *
 * vsd_regr3d_workspace_bytes(B, H, W): bytes of device workspace of one forward / backward pair (a few KB per batch element).
 * vsd_regr3d_forward: writes *loss (device f32 scalar) and leaves thresholds, counts, factors and the normalisation's gradient term in
 *   the workspace.  A NaN (or negative) distance makes the quantiles meaningless: the entry then returns -3 with a message.  To report
 *   that, it waits for its own kernels on `stream` before it returns (one 4-byte read); it cannot be captured into a graph.
 * vsd_regr3d_backward: from the SAME inputs and the workspace the forward filled, d_pr_pts1/2 [B, H, W, 3] and (when both pr_conf are
 *   given; else ignored, may be null) d_pr_conf1/2 [B, H, W] of grad_loss[0] * loss (grad_loss: device f32 scalar), overwritten, the
 *   gradient through the prediction's normalisation factor included.  Subgradients are torch's: 0 for |.| at 0.  The quantiles, the
 *   mask and the pseudo-GT carry no gradient.  Asynchronous on `stream`.
 */
#ifndef VICASPLAT_DISTILL_H
#define VICASPLAT_DISTILL_H
#include "vicasplat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t vsd_regr3d_workspace_bytes(int32_t B, int32_t H, int32_t W);
int vsd_regr3d_forward(const float *gt_pts1, const float *gt_pts2, const float *pr_pts1, const float *pr_pts2, const float *gt_conf1,
                       const float *gt_conf2, const float *pr_conf1, const float *pr_conf2, int32_t B, int32_t H, int32_t W,
                       int32_t normalize_pts, void *workspace, int64_t workspace_bytes, float *loss, vs_stream_t stream);
int vsd_regr3d_backward(const float *gt_pts1, const float *gt_pts2, const float *pr_pts1, const float *pr_pts2, const float *gt_conf1,
                        const float *gt_conf2, const float *pr_conf1, const float *pr_conf2, int32_t B, int32_t H, int32_t W,
                        int32_t normalize_pts, const float *grad_loss, const void *workspace, int64_t workspace_bytes, float *d_pr_pts1,
                        float *d_pr_pts2, float *d_pr_conf1, float *d_pr_conf2, vs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VICASPLAT_DISTILL_H */
