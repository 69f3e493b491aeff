/* vicasplat_metrics.h -- the evaluation-metric entries of libvicasplat_hip.so (csrc/trajectory.hip): the trajectory metrics of the test step.
 *
 * A fifth public header of the same library: vicasplat_hip.h and its ABI version are unchanged by it, and so are vicasplat_distill.h,
 * vicasplat_loss.h and vicasplat_teacher.h.  Its entries carry the prefix vsm_; they report errors as the entries of vicasplat_hip.h do (a
 * negative return and a message behind the library's error call) and take the same stream type.
 *
 * camera_eval_metrics (src/evaluation/metrics.py:148-265, called by src/model/model_wrapper.py:367-381 and
 * src/evaluation/pose_evaluator.py:157-174): ATE, RPE-trans and RPE-rot of an estimated trajectory against the ground truth, as evo's ape
 * and rpe compute them with align=True, correct_scale=True, delta in frames, all_pairs=True.  evo is not available offline: the metrics are
 * restated from the published algorithm (Umeyama 1991 for the alignment) and are UNVERIFIED against evo.  Batched over scenes, float64:
 *   pred, gt: [B, V, 4, 4] camera-to-world poses, contiguous device memory, f32 (dtype 0) or f64 (dtype 5: the codes of
 *   vicasplat_hip.h continue, so that a 16-bit code is refused and not misread), promoted on load.
 *   x_i, y_i: the positions of the estimate and of the truth; Rp_i, Rq_i: their rotation blocks, used as given (the reference passes them
 *   through a quaternion and back: a stated deviation).
 *   mu_x, mu_y: the means; sigma_x^2 = (1/V) sum |x_i - mu_x|^2; C = (1/V) sum (y_i - mu_y)(x_i - mu_x)^T = U diag(d) V^T, d descending;
 *   S = I with S_33 = -1 when det U det V < 0; R = U S V^T, c = tr(diag(d) S) / sigma_x^2, t = mu_y - c R mu_x.
 *   A scene is degenerate when fewer than two d_k exceed 2^-52 (evo's absolute test), when V < 3 (two points are collinear), when
 *   delta >= V, or when any of its 32 V input elements is not finite: valid = 0, the three metrics 0, the alignment the identity (the
 *   reference's bare `except` turns evo's exception into 0.0 for all three, model_wrapper.py:374-377).  Other scenes are not affected.
 *   ATE = sqrt(mean_i |c R x_i + t - y_i|^2).
 *   RPE over the pairs (i, j = i + delta), j < V: A = Rq_i^T Rq_j, a = Rq_i^T (y_j - y_i), B = Rp_i^T Rp_j, b = c Rp_i^T (x_j - x_i) (the
 *   alignment leaves relative rotations unchanged and scales relative translations by c), E_R = A^T B, E_t = A^T (b - a);
 *   RPE-trans = sqrt(mean |E_t|^2); RPE-rot = sqrt(mean theta^2), theta the rotation angle of E_R in DEGREES,
 *   theta = atan2(|(E32 - E23, E13 - E31, E21 - E12)| / 2, (tr E_R - 1) / 2).
 *   The sums over the poses are compensated and combined across the wave in a fixed order; the 3 x 3 SVD is a cyclic one-sided Jacobi
 *   method with a constant bound on its sweeps, the third singular vectors completed from the first two.  There are no atomics: the same
 *   inputs give the same bits, and a scene's result does not depend on the batch it is in.
 *
 * vsm_trajectory_metrics: metrics [B, 3] = (ate, rpe_trans, rpe_rot) f64; valid [B] int32; align [B, 13] f64 = R row-major, t, c -- or null.
 *   Asynchronous on `stream`, no host synchronisation, no workspace: it can be captured into a graph.  B = 0 is a no-op.  Null pred, gt,
 *   metrics or valid, an unknown dtype, B < 0, V < 1 or delta < 1 return a negative code and a message before any HIP call.
 */
#ifndef VICASPLAT_METRICS_H
#define VICASPLAT_METRICS_H
#include "vicasplat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int vsm_trajectory_metrics(const void *pred, const void *gt, int32_t dtype, int32_t B, int32_t V, int32_t delta, double *metrics,
                           int32_t *valid, double *align, vs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VICASPLAT_METRICS_H */
