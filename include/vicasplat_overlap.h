/* vicasplat_overlap.h -- the view-overlap entry of libvicasplat_hip.so (csrc/overlap.hip): how many rays of one camera have an epipolar
 * segment that crosses another camera's image, for a list of ordered camera pairs in one launch.
 *
 * An eighth public header of the same library: vicasplat_hip.h and its ABI version are unchanged by it, and so are the other six.  Its
 * entry carries the prefix vso_; it reports errors as the entries of vicasplat_hip.h do (a negative return and a message behind the
 * library's error call) and takes the same stream type.
 *
 * project_rays(...)["overlaps_image"] (src/geometry/epipolar_lines.py:157-251 with near = far = None, over the rays of
 * get_world_rays(sample_image_grid((H, W)), ...), src/geometry/projection.py:91-151), as src/evaluation/evaluation_index_generator.py
 * calls it, reduced to a closed form.  For the ordered pair (i -> j): the rays of camera i, the image of camera j, eps = 1e-6,
 * eps32 = 2^-23, N = H W.
 *   M = inv(E_j) E_i, R = M[:3, :3], o = M[:3, 3]: every ray of camera i starts at o in camera j's frame.  The extrinsics are read as
 *   affine maps (last row 0 0 0 1), not as rigid ones: inv([A t]) = [A^-1, -A^-1 t], A^-1 by the adjugate; o = A_j^-1 (t_i - t_j).
 *   Ray n = r W + c is the pixel centre x = (c + 0.5) / W, y = (r + 0.5) / H (formed in f32, as sample_image_grid does);
 *   u = K_i^-1 (x, y, 1); d = R (u / |u|).
 *   Frame lines f in {x = 0, x = 1, y = 0, y = 1}, s the line's own axis and q the other one:
 *     c_f = (value - K_j[s, 2]) / K_j[s, s];  t = (c_f o_z - o_s) / (d_s - c_f d_z);
 *     other = K_j[q, 2] + (K_j[q, q] (o_q (c_f d_z - d_s) + d_q (o_s - c_f o_z))) / (d_z o_s - d_s o_z);
 *     valid_f = (-eps <= other <= 1 + eps) and (o_z + t d_z > -eps) and (t > -eps);  any_f = the OR over the four lines.
 *     (The reference's argmin / argmax over the four lines pick among them; both of its `valid` results equal any_f.)
 *   Point projections: project(p) = the first two coordinates of K_j nan_to_num(p / (p_z + eps32), nan -> 0, +-inf -> +-1e8);
 *     in_bounds(xy): both coordinates in [-eps, 1 + eps];
 *     valid_inf = in_bounds(project(d)) and d_z > -eps;  at_camera = |o| < eps;
 *     valid_0 = valid_inf when at_camera, else in_bounds(project(o)) and o_z > -eps and not (o_z < eps).
 *   overlaps = (valid_0 and valid_inf) or any_f; counts[p] = the number of rays with `overlaps`.  NaN and inf follow IEEE: a comparison
 *   with a NaN is false.
 *   ONE STATED DEVIATION: when at_camera holds the frame-line terms use o = 0 exactly, so that their quotients are
 *   0 / 0, any_f is false and the count is the number of camera i's rays that point into image j.  In the reference o is rounding noise of
 *   size 1e-8 there and any_f is decided by that noise.
 *
 * Precision.  Per pair, M, K_i^-1 and the four c_f are computed in float64 from the inputs (f32 or f64, promoted on load) and rounded
 * once to f32.  Per ray everything runs in f32, the reference's working precision: eps is f32(1e-6), 1 + eps is f32(1.000001), every
 * product, sum, quotient and square root is rounded once, in the order written above (sums of three terms from the left).  Division and
 * square root are correctly rounded and nothing is contracted into an fma, whatever the library's default flags are: csrc/overlap.hip
 * switches contraction off with `#pragma clang fp contract(off)`, refuses to compile under fast-math (`#error` on __FAST_MATH__), and the
 * Makefile appends -fhip-fp32-correctly-rounded-divide-sqrt -fno-fast-math -ffp-contract=off to this one object's flags, after the
 * defaults, so that they win; no reciprocal or __fdividef appears in the file.
 *
 * vso_view_overlap_counts: extrinsics [V, 4, 4] camera-to-world, intrinsics [V, 3, 3] normalised, both contiguous device memory, f32
 *   (dtype 0) or f64 (dtype 5: the codes of vicasplat_hip.h continue, so that a 16-bit code is refused and not misread); pairs [P, 2]
 *   int32 = (i, j) on the device; counts [P] int32.
 *   One lane per ray: workgroups of VSO_THREADS threads, each taking VSO_CHUNK consecutive rays of one pair (grid = P x ceil(N /
 *   VSO_CHUNK), so two pairs at 256 x 256 fill 64 workgroups); the pair's constants sit in scalar registers; the flag is reduced with a
 *   wave ballot and a population count, the waves of a workgroup are summed in LDS and added to counts[p] with one integer atomic, after a
 *   hipMemsetAsync of counts on the same stream.  Integer sums do not depend on the arrival order: the same inputs give the same bits,
 *   and a pair's count does not depend on the list it is in.  Every element of counts is written, whatever it held before.
 *   A pair with an index outside [0, V) cannot be refused without a synchronisation: its count is -1 and nothing else is touched.
 *   Asynchronous on `stream`, no host synchronisation, no workspace: it can be captured into a graph.  P = 0 is a no-op.
 *   Refused with a negative code and a message before any HIP call: a null pointer with P > 0, an unknown dtype, V < 1, H < 1 or W < 1,
 *   P < 0, H W > 2^30, and P ceil(N / VSO_CHUNK) > 2^31 - 1 (the grid).
 */
#ifndef VICASPLAT_OVERLAP_H
#define VICASPLAT_OVERLAP_H
#include "vicasplat_hip.h"

#define VSO_THREADS 256
#define VSO_CHUNK 2048

#ifdef __cplusplus
extern "C" {
#endif

int vso_view_overlap_counts(const void *extrinsics, const void *intrinsics, int32_t dtype, int32_t V, int32_t H, int32_t W,
                            const int32_t *pairs, int32_t P, int32_t *counts, vs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VICASPLAT_OVERLAP_H */
