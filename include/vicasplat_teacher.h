/* vicasplat_teacher.h -- the distillation teacher's entries of libvicasplat_hip.so (csrc/teacher.hip): the tail that turns the raw output
 * of a four-channel pts3d DPT head into points and confidences.
 *
 * A fourth public header of the same library: vicasplat_hip.h and its ABI version are unchanged by it, and so are vicasplat_distill.h and
 * vicasplat_loss.h.  Its entries carry the prefix vst_; they report errors as the entries of vicasplat_hip.h do (a negative return and a
 * message behind the library's error call) and take the same stream type.
 *
 * vst_points_conf: heads/postprocess.py:46-56, 73-74 with the DUSt3R modes ('exp', -inf, inf) and ('exp', 1, inf), one streaming pass.
 *   raw [n, H, W, 4]: x, y, z, c per pixel, contiguous (pixel stride 4), f32 (raw_is_f16 == 0; 16-byte aligned) or f16 (raw_is_f16 != 0;
 *   8-byte aligned); transform [n, 3, 4] f32 rows of (R | t), one per image, or null; pts [n, H, W, 3] f32; conf [n, H, W] f32.
 *   d = |xyz|; p = xyz / max(d, 1e-8) * expm1(d); pts = R p + t with a transform, p without; conf = 1 + exp(c).
 *   The arithmetic is f64 on the f32 (or f16) inputs and rounds once, except that expm1(d) is +inf from where its f32 value is (d > 88.72):
 *   there a component is +-inf, or exactly 0 where the input component is 0 -- the reference's f32 result but for its 0 * inf, which is NaN
 *   there and 0 here.  The zero vector gives exactly zero.  A product of the transform with a zero factor is skipped, so a zero entry of R
 *   meets an infinite component without a NaN; infinite components of opposite sign under one row of R remain NaN.  conf is +inf from
 *   c > 88.72 on and 1 at c = -inf.  Asynchronous on `stream`; n * H * W is arbitrary.
 */
#ifndef VICASPLAT_TEACHER_H
#define VICASPLAT_TEACHER_H
#include "vicasplat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int vst_points_conf(const void *raw, int32_t raw_is_f16, const float *transform, int32_t n, int32_t H, int32_t W, float *pts, float *conf,
                    vs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VICASPLAT_TEACHER_H */
