/* vicasplat_loss.h -- the image-space loss entries of libvicasplat_hip.so (csrc/depth_loss.hip): the depth-smoothness loss.
 *
 * A third public header of the same library: vicasplat_hip.h and its ABI version are unchanged by it, and so is vicasplat_distill.h.  Its
 * entries carry the prefix vsl_; they report errors as the entries of vicasplat_hip.h do (a negative return and a message behind the
 * library's error call) and take the same stream type.
 *
 * LossDepth (src/loss/loss_depth.py:34-60), all f32, contiguous device memory, N = batch * views, H and W arbitrary:
 *   depth [N, H, W]; near, far [N]; image [N, 3, H, W] (the target colours) or null.
 *   ln = log(near), lf = log(far), once per view; d = (max(min(depth, lf), ln) - ln) / (lf - ln): the minimum first, the log on near and
 *   far only, as the reference has it.  A NaN depth stays NaN (torch.minimum / torch.maximum).
 *   dx = diff(d, W), dy = diff(d, H); use_second_derivative != 0: each differenced once more along its own axis (s = 1, else s = 0).
 *   image given: cx = max over the three channels of the SIGNED diff(image, W) (with s = 1: cx[j] = max(cx[j + 1], cx[j])), cy the same
 *   along H; dx *= exp(-cx * sigma_image), dy *= exp(-cy * sigma_image).  image null: no weights, sigma_image is not read.
 *   loss = weight * (sum |dx| / (N H (W - 1 - s)) + sum |dy| / (N (H - 1 - s) W)).
 *   H or W below 2 + s leaves a mean empty (torch: NaN); here it is an error.
 *   Every reduction has two stages in a fixed order and there are no float atomics: the same inputs give the same bits.
 *
 * vsl_depth_smooth_workspace_bytes(N, H, W): bytes of device workspace of one forward (8 per view + 8 per 16 x 64 pixel tile).
 * vsl_depth_smooth_forward: writes *loss (device f32 scalar) and, when d_depth_unit is not null, d loss / d depth [N, H, W] for an upstream
 *   gradient of 1, in the same pass over the inputs.  Subgradients are torch's: 0 for |.| at 0; one half where depth equals log(far) or
 *   log(near) bit for bit; near, far and image carry no gradient.  Asynchronous on `stream`: no host synchronisation.
 * vsl_depth_smooth_backward: d_depth [N, H, W] = grad_loss[0] * d_depth_unit (grad_loss: device f32 scalar; d_depth may be d_depth_unit
 *   itself).  Asynchronous on `stream`.
 */
#ifndef VICASPLAT_LOSS_H
#define VICASPLAT_LOSS_H
#include "vicasplat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t vsl_depth_smooth_workspace_bytes(int32_t N, int32_t H, int32_t W);
int vsl_depth_smooth_forward(const float *depth, const float *near, const float *far, const float *image, int32_t N, int32_t H, int32_t W,
                             float sigma_image, int32_t use_second_derivative, float weight, void *workspace, int64_t workspace_bytes,
                             float *loss, float *d_depth_unit, vs_stream_t stream);
int vsl_depth_smooth_backward(const float *d_depth_unit, const float *grad_loss, int32_t N, int32_t H, int32_t W, float *d_depth,
                              vs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VICASPLAT_LOSS_H */
