"""Harness for the callers either side of the hot path.

What is here runs on the HIP rasterizer through `DecoderSplattingCUDA` and is what the reference's evaluation and demo
scripts do around the encoder/decoder:
  * `mse_loss`                — LossMse.forward, src/loss/loss_mse.py:23-31
  * `compute_psnr`            — src/evaluation/metrics.py:21-29
  * `compute_ssim`            — src/evaluation/metrics.py:46-62 (skimage structural_similarity, per image) on the HIP SSIM kernels
  * `ssim`                    — src/loss/loss_ssim.py:129-190 (the differentiable SSIM of pose_evaluator.py:136-141; `_ssim` :58-126)
  * `se3_exp`, `update_pose`  — src/misc/cam_utils.py:59-142 (batched, no per-camera Python loop)
  * `align_poses`             — ModelWrapper.test_step_align, src/model/model_wrapper.py:442-513
  * `export_ply`              — src/model/ply_export.py:31-90 (own binary writer, no plyfile dependency)
  * `export_transforms`       — src/model/model_wrapper.py:390-400 (transforms.json)
  * `load_images`             — demo.py:75-132 (resize short side to 256, centre crop, normalise to [-1, 1])
  * `inference`, `interpolate_extrinsics`, `interpolate_intrinsics`, `render_video_interpolation` — demo.py:180-243 with
    src/visualization/camera_trajectory/interpolation.py (the 70-view demo video: cameras share ONE Gaussian set)
  * `camera_loss`, `camera_dq_loss` — src/loss/loss_camera.py:30-80 (dual-quaternion algebra of src/misc/dq.py restated)
  * `LossLpips` — src/loss/loss_lpips.py:27-54 (published LPIPS-VGG algorithm; the pretrained weights must be supplied, see the class)
  * `LpipsVgg`, `compute_lpips` — lpips.LPIPS(net="vgg") and src/evaluation/metrics.py:37-44 on the HIP kernels (LossLpips(backend="hip"))
  * `Regr3D`, `distillation_loss` — src/loss/loss_conf_point.py:188-252 and the glue of model_wrapper.py:260-299 (training stage 1: the point loss
    against a DUSt3R teacher's outputs) on csrc/distill.hip; `training_step(distill=...)` applies it
  * `sample_anchor_frames`, `distill_targets` — model_wrapper.py:153-182, 248-271: the anchor frames of a step and the teacher's targets for it,
    from vicasplat_amd.model.distiller (the DUSt3R two-view network on the HIP kernels; its tail is csrc/teacher.hip)
  * `LossDepth`, `depth_smoothness_loss` — src/loss/loss_depth.py:26-60 (edge-aware first / second differences of the rendered depth between
    log(near) and log(far)) on csrc/depth_loss.hip; plugs into `training_step(extra_losses=[...])` and drives the rasterizer's dL_ddepth
  * `camera_eval_metrics` — src/evaluation/metrics.py:148-265 (ATE, RPE-trans, RPE-rot: evo's ape / rpe restated, UNVERIFIED against evo) on
    csrc/trajectory.hip, batched over scenes, device tensors out
  * `test_step` — ModelWrapper.test_step, src/model/model_wrapper.py:323-381: the six numbers it logs, per scene, batched
  * `save_test_outputs` — the file output of ModelWrapper.test_step, model_wrapper.py:386-407: context frames, transforms.json and the rendered
    targets beside their depth maps as PNG files made on the device (misc/image_io.py, csrc/png.hip), one encoder call per frame shape
  * `pose_eval_step` — PoseEvaluator.test_step, src/evaluation/pose_evaluator.py:77-174: the pose metrics before and after refinement
  * `render_video_wobble_step`, `render_video_interpolation_exaggerated_step`, `camera_trajectory_plot` — model_wrapper.py:685-707, 733-773 and
    the stated substitute for the plotly camera figure of :668-679, on csrc/draw.hip (visualization/drawing, camera_trajectory/wobble.py)
  * `validation_step`, `render_video_generic`, `render_video_interpolation_step`, `depth_video_frames` — ModelWrapper.validation_step and
    render_video_generic / render_video_interpolation (model_wrapper.py:524-704, 710-730, 776-815): metrics, the comparison image, the
    projections and the uint8 video frames as device tensors, on csrc/viz.hip (depth range, colour maps, frames)
  * `configure_optimizer`, `training_step` — ModelWrapper.configure_optimizers / training_step (model_wrapper.py:884-951,
    184-321): AdamW(lr, wd 0.05, betas 0.9/0.95) with the backbone-lr multiplier, encoder -> rasterizer -> MSE ->
    backward on the HIP kernels (vicasplat_amd.autograd) -> optional gradient all-reduce -> clip 0.5 -> step.
"""
from __future__ import annotations

import json
import math
from pathlib import Path

import numpy as np
import torch
from torch import Tensor

from .model.types import Gaussians


def mse_loss(color: Tensor, target: Tensor, weight: float = 1.0) -> Tensor:
    return weight * ((color - target) ** 2).mean()


@torch.no_grad()
def compute_psnr(ground_truth: Tensor, predicted: Tensor) -> Tensor:
    gt = ground_truth.clip(0, 1)
    pr = predicted.clip(0, 1)
    return -10 * ((gt - pr) ** 2).flatten(1).mean(1).log10()


def _gaussian_taps_f64(sigma: float, radius: int) -> list[float]:
    """Taps of scipy.ndimage.gaussian_filter (what skimage's gaussian_weights uses): exp(-x^2 / (2 sigma^2)), x = -radius..radius, sum 1."""
    x = np.arange(-radius, radius + 1, dtype=np.float64)
    g = np.exp(-0.5 / (sigma * sigma) * x * x)
    return (g / g.sum()).tolist()


_SSIM_METRIC_TAPS = _gaussian_taps_f64(1.5, int(3.5 * 1.5 + 0.5))     # sigma 1.5, truncate 3.5: radius 5, 11 taps


@torch.no_grad()
def compute_ssim(ground_truth: Tensor, predicted: Tensor) -> Tensor:
    """SSIM per image of [batch, channel, h, w] tensors: skimage structural_similarity(gt, hat, win_size=11, gaussian_weights=True,
    channel_axis=0, data_range=1.0), as metrics.py:46-62 applies it, without the host round trip: one HIP forward over every plane
    (vs_ssim_forward; sample covariances, cov_norm = 121 / 120; the map mean over the 5-pixel-cropped interior, averaged over channels).
    No clipping of the inputs.  Returns a device tensor [batch] of predicted.dtype; no host synchronisation."""
    from . import ops
    if ground_truth.shape != predicted.shape or predicted.dim() != 4:
        raise ValueError(f"compute_ssim takes two [batch, channel, h, w] tensors of one shape, got {tuple(ground_truth.shape)} "
                         f"and {tuple(predicted.shape)}")
    if min(predicted.shape[-2:]) < 11:
        raise ValueError(f"win_size exceeds image extent: an image of {tuple(predicted.shape[-2:])} is smaller than the 11 x 11 window")
    _, per_image = ops.ssim_forward(ground_truth, predicted, _SSIM_METRIC_TAPS, 121.0 / 120.0, 0.01 ** 2, 0.03 ** 2,
                                     unit_window=True)
    return per_image[0].to(predicted.dtype)


def _fspecial_gauss_1d(size: int, sigma: float) -> Tensor:
    """The loss window of loss_ssim.py:12-26, in float32 on the host (the same float32 operations, so the same taps)."""
    coords = torch.arange(size, dtype=torch.float) - size // 2
    g = torch.exp(-(coords ** 2) / (2 * sigma ** 2))
    return g / g.sum()


def ssim(X: Tensor, Y: Tensor, data_range: float = 255, size_average: bool = True, win_size: int = 11, win_sigma: float = 1.5,
         win: Tensor | None = None, K=(0.01, 0.03), nonnegative_ssim: bool = False, retrun_seprate: bool = False):
    """The SSIM loss of loss_ssim.py:129-190 (keyword names included) on the HIP kernels: valid convolution with the 1-D Gaussian window,
    no covariance correction.  Returns (ssim, brightness, contrast, structure): scalars with size_average, else per-image [N] means over
    channels; the last three are zeros unless retrun_seprate.  Differentiable in X and Y through ssim and structure (autograd.SsimFn);
    brightness and contrast are not.  A caller-supplied `win` is one 1-D window (its first row if it holds one per channel).  [N, C, H, W]
    inputs only, H and W >= win_size."""
    from . import autograd as A
    if X.shape != Y.shape:
        raise ValueError(f"Input images should have the same dimensions, but got {X.shape} and {Y.shape}.")
    for d in range(X.dim() - 1, 1, -1):
        X, Y = X.squeeze(dim=d), Y.squeeze(dim=d)
    if X.dim() != 4:
        raise ValueError(f"Input images should be 4-d tensors [N, C, H, W] (5-d inputs are not supported), but got {X.shape}")
    if win is not None:
        win_size = win.shape[-1]
    if win_size % 2 != 1:
        raise ValueError("Window size should be odd.")
    if min(X.shape[-2:]) < win_size:
        raise ValueError(f"SSIM needs images of at least {win_size} x {win_size}, got {tuple(X.shape[-2:])}")
    taps = (_fspecial_gauss_1d(win_size, win_sigma) if win is None else win.detach().reshape(-1, win_size)[0].float().cpu()).tolist()
    K1, K2 = K
    s, b, c, t = A.SsimFn.apply(X, Y, tuple(taps), (K1 * data_range) ** 2, (K2 * data_range) ** 2, bool(retrun_seprate))
    if nonnegative_ssim:
        s = torch.relu(s)
    out = (s, b, c, t) if not X.is_floating_point() else tuple(v.to(X.dtype) for v in (s, b, c, t))
    return tuple(v.mean() for v in out) if size_average else tuple(v.mean(1) for v in out)


def _skew(w: Tensor) -> Tensor:
    z = torch.zeros_like(w[..., 0])
    return torch.stack([z, -w[..., 2], w[..., 1], w[..., 2], z, -w[..., 0], -w[..., 1], w[..., 0], z], -1).unflatten(-1, (3, 3))


def se3_exp(tau: Tensor) -> Tensor:
    """tau [..., 6] = (rho, theta) -> 4x4; small-angle series below 1e-5 rad exactly as cam_utils.py:70-115."""
    rho, theta = tau[..., :3], tau[..., 3:]
    W = _skew(theta)
    W2 = W @ W
    angle = theta.norm(dim=-1)[..., None, None]
    small = angle < 1e-5
    a = torch.where(small, torch.ones_like(angle), angle)
    eye = torch.eye(3, dtype=tau.dtype, device=tau.device).expand_as(W)
    Rm = torch.where(small, eye + W + 0.5 * W2, eye + (torch.sin(a) / a) * W + ((1 - torch.cos(a)) / a**2) * W2)
    Vm = torch.where(small, eye + 0.5 * W + W2 / 6.0, eye + W * ((1 - torch.cos(a)) / a**2) + W2 * ((a - torch.sin(a)) / a**3))
    T = torch.zeros(*tau.shape[:-1], 4, 4, dtype=tau.dtype, device=tau.device)
    T[..., :3, :3] = Rm
    T[..., :3, 3] = (Vm @ rho[..., None])[..., 0]
    T[..., 3, 3] = 1
    return T


def update_pose(cam_trans_delta: Tensor, cam_rot_delta: Tensor, extrinsics: Tensor) -> Tensor:
    """c2w' = (Exp([trans, rot]) · w2c)^-1   (cam_utils.py:118-137)."""
    tau = torch.cat([cam_trans_delta, cam_rot_delta], dim=-1)
    return (se3_exp(tau) @ extrinsics.inverse()).inverse()


def align_poses(decoder, gaussians, target_image: Tensor, extrinsics: Tensor, intrinsics: Tensor, near: Tensor, far: Tensor,
                steps: int = 100, rot_lr: float = 0.005, trans_lr: float = 0.005, mse_weight: float = 1.0,
                return_history: bool = False, ssim_structure_weight: float = 0.0):
    """Test-time pose alignment: Adam on per-camera twist deltas through the rasterizer's camera-Jacobian backward,
    folding the delta into the extrinsics after every step (model_wrapper.py:442-513).
    target_image [b,v,3,h,w]; extrinsics [b,v,4,4] c2w. Returns the refined extrinsics (and the loss history).
    ssim_structure_weight w != 0 adds w * (1 - structure) of ssim(target, render, data_range=1.0, retrun_seprate=True) to every step's
    loss, the structure term of pose_evaluator.py:136-141 (off by default, as that loop ships with number_steps = 0)."""
    b, v, _, h, w = target_image.shape
    dev = target_image.device
    gaussians = Gaussians(gaussians.means.detach(), gaussians.covariances.detach(), gaussians.harmonics.detach(),
                          gaussians.opacities.detach())
    rot = torch.nn.Parameter(torch.zeros(b, v, 3, device=dev))
    trans = torch.nn.Parameter(torch.zeros(b, v, 3, device=dev))
    from . import raster
    ext0 = extrinsics.clone()

    def run(sync_free: bool):
        """All steps of the alignment from the initial poses.  sync_free: after the first (exact) render the steps run in the capacity
        mode; the overflow flags of ALL rasterizer calls of a step are accumulated on the device (raster.CapacityScope) and read once
        at the end."""
        extr, history, flags, cap = ext0.clone(), [], [], None
        with torch.no_grad():
            rot.zero_(); trans.zero_()
        with torch.enable_grad():
            for it in range(steps):
                opt_.zero_grad()
                # the first render runs in the exact mode and tells how many (Gaussian, tile) instances these cameras produce; the others
                # run without the per-call host synchronisation, in buffers 1.5x that size (the poses move by millimetres per step)
                with raster.instance_capacity(cap if (sync_free and it > 0) else None) as scope:
                    out = decoder.forward(gaussians, extr, intrinsics, near, far, (h, w), cam_rot_delta=rot, cam_trans_delta=trans)
                if sync_free and scope.calls:
                    if it == 0:
                        cap = int(max(r for r, _ in scope.calls) * 1.5) + 65536
                    else:
                        flags.append(scope.overflow_flag())
                loss = mse_loss(out.color, target_image, mse_weight)
                if ssim_structure_weight != 0.0:
                    structure = ssim(target_image.flatten(0, 1), out.color.flatten(0, 1), size_average=True, data_range=1.0,
                                     retrun_seprate=True, win_size=11)[3]
                    loss = loss + ssim_structure_weight * (1 - structure)
                loss.backward()
                history.append(loss.detach())
                with torch.no_grad():
                    opt_.step()
                    extr = update_pose(trans.flatten(0, 1), rot.flatten(0, 1), extr.flatten(0, 1)).unflatten(0, (b, v))
                    rot.zero_()
                    trans.zero_()
        return extr, history, (bool(torch.stack(flags).max().item() != 0) if flags else False)

    opt_ = torch.optim.Adam([{"params": [rot], "lr": rot_lr}, {"params": [trans], "lr": trans_lr}])
    extrinsics, history, overflowed = run(True)
    if overflowed:      # some step outgrew the buffers (its render was empty): repeat with exact sizing (fresh optimizer state)
        opt_ = torch.optim.Adam([{"params": [rot], "lr": rot_lr}, {"params": [trans], "lr": trans_lr}])
        extrinsics, history, _ = run(False)
    return (extrinsics, torch.stack(history)) if return_history else extrinsics


def _ply_attributes(num_rest: int) -> list[str]:
    names = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"]
    names += [f"f_rest_{i}" for i in range(num_rest)]
    names += ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
    return names


def export_ply(means: Tensor, scales: Tensor, rotations: Tensor, harmonics: Tensor, opacities: Tensor, path,
               save_sh_dc_only: bool = False) -> int:
    """3DGS-compatible binary PLY: pruned at opacity < 0.005, sorted by opacity (descending), opacity as a logit, scales
    as logs, rotation xyzw -> unit wxyz (ply_export.py:31-90; the vertex table is checked against the reference's own in
    tests/test_callers_cpu.py). Returns the number of vertices written."""
    mask = opacities >= 0.005
    op, idx = torch.sort(opacities[mask], descending=True)
    means, scales, rotations, harmonics = (t[mask][idx] for t in (means, scales, rotations, harmonics))
    q = rotations / rotations.norm(dim=-1, keepdim=True)
    # the reference round-trips the quaternion through a rotation matrix (scipy, ply_export.py:52-55), which fixes its sign: the
    # component of largest magnitude comes back positive
    lead = torch.gather(q, 1, q.abs().argmax(dim=1, keepdim=True))
    q = q * torch.where(lead < 0, -torch.ones_like(lead), torch.ones_like(lead))
    q = torch.cat([q[:, 3:], q[:, :3]], dim=-1)
    f_dc = harmonics[..., 0]
    f_rest = harmonics[..., 1:].flatten(1)
    cols = [means, torch.zeros_like(means), f_dc]
    if not save_sh_dc_only:
        cols.append(f_rest)
    cols += [torch.log(op / (1 - op))[:, None], scales.log(), q]
    table = torch.cat([c.detach().float().cpu() for c in cols], dim=1).numpy().astype("<f4")
    names = _ply_attributes(0 if save_sh_dc_only else f_rest.shape[1])
    assert table.shape[1] == len(names)
    path = Path(path)
    path.parent.mkdir(exist_ok=True, parents=True)
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % table.shape[0]
    header += "".join(f"property float {n}\n" for n in names) + "end_header\n"
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(np.ascontiguousarray(table).tobytes())
    return table.shape[0]


def read_ply(path) -> dict[str, np.ndarray]:
    """Reader for the files `export_ply` writes (round-trip tests)."""
    with open(path, "rb") as f:
        names, n = [], 0
        while True:
            line = f.readline().decode("ascii").strip()
            if line.startswith("element vertex"):
                n = int(line.split()[-1])
            elif line.startswith("property float"):
                names.append(line.split()[-1])
            elif line == "end_header":
                break
        table = np.frombuffer(f.read(), dtype="<f4").reshape(n, len(names))
    return {k: table[:, i] for i, k in enumerate(names)}


def export_transforms(extrinsics: Tensor, path, file_names: list[str] | None = None) -> None:
    """transforms.json: a list of `{file_path, transform_matrix}` (4x4 c2w) per context frame (model_wrapper.py:390-400)."""
    ext = extrinsics.detach().float().cpu().reshape(-1, 4, 4)
    frames = [{"file_path": file_names[i] if file_names else f"context/{i:0>6}.png", "transform_matrix": ext[i].tolist()}
              for i in range(ext.shape[0])]
    path = Path(path)
    path.parent.mkdir(exist_ok=True, parents=True)
    with open(path, "w") as f:
        json.dump(frames, f, indent=4)


_IMAGE_EXT = (".jpg", ".jpeg", ".png")


def load_images(folder_or_list, size: int = 256) -> Tensor:
    """Demo pre-processing (demo.py:75-132): EXIF-upright RGB, short side resized to `size` (Lanczos when shrinking,
    bicubic when enlarging), centre square crop, then (x/255 - 0.5) / 0.5.  Returns [V, 3, size, size] f32, files in
    name order.  Host-side (PIL); the frames go to the GPU with the batch."""
    import os
    from PIL import Image, ImageOps
    if isinstance(folder_or_list, (str, os.PathLike)):
        root = os.fspath(folder_or_list)
        paths = [os.path.join(root, f) for f in sorted(os.listdir(root))]
    else:
        paths = sorted((os.fspath(f) for f in folder_or_list), key=lambda f: f.split("/")[-1])
    frames = []
    for path in paths:
        if not path.lower().endswith(_IMAGE_EXT):
            continue
        img = ImageOps.exif_transpose(Image.open(path)).convert("RGB")
        w, h = img.size
        long_edge = round(size * max(w / h, h / w))   # short side -> size
        big = max(w, h)
        interp = Image.LANCZOS if big > long_edge else Image.BICUBIC
        img = img.resize((int(round(w * long_edge / big)), int(round(h * long_edge / big))), interp)
        w, h = img.size
        cx, cy = w // 2, h // 2
        half = min(cx, cy)
        img = img.crop((cx - half, cy - half, cx + half, cy + half))
        x = torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).float() / 255.0
        frames.append((x - 0.5) / 0.5)
    if not frames:
        raise FileNotFoundError(f"no .jpg/.jpeg/.png images in {folder_or_list!r}")
    return torch.stack(frames, 0)


# ---------------------------------------------------------------------------------------------------------------------------
# demo video path (demo.py:180-243): cameras interpolated between consecutive predicted poses, ALL of them rendered from the one
# shared Gaussian set in a single batched rasterizer call (the rasterizer's shared-Gaussian mode, cam_scene = 0)
# ---------------------------------------------------------------------------------------------------------------------------
def interpolate_intrinsics(initial: Tensor, final: Tensor, t: Tensor) -> Tensor:
    """[...,3,3] x2, t [S] -> [...,S,3,3] linear blend (visualization/camera_trajectory/interpolation.py:8-16)."""
    return initial[..., None, :, :] + (final - initial)[..., None, :, :] * t[:, None, None]


def _frame_yz(y: Tensor, z: Tensor) -> Tensor:
    return torch.stack([torch.linalg.cross(y, z, dim=-1), y, z], dim=-1)   # columns (y x z, y, z)


def _euler_yxz(R: Tensor):
    """R = Ry(a) Rx(b) Rz(c) (intrinsic Y-X-Z, what scipy's as_euler('YXZ') returns) -> (a, b, c)."""
    return torch.atan2(R[..., 0, 2], R[..., 2, 2]), torch.asin((-R[..., 1, 2]).clamp(-1, 1)), torch.atan2(R[..., 1, 0], R[..., 1, 1])


def _blend_angle(a: Tensor, b: Tensor, t: Tensor) -> Tensor:
    """Shortest-arc interpolation of angles taken mod 2 pi (interpolation.py:163-188)."""
    tau = 2 * math.pi
    a, b = a % tau, b % tau
    d0, dl, dr = (b - a).abs(), (b - (a - tau)).abs(), (b - (a + tau)).abs()
    use0 = (d0 < dl) & (d0 < dr)
    usel = (dl < dr) & ~use0
    a = torch.where(use0, a, torch.where(usel, a - tau, a + tau))
    return a + (b - a) * t


@torch.no_grad()
def interpolate_extrinsics(initial: Tensor, final: Tensor, t: Tensor, eps: float = 1e-4) -> Tensor:
    """c2w [N,4,4] x2, t [S] -> [N,S,4,4]: every pair is interpolated by rotating about its "focus point" -- the least-squares
    intersection of the two look rays, or the midpoint of the origins when the look vectors are parallel -- in the 5-parameter
    pivot form (3 offsets in the frame (pivot axis x look, pivot axis, look), in-plane angle, twist); the out-of-plane Euler angle
    is dropped on the way back (interpolation.py:208-259, float64 inside like the reference)."""
    A, B, t = initial.double(), final.double(), t.double()
    la, lb = A[..., :3, 2], B[..., :3, 2]
    oa, ob = A[..., :3, 3], B[..., :3, 3]
    par = ((la * lb).sum(-1).abs() - 1).abs() < eps
    eye = torch.eye(3, dtype=torch.float64, device=A.device)
    Na, Nb = la[..., :, None] * la[..., None, :] - eye, lb[..., :, None] * lb[..., None, :] - eye
    lhs, rhs = Na + Nb, (Na @ oa[..., None] + Nb @ ob[..., None])[..., 0]
    lhs = torch.where(par[..., None, None], eye.expand_as(lhs), lhs)                # (unused rows: keep the solve well-posed)
    pivot = torch.where(par[..., None], 0.5 * (oa + ob), torch.linalg.lstsq(lhs, rhs[..., None]).solution[..., 0])
    # pivot frame: Y normal to the plane of the two look vectors; a look vector parallel to the other is replaced by z, then y
    b2 = lb.clone()
    for alt in ((0.0, 0.0, 1.0), (0.0, 1.0, 0.0)):
        p_ = ((la * b2).sum(-1).abs() - 1).abs() < eps
        b2 = torch.where(p_[..., None], b2.new_tensor(alt).expand_as(b2), b2)
    n = torch.linalg.cross(la, b2, dim=-1)
    F = _frame_yz(n / n.norm(dim=-1, keepdim=True), la)
    axis = F[..., :, 1]

    def to_params(E):
        tf = _frame_yz(axis, E[..., :3, 2])
        tr = (tf * (pivot - E[..., :3, 3])[..., :, None]).sum(-2)
        y, _, z = _euler_yxz(torch.linalg.inv(F) @ E[..., :3, :3])
        return tr, y, z

    ta, ya, za = to_params(A)
    tb, yb, zb = to_params(B)
    tt = t[:, None]
    tr = ta[..., None, :] + (tb - ta)[..., None, :] * tt
    y, z = _blend_angle(ya[..., None], yb[..., None], t), _blend_angle(za[..., None], zb[..., None], t)
    # back to matrices in float32 (the reference converts the parameters to f32 first)
    tr, y, z, F32, piv = tr.float(), y.float(), z.float(), F.float()[..., None, :, :], pivot.float()[..., None, :]
    cy, sy, cz, sz = y.cos(), y.sin(), z.cos(), z.sin()
    o, l = torch.zeros_like(y), torch.ones_like(y)
    Ry = torch.stack([cy, o, sy, o, l, o, -sy, o, cy], -1).unflatten(-1, (3, 3))
    Rz = torch.stack([cz, -sz, o, sz, cz, o, o, o, l], -1).unflatten(-1, (3, 3))
    Rm = F32 @ (Ry @ Rz)
    tf = _frame_yz(F32[..., :, 1].expand_as(Rm[..., :, 2]), Rm[..., :, 2])
    origin = piv - (tf @ tr[..., None])[..., 0]
    out = torch.eye(4, dtype=torch.float32, device=A.device).repeat(*origin.shape[:-1], 1, 1)
    out[..., :3, :3] = Rm
    out[..., :3, 3] = origin
    return out


@torch.no_grad()
def inference(model, imgs: Tensor, fovx_deg: float | None = None, fovy_deg: float | None = None) -> dict:
    """demo.py:180-202: imgs [1,V,3,H,W] in [-1,1] (load_images) -> Gaussians, points, c2w poses, intrinsics; the intrinsic embedding is
    fed the pinhole K of the given field of view (cam_utils.py:220-234) when the backbone uses it."""
    inputs = {"image": imgs}
    intr = None
    if model.backbone.config.use_intrinsic_embedding:
        assert (fovx_deg or 0) > 0 or (fovy_deg or 0) > 0, "need to provide valid fovx and fovy"
        fx = math.radians(fovx_deg) if (fovx_deg or 0) > 0 else None
        fy = math.radians(fovy_deg) if (fovy_deg or 0) > 0 else None
        fov = (fx or fy, fy or fx)
        intr = torch.eye(3, device=imgs.device)
        intr[0, 0], intr[1, 1] = 0.5 / math.tan(0.5 * fov[0]), 0.5 / math.tan(0.5 * fov[1])
        intr[0, 2] = intr[1, 2] = 0.5
        intr = intr[None]
        inputs["intrinsics"] = intr[None].expand(imgs.shape[0], imgs.shape[1], 3, 3).contiguous()
    out = model(inputs, compute_viewspace_depth=False)
    return dict(imgs=imgs * 0.5 + 0.5, gaussians=out["gaussians"], pts3d=out["gaussian_centers"], camera_poses=out["gaussian_camera_extrins"],
                camera_intrins=out["gaussian_camera_intrins"] if intr is None else intr)


@torch.no_grad()
def render_video_interpolation(gaussians, camera_poses: Tensor, camera_intrins: Tensor, n_interp_per_interv: int = 10, near: float = 0.01,
                               far: float = 100.0, image_shape=(256, 256)) -> Tensor:
    """demo.py:204-243: camera_poses [V,4,4] c2w, camera_intrins [V,3,3] | [1,3,3] -> frames [2 * (V-1) * n, 3, H, W] (forward pass of
    the path followed by its reverse).  The (V-1) * n cameras share ONE Gaussian set: one batched rasterizer call, no replication."""
    from .model.decoder.cuda_splatting import render_cuda
    dev = camera_poses.device
    if camera_intrins.shape[0] == 1:
        camera_intrins = camera_intrins.expand(camera_poses.shape[0], 3, 3)
    t = torch.linspace(0, 1, n_interp_per_interv, dtype=torch.float32, device=dev)
    E = interpolate_extrinsics(camera_poses[:-1], camera_poses[1:], t).reshape(-1, 4, 4)
    K = interpolate_intrinsics(camera_intrins[:-1].float(), camera_intrins[1:].float(), t).reshape(-1, 3, 3)
    v = E.shape[0]
    images, _depth = render_cuda(E, K, torch.full((v,), near, device=dev), torch.full((v,), far, device=dev), image_shape,
                                 torch.zeros(v, 3, device=dev), gaussians.means.reshape(-1, 3), gaussians.covariances.reshape(-1, 3, 3),
                                 gaussians.harmonics.reshape(-1, *gaussians.harmonics.shape[-2:]), gaussians.opacities.reshape(-1),
                                 scale_invariant=False)
    return torch.cat([images, images.flip(dims=(0,))], dim=0)


def configure_optimizer(encoder, lr: float = 4e-5, backbone_lr_multiplier: float = 0.25,
                        new_param_keywords=("gaussian_param_head", "intrinsic_encoder"), weight_decay: float = 0.05, warm_up_steps: int = 0,
                        lr_cosine_annealing: bool = False, max_steps: int | None = None):
    """AdamW with the reference's two learning-rate groups (model_wrapper.py:884-951): parameters whose name contains one of
    `new_param_keywords` train at `lr`, the pretrained rest at `lr * backbone_lr_multiplier` (every released experiment sets
    new_param_keywords = [gaussian_param_head, intrinsic_encoder]: config/experiment/re10k_*.yaml; distillation passes None -> one
    group at `lr`).  Schedule: LinearLR warm-up (1/warm_up_steps -> 1), then -- `lr_cosine_annealing` (2- and 4-view configs) --
    CosineAnnealingLR(T_max=max_steps, eta_min=0.1 * lr) chained with SequentialLR at the warm-up milestone (:930-935)."""
    new, old = [], []
    kws = tuple(new_param_keywords or ())
    for name, p in encoder.named_parameters():
        if p.requires_grad:
            (new if any(k in name for k in kws) else old).append(p)
    groups = [dict(params=new, lr=lr), dict(params=old, lr=lr * backbone_lr_multiplier)] if new else [dict(params=old, lr=lr)]
    kw = dict(lr=lr, weight_decay=weight_decay, betas=(0.9, 0.95))
    opt = None
    if old and old[0].is_cuda:
        try:   # one multi-tensor kernel per step instead of ~10 foreach passes over the 578 M parameters
            opt = torch.optim.AdamW(groups, fused=True, **kw)
        except (RuntimeError, TypeError, ValueError):
            opt = None
    if opt is None:
        opt = torch.optim.AdamW(groups, **kw)
    sched = torch.optim.lr_scheduler.LinearLR(opt, 1 / warm_up_steps, 1, total_iters=warm_up_steps) if warm_up_steps > 0 else None
    if lr_cosine_annealing:
        if max_steps is None:
            raise ValueError("lr_cosine_annealing needs max_steps (trainer.max_steps of the experiment)")
        cos = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=max_steps, eta_min=lr * 0.1)
        sched = cos if sched is None else torch.optim.lr_scheduler.SequentialLR(opt, schedulers=[sched, cos], milestones=[warm_up_steps])
    return opt, sched


# ---------------------------------------------------------------------------------------------------------------------------
# camera (dual-quaternion) loss -- src/loss/loss_camera.py:30-80 with the quaternion algebra of src/misc/dq.py (pypose's SO3 product
# / inverse restated on xyzw tensors) and pytorch3d's matrix_to_quaternion (restated: the best-conditioned of the four candidates)
# ---------------------------------------------------------------------------------------------------------------------------
def quat_mul_xyzw(a: Tensor, b: Tensor) -> Tensor:
    x1, y1, z1, w1 = a.unbind(-1)
    x2, y2, z2, w2 = b.unbind(-1)
    return torch.stack([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                        w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2], -1)


def quat_conj_xyzw(q: Tensor) -> Tensor:
    return q * q.new_tensor([-1.0, -1.0, -1.0, 1.0])


def matrix_to_quaternion_wxyz(R: Tensor) -> Tensor:
    """[...,3,3] rotation -> [...,4] quaternion (real part first), the candidate with the largest denominator of the four
    square-root forms (what cam_utils.py:200-201 gets from pytorch3d.transforms.matrix_to_quaternion before normalising)."""
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = R.flatten(-2).unbind(-1)
    q_abs = torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22], -1)
    q_abs = torch.where(q_abs > 0, q_abs.clamp_min(0).sqrt(), torch.zeros_like(q_abs))
    cand = torch.stack([
        torch.stack([q_abs[..., 0] ** 2, m21 - m12, m02 - m20, m10 - m01], -1),
        torch.stack([m21 - m12, q_abs[..., 1] ** 2, m10 + m01, m02 + m20], -1),
        torch.stack([m02 - m20, m10 + m01, q_abs[..., 2] ** 2, m12 + m21], -1),
        torch.stack([m10 - m01, m20 + m02, m21 + m12, q_abs[..., 3] ** 2], -1)], -2)
    cand = cand / (2.0 * q_abs[..., None].clamp_min(0.1))
    best = q_abs.argmax(-1)
    q = torch.gather(cand, -2, best[..., None, None].expand(*best.shape, 1, 4))[..., 0, :]
    # standardize_quaternion (pytorch3d main applies it at the end of matrix_to_quaternion): the representative with a non-negative real
    # part -- the L1 / dual-quaternion losses are sign-sensitive and the pose head predicts w ~ +1
    return torch.where(q[..., :1] < 0, -q, q)


def camera_dq_array_from_Rt(R: Tensor, t: Tensor) -> Tensor:
    """(R [...,3,3], t [...,3]) -> dual quaternion [...,8] = (q_r xyzw | q_d xyzw), q_d = 0.5 (t, 0) (x) q_r
    (cam_utils.py:213-218, dq.py:114-129)."""
    q = torch.nn.functional.normalize(matrix_to_quaternion_wxyz(R), dim=-1)[..., [1, 2, 3, 0]]
    q = q / q.norm(dim=-1, keepdim=True)
    qd = quat_mul_xyzw(0.5 * torch.cat([t, torch.zeros_like(t[..., :1])], -1), q)
    return torch.cat([q, qd], -1)


def dq_mul(a: Tensor, b: Tensor) -> Tensor:
    """(r1 + e d1)(r2 + e d2) = r1 r2 + e (r1 d2 + d1 r2)   (dq.py:38-41)."""
    return torch.cat([quat_mul_xyzw(a[..., :4], b[..., :4]),
                      quat_mul_xyzw(a[..., :4], b[..., 4:]) + quat_mul_xyzw(a[..., 4:], b[..., :4])], -1)


def dq_conj(a: Tensor) -> Tensor:
    return torch.cat([quat_conj_xyzw(a[..., :4]), quat_conj_xyzw(a[..., 4:])], -1)


def camera_dq_loss(prediction: Tensor, target: Tensor) -> Tensor:
    """L1(pred (x) target*, identity) + L1(target (x) pred*, identity)   (loss_camera.py:30-45)."""
    ident = torch.zeros_like(prediction)
    ident[..., 3] = 1.0
    return (dq_mul(prediction, dq_conj(target)) - ident).abs().mean() + (dq_mul(target, dq_conj(prediction)) - ident).abs().mean()


def camera_loss(pred_extrins: Tensor, context_extrinsics: Tensor, weight: float = 1.0, use_dq_loss: bool = True,
                pred_intrins: Tensor | None = None, context_intrinsics: Tensor | None = None) -> Tensor:
    """LossCamera.forward for camera_type 'dq' (loss_camera.py:47-80): pred_extrins [B,V-1,8] against the dual quaternions of the
    context cameras 1.. (c2w [B,V,4,4], already expressed in frame 0); with a fov head (the *_no_intrin configurations: pred_intrins
    [B,2]) the reference adds l2(pred_intrins, get_fov(mean over views of the context intrinsics)) (:76-79)."""
    E = context_extrinsics[:, 1:]
    tgt = camera_dq_array_from_Rt(E[..., :3, :3], E[..., :3, 3])
    l1 = (pred_extrins - tgt).abs().mean()
    loss = (camera_dq_loss(pred_extrins, tgt) + l1) if use_dq_loss else l1
    if pred_intrins is not None:
        if context_intrinsics is None:
            raise ValueError("camera_loss: a fov head (pred_intrins) needs the context intrinsics for its target")
        from .geometry.projection import get_fov
        loss = loss + ((pred_intrins - get_fov(context_intrinsics.float().mean(dim=1))) ** 2).mean()
    return weight * loss


# ---------------------------------------------------------------------------------------------------------------------------
# LPIPS(VGG) -- src/loss/loss_lpips.py:27-54.  The reference instantiates `lpips.LPIPS(net="vgg")` (un-vendored pip package, pretrained
# VGG-16 + learned linear heads downloaded at construction): neither the package nor its weights exist offline, so the published
# algorithm is restated here and the WEIGHTS must be supplied -- `torch.save(lpips.LPIPS(net="vgg").state_dict(), path)` on a machine that
# has them.  Without weights the constructor raises; nothing is silently substituted.  backend="torch" (the default) runs the loss network
# on PyTorch convolutions; backend="hip" runs the same definition on LpipsVgg (split-class convolutions + csrc/lpips.hip).
# ---------------------------------------------------------------------------------------------------------------------------
# STATUS: UNVERIFIED -- no reference weights, package or fixture exists offline, so nothing pins this class against `lpips.LPIPS`; it is
# NOT part of any parity claim and does NOT count toward SURVEY 8(f)-4.  It is kept as a plug-in point (`extra_losses`).
class LossLpips(torch.nn.Module):
    """LPIPS with the VGG-16 backbone ("vgg" variant, v0.1): inputs in [0, 1] (`normalize=True` of loss_lpips.py:48-52), scaling layer,
    the five ReLU taps relu1_2 / 2_2 / 3_3 / 4_3 / 5_3, channel-unit-normalised squared differences, non-negative 1x1 linear heads, spatial
    mean, sum over the taps.  forward(prediction [b,v,3,h,w], target [b,v,3,h,w], global_step) -> weight * mean over images; zero before
    `apply_after_step` (config/loss/lpips.yaml).  backend="hip": the same value and its gradient on the HIP kernels (LpipsVgg, weights
    packed once on `device`; h and w multiples of 16, inputs on that device)."""
    _SLICES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))   # torchvision vgg16.features conv indices per slice
    _CHANNELS = ((3, 64, 64), (64, 128, 128), (128, 256, 256, 256), (256, 512, 512, 512), (512, 512, 512, 512))

    def __init__(self, weights, weight: float = 0.05, apply_after_step: int = 0, backend: str = "torch", device=None):
        super().__init__()
        if weights is None:
            raise RuntimeError("LossLpips needs the state_dict of lpips.LPIPS(net='vgg') (pretrained VGG-16 + linear heads); it is not "
                               "available offline and is never replaced by random weights")
        if backend not in ("torch", "hip"):
            raise ValueError(f'LossLpips: backend must be "torch" or "hip", got {backend!r}')
        sd = torch.load(weights, map_location="cpu") if isinstance(weights, (str, Path)) else dict(weights)
        self.weight, self.apply_after_step, self.backend = weight, apply_after_step, backend
        # backend="hip": the same definition on LpipsVgg (split-class convolutions + csrc/lpips.hip), its weights packed once on `device`
        self._hip = LpipsVgg(sd, device=device) if backend == "hip" else None
        self.register_buffer("shift", torch.tensor([-0.030, -0.088, -0.188]).view(1, 3, 1, 1), persistent=False)
        self.register_buffer("scale", torch.tensor([0.458, 0.448, 0.450]).view(1, 3, 1, 1), persistent=False)
        for s_, idxs in enumerate(self._SLICES):
            for j, li in enumerate(idxs):
                w, b = sd[f"net.slice{s_ + 1}.{li}.weight"], sd[f"net.slice{s_ + 1}.{li}.bias"]
                assert tuple(w.shape) == (self._CHANNELS[s_][j + 1], self._CHANNELS[s_][j], 3, 3), (s_, li, tuple(w.shape))
                self.register_buffer(f"w{s_}_{j}", w.float().clone(), persistent=False)
                self.register_buffer(f"b{s_}_{j}", b.float().clone(), persistent=False)
            lin = sd.get(f"lin{s_}.model.1.weight", sd.get(f"lins.{s_}.model.1.weight"))
            assert lin is not None and lin.shape[1] == self._CHANNELS[s_][-1]
            self.register_buffer(f"lin{s_}", lin.float().clone(), persistent=False)

    def features(self, x: Tensor):
        import torch.nn.functional as F
        x = (2 * x - 1 - self.shift) / self.scale
        taps = []
        for s_, idxs in enumerate(self._SLICES):
            if s_ > 0:
                x = F.max_pool2d(x, 2, 2)
            for j in range(len(idxs)):
                x = F.relu(F.conv2d(x, getattr(self, f"w{s_}_{j}"), getattr(self, f"b{s_}_{j}"), padding=1))
            taps.append(x)
        return taps

    def distance(self, a: Tensor, b: Tensor) -> Tensor:
        """[n,3,h,w] x2 in [0,1] -> [n] LPIPS distances."""
        import torch.nn.functional as F
        total = 0
        for s_, (fa, fb) in enumerate(zip(self.features(a), self.features(b))):
            na = fa / (fa.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
            nb = fb / (fb.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
            total = total + F.conv2d((na - nb) ** 2, getattr(self, f"lin{s_}")).mean(dim=(2, 3))[:, 0]
        return total

    def forward(self, prediction: Tensor, target: Tensor, global_step: int = 0) -> Tensor:
        if global_step < self.apply_after_step:
            return torch.zeros((), dtype=torch.float32, device=target.device)
        if self._hip is not None:
            return self.weight * self._hip(prediction.flatten(0, 1), target.flatten(0, 1), normalize=True).mean()
        return self.weight * self.distance(prediction.flatten(0, 1).float(), target.flatten(0, 1).float()).mean()


class LpipsVgg(torch.nn.Module):
    """lpips.LPIPS(net="vgg", version="0.1") in eval mode on the HIP kernels: forward(in0, in1, normalize=False) -> [N, 1, 1, 1], the call of
    lpips.LPIPS.forward.  The definition is LossLpips.features / .distance (scaling layer on 2x - 1 when `normalize`, VGG-16 up to relu5_3,
    unit-normalised taps, non-negative 1x1 heads, spatial mean, sum over the taps); `weights` is the state dict LossLpips reads.
    The 13 convolutions run in the split operand class (vs_conv3x3_split_nhwc: f32 activations, f16 (hi, lo) weight pairs), the glue on
    csrc/lpips.hip.  Their weights and the flipped, channel-transposed weights of the data gradient are packed ONCE, here, on `device`
    (default: the current HIP device); calls are free of host synchronisation.  Differentiable in in0 and in1 (autograd.LpipsFn): each side
    that needs a gradient keeps its 13 post-ReLU activations, 70.8 MB per 256 x 256 image (20.4 GB for 288 views).
    Conventions, each pinned by tests/test_lpips_*.py: at a pixel where a tap's whole channel vector is 0 the normalisation's derivative is
    the finite limit I / (r + eps) (torch autograd gives NaN there); max-pool ties go to the first maximum in row-major window order, as
    torch's; the lpips heads' nn.Dropout is off (eval mode) -- the reference's training run has it active, and this is its expectation.
    Inputs: [N, 3, H, W] on a HIP device, H and W multiples of 16; anything else raises ValueError (there is no CPU path)."""

    def __init__(self, weights, device=None):
        super().__init__()
        from . import ops
        if weights is None:
            raise RuntimeError("LpipsVgg needs the state_dict of lpips.LPIPS(net='vgg'); it is never replaced by random weights")
        sd = torch.load(weights, map_location="cpu") if isinstance(weights, (str, Path)) else dict(weights)
        if not torch.cuda.is_available():
            raise ValueError("LpipsVgg runs on the HIP kernels and needs a HIP device; use LossLpips(backend='torch') on the CPU")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise ValueError(f"LpipsVgg needs a HIP device, got {dev}")
        self.device = dev
        self.convs, self.lins = [], []       # convs[k] = (forward weight, bias, data-gradient weight), k = 0..12 in VGG order

        def pack(w: Tensor, cin_pad: int = 0):
            w = w.float().contiguous()
            if cin_pad > w.shape[-1]:
                w = torch.nn.functional.pad(w, (0, cin_pad - w.shape[-1]))
            return ops.split_pack_weight(w.to(dev), ops.split_scale_exp(w))      # the exponent from the host copy: no device read

        for s_, idxs in enumerate(LossLpips._SLICES):
            for j, li in enumerate(idxs):
                w, b = sd[f"net.slice{s_ + 1}.{li}.weight"].detach().float().cpu(), sd[f"net.slice{s_ + 1}.{li}.bias"].detach().float()
                assert tuple(w.shape) == (LossLpips._CHANNELS[s_][j + 1], LossLpips._CHANNELS[s_][j], 3, 3), (s_, li, tuple(w.shape))
                first = s_ == 0 and j == 0
                wf = pack(w.permute(0, 2, 3, 1), 32 if first else 0)                       # [Cout, 3, 3, Cin(32)]
                wd = w.flip(2, 3).permute(1, 2, 3, 0)                                       # [Cin, 3, 3, Cout]
                if first:
                    wd = torch.nn.functional.pad(wd, (0, 0, 0, 0, 0, 0, 0, 32 - wd.shape[0]))  # 32 output channels, the last 29 zero
                self.convs.append((wf, b.contiguous().to(dev), pack(wd)))
            lin = sd.get(f"lin{s_}.model.1.weight", sd.get(f"lins.{s_}.model.1.weight"))
            assert lin is not None and lin.shape[1] == LossLpips._CHANNELS[s_][-1]
            self.lins.append(lin.detach().float().reshape(-1).contiguous().to(dev))
        self._first = [0, 2, 4, 7, 10]         # index of each slice's first convolution
        self._taps = [1, 3, 6, 9, 12]          # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3

    def taps(self, acts):
        return [acts[k] for k in self._taps]

    def features(self, x: Tensor, normalize: bool, keep_all: bool = True):
        """The 13 post-ReLU activations (NHWC f32) of the VGG-16 trunk for images x [N, 3, H, W]; without keep_all only the five taps are
        kept (the other entries are None), so a side that needs no gradient holds 32 MB per 256 x 256 image instead of 71 MB."""
        from . import ops
        h = ops.lpips_prep(x, normalize)
        acts = []
        for k, (wf, b, _) in enumerate(self.convs):
            if k in self._first and k > 0:
                h = ops.lpips_maxpool(h)
            h = ops.conv3x3_nhwc(h, wf, b, relu_out=True)
            acts.append(h if keep_all or k in self._taps else None)
        return acts

    def features_backward(self, acts, dtaps, g: Tensor, normalize: bool) -> Tensor:
        """Image gradient [N, 3, H, W] from the heads' gradients dtaps (ReLU-masked, at ops.lpips_scale_log2) and the activations."""
        from . import ops
        grad = dtaps[4]                                        # w.r.t. conv5_3's pre-activation
        for k in range(len(self.convs) - 1, -1, -1):
            wd = self.convs[k][2]
            if k in self._first:
                grad = ops.conv3x3_nhwc(grad, wd, None)        # w.r.t. the slice's input: the pooled tensor or the prepared image
                if k > 0:                                      # through the pool into the previous tap, + its head gradient, ReLU mask
                    s_ = self._first.index(k)
                    grad = ops.lpips_maxpool_backward(grad, acts[k - 1], dtaps[s_ - 1])
            else:
                grad = ops.conv3x3_nhwc(grad, wd, None, mask_by=acts[k - 1])
        return ops.lpips_prep_backward(grad, g, normalize)

    def _check(self, in0: Tensor, in1: Tensor):
        if in0.shape != in1.shape or in0.dim() != 4 or in0.shape[1] != 3 or in0.shape[0] == 0:
            raise ValueError(f"LPIPS takes two [N, 3, H, W] tensors of one shape, got {tuple(in0.shape)} and {tuple(in1.shape)}")
        H, W = in0.shape[-2:]
        if H % 16 or W % 16:
            raise ValueError(f"LPIPS on the HIP kernels needs H and W that are multiples of 16 (four 2 x 2 max-pools), got {H} x {W}")
        for t in (in0, in1):
            if t.device != self.device:
                raise ValueError(f"LpipsVgg was built on {self.device}; got an input on {t.device} (there is no CPU fallback)")

    def forward(self, in0: Tensor, in1: Tensor, normalize: bool = False) -> Tensor:
        from . import autograd as A
        self._check(in0, in1)
        return A.LpipsFn.apply(in0, in1, self, bool(normalize))


@torch.no_grad()
def compute_lpips(ground_truth: Tensor, predicted: Tensor, net: LpipsVgg) -> Tensor:
    """LPIPS per image of [batch, 3, h, w] tensors in [0, 1], as metrics.py:37-44 computes it (lpips.LPIPS(net="vgg").forward(gt, pred,
    normalize=True)[:, 0, 0, 0]) on the HIP kernels of `net`.  Returns a device tensor [batch] of predicted.dtype; no host synchronisation."""
    return net(ground_truth, predicted, normalize=True)[:, 0, 0, 0].to(predicted.dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# distillation point loss -- src/loss/loss_conf_point.py:188-252 (Regr3D) as ModelWrapper.training_step applies it
# (model_wrapper.py:248-301).  The teacher is vicasplat_amd.model.distiller (get_distiller); `distill_targets` samples the anchor frames, runs
# it and returns what `training_step(distill=...)` takes.  Points and confidences of any other teacher still enter as tensors.
# ---------------------------------------------------------------------------------------------------------------------------
class Regr3D(torch.nn.Module):
    """The reference's Regr3D: pixels whose pseudo-GT distance lies within the [1 %, 99 %] quantiles of their view (per batch element,
    torch.quantile's linear interpolation) are valid; loss = mean over valid of gt_conf |gt - pr|, per view, summed, plus -- when both
    predicted confidences are given -- mean |pr_conf - gt_conf| per view.  normalize_pts divides prediction and pseudo-GT each by their own
    average valid distance over both views (normalize_pointcloud 'avg_dis', ptc_geometry.py:270-328).  forward has the reference's signature
    and order; `dist_clip` and `disable_view1` are accepted and, as there, never read, and so are `alpha` and `gt_scale`.
    backend="hip": csrc/distill.hip (selection instead of sorting, two streaming passes, one backward pass; HIP device tensors, no
    fallback).  backend="torch": the plain restatement in PyTorch (CPU tests, the benchmark's baseline)."""

    def __init__(self, norm_mode: str = "avg_dis", alpha: float = 0.2, gt_scale: bool = False, backend: str = "hip"):
        super().__init__()
        if norm_mode != "avg_dis":
            raise NotImplementedError(f"Regr3D: only norm_mode='avg_dis' (every released configuration) is implemented, got {norm_mode!r}")
        if backend not in ("torch", "hip"):
            raise ValueError(f'Regr3D: backend must be "torch" or "hip", got {backend!r}')
        self.norm_mode, self.alpha, self.gt_scale, self.backend = norm_mode, alpha, gt_scale, backend

    @staticmethod
    def _normalize(p1: Tensor, p2: Tensor, valid1: Tensor, valid2: Tensor):
        B = p1.shape[0]
        zero = lambda p, valid: torch.where(valid[..., None], p, torch.zeros_like(p))      # invalid_to_zeros: assigned, not multiplied (a non-finite point outside the mask is ignored)
        dis = torch.cat([zero(p1, valid1).reshape(B, -1, 3), zero(p2, valid2).reshape(B, -1, 3)], dim=1).norm(dim=-1)
        nnz = valid1.reshape(B, -1).sum(dim=1) + valid2.reshape(B, -1).sum(dim=1)
        f = (dis.sum(dim=1) / (nnz + 1e-8)).clip(min=1e-8).view(B, 1, 1, 1)
        return p1 / f, p2 / f

    def forward(self, gt_pts1, gt_pts2, pr_pts1, pr_pts2, gt_conf1, gt_conf2, pr_conf1=None, pr_conf2=None, dist_clip=None,
                normalize_pts=False, disable_view1=False):
        if self.backend == "hip":
            from . import autograd as A
            if pr_conf1 is None or pr_conf2 is None:
                pr_conf1 = pr_conf2 = None
            return A.Regr3DFn.apply(gt_pts1, gt_pts2, pr_pts1, pr_pts2, gt_conf1, gt_conf2, pr_conf1, pr_conf2, bool(normalize_pts))
        dis1, dis2 = gt_pts1.norm(dim=-1), gt_pts2.norm(dim=-1)
        q = torch.tensor([0.01, 0.99], dtype=dis1.dtype, device=dis1.device)
        q1, q2 = torch.quantile(dis1.flatten(1), q, dim=1), torch.quantile(dis2.flatten(1), q, dim=1)
        valid1 = (dis1 >= q1[0].view(-1, 1, 1)) & (dis1 <= q1[1].view(-1, 1, 1))
        valid2 = (dis2 >= q2[0].view(-1, 1, 1)) & (dis2 <= q2[1].view(-1, 1, 1))
        if normalize_pts:
            pr_pts1, pr_pts2 = self._normalize(pr_pts1, pr_pts2, valid1, valid2)
            gt_pts1, gt_pts2 = self._normalize(gt_pts1, gt_pts2, valid1, valid2)
        l1 = gt_conf1 * torch.norm(gt_pts1 - pr_pts1, dim=-1)
        l2 = gt_conf2 * torch.norm(gt_pts2 - pr_pts2, dim=-1)
        loss = l1[valid1].mean() + l2[valid2].mean()
        if pr_conf1 is not None and pr_conf2 is not None:
            loss = loss + (pr_conf1 - gt_conf1).abs().mean() + (pr_conf2 - gt_conf2).abs().mean()
        return loss


def sample_anchor_frames(video_frames: Tensor, temporal_compression: int = 4, n_frames: int | None = None):
    """ModelWrapper._sample_anchor_frames (model_wrapper.py:153-182): two anchor frames per scene from adjacent segments of
    `temporal_compression` frames, with the same np.random draws in the same order (a caller who seeds numpy gets the reference's indices).
    video_frames [B, V, C, H, W] -> (anchor_frames [B, 2, C, H, W], idx [B, 2], segment_idx [B, 2]), the indices int64 on the frames' device.
    An odd number of frames treats the first as the reference frame: the segments start after it and the indices shift back, clamped at 0."""
    B, V, C, H, W = video_frames.shape
    odd = V % 2 != 0
    n_segments = (V - 1) // temporal_compression + 1 if odd else V // temporal_compression
    n_frames = n_frames or n_segments
    if n_frames != 2:
        raise ValueError(f"sample_anchor_frames: the teacher takes two frames, got n_frames = {n_frames} ({V} frames in segments of {temporal_compression})")
    idx = torch.from_numpy(np.random.choice(temporal_compression, (B, n_frames))).long().to(video_frames.device)
    seg = np.stack([np.random.choice(n_segments - 1, (n_frames - 1,), replace=False) for _ in range(B)], axis=0)
    segment_idx = torch.from_numpy(seg).long().to(video_frames.device)
    segment_idx = torch.cat([segment_idx, segment_idx + 1], dim=-1)
    idx = idx + segment_idx * temporal_compression
    if odd:
        idx = (idx + 1 - temporal_compression).clamp_min(0).long()
    anchor_frames = torch.gather(video_frames, 1, idx[..., None, None, None].expand(-1, -1, C, H, W))
    return anchor_frames, idx, segment_idx


def distill_targets(distiller, context: dict, **extra) -> dict:
    """The `distill` argument of `training_step` from the images alone (model_wrapper.py:248-271): samples two anchor frames per scene
    (n_frames=2, temporal_compression=1), runs the frozen teacher on them with the first anchor's extrinsics as the tail kernel's transform
    -- the teacher's points leave the kernel already in the first video frame's space, so the dict carries pts_in_first_frame=True and
    `distillation_loss` skips its own einsum -- and returns {pseudo_gt1, pseudo_gt2, frame_idx, segment_idx, pts_in_first_frame}.
    context: {"image" [B, V, 3, H, W] in [-1, 1], "extrinsics" [B, V, 4, 4]}; `extra` (weight, loss_fn, only) is passed through."""
    anchors, frame_idx, segment_idx = sample_anchor_frames(context["image"], n_frames=2, temporal_compression=1)
    E = torch.gather(context["extrinsics"].float(), 1, frame_idx[:, :1, None, None].expand(-1, 1, 4, 4)).squeeze(1)
    with torch.no_grad():
        gt1, gt2 = distiller({"image": anchors}, False, transform=E[:, :3])
    return dict(pseudo_gt1=gt1, pseudo_gt2=gt2, frame_idx=frame_idx, segment_idx=segment_idx, pts_in_first_frame=True, **extra)


def distillation_loss(out: dict, pseudo_gt1: dict, pseudo_gt2: dict, frame_idx: Tensor, segment_idx: Tensor, context_extrinsics: Tensor,
                      weight: float = 1.0, loss_fn: Regr3D | None = None, pts_in_first_frame: bool = False) -> Tensor:
    """The distillation term of ModelWrapper.training_step (model_wrapper.py:260-299) from the teacher's outputs.
    out: the encoder's outputs (`gaussian_centers` [B,V,H,W,3], `confidence` [B,V,H,W] or None); pseudo_gt1 / pseudo_gt2: the teacher's
    {"pts3d" [B,H,W,3], "conf" [B,H,W]} for the two anchor frames, in the first anchor's camera space; frame_idx [B,2] (int64): the
    anchors' frame numbers; segment_idx [B,2] (int64): the views whose predictions they are compared with; context_extrinsics [B,V,4,4].
    The teacher's points are moved into the first video frame's space by the first anchor's extrinsics; the points are normalised when
    the video has more than two views; the result is multiplied by `weight` (train.distill_weight).  `loss_fn`: a Regr3D (default: the
    HIP backend).  pts_in_first_frame: the teacher's points are in the first video frame's space already (the teacher's tail kernel moved
    them: `distill_targets`), so they are taken as they are."""
    loss_fn = Regr3D() if loss_fn is None else loss_fn
    if pts_in_first_frame:
        gt1, gt2 = pseudo_gt1["pts3d"].float(), pseudo_gt2["pts3d"].float()
    else:
        E = torch.gather(context_extrinsics.float(), 1, frame_idx[:, :1, None, None].expand(-1, 1, 4, 4)).squeeze(1)
        R, t = E[:, :3, :3], E[:, None, None, :3, 3]
        gt1 = torch.einsum("bij,bhwj->bhwi", R, pseudo_gt1["pts3d"].float()) + t
        gt2 = torch.einsum("bij,bhwj->bhwi", R, pseudo_gt2["pts3d"].float()) + t
    xyz, conf = out["gaussian_centers"], out.get("confidence")
    pr1, pr2 = torch.gather(xyz, 1, segment_idx[..., None, None, None].expand(-1, -1, *xyz.shape[-3:])).unbind(1)
    pc1 = pc2 = None
    if conf is not None:
        pc1, pc2 = torch.gather(conf, 1, segment_idx[..., None, None].expand(-1, -1, *conf.shape[-2:])).unbind(1)
    return loss_fn(gt1, gt2, pr1, pr2, pseudo_gt1["conf"].float(), pseudo_gt2["conf"].float(), pc1, pc2,
                   normalize_pts=xyz.shape[1] > 2) * weight


# ---------------------------------------------------------------------------------------------------------------------------
# depth-smoothness loss -- src/loss/loss_depth.py:26-60 (LossDepth, config/loss/depth.yaml)
# ---------------------------------------------------------------------------------------------------------------------------
def depth_smoothness_loss(depth: Tensor, near: Tensor, far: Tensor, image: Tensor | None = None, weight: float = 1.0,
                          sigma_image: float | None = None, use_second_derivative: bool = False, backend: str = "hip") -> Tensor:
    """LossDepth.forward on tensors: depth [..., H, W] with near and far [...] (one pair per view) and, for the bilateral weights
    (sigma_image not None), the target colours image [..., 3, H, W].  d = (depth clamped to [log near, log far] - log near) / (log far -
    log near) -- the minimum first, the log on near and far only, as the reference writes it --; first or second differences of d along W
    and along H, each times exp(-sigma_image * max over the channels of the SIGNED colour difference) (second: the larger of the two
    neighbouring maxima); weight * (mean |dx| + mean |dy|), the means over all views at once.  Differentiable in depth only.
    backend="hip": csrc/depth_loss.hip (one stencil pass that also writes the gradient; HIP device tensors, no fallback; H or W too small
    for a non-empty difference raises ValueError).  backend="torch": the plain restatement (CPU tests, the benchmark's baseline)."""
    if backend not in ("torch", "hip"):
        raise ValueError(f'depth_smoothness_loss: backend must be "torch" or "hip", got {backend!r}')
    if sigma_image is not None and image is None:
        raise ValueError("depth_smoothness_loss: sigma_image is given, so the target image is needed")
    if backend == "hip":
        from . import autograd as A
        H, W = depth.shape[-2:]
        return A.DepthSmoothFn.apply(depth.reshape(-1, H, W), near.reshape(-1), far.reshape(-1),
                                     None if sigma_image is None else image.reshape(-1, 3, H, W), sigma_image, bool(use_second_derivative),
                                     float(weight))
    ln, lf = near[..., None, None].log(), far[..., None, None].log()
    d = depth.minimum(lf).maximum(ln)
    d = (d - ln) / (lf - ln)
    dx, dy = d.diff(dim=-1), d.diff(dim=-2)
    if use_second_derivative:
        dx, dy = dx.diff(dim=-1), dy.diff(dim=-2)
    if sigma_image is not None:
        cx, cy = image.diff(dim=-1).amax(dim=-3), image.diff(dim=-2).amax(dim=-3)
        if use_second_derivative:
            cx = cx[..., :, 1:].maximum(cx[..., :, :-1])
            cy = cy[..., 1:, :].maximum(cy[..., :-1, :])
        dx = dx * torch.exp(-cx * sigma_image)
        dy = dy * torch.exp(-cy * sigma_image)
    return weight * (dx.abs().mean() + dy.abs().mean())


class LossDepth(torch.nn.Module):
    """The reference's LossDepth with its configuration (weight, sigma_image, use_second_derivative: config/loss/depth.yaml has 0.25, null,
    false) and its forward(prediction, batch, gaussians, global_step): reads prediction.depth [B, V, H, W] and batch["target"]["near" |
    "far"] [B, V] (and ["image"] [B, V, 3, H, W] when sigma_image is set).  `__name__` is the reference's loss name, so an instance in
    `training_step(extra_losses=[...])` is called as (render, batch, out) and reported as `loss_depth`; its gradient reaches the
    rasterizer as dL_ddepth.  The reference's decoder ignores depth_mode and so renders plain depth while only near and far are
    logged; that is kept.  backend: see depth_smoothness_loss."""
    __name__ = "depth"

    def __init__(self, weight: float = 0.25, sigma_image: float | None = None, use_second_derivative: bool = False, backend: str = "hip"):
        super().__init__()
        if backend not in ("torch", "hip"):
            raise ValueError(f'LossDepth: backend must be "torch" or "hip", got {backend!r}')
        self.weight, self.sigma_image, self.use_second_derivative, self.backend = weight, sigma_image, use_second_derivative, backend

    def forward(self, prediction, batch, gaussians=None, global_step: int = 0) -> Tensor:
        if getattr(prediction, "depth", None) is None:
            raise ValueError("LossDepth needs a rendered depth (prediction.depth [B, V, H, W])")
        tgt = batch["target"]
        return depth_smoothness_loss(prediction.depth, tgt["near"], tgt["far"], tgt["image"] if self.sigma_image is not None else None,
                                     self.weight, self.sigma_image, self.use_second_derivative, self.backend)


class LossScaler:
    """Dynamic loss scale for the 16-bit activation gradients (what torch.amp.GradScaler does for f16): halve on a non-finite
    gradient norm (that step is skipped), double after `growth_interval` clean steps."""

    def __init__(self, init_scale: float = 1024.0, growth_interval: int = 200, min_scale: float = 1.0, max_scale: float = 65536.0):
        self.scale, self.growth_interval, self.min_scale, self.max_scale = float(init_scale), growth_interval, min_scale, max_scale
        self.good = 0

    def update(self, finite: bool) -> None:
        if finite:
            self.good += 1
            if self.good >= self.growth_interval:
                self.scale, self.good = min(self.scale * 2.0, self.max_scale), 0
        else:
            self.scale, self.good = max(self.scale * 0.5, self.min_scale), 0


def training_step(encoder, decoder, batch: dict, optimizer, *, scheduler=None, compute_dtype=torch.float16,
                  loss_scale: float | LossScaler | None = None, clip: float = 0.5, mse_weight: float = 1.0, camera_weight: float = 0.0,
                  extra_losses=(), allreduce: bool = False, reducer=None, global_step: int = 0, forward_fn=None,
                  distill: dict | None = None) -> dict:
    """One optimisation step of the reference's objective (training_step, model_wrapper.py:184-321): MSE (loss_mse.py) + camera
    dual-quaternion loss (loss_camera.py, `camera_weight` > 0 and batch["context"]["extrinsics"] present) + `extra_losses`
    (callables (render, batch, out) -> scalar; the reference's LPIPS term needs VGG weights that are not available offline and plugs
    in here).

    batch: {"context": {"image" [B,V,3,H,W] in [-1,1], "intrinsics" [B,V,3,3], ("extrinsics" [B,V,4,4])},
            "target":  {"image" [B,Vt,3,H,W] in [0,1], "extrinsics", "intrinsics", "near", "far"}}
    The encoder runs its differentiable HIP forward (train_forward.forward_train, `global_step` drives the opacity mapping as
    model_wrapper.py:207), the Gaussians are rendered by the HIP rasterizer, and the backward pass runs on the HIP backward kernels.
    `loss_scale`: a LossScaler (dynamic; default: one kept on the optimizer), or a fixed float.  f16 needs it for the 16-bit
    activation gradients; gradients are unscaled before clipping; an overflowed step is skipped, its gradients dropped.
    Gradient exchange: `reducer` (vicasplat_amd.dist.GradReducer: buckets all-reduced DURING backward, RCCL over xGMI) or
    allreduce=True (bucketed all-reduce after backward).  The skip decision of an overflowed step is taken from the norm of the
    REDUCED gradients, so every rank takes the same decision (an inf / nan on one rank reaches all of them through the sum).
    `forward_fn(encoder, image, intrinsics, compute_dtype, global_step=) -> dict` replaces the HIP training forward (tests drive the
    step's control flow -- loss scaling, gradient exchange, clipping, skipping -- with a toy encoder / decoder on CPU).
    `distill`: the distillation stage (model_wrapper.py:248-301) -- a dict with the arguments of `distillation_loss` (pseudo_gt1, pseudo_gt2,
    frame_idx, segment_idx; optional weight, loss_fn, pts_in_first_frame; the extrinsics are the context's) and `only`; `distill_targets` makes
    it from the images alone with the package's teacher.  The term enters the result as
    `loss_distill`.  With `only` (distill_only, stage 1 of the recipe) the forward runs with distill=True, nothing is rendered, only the
    camera and distillation terms are summed and the result has no `psnr` (the reference's distill_only keeps the camera term alone of
    its losses: `extra_losses` have no render to work on there and passing any raises); without it the term is added to the usual
    objective."""
    only = distill is not None and bool(distill.get("only", False))
    if only and len(extra_losses):
        raise ValueError("training_step: distill['only'] renders nothing, so `extra_losses` cannot be applied; pass none")
    if forward_fn is None:
        from .model.encoder.train_forward import forward_train as forward_fn
    ctx, tgt = batch["context"], batch["target"]
    if loss_scale is None:
        loss_scale = getattr(optimizer, "_vs_loss_scaler", None)
        if loss_scale is None:
            # f16: the 16-bit activation gradients need the scale; split class ("split": f32 gradients whose MFMA operands are f16 (hi, lo)
            # pairs): the scale keeps hi in the f16 normal range and lo out of the subnormals -- larger is better until hi overflows,
            # which the dynamic scaler finds by itself (an overflowed step is skipped, the scale halved)
            if compute_dtype == "split":
                loss_scale = LossScaler(8192.0, max_scale=2.0 ** 24)
            else:
                loss_scale = LossScaler(1024.0 if compute_dtype == torch.float16 else 1.0)
            optimizer._vs_loss_scaler = loss_scale
    scale = loss_scale.scale if isinstance(loss_scale, LossScaler) else float(loss_scale)
    if reducer is not None:
        reducer.zero_grad()
    else:
        optimizer.zero_grad(set_to_none=True)
    if only:
        out = forward_fn(encoder, ctx["image"], ctx["intrinsics"], compute_dtype, global_step=global_step, distill=True)
        render, parts = None, {}
    else:
        out = forward_fn(encoder, ctx["image"], ctx["intrinsics"], compute_dtype, global_step=global_step)
        g = out["gaussians"]
        gs = Gaussians(g["means"].flatten(1, 3), g["covariances"].flatten(1, 3), g["harmonics"].flatten(1, 3), g["opacities"].flatten(1))
        h, w = tgt["image"].shape[-2:]
        render = decoder.forward(gs, tgt["extrinsics"], tgt["intrinsics"], tgt["near"], tgt["far"], (h, w))
        parts = dict(mse=mse_loss(render.color, tgt["image"], mse_weight))
    if camera_weight > 0 and "extrinsics" in ctx:
        parts["camera"] = camera_loss(out["pred_extrins"], ctx["extrinsics"].float(), camera_weight, pred_intrins=out.get("pred_intrins"),
                                      context_intrinsics=ctx["intrinsics"])
    for i, fn in enumerate(extra_losses):
        parts[getattr(fn, "__name__", f"extra{i}")] = fn(render, batch, out)
    if distill is not None:
        parts["distill"] = distillation_loss(out, distill["pseudo_gt1"], distill["pseudo_gt2"], distill["frame_idx"], distill["segment_idx"],
                                             ctx["extrinsics"], distill.get("weight", 1.0), distill.get("loss_fn"),
                                             pts_in_first_frame=bool(distill.get("pts_in_first_frame", False)))
    loss = sum(parts.values())
    (loss * scale).backward()
    params = [p for p in encoder.parameters() if p.requires_grad]
    if reducer is not None:
        reducer.finish()
    elif allreduce:
        from . import dist as vdist
        vdist.bucketed_allreduce_grads(params)   # all trainable parameters: unused ones are zero-filled so every rank reduces identical buckets
    grads = [p.grad for p in params if p.grad is not None]
    # unscale and clip in ONE pass over the gradients: norm of the scaled gradients, then a single multiply by
    # min(1, clip / (norm + 1e-6)) / scale (= torch's clip_grad_norm_ on the unscaled gradients)
    gnorm = torch.linalg.vector_norm(torch.stack(torch._foreach_norm(grads))) / scale
    finite = bool(torch.isfinite(gnorm))
    if finite:
        torch._foreach_mul_(grads, torch.clamp(clip / (gnorm + 1e-6), max=1.0) / scale)
        optimizer.step()
        if scheduler is not None:
            scheduler.step()
    elif reducer is None:                                     # overflowed step: skipped, as torch.amp's GradScaler would; drop the gradients
        optimizer.zero_grad(set_to_none=True)
    if isinstance(loss_scale, LossScaler):
        loss_scale.update(finite)
    res = dict(loss=loss.detach())
    if not only:
        with torch.no_grad():
            res["psnr"] = compute_psnr(tgt["image"].flatten(0, 1), render.color.detach().flatten(0, 1)).mean()
    res.update(grad_norm=gnorm, skipped=not finite, pred_extrins=out["pred_extrins"].detach(), loss_scale=scale,
               **{"loss_" + k: v.detach() for k, v in parts.items()})
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# trajectory metrics and the test step -- src/evaluation/metrics.py:148-265, src/model/model_wrapper.py:323-381,
# src/evaluation/pose_evaluator.py:77-174.  The reference hands every scene to evo on the host (a device -> host copy, a scipy rotation per
# pose, three evo calls); evo is not available offline, so its ape / rpe (align=True, correct_scale=True, delta in frames, all_pairs=True) are
# restated from the published algorithm -- Umeyama's alignment, then the residuals -- as include/vicasplat_metrics.h writes it out.
# ---------------------------------------------------------------------------------------------------------------------------
# STATUS: UNVERIFIED against evo -- no package, no fixture of its numbers exists offline; the kernel, the torch backend and the float64
# restatement of tests/trajectory_f64.py agree with one another and with closed forms, which pins the algorithm as stated, not evo's code.
def _det3(M: Tensor) -> Tensor:
    return (M[..., 0, 0] * (M[..., 1, 1] * M[..., 2, 2] - M[..., 1, 2] * M[..., 2, 1])
            - M[..., 0, 1] * (M[..., 1, 0] * M[..., 2, 2] - M[..., 1, 2] * M[..., 2, 0])
            + M[..., 0, 2] * (M[..., 1, 0] * M[..., 2, 1] - M[..., 1, 1] * M[..., 2, 0]))


def _trajectory_metrics_torch(P: Tensor, Q: Tensor, delta: int):
    """The algorithm of include/vicasplat_metrics.h in plain float64 torch, batched: (metrics [B, 3], valid [B] bool)."""
    P, Q = P.double(), Q.double()
    B, V = P.shape[:2]
    finite = torch.isfinite(P).flatten(1).all(1) & torch.isfinite(Q).flatten(1).all(1)
    if V < 3 or delta >= V:
        return torch.zeros(B, 3, dtype=torch.float64, device=P.device), torch.zeros_like(finite)
    eye = torch.eye(4, dtype=torch.float64, device=P.device)
    P = torch.where(finite[:, None, None, None], P, eye)       # a non-finite scene must not reach the SVD; it is masked below
    Q = torch.where(finite[:, None, None, None], Q, eye)
    x, y, Rp, Rq = P[..., :3, 3], Q[..., :3, 3], P[..., :3, :3], Q[..., :3, :3]
    mux, muy = x.mean(1), y.mean(1)
    dx, dy = x - mux[:, None], y - muy[:, None]
    sig2 = (dx * dx).sum((1, 2)) / V
    C = torch.einsum("bvi,bvj->bij", dy, dx) / V
    U, d, Vh = torch.linalg.svd(C)
    valid = finite & ((d > 2.0 ** -52).sum(1) >= 2)
    S = torch.ones_like(d)
    S[:, 2] = torch.where(_det3(U) * _det3(Vh) < 0, -1.0, 1.0)
    R = (U * S[:, None, :]) @ Vh
    c = (d * S).sum(1) / sig2
    t = muy - c[:, None] * (R @ mux[..., None])[..., 0]
    res = c[:, None, None] * (x @ R.transpose(1, 2)) + t[:, None] - y
    ate = (res * res).sum(-1).mean(1).sqrt()
    i, j = slice(0, V - delta), slice(delta, V)
    A, a = Rq[:, i].transpose(-1, -2) @ Rq[:, j], (Rq[:, i].transpose(-1, -2) @ (y[:, j] - y[:, i])[..., None])[..., 0]
    Bm, b = Rp[:, i].transpose(-1, -2) @ Rp[:, j], c[:, None, None] * (Rp[:, i].transpose(-1, -2) @ (x[:, j] - x[:, i])[..., None])[..., 0]
    E, Et = A.transpose(-1, -2) @ Bm, (A.transpose(-1, -2) @ (b - a)[..., None])[..., 0]
    w = torch.stack([E[..., 2, 1] - E[..., 1, 2], E[..., 0, 2] - E[..., 2, 0], E[..., 1, 0] - E[..., 0, 1]], -1)
    theta = torch.atan2(0.5 * w.norm(dim=-1), 0.5 * (E.diagonal(dim1=-2, dim2=-1).sum(-1) - 1.0)) * (180.0 / math.pi)
    out = torch.stack([ate, (Et * Et).sum(-1).mean(1).sqrt(), (theta * theta).mean(1).sqrt()], -1)
    return torch.where(valid[:, None], out, torch.zeros_like(out)), valid


@torch.no_grad()
def camera_eval_metrics(pred_c2ws: Tensor, gt_c2ws: Tensor, sample_stride: int = 1, *, backend: str | None = None, return_valid: bool = False):
    """(ate, rpe_trans, rpe_rot) of estimated against true camera-to-world poses, [V, 4, 4] (0-d results) or [B, V, 4, 4] ([B] results), as
    metrics.py:185-265 asks evo for them: Umeyama alignment with scale, the RMSE of the aligned positions, and the RMSE of the relative pose
    errors between consecutive frames (translation norm; rotation angle in degrees).  Float64 tensors on the inputs' device, never Python
    floats; no host synchronisation.  sample_stride > 1 keeps every sample_stride-th pose (:189-196).  A scene evo would refuse (the
    reference's bare `except` logs 0.0 for it, model_wrapper.py:374-377: collinear or coincident positions, fewer than 3 poses) or one with a
    non-finite pose gives three zeros; return_valid adds the flag ([B] or 0-d bool) that tells such a scene from a perfect one.
    backend="hip" (the default for HIP tensors): csrc/trajectory.hip, one launch for the batch; backend="torch" (the default for CPU
    tensors): the same algorithm in plain float64 torch (CPU tests, the bench tool's comparison).  Half-precision poses are promoted to f32.
    UNVERIFIED against evo (see above); rotations are used as given, not passed through a quaternion."""
    if backend is None:
        backend = "hip" if pred_c2ws.is_cuda else "torch"
    if backend not in ("torch", "hip"):
        raise ValueError(f'camera_eval_metrics: backend must be "torch" or "hip", got {backend!r}')
    single = pred_c2ws.dim() == 3
    P, Q = (pred_c2ws[None], gt_c2ws[None]) if single else (pred_c2ws, gt_c2ws)
    if P.dim() != 4 or tuple(P.shape[-2:]) != (4, 4) or P.shape != Q.shape:
        raise ValueError(f"camera_eval_metrics takes poses [V, 4, 4] or [B, V, 4, 4] of one shape, got {tuple(pred_c2ws.shape)} and "
                         f"{tuple(gt_c2ws.shape)}")
    if int(sample_stride) != sample_stride or sample_stride < 1:
        raise ValueError(f"camera_eval_metrics: sample_stride must be a positive integer, got {sample_stride!r}")
    if sample_stride > 1:
        P, Q = P[:, ::sample_stride], Q[:, ::sample_stride]
    if backend == "hip":
        from . import ops
        dt = torch.float64 if torch.float64 in (P.dtype, Q.dtype) else torch.float32
        m, valid = ops.trajectory_metrics(P.detach().to(dt).contiguous(), Q.detach().to(dt).contiguous(), 1)
        valid = valid != 0
    else:
        m, valid = _trajectory_metrics_torch(P.detach(), Q.detach(), 1)
    if single:
        m, valid = m[0], valid[0]
    out = (m[..., 0], m[..., 1], m[..., 2])
    return out + (valid,) if return_valid else out


def _per_scene(per_image: Tensor, b: int, v: int) -> Tensor:
    return per_image.unflatten(0, (b, v)).mean(1)


def test_step(encoder, decoder, batch: dict, *, lpips_net: LpipsVgg | None = None, align_pose: bool = False, align_kwargs: dict | None = None) -> dict:
    """ModelWrapper.test_step's scores (model_wrapper.py:323-381), batched over scenes (the reference asserts b == 1): the encoder under
    no_grad on batch["context"]; the target views rendered from its Gaussians -- with align_pose (test_cfg.align_pose, :339-340) from the
    target extrinsics `align_poses` refines first (`align_kwargs`: its keyword arguments); then per scene, as device tensors [B]:
      psnr_ours, ssim_ours, lpips_ours   the means over the scene's target views of compute_psnr / compute_ssim / compute_lpips (:357-364);
                                         lpips_ours only when `lpips_net` (an LpipsVgg) is given -- its weights are not available offline
      ate_ours, rpe-trans_ours, rpe-rot_ours   camera_eval_metrics of model_outs["gaussian_camera_extrins"] against
                                         batch["context"]["extrinsics"] (:367-381), float64
      pose_valid                         False where the reference's bare `except` would have logged zeros
    No .item(), no host copy: a caller logs or reduces the tensors when it chooses to.
    batch: {"context": {"image" [B,V,3,H,W] in [-1,1], "intrinsics", "extrinsics" [B,V,4,4], ...},
            "target":  {"image" [B,Vt,3,H,W] in [0,1], "extrinsics", "intrinsics", "near", "far"}}"""
    ctx, tgt = batch["context"], batch["target"]
    b, v, _, h, w = tgt["image"].shape
    with torch.no_grad():
        model_outs = encoder(ctx)
    gaussians = model_outs["gaussians"]
    extrinsics = tgt["extrinsics"]
    if align_pose:
        extrinsics = align_poses(decoder, gaussians, tgt["image"], extrinsics, tgt["intrinsics"], tgt["near"], tgt["far"], **(align_kwargs or {}))
    with torch.no_grad():
        output = decoder.forward(gaussians, extrinsics, tgt["intrinsics"], tgt["near"], tgt["far"], (h, w))
        rgb_pred, rgb_gt = output.color.flatten(0, 1), tgt["image"].flatten(0, 1)
        scores = {"psnr_ours": _per_scene(compute_psnr(rgb_gt, rgb_pred), b, v), "ssim_ours": _per_scene(compute_ssim(rgb_gt, rgb_pred), b, v)}
        if lpips_net is not None:
            scores["lpips_ours"] = _per_scene(compute_lpips(rgb_gt, rgb_pred, lpips_net), b, v)
        ate, rpe_trans, rpe_rot, valid = camera_eval_metrics(model_outs["gaussian_camera_extrins"], ctx["extrinsics"], return_valid=True)
        scores.update({"ate_ours": ate, "rpe-trans_ours": rpe_trans, "rpe-rot_ours": rpe_rot, "pose_valid": valid})
    return scores


def save_test_outputs(batch: dict, model_outs: dict, output, path, *, save_image: bool = True) -> list[Path]:
    """The files ModelWrapper.test_step writes for a scene (model_wrapper.py:386-407), for every scene of the batch (the reference asserts
    b == 1), under `path` (the reference's test_cfg.output_path / name):
      <scene>/context/<index:0>6>.png   every context frame, image * 0.5 + 0.5 -- always
      <scene>/transforms.json           export_transforms of model_outs["gaussian_camera_extrins"] with those file names -- always
      <scene>/color/<index:0>6>.png     with save_image (test_cfg.save_image): hcat(color, vis_depth_map(depth)) of every rendered target,
                                        the depth range taken per scene as the reference takes it
    batch: {"scene": [B names], "context": {"image" [B,V,3,H,W] in [-1,1], "index" [B,V]}, "target": {"index" [B,Vt]}};
    output: the decoder's, .color [B,Vt,3,H,W] and .depth [B,Vt,H,W].  All frames of one shape go through ONE encode_png_batch call: the
    pixels never cross to the host, the files do.  save_compare (it needs a font) and save_video are not built.  Returns the image paths."""
    from .misc import image_io
    from .misc.utils import vis_depth_map
    path = Path(path)
    scenes = list(batch["scene"])
    ctx_index = torch.as_tensor(batch["context"]["index"]).tolist()
    names = [[f"context/{index:0>6}.png" for index in row] for row in ctx_index]
    frames = batch["context"]["image"].detach() * 0.5 + 0.5
    paths = [path / scene / name for scene, row in zip(scenes, names) for name in row]
    image_io.save_images(frames.flatten(0, 1), paths)
    for b, scene in enumerate(scenes):
        export_transforms(model_outs["gaussian_camera_extrins"][b], path / scene / "transforms.json", file_names=names[b])
    if save_image:
        color = output.color.detach().float()
        depth = torch.stack([vis_depth_map(output.depth[b]) for b in range(len(scenes))]).to(color.dtype)
        gap = color.new_ones(color.shape[:-1] + (8,))          # layout.hcat's white gap of 8 columns between images of one height
        tgt_index = torch.as_tensor(batch["target"]["index"]).tolist()
        tgt_paths = [path / scene / f"color/{index:0>6}.png" for scene, row in zip(scenes, tgt_index) for index in row]
        image_io.save_images(torch.cat([color, gap, depth], dim=-1).flatten(0, 1), tgt_paths)
        paths += tgt_paths
    return paths


def pose_eval_step(encoder, decoder, batch: dict, *, steps: int = 0, rot_lr: float = 0.005, trans_lr: float = 0.005, mse_weight: float = 1.0,
                   ssim_structure_weight: float = 1.0, sample_stride: int = 1) -> dict:
    """PoseEvaluator.test_step (pose_evaluator.py:77-174), batched over scenes: the encoder under no_grad; the predicted poses of the context
    views other than the first refined by `steps` of `align_poses` against those views' own images (image * 0.5 + 0.5) with the SSIM
    structure term on (:136-141) -- steps = 0, as the reference ships it (number_steps = 0, :112), refines nothing --; then
    camera_eval_metrics of [true first pose | refined poses] (:159) and of the unrefined prediction against batch["context"]["extrinsics"].
    Returns per-scene float64 device tensors [B]: ate / rpe_trans / rpe_rot _after_opt and _before_opt, and pose_valid_after_opt /
    pose_valid_before_opt.  No host copy."""
    ctx = batch["context"]
    with torch.no_grad():
        model_outs = encoder(ctx)
    pred = model_outs["gaussian_camera_extrins"]
    extrinsics = pred[:, 1:].clone()
    if steps > 0:
        extrinsics = align_poses(decoder, model_outs["gaussians"], ctx["image"][:, 1:] * 0.5 + 0.5, extrinsics, ctx["intrinsics"][:, 1:],
                                 ctx["near"][:, 1:], ctx["far"][:, 1:], steps=steps, rot_lr=rot_lr, trans_lr=trans_lr, mse_weight=mse_weight,
                                 ssim_structure_weight=ssim_structure_weight)
    gt = ctx["extrinsics"]
    eval_pose = torch.cat([gt[:, :1].to(extrinsics.dtype), extrinsics.detach()], dim=1)
    after = camera_eval_metrics(eval_pose, gt, sample_stride, return_valid=True)
    before = camera_eval_metrics(pred, gt, sample_stride, return_valid=True)
    names = ("ate", "rpe_trans", "rpe_rot", "pose_valid")
    return {**{f"{n}_after_opt": t for n, t in zip(names, after)}, **{f"{n}_before_opt": t for n, t in zip(names, before)}}


# ---- validation step: colour maps, comparison image, projections, video (model_wrapper.py:524-704, 776-813) --------------------------------
def depth_video_frames(color: Tensor, depth: Tensor, gap: int = 8) -> Tensor:
    """color [F, 3, H, W], depth [F, H, W] -> uint8 [F, 3, 2 H + gap, W]: each frame over its `turbo` depth map (the range taken over all
    F depth maps, as vis_depth_map(output.depth[0]) takes it), a white gap between them -- render_video_generic's
    vcat(rgb, depth) ... (video.clip(0, 1) * 255).type(torch.uint8) as one selection and one frame kernel (csrc/viz.hip)."""
    from . import ops
    from .visualization.color_map import device_table
    depth = depth.detach().float().contiguous()
    return ops.video_frames(color.detach().float().contiguous(), depth, sliced_depth_range(depth), device_table("turbo", depth.device), gap)


def first_positives(flat: Tensor, limit: int) -> Tensor:
    """[limit]: the first `limit` values > 0 of flat [n], in order, then zeros -- flat[flat > 0][:limit] at a fixed size, so that nothing is
    read back to the host: every positive value is scattered to its rank, the ones past the limit (and everything else) to a spare slot."""
    positive = flat > 0
    rank = positive.cumsum(0) - 1
    slot = torch.where(positive & (rank < limit), rank, torch.full_like(rank, limit))
    return torch.zeros(limit + 1, dtype=flat.dtype, device=flat.device).scatter_(0, slot, flat)[:limit]


def sliced_depth_range(depth: Tensor) -> Tensor:
    """(near, far) [2] of vis_depth_map (src/misc/utils.py:13-22) for any number of values: ops.depth_range itself up to its limit of
    VSV_MAX_RANGE_N = 16 000 000 values; beyond it (the 300 frames of the exaggerated video at 256 x 256) the reference's two slices -- far
    over the first 16 000 000 values, near over the first 16 000 000 positive ones -- each formed at a fixed size and handed to the same kernel."""
    from . import _lib, ops
    limit = _lib.VSV_MAX_RANGE_N
    flat = depth.reshape(-1)
    if flat.numel() <= limit:
        return ops.depth_range(depth)
    far = ops.depth_range(flat[:limit].contiguous())[1]
    near = ops.depth_range(first_positives(flat, limit))[0]
    return torch.stack((near, far))


@torch.no_grad()
def render_video_generic(encoder, decoder, batch: dict, trajectory_fn, num_frames: int = 30, smooth: bool = True, loop_reverse: bool = True,
                         save_depth: bool = True) -> Tensor:
    """ModelWrapper.render_video_generic (model_wrapper.py:776-815) up to the frames it hands to wandb: the encoder on batch["context"],
    `trajectory_fn(t) -> (extrinsics [1, F, 4, 4], intrinsics [1, F, 3, 3])` for t = linspace(0, 1, num_frames) (smooth: eased by
    (cos(pi (t + 1)) + 1) / 2), the first context view's near and far for every frame, one render with depth, and the frames as uint8
    [F', 3, Hf, W] ON THE DEVICE: Hf = 2 H + 8 with save_depth (depth_video_frames), else H; loop_reverse appends video[::-1][1:-1].
    Out of scope: the mp4 / wandb / file output (a caller copies the frames to the host when it wants them)."""
    ctx = batch["context"]
    gaussians = encoder(ctx, compute_viewspace_depth=False)["gaussians"]
    t = torch.linspace(0, 1, num_frames, dtype=torch.float32, device=ctx["extrinsics"].device)
    if smooth:
        t = (torch.cos(torch.pi * (t + 1)) + 1) / 2
    extrinsics, intrinsics = trajectory_fn(t)
    h, w = ctx["image"].shape[-2:]
    near, far = ctx["near"][:, :1].expand(-1, num_frames), ctx["far"][:, :1].expand(-1, num_frames)
    output = decoder.forward(gaussians, extrinsics, intrinsics, near, far, (h, w), "depth")
    if save_depth:
        video = depth_video_frames(output.color[0], output.depth[0])
    else:
        video = (output.color[0].clip(min=0, max=1) * 255).type(torch.uint8)
    if loop_reverse:
        video = torch.cat([video, video.flip(dims=(0,))[1:-1]], dim=0)
    return video


def render_video_interpolation_step(encoder, decoder, batch: dict, **kw) -> Tensor:
    """ModelWrapper.render_video_interpolation (model_wrapper.py:710-730): render_video_generic along the interpolation between the first
    and the last context camera of scene 0.  (`render_video_interpolation` above is the demo's multi-view variant and is unchanged.)"""
    ctx = batch["context"]

    def trajectory_fn(t):
        return (interpolate_extrinsics(ctx["extrinsics"][:1, 0], ctx["extrinsics"][:1, -1], t),
                interpolate_intrinsics(ctx["intrinsics"][:1, 0].float(), ctx["intrinsics"][:1, -1].float(), t))

    return render_video_generic(encoder, decoder, batch, trajectory_fn, **kw)


def render_video_wobble_step(encoder, decoder, batch: dict, **kw) -> Tensor:
    """ModelWrapper.render_video_wobble (model_wrapper.py:685-707): 60 frames of the first context camera on a spiral in its own image
    plane that opens to a quarter of the distance between the first and the last context camera (camera_trajectory/wobble.py)."""
    from .visualization.camera_trajectory.wobble import generate_wobble
    ctx = batch["context"]

    def trajectory_fn(t):
        delta = (ctx["extrinsics"][:, 0, :3, 3] - ctx["extrinsics"][:, -1, :3, 3]).norm(dim=-1)
        return (generate_wobble(ctx["extrinsics"][:, 0].float(), delta * 0.25, t),
                ctx["intrinsics"][:, 0, None].float().expand(-1, t.shape[0], -1, -1))

    return render_video_generic(encoder, decoder, batch, trajectory_fn, **{"num_frames": 60, **kw})


def render_video_interpolation_exaggerated_step(encoder, decoder, batch: dict, **kw) -> Tensor:
    """ModelWrapper.render_video_interpolation_exaggerated (model_wrapper.py:733-773): 300 frames, not eased and not looped, along the
    interpolation between the first and the last context camera of scene 0 carried two intervals beyond either end (t * 5 - 2), each pose
    followed by five turns on a circle of half the cameras' distance in its image plane."""
    from .visualization.camera_trajectory.wobble import generate_wobble_transformation
    ctx = batch["context"]

    def trajectory_fn(t):
        delta = (ctx["extrinsics"][:, 0, :3, 3] - ctx["extrinsics"][:, -1, :3, 3]).norm(dim=-1)
        tf = generate_wobble_transformation(delta * 0.5, t, 5, scale_radius_with_t=False)
        s = t * 5 - 2
        return (interpolate_extrinsics(ctx["extrinsics"][:1, 0], ctx["extrinsics"][:1, -1], s) @ tf[:1],
                interpolate_intrinsics(ctx["intrinsics"][:1, 0].float(), ctx["intrinsics"][:1, -1].float(), s))

    return render_video_generic(encoder, decoder, batch, trajectory_fn, **{"num_frames": 300, "smooth": False, "loop_reverse": False, **kw})


CAMERA_PLOT_GT_COLOR = (0.0, 0.75, 0.0)      # ground truth in green, prediction in red
CAMERA_PLOT_PRED_COLOR = (1.0, 0.0, 0.0)


def camera_trajectory_plot(gt_extrinsics: Tensor, gt_intrinsics: Tensor, pred_extrinsics: Tensor, pred_intrinsics: Tensor,
                           resolution: int = 256) -> Tensor:
    """[3, R, 3 R] f32: the ground-truth cameras [V, 4, 4] / [V, 3, 3] and the predicted ones in two colours, drawn by draw_cameras and seen
    along the three axes side by side.  A STATED SUBSTITUTE for the plotly / pytorch3d figure of model_wrapper.py:668-679
    (create_plotly_cameras_visualization), which is not built: the same information -- where the predicted trajectory leaves the true
    one -- as three orthographic views instead of one perspective view, without axes and without a dashed line style."""
    from .visualization import layout
    from .visualization.drawing import draw_cameras
    n_gt, n_pred = gt_extrinsics.shape[0], pred_extrinsics.shape[0]
    color = torch.tensor([CAMERA_PLOT_GT_COLOR] * n_gt + [CAMERA_PLOT_PRED_COLOR] * n_pred, dtype=torch.float32, device=gt_extrinsics.device)
    views = draw_cameras(resolution, torch.cat((gt_extrinsics.float(), pred_extrinsics.float())),
                         torch.cat((gt_intrinsics.float(), pred_intrinsics.float())), color)
    return layout.hcat(*views, gap=0)


@torch.no_grad()
def validation_step(encoder, decoder, batch: dict, *, lpips_net: LpipsVgg | None = None, distiller=None, distill_only: bool = False,
                    video: bool = True, projections: bool = True, cameras: bool = False, extended_visualization: bool = False) -> dict:
    """ModelWrapper.validation_step (model_wrapper.py:524-704) for a batch of one scene, as device tensors: no .item() and no host copy of
    a result here or in the visualisation functions it calls.  (The decoder's camera set-up, `camera_matrices`, inverts the poses with
    torch.linalg.inv, which looks at its status on the host: rendering waits for the device there, as it does in every other caller.)
      psnr, ssim, lpips     the means over the target views (lpips only with `lpips_net`); not in the distill-only variant, as in the reference
      comparison            [3, Hc, Wc] f32: hcat of the vcat columns context | context depth | target | prediction | predicted depth
                            (:614-620), or with distill_only (needs `distiller`, the teacher of distill_targets) context | teacher depth |
                            teacher confidence | predicted depth | predicted confidence when the encoder returns one (:559-585)
      projections           [3, P, 3 P'] f32 (projections=True, not distill_only): hcat of render_projections(gaussians, 256)[0] (:624-630)
      video                 uint8 frames of render_video_interpolation_step (video=True, not distill_only; :696-704 render it for two views)
      cameras               [3, 256, 3 * 256 + 16] f32 (cameras=True, not distill_only): hcat of render_cameras(batch, 256), the context and
                            target cameras with their near and far planes (validation_in_3d.py:100-122)
      camera_traj           [3, 256, 3 * 256] f32 (cameras=True, not distill_only): camera_trajectory_plot of the context cameras against
                            model_outs["gaussian_camera_extrins"] / ["gaussian_camera_intrins"] (the context intrinsics when the encoder
                            returns none), the stated substitute for the plotly figure of :658-679
      video_exaggerated     uint8 frames of render_video_interpolation_exaggerated_step (extended_visualization=True and video=True, not
                            distill_only; :647-648)
    Both options are off by default, and every other output is the same with and without them.  render_video_wobble_step is built but, as
    in the reference (:646), not called here.
    Out of scope: text labels (add_label needs a font file), the plotly figure itself, and the wandb, file and mp4 output."""
    from .misc import utils as viz
    from .visualization import layout, validation_in_3d
    ctx, tgt = batch["context"], batch["target"]
    b, _, _, h, w = tgt["image"].shape
    assert b == 1, "validation_step takes one scene, as the reference does"
    if distill_only and distiller is None:
        raise ValueError("validation_step(distill_only=True) needs the distiller")
    model_outs = encoder(ctx, distill=True, compute_viewspace_depth=True) if distill_only else encoder(ctx, compute_viewspace_depth=True)
    context_img = viz.inverse_normalize(ctx["image"][0])
    out = {}
    if distill_only:
        gt1, gt2 = distiller(ctx, False)
        pts1, pts2 = gt1["pts3d"], gt2["pts3d"]
        c2w = ctx["extrinsics"][:, 1].float()
        # the second view's points in its own camera: R^-1 (p - t), only the depth row; R is a rotation, the reference inverts it
        rel = pts2 - c2w[:, None, None, :3, 3]
        depth2 = (torch.linalg.inv_ex(c2w[:, :3, :3]).inverse[:, None, None, 2, :] * rel).sum(-1)
        teacher_depth = viz.vis_depth_map(torch.cat([pts1[..., -1], depth2]))
        teacher_conf = viz.confidence_map(torch.cat([gt1["conf"], gt2["conf"]]))
        columns = [layout.vcat(*context_img), layout.vcat(*teacher_depth), layout.vcat(*teacher_conf),
                   layout.vcat(*viz.vis_depth_map(model_outs["context_view_depths"][0]))]
        if model_outs.get("confidence") is not None:
            columns.append(layout.vcat(*viz.confidence_map(model_outs["confidence"][0])))
        out["comparison"] = layout.hcat(*columns)
        return out
    gaussians = model_outs["gaussians"]
    output = decoder.forward(gaussians, tgt["extrinsics"], tgt["intrinsics"], tgt["near"], tgt["far"], (h, w), "depth")
    rgb_pred, rgb_gt = output.color[0], tgt["image"][0]
    out["psnr"] = compute_psnr(rgb_gt, rgb_pred).mean()
    out["ssim"] = compute_ssim(rgb_gt, rgb_pred).mean()
    if lpips_net is not None:
        out["lpips"] = compute_lpips(rgb_gt, rgb_pred, lpips_net).mean()
    out["comparison"] = layout.hcat(layout.vcat(*context_img), layout.vcat(*viz.vis_depth_map(model_outs["context_view_depths"][0])),
                                    layout.vcat(*rgb_gt), layout.vcat(*rgb_pred), layout.vcat(*viz.vis_depth_map(output.depth[0])))
    if projections:
        out["projections"] = layout.hcat(*validation_in_3d.render_projections(gaussians, 256, extra_label="")[0])
    if video:
        out["video"] = render_video_interpolation_step(lambda c, **kw: dict(gaussians=gaussians), decoder, batch)
        if extended_visualization:
            out["video_exaggerated"] = render_video_interpolation_exaggerated_step(lambda c, **kw: dict(gaussians=gaussians), decoder, batch)
    if cameras:
        out["cameras"] = layout.hcat(*validation_in_3d.render_cameras(batch, 256))
        pred_intrinsics = model_outs.get("gaussian_camera_intrins")
        out["camera_traj"] = camera_trajectory_plot(ctx["extrinsics"][0], ctx["intrinsics"][0], model_outs["gaussian_camera_extrins"][0],
                                                    ctx["intrinsics"][0] if pred_intrinsics is None else pred_intrinsics[0])
    return out
