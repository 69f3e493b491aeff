"""prep_image, save_image of the reference's src/misc/image_io.py:38-68, with the PNG files made on the device (csrc/png.hip).

The reference quantises on the device, copies the raw frame to the host and lets PIL compress it on one core.  Here the frames stay where
they are: one call of vse_png_encode writes every frame's complete file into one device buffer, and what crosses to the host is the
lengths and the used bytes.  include/vicasplat_png.h states the stream; any PNG reader decodes it to exactly the reference's pixels,
uint8(trunc(clip(x, 0, 1) * 255)) (a NaN gives 0, where the reference's cast is undefined).  There is no fallback to PIL.
"""
from __future__ import annotations

from pathlib import Path

import torch
from torch import Tensor

from .. import _lib as L

FILTERS = {"none": L.VSE_FILTER_NONE, "sub": L.VSE_FILTER_SUB, "up": L.VSE_FILTER_UP, "average": L.VSE_FILTER_AVERAGE,
           "paeth": L.VSE_FILTER_PAETH, "adaptive": L.VSE_FILTER_ADAPTIVE}


def _chw(image: Tensor) -> Tensor:
    """The reference's shape rules: [H, W], [C, H, W] or [B, C, H, W] (the batch side by side, b c h w -> c h (b w)) -> [3 or 4, H, W]."""
    if image.ndim == 4:
        b, c, h, w = image.shape
        image = image.permute(1, 2, 0, 3).reshape(c, h, b * w)
    if image.ndim == 2:
        image = image[None]
    if image.ndim != 3:
        raise ValueError(f"an image has 2, 3 or 4 dimensions, got {tuple(image.shape)}")
    if image.shape[0] == 1:
        image = image.expand(3, -1, -1)
    if image.shape[0] not in (3, 4):
        raise ValueError(f"an image has 1, 3 or 4 channels, got {image.shape[0]}")
    return image


def prep_image(image: Tensor) -> Tensor:
    """image f32 in [0, 1] -> uint8 [H, W, C] ON THE DEVICE (the reference returns a numpy array): its shape rules, then
    clip, * 255 in f32 and truncation.  encode_png_batch does this quantisation inside its kernel; this function is for callers that want
    the bytes themselves."""
    L.require_device(image)
    x = _chw(image).detach().float()
    zero, one = x.new_zeros(()), x.new_ones(())
    x = torch.where(x > 0, x, zero)          # a NaN compares false: 0
    x = torch.where(x < 1, x, one)
    return (x * 255).to(torch.uint8).permute(1, 2, 0).contiguous()


def encode_png_device(images: Tensor, filter="adaptive", layout: str | None = None) -> tuple[Tensor, Tensor]:
    """(files uint8 [N, stride], lengths int32 [N]) on the device: file i is files[i, :lengths[i]].  The one call of vse_png_encode, on the
    current stream, without any host synchronisation (it can be captured into a graph).  The arguments are encode_png_batch's."""
    if images.ndim != 4 or images.shape[0] == 0:
        raise ValueError(f"the encoder takes [N, C, H, W] floats or [N, H, W, C] bytes with N >= 1, got {tuple(images.shape)}")
    dev = L.require_device(images)
    mode = FILTERS[filter] if isinstance(filter, str) else int(filter)
    images = images.detach()
    if images.dtype == torch.uint8:
        if layout not in (None, "hwc", "chw"):
            raise ValueError(f"layout is 'hwc' or 'chw', got {layout!r}")
        code = L.VSP_LAYOUT_U8_CHW if layout == "chw" else L.VSP_LAYOUT_U8_HWC
        n, (c, h, w) = images.shape[0], (images.shape[1:] if layout == "chw" else (images.shape[3], images.shape[1], images.shape[2]))
    elif images.is_floating_point():
        code, images = L.VSP_LAYOUT_F32_CHW, images.float()
        n, c, h, w = images.shape
    else:
        raise ValueError(f"images are floating point or uint8, got {images.dtype}")
    images = images.contiguous()
    bound = L.call("vse_png_bound", dev, h, w, c)
    need = L.call("vse_png_workspace_bytes", dev, n, h, w, c)
    stride = (bound + 15) // 16 * 16
    workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty((n, stride), dtype=torch.uint8, device=dev)
    lengths = torch.empty(n, dtype=torch.int32, device=dev)
    L.call("vse_png_encode", dev, L.ptr(images), code, n, h, w, c, mode, L.ptr(workspace), need, L.ptr(out), stride, L.ptr(lengths))
    return out, lengths


def encode_png_batch(images, filter="adaptive", layout: str | None = None) -> list[bytes]:
    """The PNG file of every image, as bytes.  images: a tensor or a list of equally shaped tensors on a HIP device, floating point
    [N, C, H, W] in [0, 1] (quantised in the kernel) or uint8 [N, H, W, C] (`layout="chw"`: uint8 [N, C, H, W]); C = 1 (grey), 3 or 4.
    filter: "adaptive" (per row the type with the smallest sum of absolute values) or "none" / "sub" / "up" / "average" / "paeth" (or the
    VSE_FILTER_* code) for that type on every row.  One entry call for the whole batch (encode_png_device), then one copy of the lengths
    and one of the used bytes."""
    if not isinstance(images, Tensor):
        images = list(images)
        if not images:
            return []
        images = torch.stack(images)
    if images.ndim == 4 and images.shape[0] == 0:
        return []
    out, lengths = encode_png_device(images, filter, layout)
    sizes = lengths.cpu()
    used = out[torch.arange(out.shape[1], device=out.device)[None, :] < lengths[:, None]].cpu().numpy().tobytes()
    files, at = [], 0
    for size in sizes.tolist():
        files.append(used[at:at + size])
        at += size
    return files


def save_images(images, paths, filter="adaptive") -> None:
    """One PNG file per image of the batch (encode_png_batch's forms) at the path of the same index; parent directories are made."""
    paths = [Path(p) for p in paths]
    files = encode_png_batch(images, filter=filter)
    if len(files) != len(paths):
        raise ValueError(f"{len(files)} images for {len(paths)} paths")
    for path, data in zip(paths, files):
        path.parent.mkdir(exist_ok=True, parents=True)
        with open(path, "wb") as f:
            f.write(data)


def save_image(image: Tensor, path) -> None:
    """Save an image, assumed to be in the range 0 - 1: [H, W], [C, H, W] or [B, C, H, W], as the reference takes them."""
    L.require_device(image)
    save_images(_chw(image)[None], [path])
