"""The data side on the HIP path: what turns frames as a dataset delivers them into the batch the encoder and callers.training_step take.

Built: the two shims every loader of the reference ends in (shims.augmentation_shim, shims.crop_shim) and `preprocess_batch`, which applies
them to a collated batch with one launch per view group; and the decode they start from (jpeg): `decode_jpeg_batch` turns the JPEG frames
of a chunk into the packed uint8 buffer the crop shim reads, byte for byte PIL's pixels, and `convert_images` is the reference's function of
that name.  Not built: the dataset readers and the view samplers.
"""
from __future__ import annotations

import torch

from .jpeg import JpegError, convert_images, decode_jpeg_batch, pack_jpeg_batch  # noqa: F401
from .shims.augmentation_shim import apply_augmentation_shim, draw_augmentation, reflect_extrinsics, reflect_views  # noqa: F401
from .shims.crop_shim import MIRROR_KEY, apply_crop_shim, apply_crop_shim_to_views, center_crop, rescale, rescale_and_crop, resample_tables  # noqa: F401


def preprocess_batch(batch: dict, shape: tuple[int, int], *, augment: bool = False, generator: torch.Generator | None = None,
                     normalize_context=None) -> dict:
    """A collated batch of frames at their original resolution -> the batch the encoder and callers.training_step take.

    batch: {"context": {"image" [B, V, 3, h, w], "intrinsics" [B, V, 3, 3], "extrinsics" [B, V, 4, 4], ...}, "target": {the same, Vt views}} on
    a HIP device; the images uint8 (planar, or a decoder's HWC buffer as a permuted view) or float32 in [0, 1].
    augment: one decision per scene, drawn as the reference's apply_augmentation_shim draws it (torch.rand(()) from `generator`, scene 0
    first); a chosen scene has all its views, context and target, mirrored and its extrinsics reflected.
    normalize_context: (mean, std) applied to the context images only, as the reference's apply_normalize_shim does; ((0.5,) * 3, (0.5,) * 3)
    gives the [-1, 1] range the encoder takes.  The target images stay in [0, 1].
    The reference's order holds -- augmentation, then rescale and crop --, at one launch per view group; other keys pass through."""
    ctx, tgt = dict(batch["context"]), dict(batch["target"])
    if augment:
        B = ctx["image"].shape[0]
        chosen = torch.tensor([draw_augmentation(generator) for _ in range(B)], dtype=torch.bool).to(ctx["image"].device)
        for views in (ctx, tgt):
            if views["image"].dim() < 5 or views["image"].shape[0] != B:
                raise ValueError(f"preprocess_batch(augment=True) takes images [B, V, 3, h, w], got {tuple(views['image'].shape)}")
            views["extrinsics"] = torch.where(chosen.view(B, 1, 1, 1), reflect_extrinsics(views["extrinsics"]), views["extrinsics"])
            views[MIRROR_KEY] = chosen.view(B, 1).expand(views["image"].shape[:2]).to(torch.uint8)
    return {
        **batch,
        "context": apply_crop_shim_to_views(ctx, shape, normalize=normalize_context),
        "target": apply_crop_shim_to_views(tgt, shape),
    }
