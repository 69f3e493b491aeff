"""The augmentation shim of the reference's dataset loaders (src/dataset/shims/augmentation_shim.py): with probability 1/2, mirror every
image of an example left-right and reflect the extrinsics.

In this package the mirror is not a pass of its own.  `reflect_views` reflects the extrinsics and MARKS the views: it sets
views[crop_shim.MIRROR_KEY], a uint8 flag per view (a second reflection clears it again).  The crop shim, which follows the augmentation shim in
every loader of the reference, consumes the flag, hands it to the kernel -- which reads the mirrored source column, so that the order is the
reference's: mirror, resample, crop -- and removes the key.  The images of marked views are therefore NOT yet mirrored between the two shims.
"""
from __future__ import annotations

import torch
from torch import Tensor

from .crop_shim import MIRROR_KEY


def reflect_extrinsics(extrinsics: Tensor) -> Tensor:
    reflect = torch.eye(4, dtype=torch.float32, device=extrinsics.device)
    reflect[0, 0] = -1
    return reflect @ extrinsics @ reflect


def reflect_views(views: dict) -> dict:
    image = views["image"]
    flag = torch.ones(image.shape[:-3], dtype=torch.uint8, device=image.device)
    if MIRROR_KEY in views:
        flag = flag ^ views[MIRROR_KEY].to(torch.uint8)
    return {
        **views,
        "extrinsics": reflect_extrinsics(views["extrinsics"]),
        MIRROR_KEY: flag,
    }


def draw_augmentation(generator: torch.Generator | None = None) -> bool:
    """The reference's draw: torch.rand(()) from the generator; below 0.5 means unchanged.  True: reflect."""
    return not bool(torch.rand(tuple(), generator=generator) < 0.5)


def apply_augmentation_shim(example: dict, generator: torch.Generator | None = None) -> dict:
    """Randomly augment the training images."""
    # Do not augment with 50% chance.
    if not draw_augmentation(generator):
        return example

    return {
        **example,
        "context": reflect_views(example["context"]),
        "target": reflect_views(example["target"]),
    }
