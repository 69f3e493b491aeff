"""The distillation teacher of training stage 1 (src/model/distiller/__init__.py): `get_distiller(name)` builds the DUSt3R two-view network
on the HIP kernels.  Parity with the published DUSt3R weights is UNVERIFIED (no checkpoint is available where this package is tested);
the network is pinned against the real reference on seeded weights."""
from __future__ import annotations

import argparse
from typing import Optional

import torch

from .dust3r import Dust3R

DUST3R_SHAPE = dict(enc_depth=24, dec_depth=12, enc_embed_dim=1024, dec_embed_dim=768, enc_num_heads=16, dec_num_heads=12)


def get_distiller(name: str, weight_path: Optional[str] = None, compute_dtype="split") -> Dust3R:
    """The reference's get_distiller: the `dust3r` shape (24 / 12 blocks, widths 1024 / 768, 16 / 12 heads, RoPE100, DPT heads, 512 x 512
    nominal size), in eval mode with frozen parameters.  weight_path: a DUSt3R checkpoint (DUSt3R_ViTLarge_BaseDecoder_512_dpt.pth), whose
    ['model'] is loaded strictly; None leaves the random initialisation (the reference always loads ./pretrained_weights/...).
    'mast3r' raises NotImplementedError: its checkpoint has another head (catmlp + dpt with descriptors), which the reference loads
    non-strictly into this shape and so runs with randomly initialised head layers."""
    if name == "mast3r":
        raise NotImplementedError("get_distiller('mast3r'): the MASt3R checkpoint has another head than this network; only 'dust3r' is implemented")
    if name != "dust3r":
        raise ValueError(f"unexpected name={name!r}: the distillers are 'dust3r' and 'mast3r'")
    distiller = Dust3R(pos_embed="RoPE100", img_size=(512, 512), head_type="dpt", output_mode="pts3d", depth_mode=("exp", -float("inf"), float("inf")),
                       conf_mode=("exp", 1, float("inf")), compute_dtype=compute_dtype, **DUST3R_SHAPE)
    if weight_path is not None:
        load_checkpoint(distiller, weight_path)
    return distiller


def load_checkpoint(distiller: Dust3R, weight_path: str) -> Dust3R:
    """Loads ['model'] of a DUSt3R checkpoint strictly.  The published files carry the training arguments as an argparse.Namespace under
    'args' beside the weights; the weights-only unpickler is told to admit that one class instead of being switched off."""
    with torch.serialization.safe_globals([argparse.Namespace]):
        ckpt = torch.load(weight_path, map_location="cpu", weights_only=True)
    distiller.load_state_dict(ckpt["model"], strict=True)
    return distiller


__all__ = ["Dust3R", "get_distiller", "load_checkpoint", "DUST3R_SHAPE"]
