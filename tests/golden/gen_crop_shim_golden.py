"""Generates tests/golden/crop_shim.npz from the real reference: `apply_crop_shim`, `reflect_views` and `apply_augmentation_shim` of
src/dataset/shims (imported on CPU through ref_import.py; the resize is the installed Pillow's, as in the reference) on the deterministic
examples of tests/data_shims_ref.py golden_example: 2 context + 3 target views of 45 x 80 -> (32, 32) (scaled 32 x 57, crop column 12: an
odd difference) and of 80 x 45 -> (32, 32) (a vertical crop of 12 rows), float inputs as the reference takes them.

Keys, per example <ex> in (wide, tall), per <form> in (plain, reflected = reflect_views ahead of the crop shim), per <g> in (context, target):
  <ex>_<form>_<g>_image_u8 [V, 3, 32, 32] uint8 -- the reference's float image times 255; the generator asserts that float32(u) / 255
  reproduces the reference's float32 output bit for bit, so the bytes lose nothing; <ex>_<form>_<g>_intrinsics, <ex>_<form>_<g>_extrinsics:
  the reference's own float32 outputs.  <ex>_sha256: the digest of the inputs (data_shims_ref.example_digest).
  augmentation_unchanged [16] bool: whether apply_augmentation_shim returned the example unchanged, for the first 16 draws of a
  torch.Generator seeded with 0.  pillow_version, torch_version.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_crop_shim_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main() -> None:
    import PIL
    import torch
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    import ref_import
    ref_import.install()
    from src.dataset.shims.augmentation_shim import apply_augmentation_shim, reflect_views
    from src.dataset.shims.crop_shim import apply_crop_shim
    from data_shims_ref import GOLDEN_EXAMPLES, GOLDEN_SHAPE, example_digest, golden_example

    out = {}
    for ex_name in GOLDEN_EXAMPLES:
        ex_np = golden_example(ex_name)
        out[f"{ex_name}_sha256"] = np.array(example_digest(ex_np))
        example = {g: {k: torch.tensor(v) for k, v in ex_np[g].items()} for g in ("context", "target")}
        forms = dict(plain=example, reflected=dict(context=reflect_views(example["context"]), target=reflect_views(example["target"])))
        for form, ex in forms.items():
            got = apply_crop_shim(ex, GOLDEN_SHAPE)
            for g in ("context", "target"):
                image = got[g]["image"]
                assert image.dtype == torch.float32 and tuple(image.shape[-2:]) == GOLDEN_SHAPE
                u = torch.round(image * 255).to(torch.uint8)
                assert torch.equal(u.to(torch.float32) / 255, image)
                out[f"{ex_name}_{form}_{g}_image_u8"] = u.numpy()
                out[f"{ex_name}_{form}_{g}_intrinsics"] = got[g]["intrinsics"].numpy()
                out[f"{ex_name}_{form}_{g}_extrinsics"] = got[g]["extrinsics"].numpy()
                print(ex_name, form, g, tuple(image.shape), float(image.mean()))
    gen = torch.Generator().manual_seed(0)
    token = dict(context=dict(image=torch.zeros(1, 3, 2, 2), extrinsics=torch.eye(4)[None]), target=dict(image=torch.zeros(1, 3, 2, 2), extrinsics=torch.eye(4)[None]))
    out["augmentation_unchanged"] = np.array([apply_augmentation_shim(token, gen) is token for _ in range(16)])
    print("unchanged:", out["augmentation_unchanged"].astype(int))
    out["pillow_version"] = np.array(PIL.__version__)
    out["torch_version"] = np.array(torch.__version__)
    np.savez_compressed(os.path.join(HERE, "crop_shim.npz"), **out)
    print(os.path.getsize(os.path.join(HERE, "crop_shim.npz")), "bytes")


if __name__ == "__main__":
    main()
