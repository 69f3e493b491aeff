"""Generates tests/golden/depth_loss.npz from the real reference: `LossDepth` of src/loss/loss_depth.py (imported on CPU through
ref_import.py) on the inputs of tests/depth_loss_f64.py make_inputs(2 * 3, 24, 20, seed 5) reshaped to [2, 3, ...], in float32 and in
float64: the loss and its autograd gradient with respect to the rendered depth for the four configurations of depth_loss_f64.CONFIGS
(sigma_image None / 4.0, first / second derivative; weight 0.25).  Keys: f32_<tag>_loss, f32_<tag>_d_depth, f64_... with <tag> =
depth_loss_f64.tag(sigma, second).  The inputs are not stored: the generator is deterministic, and the fixture keeps the SHA-256 of their
bytes (depth_loss_f64.inputs_digest) so that a consumer knows it regenerated the same ones.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_depth_loss_golden.py
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPE = (2, 3, 24, 20)
SEED = 5


def main() -> None:
    import torch
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    import ref_import
    ref_import.install()
    from src.loss.loss_depth import LossDepth, LossDepthCfg, LossDepthCfgWrapper
    from depth_loss_f64 import CONFIGS, WEIGHT, inputs_digest, make_inputs, tag

    B, V, H, W = SHAPE
    z = make_inputs(B * V, H, W, SEED)
    out = dict(inputs_sha256=np.array(inputs_digest(z)))
    for name, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        for sigma, second in CONFIGS:
            loss_fn = LossDepth(LossDepthCfgWrapper(LossDepthCfg(WEIGHT, sigma, second)))
            depth = torch.tensor(z["depth"], dtype=dtype).reshape(B, V, H, W).requires_grad_(True)
            batch = dict(target=dict(near=torch.tensor(z["near"], dtype=dtype).reshape(B, V), far=torch.tensor(z["far"], dtype=dtype).reshape(B, V),
                                     image=torch.tensor(z["image"], dtype=dtype).reshape(B, V, 3, H, W)))
            loss = loss_fn(types.SimpleNamespace(depth=depth), batch, None, 0)
            (g,) = torch.autograd.grad(loss, depth)
            out[f"{name}_{tag(sigma, second)}_loss"] = loss.detach().numpy()
            out[f"{name}_{tag(sigma, second)}_d_depth"] = g.numpy()
            print(name, tag(sigma, second), float(loss.detach()))
    out["torch_version"] = np.array(torch.__version__)
    np.savez_compressed(os.path.join(HERE, "depth_loss.npz"), **out)


if __name__ == "__main__":
    main()
