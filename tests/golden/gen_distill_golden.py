"""Generates tests/golden/distill_regr3d.npz from the real reference: `Regr3D` of src/loss/loss_conf_point.py (imported on CPU through
ref_import.py) in float32 -- torch.quantile wants its q tensor in the input's dtype and the reference builds q in f32 -- on the inputs of
tests/distill_f64.py make_inputs(2, 24, 20, seed 5): the loss and its autograd gradients for normalize_pts off / on, without / with the
predicted confidences (cases n0c0, n0c1, n1c0, n1c1).  The inputs are not stored: the generator is deterministic, and the fixture keeps
the SHA-256 of their bytes (distill_f64.inputs_digest) so that a consumer knows it regenerated the same ones.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_distill_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main() -> None:
    import torch
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    import ref_import
    ref_import.install()
    from src.loss.loss_conf_point import Regr3D
    from distill_f64 import inputs_digest, make_inputs

    z = make_inputs(2, 24, 20, 5)
    out = dict(inputs_sha256=np.array(inputs_digest(z)))
    loss_fn = Regr3D()
    for norm in (0, 1):
        for conf in (0, 1):
            t = {k: torch.tensor(v, requires_grad=k[:2] in ("pr", "pc")) for k, v in z.items()}
            loss = loss_fn(t["gt1"], t["gt2"], t["pr1"], t["pr2"], t["cg1"], t["cg2"], t["pc1"] if conf else None, t["pc2"] if conf else None,
                           normalize_pts=bool(norm))
            wrt = [t["pr1"], t["pr2"]] + ([t["pc1"], t["pc2"]] if conf else [])
            grads = torch.autograd.grad(loss, wrt)
            tag = f"n{norm}c{conf}"
            out[tag + "_loss"] = loss.detach().numpy()
            for name, g in zip(("d_pts1", "d_pts2", "d_conf1", "d_conf2"), grads):
                out[f"{tag}_{name}"] = g.numpy()
            print(tag, float(loss.detach()))
    out["torch_version"] = np.array(torch.__version__)
    np.savez_compressed(os.path.join(HERE, "distill_regr3d.npz"), **out)


if __name__ == "__main__":
    main()
