"""Generates tests/golden/teacher_tiny.npz, shapes_teacher_{tiny,full}.json and teacher_anchors.npz by running the REAL reference teacher
(src/model/distiller/dust3d_backbone.py, imported on CPU through ref_import.py) on a seeded input with key-seeded golden weights, in
float32 AND float64, and its anchor-frame sampler under fixed numpy seeds.

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_teacher_golden.py
The fixtures are data (weights and inputs are re-derivable from seeds; outputs are recorded results), never reference source.

The tiny configuration: enc_depth 2, dec_depth 12 (create_dpt_head asserts dec_depth > 9), enc_embed_dim 128 with 2 heads, dec_embed_dim 64
with 1 head (the HIP attention needs 64 per head), RoPE100, DPT heads, 2 scenes of 32 x 32 pixels: 2 x 2 tokens per frame, the smallest
grid the DPT heads take (the stride-2 convolution of the last hook leaves one pixel).  The float64 run calls _encode_symmetrized(force_asym
=True), _decoder and _downstream_head directly, because forward() casts the tokens with .float() before the heads.
"""
from __future__ import annotations

import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ref_import  # noqa: E402
from vicasplat_amd.synthetic import golden_weights  # noqa: E402
from tests.teacher_f64 import TINY, teacher_input  # noqa: E402  (the seeded input and the tiny shape, shared with the tests)

inf = float("inf")
FULL = dict(enc_depth=24, dec_depth=12, enc_embed_dim=1024, dec_embed_dim=768, enc_num_heads=16, dec_num_heads=12)
B, H, W, SEED = 2, 32, 32, 0
PROBE = (0, 1, 7, 100, 1000, 5000, 20000, 50000)


def build(cfg, device="cpu"):
    ref_import.install()
    from src.model.distiller.dust3d_backbone import Dust3R
    with torch.device(device):
        return Dust3R(pos_embed="RoPE100", patch_embed_cls="PatchEmbedDust3R", img_size=(512, 512), head_type="dpt", output_mode="pts3d",
                      depth_mode=("exp", -inf, inf), conf_mode=("exp", 1, inf), **cfg).eval()


def checksum(t):
    f = t.detach().double().flatten()
    idx = torch.tensor([p % f.numel() for p in PROBE])
    return torch.cat([f.mean()[None], f.abs().mean()[None], f[idx]]).numpy()


def run(model, image, dtype):
    model = model.to(dtype)
    sums, hooks = {}, []

    def hook(name, first):
        def h(m, a, o):
            sums[name] = checksum(o[0] if first else o)
        return h

    for i, blk in enumerate(model.enc_blocks):
        hooks.append(blk.register_forward_hook(hook(f"enc{i:02d}", False)))
    for i, (b1, b2) in enumerate(zip(model.dec_blocks, model.dec_blocks2)):
        hooks.append(b1.register_forward_hook(hook(f"dec{i:02d}_1", True)))
        hooks.append(b2.register_forward_hook(hook(f"dec{i:02d}_2", True)))
    img = image.to(dtype)
    with torch.no_grad():
        if dtype == torch.float32:
            res1, res2 = model(dict(image=img))
        else:
            (s1, s2), (f1, f2), (p1, p2) = model._encode_symmetrized(dict(img=img[:, 0]), dict(img=img[:, 1]), force_asym=True)
            d1, d2 = model._decoder(f1, p1, f2, p2)
            res1, res2 = model._downstream_head(1, list(d1), s1), model._downstream_head(2, list(d2), s2)
    for h in hooks:
        h.remove()
    names = sorted(sums)
    return dict(pts1=res1["pts3d"].double().numpy(), conf1=res1["conf"].double().numpy(), pts2=res2["pts3d"].double().numpy(),
                conf2=res2["conf"].double().numpy(), blocks=np.stack([sums[k] for k in names]), block_names=np.array(names))


def make_tiny():
    t0 = time.time()
    model = build(TINY)
    shapes = {k: list(v.shape) for k, v in model.state_dict().items()}
    json.dump(shapes, open(os.path.join(HERE, "shapes_teacher_tiny.json"), "w"))
    Wt = golden_weights(shapes, seed=SEED)
    model.load_state_dict(Wt, strict=True)
    image = teacher_input(B, H, W, SEED)
    out = {}
    r32, r64 = run(model, image, torch.float32), run(model, image, torch.float64)
    for k, v in r32.items():
        out["f32_" + k] = v
    for k, v in r64.items():
        out["f64_" + k] = v
    out.update(cfg_B=B, cfg_H=H, cfg_W=W, cfg_seed=SEED, cfg=np.array(repr(sorted(TINY.items()))), lattice_step=1,
               n_params=sum(int(np.prod(s)) for s in shapes.values()))
    for k in ("pts1", "conf1", "pts2", "conf2"):
        out["ref_err_" + k] = np.abs(r32[k] - r64[k]).max() / np.abs(r64[k]).max()
        out["mag_" + k] = np.abs(r64[k]).max()
    path = os.path.join(HERE, "teacher_tiny.npz")
    np.savez_compressed(path, **out)
    print(f"[golden] {path}: {os.path.getsize(path) / 1e3:.0f} kB in {time.time() - t0:.1f}s, {out['n_params'] / 1e6:.1f} M parameters")
    for k in ("pts1", "conf1", "pts2", "conf2"):
        print(f"    {k}: max |f64| {out['mag_' + k]:.4g}   reference f32 - f64, relative to it: {out['ref_err_' + k]:.3e}")


def make_full_shapes():
    model = build(FULL)      # (on the CPU: the meta device trips over the stubbed packages)
    json.dump({k: list(v.shape) for k, v in model.state_dict().items()}, open(os.path.join(HERE, "shapes_teacher_full.json"), "w"))
    print("[golden] shapes_teacher_full.json:", len(model.state_dict()), "keys")


def make_anchors():
    """idx / segment_idx of the reference's ModelWrapper._sample_anchor_frames for B in {1, 3} and V in {2, 5, 8}, as training_step calls
    it (n_frames=2, temporal_compression=1) and, for V in {5, 8}, with its default temporal_compression=4 (the odd-length shift shows only
    there), numpy seeded with 100 B + V.  model_wrapper.py does not import under the stubs (Lightning's logger module checks the
    TensorBoard version and raises), so the method is taken out of the module's source with `ast` at generation time and run with its own
    globals, as reference_load_images does for demo.py."""
    import ast
    from typing import Optional
    src = open(os.path.join(ref_import.REF, "src", "model", "model_wrapper.py")).read()
    cls = next(n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == "ModelWrapper")
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "_sample_anchor_frames")
    fn.returns = None
    for a in fn.args.args:
        a.annotation = None
    ns = dict(torch=torch, np=np, Optional=Optional)
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "model_wrapper.py", "exec"), ns)
    out = {}
    for b in (1, 3):
        for v, tc in ((2, 1), (5, 1), (8, 1), (5, 4), (8, 4)):
            frames = torch.arange(b * v, dtype=torch.float32).reshape(b, v, 1, 1, 1)
            np.random.seed(100 * b + v)
            anchors, idx, seg = ns["_sample_anchor_frames"](None, frames, n_frames=2, temporal_compression=tc)
            tag = f"B{b}_V{v}_tc{tc}"
            out[tag + "_idx"], out[tag + "_segment_idx"], out[tag + "_anchors"] = idx.numpy(), seg.numpy(), anchors.reshape(b, 2).numpy()
    np.savez_compressed(os.path.join(HERE, "teacher_anchors.npz"), **out)
    print("[golden] teacher_anchors.npz:", {k: v.tolist() for k, v in out.items() if k.endswith("idx")})


if __name__ == "__main__":
    which = sys.argv[1:] or ["tiny", "full_shapes", "anchors"]
    if "tiny" in which:
        make_tiny()
    if "full_shapes" in which:
        make_full_shapes()
    if "anchors" in which:
        make_anchors()
