"""Generates tests/golden/viz.npz from the real reference, imported on the CPU through ref_import.py: what its own vis_depth_map,
confidence_map, layout functions, frame-packing expression, compute_equal_aabb_with_margin and render_cuda_orthographic's `dump` give on
small inputs.  The installed matplotlib is let through for this generator only (ref_import stubs it otherwise), and `cm.get_cmap`, which
matplotlib 3.9 removed, is supplied as a behavioural shim: lambda name: matplotlib.colormaps[name].

Keys
  depth_<case> [2, 24, 32] f32 for the cases of viz_f64.DEPTH_CASES (log-uniform, 10 % zeros; `room` also has one negative value),
  near_<case>, far_<case>: the logs of the two torch.quantile results inside vis_depth_map (caught at the call), x_<case>: the f32 argument
  it hands to apply_color_map_to_image, vis_room [2, 3, 24, 32]: the colours.  conf, x_conf, vis_conf: the same for confidence_map.
  lay_a, lay_b, lay_c and lay_<name>: vcat / hcat / add_border on unequal sizes.  fr_rgb, fr_col, fr_u8, fr_loop: render_video_generic's
  vcat(rgb, depth) -> (video.clip(0, 1) * 255).type(uint8) -> pack([video, video[::-1][1:-1]]).  aabb_*: the equal AABB.  ortho_*: the
  dump of render_cuda_orthographic (filled before the rasterizer, which does not exist here, is called).  turbo, magma: the tables.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_viz_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPE = (2, 24, 32)


def main() -> None:
    import torch
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    import ref_import
    ref_import._STUB_ROOTS.discard("matplotlib")
    import matplotlib
    from matplotlib import cm
    if not hasattr(cm, "get_cmap"):
        cm.get_cmap = lambda name: matplotlib.colormaps[name]
    ref_import.install()
    import src.misc.utils as ref_utils
    from src.visualization import layout as ref_layout
    from src.visualization.drawing.cameras import compute_equal_aabb_with_margin
    from src.model.decoder.cuda_splatting import render_cuda_orthographic
    from einops import pack
    import viz_f64 as V

    out = dict(torch_version=np.array(torch.__version__), matplotlib_version=np.array(matplotlib.__version__))
    caught = {}
    real_quantile, real_apply = torch.Tensor.quantile, ref_utils.apply_color_map_to_image

    def quantile(self, q, *a, **k):
        r = real_quantile(self, q, *a, **k)
        caught[float(q)] = r.log().numpy().copy()
        return r

    def apply(image, name):
        caught["x"] = image.numpy().copy()
        return real_apply(image, name)

    torch.Tensor.quantile, ref_utils.apply_color_map_to_image = quantile, apply
    try:
        for seed, (case, (lo, hi)) in enumerate(V.DEPTH_CASES.items()):
            d = V.log_uniform(SHAPE, lo, hi, seed=10 + seed)
            if case == "room":
                d[1, 3, 5] = -2.0
            vis = ref_utils.vis_depth_map(torch.tensor(d))
            out[f"depth_{case}"], out[f"near_{case}"], out[f"far_{case}"], out[f"x_{case}"] = d, caught[0.01], caught[0.99], caught["x"]
            if case == "room":
                out["vis_room"] = vis.numpy()
            print(case, caught[0.01], caught[0.99])
        conf = 1 + np.random.default_rng(3).exponential(2.0, SHAPE).astype(np.float32)
        out["conf"], out["vis_conf"] = conf, ref_utils.confidence_map(torch.tensor(conf)).numpy()
        out["x_conf"] = caught["x"]
    finally:
        torch.Tensor.quantile, ref_utils.apply_color_map_to_image = real_quantile, real_apply

    g = np.random.default_rng(4)
    a, b, c = (g.uniform(size=s).astype(np.float32) for s in ((3, 5, 7), (3, 4, 9), (3, 6, 6)))
    ta, tb, tc = torch.tensor(a), torch.tensor(b), torch.tensor(c)
    out.update(lay_a=a, lay_b=b, lay_c=c,
               lay_vcat=ref_layout.vcat(ta, tb, tc).numpy(),
               lay_vcat_right_nogap=ref_layout.vcat(ta, tb, tc, align="right", gap=0).numpy(),
               lay_hcat_center=ref_layout.hcat(ta, tb, tc, align="center", gap=3, gap_color=[0.25, 0.5, 0.75]).numpy(),
               lay_hcat_bottom=ref_layout.hcat(ta, tb, align="bottom", gap=1, gap_color=0).numpy(),
               lay_border=ref_layout.add_border(ta, 2, 0.5).numpy())

    rgb = g.uniform(-0.2, 1.2, (3, 3, 6, 8)).astype(np.float32)
    col = g.uniform(0, 1, (3, 3, 6, 8)).astype(np.float32)
    images = [ref_layout.vcat(r, d) for r, d in zip(torch.tensor(rgb), torch.tensor(col))]
    video = (torch.stack(images).clip(min=0, max=1) * 255).type(torch.uint8).cpu().numpy()
    out.update(fr_rgb=rgb, fr_col=col, fr_u8=video, fr_loop=pack([video, video[::-1][1:-1]], "* c h w")[0])

    lo3 = np.array([[-1.0, -0.5, 0.25], [0.0, -2.0, 1.0]], np.float32)
    hi3 = np.array([[1.5, 0.75, 2.0], [0.5, 1.0, 1.25]], np.float32)
    smin, smax = compute_equal_aabb_with_margin(torch.tensor(lo3), torch.tensor(hi3), margin=0.1)
    out.update(aabb_min_in=lo3, aabb_max_in=hi3, aabb_min=smin.numpy(), aabb_max=smax.numpy())

    # one scene: the reference's move_back[2, 3] = -distance_to_near takes a batch of one only (validation_step asserts b == 1)
    E, width, height, near, far = V.projection_cameras(smin.numpy()[:1], smax.numpy()[:1], look_axis=1)
    dump = {}
    T = lambda x: torch.tensor(np.asarray(x, np.float32))
    try:
        render_cuda_orthographic(T(E), T(width), T(height), T(near), T(far), (16, 16), torch.zeros(1, 3), torch.zeros(1, 4, 3),
                                 torch.eye(3).expand(1, 4, 3, 3), torch.zeros(1, 4, 3, 1), torch.ones(1, 4), fov_degrees=10.0, dump=dump)
    except Exception as e:      # the rasterizer is a stub here; the dump is filled before it is reached
        print("render_cuda_orthographic stopped at the rasterizer:", type(e).__name__, str(e)[:300])
    assert set(dump) == {"extrinsics", "fov_x", "fov_y", "near", "far"}
    out.update(ortho_extrinsics_in=np.asarray(E, np.float32), ortho_width=np.asarray(width, np.float32), ortho_height=np.asarray(height, np.float32),
               ortho_near_in=np.asarray(near, np.float32), ortho_far_in=np.asarray(far, np.float32), ortho_fov_degrees=np.array(10.0),
               **{f"ortho_{k}": v.numpy() for k, v in dump.items()})

    for name in ("turbo", "magma"):
        out[name] = np.float32(cm.get_cmap(name)(np.arange(256))[:, :3])
    path = os.path.join(HERE, "viz.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
