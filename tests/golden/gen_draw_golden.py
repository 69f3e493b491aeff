"""Generates tests/golden/draw.npz from the real reference, imported on the CPU through ref_import.py: what its own draw_lines, draw_points,
draw_cameras, generate_wobble and generate_wobble_transformation give on the tiny scenes of tests/draw_f64.py.

torch.fx.experimental.symbolic_shapes is imported BEFORE ref_import.install(): otherwise the stub finder answers sympy's optional `flint`
import and torch.broadcast_shapes fails inside draw_lines.  cameras.add_label (it needs a font file) is replaced by the identity.

Keys
  <scene>_p<k>_out [3, H, W], _rgba [4, H, W] (the overlay render() returns, caught at the call), _mask [H, W] (the first
  detect_msaa_pixels result, caught; absent for k = 0): draw_lines / draw_points on the scenes of draw_f64.golden_scenes() with
  num_msaa_passes = k: 0, 1, 2 for the lines_<cap> scenes, 1 for points and oblique.
  cam_E, cam_K, cam_color, cam_near, cam_far: the cameras of draw_f64.cameras(4, 5); cam_plain, cam_planes [3, 3, 32, 32]: draw_cameras
  without and with near / far; cam_corners [4, 4, 3]: unproject_frustum_corners at depth cam_far; cam_aabb_lo, cam_aabb_hi: compute_aabb
  with near and far.
  wob_t, wob_radius, wob_tf (generate_wobble_transformation), wob_tf5 (5 rotations, scale_radius_with_t=False), wob_E, wob (generate_wobble).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_draw_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main() -> None:
    import torch
    import torch.fx.experimental.symbolic_shapes  # noqa: F401  (before the stub finder: see the docstring)
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    import ref_import
    ref_import.install()
    from src.visualization.drawing import cameras as ref_cameras
    from src.visualization.drawing import lines as ref_lines
    from src.visualization.drawing import points as ref_points
    from src.visualization.drawing import rendering as ref_rendering
    from src.visualization.camera_trajectory.wobble import generate_wobble, generate_wobble_transformation
    import draw_f64 as D

    out = dict(torch_version=np.array(torch.__version__))
    caught = {}
    real_render, real_detect = ref_rendering.render, ref_rendering.detect_msaa_pixels

    def render(*a, **k):
        caught["rgba"] = real_render(*a, **k)
        return caught["rgba"]

    def detect(image):
        mask = real_detect(image)
        caught.setdefault("mask", mask[0].numpy().copy())
        return mask

    ref_rendering.render, ref_rendering.detect_msaa_pixels = render, detect
    T = lambda a: torch.tensor(np.asarray(a, np.float32))
    for name, (kind, image, world, cap, x_range, y_range) in D.golden_scenes().items():
        for passes in ((0, 1, 2) if name.startswith("lines_") else (1,)):
            caught.clear()
            if kind == "lines":
                res = ref_lines.draw_lines(T(image), T(world["start"]), T(world["end"]), T(world["color"]), T(world["width"]), cap=cap,
                                           num_msaa_passes=passes, x_range=x_range, y_range=y_range)
            else:
                res = ref_points.draw_points(T(image), T(world["points"]), T(world["color"]), T(world["radius"]), T(world["inner_radius"]),
                                             num_msaa_passes=passes)
            out[f"{name}_p{passes}_out"] = res.numpy()
            out[f"{name}_p{passes}_rgba"] = caught["rgba"].numpy()
            if passes:
                out[f"{name}_p{passes}_mask"] = caught["mask"]
    ref_rendering.render, ref_rendering.detect_msaa_pixels = real_render, real_detect

    ref_cameras.add_label = lambda image, label: image
    E, K, color, near, far = D.cameras(4, 5)
    out.update(cam_E=E, cam_K=K, cam_color=color, cam_near=near, cam_far=far)
    out["cam_plain"] = ref_cameras.draw_cameras(32, T(E), T(K), T(color)).numpy()
    out["cam_planes"] = ref_cameras.draw_cameras(32, T(E), T(K), T(color), T(near), T(far)).numpy()
    out["cam_corners"] = ref_cameras.unproject_frustum_corners(T(E), T(K), T(far)).numpy()
    lo, hi = ref_cameras.compute_aabb(T(E), T(K), T(near), T(far))
    out.update(cam_aabb_lo=lo.numpy(), cam_aabb_hi=hi.numpy())

    t, radius = torch.linspace(0, 1, 7), torch.tensor([0.25, 0.5, 1.5, 2.0])
    out.update(wob_t=t.numpy(), wob_radius=radius.numpy(), wob_E=E, wob_tf=generate_wobble_transformation(radius, t).numpy(),
               wob_tf5=generate_wobble_transformation(radius, t, 5, scale_radius_with_t=False).numpy(), wob=generate_wobble(T(E), radius, t).numpy())
    path = os.path.join(HERE, "draw.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "keys")


if __name__ == "__main__":
    main()
