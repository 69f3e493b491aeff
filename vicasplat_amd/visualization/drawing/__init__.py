"""Vector drawing on images (the reference's src/visualization/drawing): lines, points and the camera plot.  The per-sample work runs in
the HIP kernels of csrc/draw.hip; the `torch` backend is the reference's algorithm in torch ops."""
from .cameras import compute_aabb, draw_cameras, unproject_frustum_corners
from .coordinate_conversion import generate_conversions
from .lines import draw_lines
from .points import draw_points

__all__ = ["compute_aabb", "draw_cameras", "draw_lines", "draw_points", "generate_conversions", "unproject_frustum_corners"]
