"""Writes vicasplat_amd/visualization/color_tables.py: the `turbo` and `magma` colour maps as 256 rows of three f32 values,
np.float32(matplotlib.colormaps[name](np.arange(256))[:, :3]), in nine significant digits (which name an f32 exactly; checked here).  Run
once where matplotlib is installed (the tables here come from matplotlib 3.10.8); nothing imports matplotlib at run time.

    python vicasplat_amd/visualization/gen_color_tables.py
"""
import os

import numpy as np

NAMES = ("turbo", "magma")


def tables() -> dict:
    import matplotlib
    return {name: np.float32(matplotlib.colormaps[name](np.arange(256))[:, :3]) for name in NAMES}


if __name__ == "__main__":
    import matplotlib
    lines = ['"""The `turbo` and `magma` colour maps of matplotlib %s as 256 rows of (r, g, b), f32 values in nine significant digits.' % matplotlib.__version__,
             'Data only, written by gen_color_tables.py: do not edit."""', "", "TABLES = {"]
    for name, t in tables().items():
        assert t.shape == (256, 3) and t.dtype == np.float32
        rows = [tuple("%.9g" % v for v in row) for row in t]
        assert np.array_equal(np.array([[float(v) for v in row] for row in rows], dtype=np.float32), t), name
        lines.append(f'    "{name}": (')
        lines += ["        (%s)," % ", ".join(row) for row in rows]
        lines.append("    ),")
    lines.append("}")
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "color_tables.py"), "w") as f:
        f.write("\n".join(lines) + "\n")
