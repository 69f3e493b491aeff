"""Writes tests/golden/jpeg_cases.npz: for every case of tests/jpeg_ref.py CASES the JPEG stream the installed PIL writes (`<case>.jpg`,
uint8) and the pixels the installed PIL decodes from it (`<case>.rgb`, uint8 [h, w, 3], through .convert("RGB")).  The machine that runs
the GPU tests then needs no encoder and no PIL.  Run from the repository root: python tests/golden/gen_jpeg_cases.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import jpeg_ref as R  # noqa: E402


def main():
    import PIL
    from PIL import features
    assert features.check_feature("libjpeg_turbo"), "the fixture is libjpeg-turbo's decode"
    out = {}
    for name in R.CASES:
        data = R.encode(name)
        out[name + ".jpg"] = np.frombuffer(data, np.uint8)
        out[name + ".rgb"] = R.pil_decode(data)
    np.savez_compressed(R.GOLDEN, **out)
    print(f"{R.GOLDEN}: {len(R.CASES)} cases, {os.path.getsize(R.GOLDEN)} bytes, Pillow {PIL.__version__}, "
          f"libjpeg-turbo {features.version_feature('libjpeg_turbo')}")


if __name__ == "__main__":
    main()
