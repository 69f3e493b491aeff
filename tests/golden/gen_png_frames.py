"""Writes tests/golden/png_frames.npz, the real-image inputs of the PNG encoder's tests (tests/png_ref.py):
  frame       uint8 [256, 256, 3]: an example frame of the reference (examples/05b1462991e38e4d/000005.png), its short side Lanczos-reduced
              to 256 and the centre cropped, as the data shims do it
  small_rgb   uint8 [40, 64, 3]: a 64 x 40 cut of it;  small_grey  uint8 [40, 64, 1]: the cut's luma
  pil_bytes   int64 [3]: the length of the file Image.fromarray(x).save(BytesIO, "PNG") writes for each, in that order (recorded, not asserted)
Data only.  Run from the repository root with the reference checkout's path: python tests/golden/gen_png_frames.py <reference root>
"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))


def pil_bytes(x):
    buf = io.BytesIO()
    Image.fromarray(x if x.shape[2] > 1 else x[:, :, 0]).save(buf, "PNG")
    return len(buf.getvalue())


def main(root):
    import PIL
    im = Image.open(os.path.join(root, "examples", "05b1462991e38e4d", "000005.png")).convert("RGB")
    scale = 256 / min(im.size)
    w, h = max(256, round(im.size[0] * scale)), max(256, round(im.size[1] * scale))
    im = im.resize((w, h), Image.LANCZOS)
    left, top = (w - 256) // 2, (h - 256) // 2
    frame = np.asarray(im.crop((left, top, left + 256, top + 256)))
    small = np.ascontiguousarray(frame[100:140, 96:160])
    grey = np.asarray(Image.fromarray(small).convert("L"))[:, :, None]
    sizes = np.asarray([pil_bytes(frame), pil_bytes(small), pil_bytes(grey)], np.int64)
    path = os.path.join(HERE, "png_frames.npz")
    np.savez_compressed(path, frame=frame, small_rgb=small, small_grey=grey, pil_bytes=sizes)
    print(f"{path}: {os.path.getsize(path)} bytes, PIL's files {sizes.tolist()}, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main(sys.argv[1])
