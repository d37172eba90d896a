"""Writes tests/golden/image_prep.npz: what the installed Pillow's ``Image.resize`` gives on small seeded uint8 images, BILINEAR and
BICUBIC, so that the GPU tests of omg_amd/image_prep.py do not depend on the Pillow of the machine they run on.

    python tests/golden/make_golden_image_prep.py

Per case ``{h}x{w}_{oh}x{ow}``: ``in.<case>`` uint8 [h, w, 3] and ``out.<case>.<resample>`` uint8 [oh, ow, 3].  Half of each larger image
is forced to 0 / 255, so the negative lobes of the bicubic filter overshoot and both ends of the 8-bit clip are exercised.  The wide
case (1 x 4200 -> 1 x 2) is a segment beyond the horizontal kernel's LDS buffer."""
import os

import numpy as np
from PIL import Image
import PIL

CASES = [(37, 53, 23, 31), (17, 19, 40, 33), (64, 48, 3, 48), (5, 7, 1, 1), (1, 9, 4, 20), (128, 96, 100, 75), (33, 33, 33, 20),
         (90, 120, 67, 89), (1, 4200, 1, 2)]
RESAMPLE = (2, 3)                       # Image.BILINEAR, Image.BICUBIC


def name(case):
    h, w, oh, ow = case
    return f"{h}x{w}_{oh}x{ow}"


def seeded_image(case):
    h, w, _, _ = case
    rs = np.random.RandomState(1000 + 7 * h + w)
    a = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    if h * w > 500:
        top = h // 2 if h > 1 else 1
        cols = w if h > 1 else w // 2
        a[:top, :cols] = np.where(rs.rand(top, cols, 3) < 0.5, 0, 255).astype(np.uint8)
    return a


def main():
    out = {"pillow_version": np.array(PIL.__version__)}
    for case in CASES:
        a = seeded_image(case)
        out["in." + name(case)] = a
        for r in RESAMPLE:
            out[f"out.{name(case)}.{r}"] = np.asarray(Image.fromarray(a).resize((case[3], case[2]), r))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "image_prep.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
