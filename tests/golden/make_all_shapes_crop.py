"""Decodes the reference's own render of its shape showcase (renders/shapes/all-shapes.png, 800 x 400, 8-bit RGB) and keeps the half on the curves' side of the centre column —
world x < 0: the camera looks down -y with +z up, so that is raster columns 0 .. 399 — as tests/golden/ref_renders/shapes_all-shapes_left.npz, the pixels exactly as the
reference wrote them.  That half holds both curves and lies clear of the subdivision surface (world x in [2, 10]) that tests/golden/ref_scenes/shapes/all-shapes.pbrt leaves
out, and of its shadow.  Reads the reference at generation time only.  Run in the build container: python3 tests/golden/make_all_shapes_crop.py"""
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
COLUMNS = (0, 400)

if __name__ == "__main__":
    img = np.asarray(Image.open("/root/reference/renders/shapes/all-shapes.png").convert("RGB"), np.uint8)
    assert img.shape == (400, 800, 3), img.shape
    crop = np.ascontiguousarray(img[:, COLUMNS[0]:COLUMNS[1]])
    np.savez_compressed(os.path.join(HERE, "ref_renders", "shapes_all-shapes_left.npz"), rgb=crop)
    print("shapes/all-shapes, columns %d .. %d" % COLUMNS, crop.shape)
