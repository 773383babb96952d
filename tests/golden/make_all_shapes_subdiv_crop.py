"""Decodes the reference's own render of its shape showcase (renders/shapes/all-shapes.png, 800 x 400, 8-bit RGB) and keeps the window around the subdivision surface — the pixels
whose centre's camera ray hits one of the surface's triangles (tests/all_shapes_surface.py, with the mesh of tests/loopsubdiv_restatement.py), padded by 8 — as
tests/golden/ref_renders/shapes_all-shapes_subdiv.npz: `rgb`, the pixels exactly as the reference wrote them, and `window` = (row0, row1, col0, col1), half open.
Reads the reference at generation time only: python3 tests/golden/make_all_shapes_subdiv_crop.py <reference root>"""
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    import all_shapes_surface as surf
    img = np.asarray(Image.open(os.path.join(sys.argv[1], "renders", "shapes", "all-shapes.png")).convert("RGB"), np.uint8)
    assert img.shape == (surf.YRES, surf.XRES, 3), img.shape
    mask = surf.hit_mask_cpu(*surf.surface_world())
    r0, r1, c0, c1 = surf.window(mask)
    crop = np.ascontiguousarray(img[r0:r1, c0:c1])
    out = os.path.join(HERE, "ref_renders", "shapes_all-shapes_subdiv.npz")
    np.savez_compressed(out, rgb=crop, window=np.array([r0, r1, c0, c1], np.int32))
    print("shapes/all-shapes, rows %d .. %d, columns %d .. %d: %d pixels on the surface" % (r0, r1, c0, c1, mask.sum()), crop.shape, os.path.getsize(out), "bytes")
