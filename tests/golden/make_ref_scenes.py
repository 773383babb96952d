"""Copies the reference's scene files that hold quadric shapes, and the two files they pull in, byte for byte -> tests/golden/ref_scenes/, keeping the relative layout of the
reference's scenes/ directory so that `Include "../geometry/cube.pbrt"` and `"../images/checkerboard.png"` resolve.  tests/test_front_end_quadrics*.py read them.
samplers/sobol.pbrt is left out: it needs a tables file and says nothing new about shapes.  Run where the reference tree is: python3 tests/golden/make_ref_scenes.py <reference root>"""
import os
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SIX_SHAPES = ["constant", "uv", "2d-checkerboard", "bilerp", "dots", "fbm", "marble", "mix", "scale", "windy", "wrinkled"]
FILES = ["textures/%s.pbrt" % n for n in SIX_SHAPES + ["2d-mappings"]] + ["cameras/depth-of-field.pbrt", "materials/bump.pbrt", "samplers/halton.pbrt", "lights/diffuse.pbrt",
                                                                          "geometry/cube.pbrt", "images/checkerboard.png"]

if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    for f in FILES:
        dst = os.path.join(HERE, "ref_scenes", f)
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        shutil.copyfile(os.path.join(sys.argv[1], "scenes", f), dst)
        print(f, os.path.getsize(dst))
