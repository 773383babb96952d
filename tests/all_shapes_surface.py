"""The subdivision surface of the reference's shape showcase (scenes/shapes/all-shapes.pbrt: `Translate 6 0 2.5  Scale 4 4 4  Shape "loopsubdiv"` of a tetrahedron at the default 3
levels) and the window of its 800 x 400 image that the surface covers: the pixels whose centre's camera ray hits one of the surface's triangles, padded by 8 pixels.  Shared by
tests/golden/make_all_shapes_subdiv_crop.py, which finds the window on the CPU and cuts it from the reference's render, and tests/test_front_end_loopsubdiv_gpu.py, which finds
it again with the device's rays."""
import numpy as np

import loopsubdiv_cases as cases
import loopsubdiv_restatement as LR

XRES, YRES, PAD = 800, 400, 8
O2W = np.array([4, 0, 0, 6, 0, 4, 0, 0, 0, 0, 4, 2.5, 0, 0, 0, 1], np.float32)
W2O = np.array([0.25, 0, 0, -1.5, 0, 0.25, 0, 0, 0, 0, 0.25, -0.625, 0, 0, 0, 1], np.float32)


def surface_world():
    r = LR.subdivide(cases.TETRA_P, cases.TETRA_IDX, 3, O2W, W2O)
    return r.P, r.indices


def pixel_centre_rays():
    """origin and directions of the rays through the pixel centres of the file's camera: LookAt 0 8 0 / 0 0 0 / 0 0 1, fov 50 over the shorter (y) axis, screen window
    [-2, 2] x [-1, 1]; camera x = world x, camera y = world z, camera z = world -y.  Rows first: direction[row * XRES + column]"""
    px = (np.arange(XRES) + 0.5) / XRES * 4.0 - 2.0
    py = 1.0 - (np.arange(YRES) + 0.5) / YRES * 2.0
    tan = np.tan(np.radians(50.0) / 2)
    X, Y = np.meshgrid(px, py)
    return np.array([0.0, 8.0, 0.0]), np.stack([X.ravel() * tan, -np.ones(X.size), Y.ravel() * tan], 1)


def hit_mask_cpu(P, idx):
    """(YRES, XRES) bool: the pixel centre's ray meets a triangle of the mesh (Moeller-Trumbore in float64)"""
    o, d = pixel_centre_rays()
    P = np.asarray(P, np.float64)
    tri = P[np.asarray(idx, np.int64).reshape(-1, 3)]
    hit = np.zeros(len(d), bool)
    for a, b, c in tri:
        e1, e2 = b - a, c - a
        pv = np.cross(d, e2)
        det = pv @ e1
        ok = np.abs(det) > 1e-14
        inv = np.where(ok, 1.0 / np.where(ok, det, 1.0), 0.0)
        tv = o - a
        u = (pv @ tv) * inv
        qv = np.cross(tv, e1)
        v = (d @ qv) * inv
        t = (qv @ e2) * inv
        hit |= ok & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
    return hit.reshape(YRES, XRES)


def window(mask):
    """(row0, row1, col0, col1), half open: the bounding box of the mask's pixels padded by PAD and cut to the image"""
    rows, cols = np.flatnonzero(mask.any(axis=1)), np.flatnonzero(mask.any(axis=0))
    return (max(int(rows[0]) - PAD, 0), min(int(rows[-1]) + 1 + PAD, YRES), max(int(cols[0]) - PAD, 0), min(int(cols[-1]) + 1 + PAD, XRES))
