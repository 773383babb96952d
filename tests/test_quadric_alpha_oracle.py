"""CPU only: the oracle alone on the stage of tests/quadric_alpha_scenes.py (quadrics behind and in front of an alpha-masked triangle grid).  The device comparison of
tests/test_quadric_alpha_gpu.py is against this renderer, so it is shown here, against arithmetic that owes nothing to it, that the mask is NOT inert in that scene: the pixels whose
rays cross the grid in a cut-out cell show the material of the quadric behind the grid, the pixels whose rays cross an opaque cell show the grid's, and a mask that is 1 everywhere
gives another film."""
import numpy as np
import pytest

import quadric_alpha_scenes as QA
from oracle_binding import OracleScene

RES, SPP = (48, 32), 16


def render(host, **kw):
    with OracleScene() as orc, QA.libm1():
        QA.mixed_scene(orc, host, plain=True, res=RES, spp=SPP, **kw)
        rays, _ = orc.generate_camera_rays([0, 0, RES[0], RES[1]], 0)
        xyz, wt, _, _ = orc.render_path_ex(max_depth=2)
        return orc.film_to_rgb(xyz, wt), rays


@pytest.fixture(scope="module")
def films(host):
    return {key: render(host, mask=key[0], inert=key[1]) for key in [("checkerboard", False), ("checkerboard", True), ("imagemap", False), ("imagemap", True)]}


def classify(rays):
    """Per pixel, from the camera ray of its first sample and plain float64 geometry: (crosses an opaque cell, crosses a cut-out cell and then meets the red sphere), each only
    where the whole pixel does the same — the crossing point keeps 0.2 (more than a pixel's footprint, 0.16) from every cell border, from the grid's edge and from the two
    quadrics in front of the grid, and the ray passes the sphere's centre within 0.45 of its radius 0.7."""
    o = rays["o"].astype(np.float64); d = rays["d"].astype(np.float64)
    t0 = -o[:, 2] / d[:, 2]
    x = o[:, 0] + t0 * d[:, 0]; y = o[:, 1] + t0 * d[:, 1]
    cell = lambda v: np.abs(((v + QA.GRID) / (2 * QA.GRID) * QA.CHECKS + 0.5) % 1.0 - 0.5) * (2 * QA.GRID / QA.CHECKS)   # distance to the nearest cell border
    safe = (np.abs(x) < QA.GRID - 0.2) & (np.abs(y) < QA.GRID - 0.2) & (cell(x) > 0.2) & (cell(y) > 0.2)
    safe &= (np.hypot(x + 1.2, y + 1.0) > 1.1) & (np.hypot(x - 1.2, y + 0.9) > 1.1)      # the cone and the paraboloid stand in front of the grid there
    opaque = QA.checker_opaque(x, y)
    c = np.asarray(QA.SPHERE_C, np.float64)
    dn = d / np.linalg.norm(d, axis=1, keepdims=True)
    oc = c - o
    dist = np.linalg.norm(oc - (oc * dn).sum(1, keepdims=True) * dn, axis=1)
    return (safe & opaque).reshape(RES[1], RES[0]), (safe & ~opaque & (dist < 0.45)).reshape(RES[1], RES[0])


def test_holes_show_the_quadric_and_opaque_texels_show_the_mesh(films):
    rgb, rays = films[("checkerboard", False)]
    on_mesh, on_sphere = classify(rays)
    assert on_mesh.sum() >= 40 and on_sphere.sum() >= 8, (int(on_mesh.sum()), int(on_sphere.sum()))
    m = rgb[on_mesh]; q = rgb[on_sphere]
    assert (m[:, 1] > 0).all() and (m[:, 1] > 3 * m[:, 0]).all() and (m[:, 1] > 3 * m[:, 2]).all()      # the grid's Kd (0.1, 0.8, 0.1)
    assert (q[:, 0] > 0).all() and (q[:, 0] > 3 * q[:, 1]).all() and (q[:, 0] > 3 * q[:, 2]).all()      # the sphere's Kd (0.8, 0.1, 0.1), seen THROUGH the grid
    # with the mask at 1 everywhere the same pixels show the grid
    inert = films[("checkerboard", True)][0][on_sphere]
    assert (inert[:, 1] > 3 * inert[:, 0]).all()


@pytest.mark.parametrize("mask", QA.MASKS)
def test_the_mask_is_not_inert(films, mask):
    cut, full = films[(mask, False)][0], films[(mask, True)][0]
    differ = (cut != full).any(-1)
    assert differ.mean() > 0.2, float(differ.mean())
    # a constant-1 mask hides everything behind the grid: no red-dominant pixel is left inside the grid's outline, while the cut-out film has some
    red = lambda im: ((im[..., 0] > 3 * im[..., 1]) & (im[..., 0] > 0.02)).sum()
    assert red(cut) >= 8 and red(full) == 0, (int(red(cut)), int(red(full)))
