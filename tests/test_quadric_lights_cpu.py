"""not gpu: tests/quadric_light_restatement.py proved without the device, the float64 yardsticks of the GPU tests held to their own closed forms, the margin of the cylinder's
pdf_li measured, and what of pbrt_hip_add_quadric_light can be checked without a GPU (the declaration, the export, the Python mirror)."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import pbrt_hip
import quadric_light_restatement as QR
import quadric_light_scenes as QS
import reference_scenes as R

F = np.float32
D = np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMA3 = 3.0 * 2.0 ** -24 / (1.0 - 3.0 * 2.0 ** -24)
ALL = range(len(QS.PROBE_LIGHTS))
IDS = [p[0] for p in QS.PROBE_LIGHTS]


def stratified(n_side):
    """n_side^2 stratified u, one jittered point per cell, seeded"""
    rng = np.random.default_rng(77)
    i, j = np.meshgrid(np.arange(n_side), np.arange(n_side), indexing="ij")
    return np.column_stack([(i.ravel() + rng.random(n_side * n_side)) / n_side, (j.ravel() + rng.random(n_side * n_side)) / n_side]).astype(F)


# ---- the C ABI as far as it goes without a device -----------------------------------------------------------------------------------------------------------------------
def test_add_quadric_light_is_declared_and_exported(product):
    header = open(os.path.join(ROOT, "include", "pbrt_hip.h")).read()
    m = re.search(r"\bint\s+pbrt_hip_add_quadric_light\s*\(([^;]*)\)\s*;", header)
    assert m, "pbrt_hip_add_quadric_light is not declared in include/pbrt_hip.h"
    args = [a.strip() for a in m.group(1).split(",")]
    q = re.search(r"\bint\s+pbrt_hip_add_quadric\s*\(([^;]*)\)\s*;", header)
    assert [re.sub(r"\s+", " ", a) for a in args[:-2]] == [re.sub(r"\s+", " ", a.strip()) for a in q.group(1).split(",")], args   # pbrt_hip_add_quadric's arguments, then two more
    assert args[-2].startswith("const float L_rgb") and args[-1] == "int two_sided", args
    assert hasattr(product.lib, "pbrt_hip_add_quadric_light")
    fp = C.POINTER(C.c_float)
    ident = np.eye(4, dtype=np.float32).ravel().ctypes.data_as(fp)
    L = np.ones(3, np.float32).ctypes.data_as(fp)
    f = product.fn("add_quadric_light")
    assert f(None, 3, ident, ident, C.c_float(1), C.c_float(0), C.c_float(0), C.c_float(360), 0, 0, L, 0) != pbrt_hip.OK   # a null handle is an error, not a crash
    assert f(None, 0, None, None, C.c_float(1), C.c_float(-1), C.c_float(1), C.c_float(360), 0, 0, None, 0) != pbrt_hip.OK


def test_python_mirror_names_its_arguments_as_add_quadric_does():
    plain = list(inspect.signature(pbrt_hip.Scene.add_quadric).parameters.values())
    light = list(inspect.signature(pbrt_hip.Scene.add_quadric_light).parameters.values())
    assert [p.name for p in light] == [p.name for p in plain] + ["L", "two_sided"]
    assert [p.default for p in light[:len(plain)]] == [p.default for p in plain]
    assert light[-1].default is False


# ---- 1. the restatement's own proof ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", ALL, ids=IDS)
def test_sampled_points_lie_on_the_shape_and_the_normal_is_unit_and_signed(host, k):
    q = QS.probe_shape(host, k)
    u = stratified(64)
    r = float(q["radius"])
    p_obj = QR.object_point(q, u).astype(D)
    if q["kind"] == QR.DISK:   # in the plane z = height exactly, within the radius; concentric_sample_disk covers the full disk, whatever inner_radius and phi_max say
        assert np.all(p_obj[:, 2] == float(q["height"]))
        rho = np.hypot(p_obj[:, 0], p_obj[:, 1])
        assert rho.max() <= r * (1.0 + GAMMA3) and rho.max() > 0.98 * r and rho.min() < 0.02 * r
        if q["inner_radius"] > 0:
            assert (rho < float(q["inner_radius"])).any()
    else:      # on the cylinder within gamma(3) in object space, before and after the re-projection; z and phi inside the cuts
        assert np.all((p_obj[:, 2] >= float(q["z_min"])) & (p_obj[:, 2] <= float(q["z_max"])))
        for pts in (p_obj, QR.cylinder_reproject(q, QR.object_point(q, u)).astype(D)):
            dev = np.abs(np.hypot(pts[:, 0], pts[:, 1]) - r)
            assert dev.max() <= GAMMA3 * r, (IDS[k], dev.max() / (GAMMA3 * r))
            phi = np.arctan2(pts[:, 1], pts[:, 0]); phi = np.where(phi < 0, phi + 2.0 * math.pi, phi)
            # the angle of the float32 point: inside [0, phi_max] up to the rounding of its coordinates (an angle just below 0 reads as just below 2 pi)
            assert np.all((phi <= float(q["phi_max"]) + 2e-7) | (phi >= 2.0 * math.pi - 2e-7)), (IDS[k], phi.max())
        phi_s = u[:, 1] * q["phi_max"]   # the sampled angle itself, as Cylinder::sample forms it
        assert phi_s.dtype == F and np.all((phi_s >= 0) & (phi_s <= q["phi_max"]))
    p, pe, n = QR.sample(q, u)
    assert np.isfinite(p).all() and np.isfinite(pe).all() and (pe >= 0).all()
    # back through world_to_object in float64: on the shape within the error bound the sample itself reports (p_error carries gamma(3) of the re-projection and of the transform)
    W = q["w2o"].astype(D).reshape(4, 4); O = q["o2w"].astype(D).reshape(4, 4)
    back = p.astype(D) @ W[:3, :3].T + W[:3, 3]
    scale = np.abs(W[:3, :3]).sum(1).max()
    slack = scale * pe.astype(D).max(1) + 4e-7 * (np.abs(back).max(1) + np.abs(W[:3, 3]).max())   # + the float32 world_to_object is not the exact inverse of object_to_world
    if q["kind"] == QR.DISK:
        assert np.all(np.abs(back[:, 2] - float(q["height"])) <= slack)
    else:
        assert np.all(np.abs(np.hypot(back[:, 0], back[:, 1]) - r) <= slack + GAMMA3 * r)
    assert np.abs(np.linalg.norm(n.astype(D), axis=1) - 1.0).max() < 4e-7
    # signed as the orientation says: the object-space normal (+z of a disk, radially outwards of a cylinder) carried by the inverse transpose, negated for reverse_orientation alone
    n_obj = np.tile([0.0, 0.0, 1.0], (len(u), 1)) if q["kind"] == QR.DISK else np.column_stack([back[:, 0], back[:, 1], np.zeros(len(u))])
    want = n_obj @ np.linalg.inv(O[:3, :3])
    want /= np.linalg.norm(want, axis=1, keepdims=True)
    cos = np.einsum("ij,ij->i", want, n.astype(D))
    assert np.all(cos < -0.999999) if q["reverse"] else np.all(cos > 0.999999), (IDS[k], cos.min(), cos.max())


@pytest.mark.parametrize("T", [F, D], ids=["float32", "float64"])
def test_solid_angle_of_a_disk_from_its_axis(host, T):
    """sum 1/pdf / N over 2^16 stratified u = the solid angle 2 pi (1 - h / sqrt(h^2 + R^2)) of a disk seen from an on-axis point, within 5 standard errors"""
    t = R.ctm(host, host.translate((0.5, -0.25, 2.0)))
    u = stratified(256)
    for rev in (False, True):
        q = QR.shape(QR.DISK, t, 0.7, 0.0, 0.0, 360.0, rev)
        for h in (0.3, 1.3, -2.0):
            ref_p = np.array([[0.5, -0.25, 2.0 + h]], T)
            p, pe, n, pdf = QR.sample_solid_angle(q, ref_p, u, T)
            w = 1.0 / pdf.astype(D)
            mean, se = w.mean(), w.std() / math.sqrt(len(w))
            want = 2.0 * math.pi * (1.0 - abs(h) / math.sqrt(h * h + 0.49))
            print("disk", T.__name__, "h", h, "estimate", mean, "se", se, "solid angle", want)
            assert abs(mean - want) <= 5.0 * se, (h, mean, se, want)
            assert se < 0.01 * want


def cylinder_solid_angle_f64(R_, zlo, zhi, ref, n=2048):
    """float64 quadrature (midpoint rule) of int |cos'| / d^2 dA over the full cylinder around the z axis"""
    phi = (np.arange(n) + 0.5) * (2.0 * math.pi / n); z = zlo + (np.arange(n) + 0.5) * ((zhi - zlo) / n)
    P, Z = np.meshgrid(phi, z, indexing="ij")
    w = np.stack([R_ * np.cos(P), R_ * np.sin(P), Z], -1)
    nn = np.stack([np.cos(P), np.sin(P), np.zeros_like(P)], -1)
    v = w - np.asarray(ref, D)
    d2 = (v * v).sum(-1)
    return float((np.abs((nn * v).sum(-1)) / d2 ** 1.5).sum() * R_ * (2.0 * math.pi / n) * ((zhi - zlo) / n))


@pytest.mark.parametrize("T", [F, D], ids=["float32", "float64"])
def test_solid_angle_of_a_cylinder_against_float64_quadrature(host, T):
    """sum 1/pdf / N = int |cos'| / d^2 dA (every point of the wall counts, seen from inside or through the wall: the default sample_solid_angle knows no visibility)"""
    q = QR.shape(QR.CYLINDER, R.ctm(host), 1.0, -0.8, 0.8, 360.0, True)
    u = stratified(256)
    on_axis = cylinder_solid_angle_f64(1.0, -0.8, 0.8, (0.0, 0.0, 0.0))
    assert abs(on_axis - 4.0 * math.pi * 0.8 / math.sqrt(0.64 + 1.0)) < 1e-6 * on_axis   # the quadrature itself: 4 pi sin(elevation of the rim) from the centre
    for ref in ((0.0, 0.0, 0.0), (0.3, -0.2, 0.1), (0.0, 0.0, 1.5), (2.5, 0.5, 0.2)):
        p, pe, n, pdf = QR.sample_solid_angle(q, np.array([ref], T), u, T)
        w = 1.0 / pdf.astype(D)
        mean, se = w.mean(), w.std() / math.sqrt(len(w))
        want = cylinder_solid_angle_f64(1.0, -0.8, 0.8, ref)
        print("cylinder", T.__name__, "ref", ref, "estimate", mean, "se", se, "quadrature", want)
        assert abs(mean - want) <= 5.0 * se, (ref, mean, se, want)
        assert se < 0.01 * want


def test_sample_li_tail_and_its_twin(host):
    """The light's tail: no sample where the pdf is 0 (the point itself, the disk's plane under a translation), radiance on the side the sampled normal faces, the float64
    twin next to the float32 restatement"""
    for k in ALL:
        q = QS.probe_shape(host, k)
        name, kind, steps, radius, a, b, phimax, rev, two = QS.PROBE_LIGHTS[k]
        ref, u = QS.sample_cases(host, k)
        o32 = QR.sample_li(q, QS.PROBE_L, two, ref, u, F)
        o64 = QR.sample_li(q, QS.PROBE_L, two, ref, u, D)
        valid = o32[:, 7] == 1
        assert valid.sum() >= 0.7 * len(ref) and (~valid).sum() >= 12, (name, int(valid.sum()), len(ref))
        assert not o32[~valid].any()
        assert (o32[-12:, 7] == 0).all()   # the touching probes
        lit = o32[valid][:, 4:7].any(1)
        assert np.all(o32[valid][lit][:, 4:7] == np.asarray(QS.PROBE_L, F))
        if two:
            assert lit.all()
        else:
            assert lit.any() and (~lit).any(), name
        both = valid & (o64[:, 7] == 1) & np.isfinite(o32[:, 3]) & (np.abs(ref[:, 0:3]).max(1) < 1e6)
        cos = np.abs(np.einsum("ij,ij->i", o64[both][:, 14:17], o64[both][:, 0:3]))
        ok = cos > 0.05
        rel = np.abs(o32[both][ok][:, 3].astype(D) - o64[both][ok][:, 3]) / o64[both][ok][:, 3]
        assert rel.max() < 2e-4, (name, rel.max())   # far points lose digits in p - ref: the twin is a sanity check here, the bit-for-bit yardstick is the float32 one


# ---- 3. the margin of the cylinder's pdf_li ------------------------------------------------------------------------------------------------------------------------------
def test_disk_restatement_against_its_float64_twin_gives_the_margin(host):
    """Measured here, no code under test in it: the disk's float32 restatement of pdf_li against its float64 twin on the conditioned probes (|n . wi| >= 0.1, distance between
    0.2 and 20 radii, hit points at least 10^-3 radii from a rim).  4 x the largest relative difference is the margin the device's cylinder pdf gets against ITS float64 twin."""
    worst, margin = QS.measured_margin(host)
    print("disk pdf_li, float32 restatement against float64 twin: largest relative difference", worst, "-> margin", margin)
    assert 1e-8 < worst < 1e-4, worst
    for k in QS.DISKS:
        ref, wi, p32, p64, keep = QS.disk_twin(host, k)
        assert (p64[keep] > 0).all() and (p32[keep] > 0).all()


@pytest.mark.parametrize("k", QS.DISKS + QS.CYLINDERS, ids=[IDS[k] for k in QS.DISKS + QS.CYLINDERS])
def test_conditioned_probes_stay_inside_the_cap(host, k):
    """The three constraints set aside at most 2 % of the probes, decided by the float64 twin alone"""
    keep = QS.disk_twin(host, k)[4] if k in QS.DISKS else QS.cylinder_twin(host, k)[3]
    print(IDS[k], "kept", int(keep.sum()), "of", len(keep))
    assert keep.mean() >= 1.0 - QS.COND_CAP, (IDS[k], float(keep.mean()))


@pytest.mark.parametrize("k", QS.CYLINDERS, ids=[IDS[k] for k in QS.CYLINDERS])
def test_reference_arithmetic_of_the_cylinder_stays_inside_the_margin(host, k):
    """The reference's own float32 arithmetic (Cylinder::intersect restated in values) against the float64 analytic hit on the conditioned probes: the generator keeps the
    origins where the quadratic's cancellation does not outgrow the disk's figure, so what the margin then measures on the device is the device"""
    worst, margin = QS.measured_margin(host)
    ref, wi, p64, keep = QS.cylinder_twin(host, k)
    p32 = QS.cylinder_restated(host, k)[2].astype(D)
    rel = np.abs(p32[keep] - p64[keep]) / p64[keep]
    print(IDS[k], "float32 restatement of Cylinder::intersect against the float64 hit: largest relative difference", rel.max(), "margin", margin)
    assert rel.max() <= margin, (IDS[k], float(rel.max()), margin)


def test_disk_pdf_cases_reach_every_exact_case(host):
    """The GPU test's disk probes, on the restatement: hits, misses, rays through the inner hole and the phi cut, rays parallel to the plane; the same bits whatever
    two_sided and orientation say"""
    got = {}
    for k in QS.DISKS:
        q = QS.probe_shape(host, k)
        ref, wi = QS.disk_pdf_cases(host, k)
        got[k], hit = QR.disk_pdf_li(q, ref, wi)
        finite = np.isfinite(ref).all(1)
        assert (got[k][hit & finite] > 0).sum() >= 30 and (~hit).sum() >= 30, (IDS[k], int(hit.sum()))
        assert (got[k][~hit] == 0).all()
    q = QS.probe_shape(host, 0)
    ref, wi = QS.disk_pdf_cases(host, 0)
    W = q["w2o"].astype(D).reshape(4, 4)
    parallel = (wi.astype(D) @ W[:3, :3].T)[:, 2] == 0
    assert parallel.sum() >= 9 and (got[0][parallel] == 0).all()
    assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32)) and np.array_equal(got[0].view(np.uint32), got[2].view(np.uint32))
    q = QS.probe_shape(host, 3)   # the annulus with a phi cut: what the hole and the cut reject
    ref, wi = QS.disk_pdf_cases(host, 3)
    full = dict(q, inner_radius=F(0), phi_max=F(2.0 * np.pi))
    cut_away = QR.disk_pdf_li(full, ref, wi)[1] & ~QR.disk_pdf_li(q, ref, wi)[1]
    assert cut_away.sum() >= 20 and (got[3][cut_away] == 0).all()


# ---- 4. the closed forms' own checks -----------------------------------------------------------------------------------------------------------------------------------------
def test_disk_form_factor_against_monte_carlo():
    """rho Le / 2 [1 - (h^2 + d^2 - R^2) / sqrt((h^2 + d^2 + R^2)^2 - 4 R^2 d^2)] against a float64 Monte Carlo integral of cos cos' / (pi d^2) over the disk"""
    rng = np.random.default_rng(5)
    n = 1 << 20
    rr = QS.DISK_R * np.sqrt(rng.random(n)); ph = 2.0 * math.pi * rng.random(n)
    for d in (0.0, 0.5, 1.4, 2.8):
        v = np.stack([rr * np.cos(ph) - d, rr * np.sin(ph), np.full(n, QS.DISK_H)], -1)
        d2 = (v * v).sum(-1)
        f = QS.DISK_H * QS.DISK_H / (d2 * d2) / math.pi * (math.pi * QS.DISK_R ** 2)
        mean, se = f.mean(), f.std() / math.sqrt(n)
        want = float(QS.disk_floor_radiance(d))
        assert abs(mean - want) <= 5.0 * se and se < 2e-3 * want, (d, mean, se, want)


def test_wall_quadrature_against_its_on_axis_form():
    assert abs(float(QS.wall_patch_radiance(0.0)) - QS.wall_on_axis()) < 1e-12
    rng = np.random.default_rng(6)
    n = 1 << 20
    ph = 2.0 * math.pi * rng.random(n); z = QS.CYL_H * rng.random(n)
    for rr in (0.1, 0.28):   # off the axis: against Monte Carlo over the wall's upper half
        v = np.stack([QS.CYL_R * np.cos(ph) - rr, QS.CYL_R * np.sin(ph), z], -1)
        d2 = (v * v).sum(-1)
        f = z * (QS.CYL_R - rr * np.cos(ph)) / (d2 * d2) / math.pi * (2.0 * math.pi * QS.CYL_R * QS.CYL_H)
        mean, se = f.mean(), f.std() / math.sqrt(n)
        want = float(QS.wall_patch_radiance(rr))
        assert abs(mean - want) <= 5.0 * se and se < 2e-3 * want, (rr, mean, se, want)
