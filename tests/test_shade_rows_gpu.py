"""-m gpu: the shade pass's rows (pbrt-v3-rs_amd/csrc/shade_shapes.h) at the edges where a wrongly picked or wrongly trimmed row would show.  Every scene is rendered three
ways — the CPU oracle (libm mode 1: the device's f64-rounded transcendentals), the device with the row its features pick, the device under PBRT_HIP_SHADE_ROW=full (the row that
compiles everything) — and film, filter weights and ray / path counters must agree bit for bit between all three.  Scenes are <= 2 000 triangles at 32 x 32 .. 48 x 48, 4 spp:
36 blocks of paths in round 0, and at depth 8 the sampler dimensions run past the LDS-staged ones and Russian roulette draws its value."""
import os

import numpy as np
import pytest

import pbrt_hip
import scenes
from oracle_binding import OracleScene, set_libm_mode

pytestmark = pytest.mark.gpu

I4 = (np.eye(4, dtype=np.float32).reshape(16),) * 2


def _bits_equal(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _counters(st):
    return (st.camera_rays, st.regular_rays, st.shadow_rays, st.paths_total, st.paths_zero_radiance)


def _oracle(cap, **kw):
    orc = OracleScene(); cap(orc)
    set_libm_mode(1)
    try:
        oxyz, owt, ost, _ = orc.render_path_ex(**kw)
    finally:
        set_libm_mode(0)
    return oxyz, owt, ost


def _same(g, o, what):
    assert _counters(g[2]) == _counters(o[2]), (what, g[2].as_dict(), o[2].as_dict())
    assert _bits_equal(g[1], o[1]), what
    nb = int((g[0].view(np.uint32) != o[0].view(np.uint32)).any(axis=2).sum())
    assert nb == 0, f"{what}: {nb} pixels differ"


def _render_rows(prod, monkeypatch, **kw):
    """the handle's render with the picked row, then with the full row"""
    monkeypatch.delenv("PBRT_HIP_SHADE_ROW", raising=False)
    picked = prod.render_path(**kw)
    monkeypatch.setenv("PBRT_HIP_SHADE_ROW", "full")
    full = prod.render_path(**kw)
    monkeypatch.delenv("PBRT_HIP_SHADE_ROW", raising=False)
    return picked, full


def _check(cap, monkeypatch, lit=True, **kw):
    o = _oracle(cap, **kw)
    prod = pbrt_hip.Scene(); cap(prod)
    picked, full = _render_rows(prod, monkeypatch, **kw)
    _same(picked, o, "picked row against the oracle")
    _same(full, o, "full row against the oracle")
    _same(picked, full, "picked row against the full row")
    assert (float(o[0].max()) > 0.0) == lit
    return picked, o


def _camera_film(s, host, res=48, spp=4, eye=(0, -4, 0)):
    w2c, c2w = host.look_at(list(eye), [0, 0, 0], [0, 0, 1])
    s.set_camera_perspective(host.perspective_raster_to_camera(40.0, res, res), c2w)
    cb, table, sb = host.film_box(res, res)
    s.set_film(res, res, cb, (0.5, 0.5), table)
    s.set_sampler(0, spp, sb)


def test_infinite_light_only(host, monkeypatch):
    """the headline row: one constant sky, Halton, long paths (dimensions past the LDS tables, Russian roulette)"""
    spec = pbrt_hip.SceneSpec(n_tris=1500, seed=31, xres=48, yres=48, spp=4, kd=(0.9, 0.9, 0.9))
    g, _ = _check(lambda s: pbrt_hip.capture_spec(spec, s, host), monkeypatch, max_depth=8)
    assert g[2].shadow_rays > 0
    _check(lambda s: pbrt_hip.capture_spec(spec, s, host), monkeypatch, max_depth=0)   # environment radiance only


def test_infinite_light_and_one_emissive_triangle(host, monkeypatch):
    """an MIS ray that lands on the sampled emitter runs the area halves of the resolve and of pdf_li; camera rays see its emission"""
    P, idx = host.gen_random_tris(1200, 32)
    tri = np.array([[-0.9, -1.3, -0.9], [0.9, -1.3, -0.9], [0.0, -1.3, 0.9]], np.float32)

    def cap(s):
        m = s.add_material_matte((0.7, 0.7, 0.7), 0.0)
        s.add_light_infinite((0.3, 0.3, 0.4))
        s.add_mesh(P, idx, m)
        lid = s.add_light_diffuse_area((6.0, 5.0, 4.0), 1, two_sided=True)
        s.add_mesh(tri, np.array([0, 1, 2], np.uint32), m, first_area_light=lid)
        _camera_film(s, host)
        s.build_accel(0, 4)
    for strategy in (0, 1):
        _check(cap, monkeypatch, max_depth=5, light_strategy=strategy)


def test_point_spot_and_distant_lights_without_an_infinite_light(host, monkeypatch):
    P, idx = host.gen_random_tris(1500, 33)

    def cap(s):
        m = s.add_material_matte((0.8, 0.6, 0.4), 0.0)
        s.add_light_point((5.0, 5.0, 4.0), (0.5, -2.0, 1.5))
        s.add_light_spot((6, 5, 4), *host.spot(I4, [0.5, -2.6, 0.9], [-0.2, 0.2, -0.3], 40.0, 10.0))
        s.add_light_distant((1.0, 0.9, 0.8), (0.0, -0.6, 0.8))
        s.add_mesh(P, idx, m)
        _camera_film(s, host, eye=(0, -4, 0.5))
        s.build_accel(0, 4)
    for strategy in (0, 2):
        _check(cap, monkeypatch, max_depth=5, light_strategy=strategy)


def test_no_light_at_all(host, monkeypatch):
    spec = pbrt_hip.SceneSpec(n_tris=800, seed=34, xres=32, yres=32, spp=4, env_L=None)
    g, _ = _check(lambda s: pbrt_hip.capture_spec(spec, s, host), monkeypatch, lit=False, max_depth=5)
    assert g[2].shadow_rays == 0 and g[2].regular_rays > g[2].camera_rays


def test_infinite_light_only_with_sobol(host, monkeypatch):
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sobol_subset.npz"))
    spec = pbrt_hip.SceneSpec(n_tris=1500, seed=35, xres=48, yres=40, spp=4)

    def cap(s):
        pbrt_hip.capture_spec(spec, s, host)
        s.set_sobol_tables(z["m32"], z["vdc"], z["vdc_inv"])
        s.set_sampler(1, 4, s.sample_bounds)
    _check(cap, monkeypatch, max_depth=4)


def _two_skies(host, spec, second=(0.1, 0.5, 0.9)):
    l2w, w2l = host.rotate(50.0, (1.0, 0.2, 0.3))

    def cap(s):
        s.add_light_infinite(second, l2w, w2l)   # ahead of the spec's own: two entries in infinite_lights
        pbrt_hip.capture_spec(spec, s, host)
    return cap


def test_infinite_lights_with_the_spatial_strategy(host, monkeypatch):
    """one light: the strategy falls back to uniform and the lean row serves it; two lights: the spatial distribution is live and the lean row must not be picked"""
    spec = pbrt_hip.SceneSpec(n_tris=1500, seed=36, xres=40, yres=40, spp=4)
    _check(lambda s: pbrt_hip.capture_spec(spec, s, host), monkeypatch, max_depth=4, light_strategy=2)
    _check(_two_skies(host, spec), monkeypatch, max_depth=4, light_strategy=2)


def test_two_infinite_lights(host, monkeypatch):
    spec = pbrt_hip.SceneSpec(n_tris=1500, seed=37, xres=40, yres=40, spp=4, env_L=(0.9, 0.6, 0.3))
    for strategy in (0, 1):
        _check(_two_skies(host, spec), monkeypatch, max_depth=5, light_strategy=strategy)


def test_one_handle_rendered_before_and_after_an_area_light_is_added(host, monkeypatch):
    """the row follows the handle's lights: lean for the sky alone, the full one once an emissive triangle exists — and lean again is never launched for it"""
    P, idx = host.gen_random_tris(1200, 38)
    tri = np.array([[-0.9, -1.3, -0.9], [0.9, -1.3, -0.9], [0.0, -1.3, 0.9]], np.float32)

    def sky(s):
        m = s.add_material_matte((0.7, 0.7, 0.7), 0.0)
        s.add_light_infinite((0.5, 0.5, 0.5))
        s.add_mesh(P, idx, m)
        _camera_film(s, host)
        s.build_accel(0, 4)
        return m

    def emitter(s, m):
        lid = s.add_light_diffuse_area((6.0, 5.0, 4.0), 1, two_sided=True)
        s.add_mesh(tri, np.array([0, 1, 2], np.uint32), m, first_area_light=lid)
        s.build_accel(0, 4)

    def both(s):
        emitter(s, sky(s))
    o_sky, o_both = _oracle(sky, max_depth=5, light_strategy=0), _oracle(both, max_depth=5, light_strategy=0)
    assert not _bits_equal(o_sky[0], o_both[0])
    prod = pbrt_hip.Scene()
    m = sky(prod)
    for g in _render_rows(prod, monkeypatch, max_depth=5, light_strategy=0):
        _same(g, o_sky, "before the area light")
    emitter(prod, m)
    for g in _render_rows(prod, monkeypatch, max_depth=5, light_strategy=0):
        _same(g, o_both, "after the area light")


def _cond_rows(L):
    """InfiniteAreaLight's 2 x 2 scalar image for a constant radiance, as add_light_infinite computes it in f32 (without the common sin(theta) factor of a row):
    y of MIPMap::triangle on the single texel at st = ((u + .5) / 2, (v + .5) / 2) — the four bilinear terms sum to tx only up to rounding, and differently for each (ds, dt)"""
    f = np.float32
    out = np.zeros((2, 2), np.float32)
    for v in range(2):
        for u in range(2):
            ds = f(f(f(u) + f(0.5)) / f(2.0)) - f(0.5); ds = f(ds - np.floor(ds))
            dt = f(f(f(v) + f(0.5)) / f(2.0)) - f(0.5); dt = f(dt - np.floor(dt))
            one = f(1.0)
            c = [f(f(f(f(tx * f(one - ds)) * f(one - dt)) + f(f(tx * f(one - ds)) * dt)) + f(f(tx * ds) * f(one - dt))) + f(f(tx * ds) * dt) for tx in map(f, L)]
            out[v, u] = f(f(f(0.212671) * c[0]) + f(f(0.715160) * c[1])) + f(f(0.072169) * c[2])
    return out


def _rows_differ_after_scaling(rows):
    """whether each row's two entries stay different when multiplied by any f32 near sin(pi / 4) (the host's sin is not pinned to the last bit here)"""
    s0 = np.float32(np.sin(np.pi / 4))
    near = [s0]
    for _ in range(3):
        near = [np.nextafter(near[0], np.float32(0)), *near, np.nextafter(near[-1], np.float32(1))]
    return all(np.float32(rows[v, 0] * s) != np.float32(rows[v, 1] * s) for v in range(2) for s in near)


def test_phi_skip_only_where_the_conditional_rows_are_flat(host, monkeypatch):
    """light_pdf_li of a rotated constant sky: with L = 1 both entries of each cond_func row are equal and phi is not computed; with a radiance whose bilinear terms round
    differently per column they differ, and phi has to choose between them as before"""
    assert np.all(_cond_rows((1.0, 1.0, 1.0))[:, 0] == _cond_rows((1.0, 1.0, 1.0))[:, 1])
    rng = np.random.default_rng(39)
    uneven = None
    for _ in range(10000):
        L = tuple(float(x) for x in rng.uniform(0.2, 1.5, 3).astype(np.float32))
        if _rows_differ_after_scaling(_cond_rows(L)):
            uneven = L
            break
    assert uneven is not None
    P, idx = host.gen_random_tris(1500, 40)
    l2w, w2l = host.rotate(37.0, (0.3, 1.0, 0.2))
    for L in ((1.0, 1.0, 1.0), uneven):
        def cap(s):
            m = s.add_material_matte((0.9, 0.9, 0.9), 0.0)
            s.add_light_infinite(L, l2w, w2l)
            s.add_mesh(P, idx, m)
            _camera_film(s, host, res=40)
            s.build_accel(0, 4)
        _check(cap, monkeypatch, max_depth=6)
