"""-m gpu: frames rendered in bands of tiles (pbrt_hip_set_sample_record_budget; csrc/band_plan.h).  The sample records of a band are resident together, the bands follow each
other through the same buffers, and each band's film pass fills its own tiles' slots.  Every case compares three renders bit for bit — film and weights as uint32, the ray and path
counters —: the banded one, the same handle's one-band render and the oracle in libm mode 1; it asserts the band count of pbrt_hip_get_render_footprint against the planner's
contract restated in tests/test_band_plan_cpu.py, and that the peak record bytes stay within the budget unless a band is a single tile.
Shapes: 16 x 16 tiles, 8 spp, so one whole tile's records are 256 * 8 * 20 = 40 960 bytes."""
import subprocess

import numpy as np
import pytest

import driver_scene as ds
import pbrt_hip
import sphere_light_scenes as sl
from oracle_binding import OracleScene, set_libm_mode
from test_band_plan_cpu import REC, greedy_bands, rank_tile_pixels
from test_whitted_gpu import recursion_scene

pytestmark = pytest.mark.gpu
TILE = 256 * REC          # bytes of one whole tile's records per sample per pixel


def _quad(a, b, c, d):
    return np.array([a, b, c, d], np.float32), np.array([0, 1, 2, 0, 2, 3], np.uint32)


def box_scene(host, filt="box", crop=(0.0, 1.0, 0.0, 1.0), xres=64, yres=48, spp=8, three_lights=False):
    """An open box lit by an emissive quad on its ceiling (two area lights), a red wall, and a tilted quad under a checkerboard texture: the texture pass runs.
    three_lights: a point light besides (the spatial strategy then has three lights to weigh per voxel)."""
    walls = [_quad([-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1]), _quad([-1, -1, 1], [-1, 1, 1], [1, 1, 1], [1, -1, 1]), _quad([-1, 1, -1], [1, 1, -1], [1, 1, 1], [-1, 1, 1]),
             _quad([-1, -1, -1], [-1, 1, -1], [-1, 1, 1], [-1, -1, 1]), _quad([1, -1, -1], [1, -1, 1], [1, 1, 1], [1, 1, -1])]

    def cap(s):
        white = s.add_material_matte((0.7, 0.7, 0.7), 0.0)
        red = s.add_material_matte((0.6, 0.1, 0.1), 15.0)
        checks = s.add_material_matte_tex(s.add_texture_checkerboard(s.add_texture_constant((0.1, 0.2, 0.7)), s.add_texture_constant((0.8, 0.8, 0.6)), su=5.0, sv=5.0))
        for k, (P, idx) in enumerate(walls):
            s.add_mesh(P, idx, red if k == 3 else white)
        lid = s.add_light_diffuse_area((8.0, 7.0, 6.0), 2)
        P, idx = _quad([-0.3, -0.3, 0.98], [0.3, -0.3, 0.98], [0.3, 0.3, 0.98], [-0.3, 0.3, 0.98])
        s.add_mesh(P, idx, white, first_area_light=lid, reverse_orientation=True)
        if three_lights:
            s.add_light_point((1.5, 1.2, 1.0), (-0.6, -0.7, 0.4))
        P, idx = _quad([-0.5, 0.2, -0.6], [0.4, 0.0, -0.7], [0.5, 0.3, 0.1], [-0.4, 0.5, 0.2])
        s.add_mesh(P, idx, checks, UV=np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32))
        _, c2w = host.look_at([0, -3.4, 0], [0, 0, 0], [0, 0, 1])
        s.set_camera_perspective(host.perspective_raster_to_camera(40.0, xres, yres), c2w)
        radius = (0.5, 0.5) if filt == "box" else (2.0, 2.0)
        cb, table, sb = host.film_box(xres, yres, crop_window=crop) if filt == "box" else host.film_filter("gaussian", xres, yres, radius, (2.0, 0.0), crop)
        s.set_film(xres, yres, cb, radius, table)
        s.set_sampler(0, spp, sb)
        s.build_accel(0, 4)
        return [int(v) for v in cb], radius[0]
    return cap


COUNTERS = ("camera_rays", "regular_rays", "shadow_rays", "paths_total", "paths_zero_radiance", "light_distributions_created")


def same(got, want, label, counters=COUNTERS):
    """film, weights and counters, bit for bit"""
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), label
    nb = int((got[0].view(np.uint32) != want[0].view(np.uint32)).any(-1).sum())
    assert nb == 0, (label, nb)
    for f in counters:
        assert getattr(got[2], f) == getattr(want[2], f), (label, f, getattr(got[2], f), getattr(want[2], f))


def oracle_path(orc, **kw):
    set_libm_mode(1)
    try:
        return orc.render_path_ex(**kw)[:3]
    finally:
        set_libm_mode(0)


def check_banded(prod, render, want, tile_px, spp, budgets, label, counters=COUNTERS):
    """render() once in one band and once under every budget: each equals the oracle's `want` and the one-band render; the footprint has the bands the planner's contract gives"""
    prod.set_sample_record_budget(0)
    one = render()
    fp = prod.render_footprint()
    assert fp["bands"] == 1 and fp["band_tiles"] == len(tile_px) and fp["record_bytes"] == sum(tile_px) * spp * REC <= fp["record_budget"], (label, fp)
    same(one, want, label + ": one band against the oracle", counters)
    assert float(one[0].max()) > 0.0
    for budget in budgets:
        prod.set_sample_record_budget(budget)
        got = render()
        fp = prod.render_footprint()
        bands = greedy_bands(tile_px, spp, budget)
        assert len(bands) > 1, (label, budget)
        assert fp["bands"] == len(bands) and fp["band_tiles"] == max(b[1] for b in bands) and fp["record_budget"] == budget, (label, budget, fp)
        assert fp["record_bytes"] == max(b[3] for b in bands) * spp * REC, (label, budget, fp)
        assert fp["record_bytes"] <= budget or fp["band_tiles"] == 1, (label, budget, fp)
        assert fp["chunk_paths"] > 0 and fp["chunk_bytes"] > 0
        same(got, one, f"{label}: budget {budget} against one band", counters)
        same(got, want, f"{label}: budget {budget} against the oracle", counters)
    prod.set_sample_record_budget(0)
    return one


@pytest.fixture(scope="module")
def box_pairs(host):
    """(product scene, oracle's render, cropped bounds, filter radius) of the box scene per (filter, crop), made once"""
    made = {}

    def get(filt, crop=(0.0, 1.0, 0.0, 1.0), **kw):
        key = (filt, crop, tuple(sorted(kw.items())))
        if key not in made:
            prod, orc = pbrt_hip.Scene(), OracleScene()
            cap = box_scene(host, filt, crop)
            cb, radius = cap(prod); cap(orc)
            made[key] = (prod, oracle_path(orc, max_depth=3, **kw), cb, radius)
            orc.close()
        return made[key]
    yield get
    for prod, _, _, _ in made.values():
        prod.close()


@pytest.mark.parametrize("filt", ["box", "gaussian"])
def test_path_integrator_in_bands_of_three_one_and_five_tiles(box_pairs, filt):
    """64 x 48 film: 12 whole tiles under the box filter; 68 x 52 samples = 20 tiles, the last column and row ragged, under a gaussian of radius 2, where a film pixel takes samples
    of up to 25 source pixels and of four tiles"""
    prod, want, cb, radius = box_pairs(filt)
    px = rank_tile_pixels(cb, radius)
    assert len(px) == (12 if filt == "box" else 20)
    budgets = [3 * 8 * TILE, 8 * TILE, 5 * 8 * TILE]
    if filt == "box":
        assert [[b[1] for b in greedy_bands(px, 8, b_)] for b_ in budgets] == [[3, 3, 3, 3], [1] * 12, [5, 5, 2]]
    check_banded(prod, lambda: prod.render_path(max_depth=3), want, px, 8, budgets, filt)


CROP = (5 / 64, 59 / 64, 3 / 48, 41 / 48)   # pixels [5, 59) x [3, 41): no edge on a multiple of 16


@pytest.mark.parametrize("filt", ["box", "gaussian"])
def test_crop_window_not_aligned_to_tiles(box_pairs, filt):
    prod, want, cb, radius = box_pairs(filt, CROP)
    assert cb == [5, 3, 59, 41]
    px = rank_tile_pixels(cb, radius)
    assert len(set(px)) > 1   # ragged tiles
    check_banded(prod, lambda: prod.render_path(max_depth=3), want, px, 8, [3 * 8 * TILE, 8 * TILE], filt + " crop")


def test_tile_part_one_of_three_through_both_entry_points(box_pairs, host):
    import torch
    prod, _, cb, radius = box_pairs("gaussian", CROP)
    _, want, _, _ = box_pairs("gaussian", CROP, tile_part=1, tile_parts=3)
    px = rank_tile_pixels(cb, radius, part=1, parts=3)
    check_banded(prod, lambda: prod.render_path(max_depth=3, tile_part=1, tile_parts=3), want, px, 8, [2 * 8 * TILE, 8 * TILE], "part 1 of 3")

    # the device tile buffers of the three parts, each rendered in bands, merged: the whole frame
    _, whole, _, _ = box_pairs("gaussian", CROP)
    bufs, stats = [], []
    prod.set_sample_record_budget(2 * 8 * TILE)
    for part in range(3):
        buf = torch.full((prod.tile_buffer_floats(16, part, 3),), float("nan"), dtype=torch.float32, device="cuda")   # every slot has to be written
        stats.append(prod.render_path_tiles_device(buf.data_ptr(), max_depth=3, tile_part=part, tile_parts=3))
        assert prod.render_footprint()["bands"] == len(greedy_bands(rank_tile_pixels(cb, radius, part=part, parts=3), 8, 2 * 8 * TILE)) > 1
        bufs.append(buf)
    prod.set_sample_record_budget(0)
    xyz, wt = prod.merge_tiles_device([b.data_ptr() for b in bufs])
    assert np.array_equal(wt.view(np.uint32), whole[1].view(np.uint32)) and np.array_equal(xyz.view(np.uint32), whole[0].view(np.uint32))
    for f in ("camera_rays", "regular_rays", "shadow_rays", "paths_total", "paths_zero_radiance"):
        assert sum(getattr(st, f) for st in stats) == getattr(whole[2], f), f


def test_samples_rounded_up_onto_the_next_pixel_at_a_band_boundary(host):
    """Beyond x = 512 an offset within 2^-15 of 1 puts pixel + offset on the next pixel's coordinate (film_tiles_kernel).  A 32 x 32 crop at x = 537 .. 569 of a 1024 x 64 film,
    512 spp: four tiles, the edge between the first two at x = 553, and a sample of pixel (552, 18) lies ON it (found by listing the camera samples; asserted below).
    One tile per band puts a band boundary on that edge, two per band on the edge between the tile rows."""
    crop = (537 / 1024, 569 / 1024, 16 / 64, 48 / 64)
    prod, orc = pbrt_hip.Scene(), OracleScene()
    cap = box_scene(host, "box", crop, xres=1024, yres=64, spp=512)
    cb, radius = cap(prod); cap(orc)
    assert cb == [537, 16, 569, 48]
    xs = np.tile(np.arange(cb[0], cb[2], dtype=np.float32), cb[3] - cb[1])
    up = on_edge = 0
    for s in range(512):
        pf = prod.generate_camera_rays(cb, s)[1]
        rounded = pf[:, 0] == xs + 1.0          # a whole number that is the NEXT pixel's coordinate (an offset of 0 gives the pixel's own)
        up += int(rounded.sum()); on_edge += int((rounded & (xs == 552.0)).sum())
    assert up > 0, "no sample's film position was rounded up onto a whole number: the case proves nothing"
    assert on_edge > 0, "no rounded-up sample on the tile edge at x = 553"
    want = oracle_path(orc, max_depth=3)
    px = rank_tile_pixels(cb, radius)
    assert px == [256] * 4
    check_banded(prod, lambda: prod.render_path(max_depth=3), want, px, 512, [512 * TILE, 2 * 512 * TILE], "x >= 512")
    prod.close(); orc.close()


def test_bands_together_with_sample_chunks(box_pairs, monkeypatch):
    prod, want, cb, radius = box_pairs("gaussian")
    px = rank_tile_pixels(cb, radius)
    prod.set_sample_record_budget(0)
    plain = prod.render_path(max_depth=3)
    prod.set_sample_record_budget(3 * 8 * TILE)
    banded = prod.render_path(max_depth=3)
    monkeypatch.setenv("PBRT_HIP_MAX_PATHS", str(3 * 256 * 3))   # the largest band has 768 pixels: three samples of each per chunk, three chunks per band
    chunked = prod.render_path(max_depth=3)
    fp = prod.render_footprint()
    assert fp["chunk_paths"] == 3 * 256 * 3 and fp["bands"] == len(greedy_bands(px, 8, 3 * 8 * TILE))
    assert chunked[2].extend_launches == 3 * banded[2].extend_launches > 3 * plain[2].extend_launches
    same(chunked, want, "bands and chunks")
    monkeypatch.delenv("PBRT_HIP_MAX_PATHS")
    monkeypatch.setenv("PBRT_HIP_TEST_CHUNK_OOM", "1")   # 8 -> 4 samples per chunk: two chunks per band
    retried = prod.render_path(max_depth=3)
    assert prod.last_error() == "" and prod.render_footprint()["chunk_paths"] == 3 * 256 * 4
    assert retried[2].extend_launches == 2 * banded[2].extend_launches
    same(retried, want, "bands and the out-of-memory retry")
    monkeypatch.delenv("PBRT_HIP_TEST_CHUNK_OOM")
    prod.set_sample_record_budget(0)


def test_spatial_light_strategy_in_bands(host):
    """Three lights: the voxel distributions made for one band serve the next, so "Distributions created" is the oracle's count"""
    prod, orc = pbrt_hip.Scene(), OracleScene()
    cap = box_scene(host, "box", three_lights=True)
    cb, radius = cap(prod); cap(orc)
    want = oracle_path(orc, max_depth=3, light_strategy=2)
    assert want[2].light_distributions_created > 10
    check_banded(prod, lambda: prod.render_path(max_depth=3, light_strategy=2), want, rank_tile_pixels(cb, radius), 8, [3 * 8 * TILE, 8 * TILE], "spatial")
    prod.close(); orc.close()


@pytest.mark.parametrize("scene", ["mirror_and_glass", "sphere_light"])
def test_whitted_in_bands_of_one_and_three_tiles(host, scene):
    prod, orc = pbrt_hip.Scene(), OracleScene()
    for s in (prod, orc):
        if scene == "mirror_and_glass":
            recursion_scene(s, host, "halton", res=48, spp=4)
        else:
            sl.capture(sl.case_cone, s, host)
    want = sl.oracle_whitted(orc, max_depth=3)
    px = rank_tile_pixels((0, 0, 48, 48), 0.5)
    assert px == [256] * 9
    check_banded(prod, lambda: prod.render_whitted(max_depth=3), want, px, 4, [4 * TILE, 3 * 4 * TILE], scene, counters=COUNTERS[:3])   # (the Whitted driver fills the three ray counters)
    prod.close(); orc.close()


def test_multi_device_handle_with_a_budget_equals_the_single_device_film(box_pairs, host):
    one, want, cb, radius = box_pairs("box")
    multi = pbrt_hip.Scene(devices=[0, 0])
    box_scene(host, "box")(multi)
    multi.set_sample_record_budget(2 * 8 * TILE)
    got = multi.render_path(max_depth=3)
    fp = multi.render_footprint()
    assert fp["bands"] == 3 and fp["band_tiles"] == 2 and fp["record_bytes"] == 2 * 8 * TILE == fp["record_budget"], fp   # six tiles per device
    one.set_sample_record_budget(0)
    same(got, one.render_path(max_depth=3), "two devices in bands against one device")
    same(got, want, "two devices in bands against the oracle")
    multi.set_sample_record_budget(0)
    same(multi.render_path(max_depth=3), want, "two devices, one band each")
    assert multi.render_footprint()["bands"] == 1
    multi.close()


def test_budget_below_one_tiles_records_renders_one_tile_per_band(box_pairs):
    prod, want, cb, radius = box_pairs("box")
    prod.set_sample_record_budget(1)
    got = prod.render_path(max_depth=3)
    fp = prod.render_footprint()
    assert fp["bands"] == 12 and fp["band_tiles"] == 1 and fp["record_budget"] == 1
    assert fp["record_bytes"] == 8 * TILE > fp["record_budget"]   # the overshoot is reported, not refused
    same(got, want, "one tile per band")
    prod.set_sample_record_budget(0)
    again = prod.render_path(max_depth=3)
    fp = prod.render_footprint()
    assert fp["bands"] == 1 and fp["band_tiles"] == 12 and fp["record_bytes"] == 12 * 8 * TILE <= fp["record_budget"]
    same(again, want, "budget 0 afterwards")


def test_front_end_writes_the_same_image_with_and_without_a_budget(tmp_path):
    path = ds.write_files(str(tmp_path))
    images = []
    for name, extra in (("plain.pfm", []), ("banded.pfm", ["--sample-record-budget", str(2 * 256 * ds.SPP * REC)])):
        r = subprocess.run([ds.RENDER_BIN, "--quiet", "--outfile", str(tmp_path / name)] + extra + [path], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        with open(tmp_path / name, "rb") as fh:
            images.append(fh.read())
    assert len(images[0]) > 1000 and images[0] == images[1]
    assert ds.XRES * ds.YRES > 2 * 256   # more pixels than one band holds: the second run was banded
