"""pbrt_hip — thin ctypes host binding over libpbrt_hip.so (include/pbrt_hip.h).

This is plumbing, not the product: every compute call goes straight through the C ABI into hand-written gfx950
kernels.  The class layout mirrors the reference's plugin surface for the path: a `Scene` is captured
with the same calls the reference's factories make (api/src/graphics_state.rs:254-720) and `render_path` stands in
for `Integrator::render` (core/src/integrator/mod.rs:16-39).

`Binding(lib, prefix)` is deliberately generic over the symbol prefix so that the TEST harness can drive its CPU
checker through the identical Python code; nothing in this package imports, loads or links the checker.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PBRT_HIP_LIB") or os.path.join(os.path.dirname(_HERE), "libpbrt_hip.so")   # PBRT_HIP_LIB: another build of the library (same-box A/B, scripts/build_variant.sh)

OK = 0
ERR_INVALID_ARG, ERR_STATE, ERR_DEVICE, ERR_NO_DEVICE, ERR_UNSUPPORTED, ERR_OOM = -1, -2, -3, -4, -5, -6

RAY_DTYPE = np.dtype([("o", "<f4", 3), ("t_max", "<f4"), ("d", "<f4", 3), ("time", "<f4")])
HIT_DTYPE = np.dtype([("t", "<f4"), ("prim", "<u4"), ("b0", "<f4"), ("b1", "<f4"), ("b2", "<f4"), ("pad", "<u4", 3)])
assert RAY_DTYPE.itemsize == 32 and HIT_DTYPE.itemsize == 32


class Stats(C.Structure):
    _fields_ = [
        ("camera_rays", C.c_uint64), ("regular_rays", C.c_uint64), ("shadow_rays", C.c_uint64),
        ("paths_zero_radiance", C.c_uint64), ("paths_total", C.c_uint64),
        ("render_seconds", C.c_double), ("extend_seconds", C.c_double), ("shadow_seconds", C.c_double),
        ("shade_seconds", C.c_double), ("extend_launches", C.c_uint64), ("shadow_launches", C.c_uint64),
        ("light_distributions_created", C.c_uint64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class PbrtHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"pbrt_hip error {code}: {msg}")
        self.code = code


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape is not None:
        a = a.reshape(shape)
    return a


def _ptr(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype)) if a is not None else None


class Binding:
    """Loads a shared library exporting the include/pbrt_hip.h entry points under `prefix`."""

    def __init__(self, path: str, prefix: str = "pbrt_hip_"):
        if not os.path.exists(path):
            raise PbrtHipError(ERR_NO_DEVICE, f"{path} not built — run __graft_entry__.build() (no CPU fallback exists)")
        self.lib = C.CDLL(path)
        self.prefix = prefix
        self.path = path
        f = self.fn
        vp, fp, ip, u32p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_uint32)
        sig = {
            "device_count": (C.c_int, []),
            "scene_create": (vp, [C.c_int]),
            "scene_destroy": (None, [vp]),
            "last_error": (C.c_char_p, [vp]),
            "add_material_matte": (C.c_int, [vp, fp, C.c_float, u32p]),
            "add_mesh": (C.c_int, [vp, fp, C.c_uint32, u32p, C.c_uint32, fp, fp, fp, C.c_uint32, C.c_int32, C.c_uint32, C.c_float, C.c_float]),
            "add_light_infinite": (C.c_int, [vp, fp, fp, fp]),
            "add_light_distant": (C.c_int, [vp, fp, fp]),
            "add_light_point": (C.c_int, [vp, fp, fp]),
            "add_light_spot": (C.c_int, [vp, fp, fp, fp, C.c_float, C.c_float]),
            "add_light_projection": (C.c_int, [vp, fp, fp, fp, C.c_float, C.c_int, C.c_int, fp]),
            "add_light_goniometric": (C.c_int, [vp, fp, fp, fp, C.c_int, C.c_int, fp]),
            "add_light_diffuse_area": (C.c_int, [vp, fp, C.c_int, C.c_uint32, u32p]),
            "set_camera_perspective": (C.c_int, [vp, fp, fp, C.c_float, C.c_float, C.c_float, C.c_float]),
            "set_camera_orthographic": (C.c_int, [vp, fp, fp, C.c_float, C.c_float, C.c_float, C.c_float]),
            "set_camera_environment": (C.c_int, [vp, fp, C.c_int, C.c_int, C.c_float, C.c_float]),
            "set_film": (C.c_int, [vp, C.c_int, C.c_int, ip, fp, fp, C.c_float, C.c_float]),
            "set_sampler": (C.c_int, [vp, C.c_int, C.c_uint32, ip, C.c_int]),
            "set_sobol_tables": (C.c_int, [vp, u32p, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_size_t]),
            "build_accel": (C.c_int, [vp, C.c_int, C.c_int]),
            "world_bound": (C.c_int, [vp, fp]),
            "intersect_batch": (C.c_int, [vp, vp, vp, C.c_uint64]),
            "occluded_batch": (C.c_int, [vp, vp, vp, C.c_uint64]),
            "render_path": (C.c_int, [vp, C.c_int, C.c_float, C.c_int, ip, C.c_int, C.c_int, C.c_int, fp, fp, C.POINTER(Stats)]),
            "film_to_rgb": (C.c_int, [vp, fp, fp, fp]),
            "generate_camera_rays": (C.c_int, [vp, ip, C.c_uint32, vp, fp]),
        }
        for name, (res, args) in sig.items():
            fn = f(name)
            fn.restype, fn.argtypes = res, args
        self._optional = {
            "intersect_batch_device": (C.c_int, [vp, vp, vp, C.c_uint64, fp]),
            "occluded_batch_device": (C.c_int, [vp, vp, vp, C.c_uint64, fp]),
            "tile_buffer_floats": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64)]),
            "render_whitted": (C.c_int, [vp, C.c_int, ip, C.c_int, C.c_int, C.c_int, fp, fp, C.POINTER(Stats)]),
            "render_whitted_devices": (C.c_int, [vp, C.c_int, ip, C.c_int, C.c_int, C.c_int, fp, fp, C.POINTER(Stats)]),
            "render_whitted_tiles_device": (C.c_int, [vp, C.c_int, ip, C.c_int, C.c_int, C.c_int, vp, C.POINTER(Stats)]),
            "render_direct": (C.c_int, [vp, C.c_int, C.c_int, ip, C.c_int, C.c_int, C.c_int, fp, fp, C.POINTER(Stats)]),
            "render_direct_devices": (C.c_int, [vp, C.c_int, C.c_int, ip, C.c_int, C.c_int, C.c_int, fp, fp, C.POINTER(Stats)]),
            "render_direct_tiles_device": (C.c_int, [vp, C.c_int, C.c_int, ip, C.c_int, C.c_int, C.c_int, vp, C.POINTER(Stats)]),
            "render_path_tiles_device": (C.c_int, [vp, C.c_int, C.c_float, C.c_int, ip, C.c_int, C.c_int, C.c_int, vp, C.POINTER(Stats)]),
            "merge_tiles_device": (C.c_int, [vp, C.c_int, C.c_int, C.POINTER(vp), fp, fp]),
            "add_material_none": (C.c_int, [vp, u32p]),
            "add_material_mirror": (C.c_int, [vp, fp, u32p]),
            "add_material_plastic": (C.c_int, [vp, fp, fp, C.c_float, C.c_int, u32p]),
            "add_material_glass": (C.c_int, [vp, fp, fp, C.c_float, C.c_float, C.c_float, C.c_int, u32p]),
            "add_material_metal": (C.c_int, [vp, fp, fp, C.c_float, C.c_float, C.c_int, u32p]),
            "add_material_uber": (C.c_int, [vp, fp, fp, fp, fp, fp, C.c_float, C.c_float, C.c_float, C.c_int, u32p]),
            "add_material_substrate": (C.c_int, [vp, fp, fp, C.c_float, C.c_float, C.c_int, u32p]),
            "add_material_translucent": (C.c_int, [vp, fp, fp, fp, fp, C.c_float, C.c_int, u32p]),
            "add_material_mix": (C.c_int, [vp, C.c_uint32, C.c_uint32, fp, u32p]),
            "object_begin": (C.c_int, [vp, u32p]),
            "object_end": (C.c_int, [vp]),
            "add_instance": (C.c_int, [vp, C.c_uint32, fp, fp]),
            "add_sphere": (C.c_int, [vp, fp, fp, C.c_float, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint32]),
            "add_sphere_light": (C.c_int, [vp, fp, fp, C.c_float, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint32, fp, C.c_int]),
            "add_quadric_light": (C.c_int, [vp, C.c_int, fp, fp, C.c_float, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint32, fp, C.c_int]),
            "add_hyperboloid": (C.c_int, [vp, fp, fp, fp, fp, C.c_float, C.c_uint32, C.c_uint32]),
            "add_quadric": (C.c_int, [vp, C.c_int, fp, fp, C.c_float, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_uint32]),
            "add_mipmap": (C.c_int, [vp, C.c_int, C.c_int, fp, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_float, u32p]),
            "add_texture_constant": (C.c_int, [vp, fp, u32p]),
            "add_texture_scale": (C.c_int, [vp, C.c_uint32, C.c_uint32, u32p]),
            "add_texture_mix": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, u32p]),
            "add_texture_imagemap": (C.c_int, [vp, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_float, u32p]),
            "add_texture_checkerboard": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, u32p]),
            "add_texture_uv": (C.c_int, [vp, C.c_float, C.c_float, C.c_float, C.c_float, u32p]),
            "add_texture_bilerp": (C.c_int, [vp, fp, fp, fp, fp, C.c_float, C.c_float, C.c_float, C.c_float, u32p]),
            "add_texture_dots": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_float, u32p]),
            "add_light_infinite_map": (C.c_int, [vp, fp, C.c_int, C.c_int, fp, fp, fp]),
            "add_texture_fbm": (C.c_int, [vp, fp, C.c_float, C.c_int, u32p]),
            "add_texture_wrinkled": (C.c_int, [vp, fp, C.c_float, C.c_int, u32p]),
            "add_texture_windy": (C.c_int, [vp, fp, u32p]),
            "add_texture_marble": (C.c_int, [vp, fp, C.c_float, C.c_int, C.c_float, C.c_float, u32p]),
            "add_texture_checkerboard3d": (C.c_int, [vp, C.c_uint32, C.c_uint32, fp, u32p]),
            "set_texture_mapping": (C.c_int, [vp, C.c_uint32, C.c_int, fp]),
            "add_material_matte_tex": (C.c_int, [vp, C.c_uint32, C.c_float, u32p]),
            "set_material_texture": (C.c_int, [vp, C.c_uint32, C.c_int, C.c_uint32]),
            "set_material_bump": (C.c_int, [vp, C.c_uint32, C.c_uint32]),
            "set_material_float_texture": (C.c_int, [vp, C.c_uint32, C.c_int, C.c_uint32]),
            "set_last_mesh_alpha_textures": (C.c_int, [vp, C.c_uint32, C.c_uint32]),
            "texture_eval_batch": (C.c_int, [vp, C.c_uint32, C.c_uint64, fp, fp]),
            "texture_eval_batch_nodiff": (C.c_int, [vp, C.c_uint32, C.c_uint64, fp, fp]),
            "mipmap_levels": (C.c_int, [vp, C.c_uint32, ip, ip]),
            "mipmap_level_texels": (C.c_int, [vp, C.c_uint32, C.c_int, fp]),
            "set_traversal_counting": (C.c_int, [vp, C.c_int]),
            "get_traversal_counts": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
            "accel_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
            "accel_copy": (C.c_int, [vp, vp, C.c_uint64, vp, C.c_uint64]),
            "build_accel_device": (C.c_int, [vp, C.c_int, C.c_int]),
            "build_accel_device_shapes": (C.c_int, [vp, C.c_int, C.c_int]),
            "scene_create_multi": (vp, [ip, C.c_int]),
            "scene_devices": (C.c_int, [vp, ip, C.c_int]),
            "selftest_rccl_gather": (C.c_int, [vp, C.c_uint32, C.POINTER(C.c_uint64)]),
            "set_sample_record_budget": (C.c_int, [vp, C.c_uint64]),
            "get_render_footprint": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
            "get_mis_escape": (C.c_int, [vp, C.POINTER(C.c_int)]),
            "bsdf_probe_batch": (C.c_int, [vp, C.c_uint32, C.c_int, C.c_int, C.c_uint64, fp, fp, fp, u32p, fp, fp]),
            "sampler_value_batch": (C.c_int, [vp, C.c_uint64, ip, u32p, u32p, C.c_int, fp]),
            "light_probe_batch": (C.c_int, [vp, C.c_uint32, C.c_int, C.c_int, C.c_uint64, fp, fp, fp, fp]),
            "raysort_probe": (C.c_int, [vp, C.c_uint32, C.c_uint32, u32p, u32p, C.c_uint32, u32p]),
            "texture_probe_batch": (C.c_int, [vp, C.c_uint32, C.c_int, C.c_uint64, fp, fp]),
            "bump_probe_batch": (C.c_int, [vp, C.c_uint32, C.c_int, C.c_uint64, fp, fp]),
            "set_path_sphere_lights": (C.c_int, [vp, C.c_int]),
            "sphere_light_probe_batch": (C.c_int, [vp, C.c_uint32, C.c_int, C.c_uint64, fp, fp, fp, fp]),
            "spatial_probe_begin": (C.c_int, [vp, ip, u32p]),
            "spatial_probe_batch": (C.c_int, [vp, C.c_uint64, fp, fp, C.c_int, C.POINTER(C.c_int32), u32p, fp, u32p]),
            "spatial_probe_voxel": (C.c_int, [vp, ip, fp, fp, fp]),
            "add_curve": (C.c_int, [vp, fp, fp, C.c_int, fp, fp, fp, C.c_int, C.c_uint32, C.c_uint32]),
            "curve_probe_batch": (C.c_int, [vp, C.c_uint32, C.c_int, C.c_uint64, vp, fp]),
            "surface_probe_batch": (C.c_int, [vp, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_uint64, vp, vp, fp, fp]),
            "loopsubdiv_mesh": (C.c_int, [vp, fp, fp, fp, C.c_uint32, u32p, C.c_uint32, C.c_int, u32p, u32p, fp, fp, u32p]),
            "add_loopsubdiv": (C.c_int, [vp, fp, fp, fp, C.c_uint32, u32p, C.c_uint32, C.c_int, C.c_uint32, C.c_int32, C.c_uint32, C.c_float, C.c_float]),
            "traverse_probe": (C.c_int, [vp, C.c_int, vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp]),
            "film_probe_layout": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64), ip, ip]),
            "film_probe": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_uint64, fp, fp, vp, fp, fp, fp]),
        }
        for name, (res, args) in self._optional.items():
            if hasattr(self.lib, prefix + name):
                fn = f(name)
                fn.restype, fn.argtypes = res, args

    def fn(self, name):
        return getattr(self.lib, self.prefix + name)

    def has(self, name):
        return hasattr(self.lib, self.prefix + name)


_default = None


def default_binding() -> Binding:
    """The product library.  Fails loudly when it has not been built."""
    global _default
    if _default is None:
        _default = Binding(LIB_PATH, "pbrt_hip_")
    return _default


class Host:
    """pbrt_hip_host_* helpers (include/pbrt_hip_host.h): the reference's scene set-up arithmetic, host side."""

    def __init__(self, binding: Binding | None = None):
        b = binding or default_binding()
        self.lib = b.lib
        fp = C.POINTER(C.c_float)
        L = self.lib
        L.pbrt_hip_host_look_at.restype = C.c_int
        L.pbrt_hip_host_gen_random_tris.argtypes = [C.c_uint64, C.c_uint64, fp, C.POINTER(C.c_uint32)]
        L.pbrt_hip_host_rotate.argtypes = [C.c_float, fp, fp, fp]
        L.pbrt_hip_host_perspective_raster_to_camera.argtypes = [C.c_float, C.c_int, C.c_int, fp, fp]
        L.pbrt_hip_host_orthographic_raster_to_camera.argtypes = [C.c_int, C.c_int, fp, fp]
        L.pbrt_hip_host_transform_points.argtypes = [fp, fp, fp, C.c_size_t]
        L.pbrt_hip_host_transform_vectors.argtypes = [fp, fp, fp, C.c_size_t]
        L.pbrt_hip_host_transform_normals.argtypes = [fp, fp, fp, C.c_size_t]
        ip = C.POINTER(C.c_int)
        L.pbrt_hip_host_film_filter.argtypes = [C.c_int, fp, C.c_int, C.c_int, fp, fp, ip, fp, ip]
        L.pbrt_hip_host_film_filter.restype = C.c_int
        L.pbrt_hip_host_spot.argtypes = [fp, fp, fp, fp, C.c_float, C.c_float, fp, fp, fp]
        L.pbrt_hip_host_swaps_handedness.argtypes = [fp]
        L.pbrt_hip_host_swaps_handedness.restype = C.c_int

    @staticmethod
    def _m():
        return np.zeros(16, np.float32)

    def look_at(self, pos, look, up):
        m, mi = self._m(), self._m()
        rc = self.lib.pbrt_hip_host_look_at(_ptr(_f32(pos), C.c_float), _ptr(_f32(look), C.c_float), _ptr(_f32(up), C.c_float), _ptr(m, C.c_float), _ptr(mi, C.c_float))
        if rc != 0:
            raise PbrtHipError(ERR_INVALID_ARG, "look_at: up vector and viewing direction are parallel")
        return m, mi  # world->camera, camera->world

    def translate(self, d):
        m, mi = self._m(), self._m()
        self.lib.pbrt_hip_host_translate(_ptr(_f32(d), C.c_float), _ptr(m, C.c_float), _ptr(mi, C.c_float))
        return m, mi

    def scale(self, s):
        m, mi = self._m(), self._m()
        self.lib.pbrt_hip_host_scale(_ptr(_f32(s), C.c_float), _ptr(m, C.c_float), _ptr(mi, C.c_float))
        return m, mi

    def rotate(self, theta_deg, axis):
        m, mi = self._m(), self._m()
        self.lib.pbrt_hip_host_rotate(C.c_float(theta_deg), _ptr(_f32(axis), C.c_float), _ptr(m, C.c_float), _ptr(mi, C.c_float))
        return m, mi

    def compose(self, a, b):
        m, mi = self._m(), self._m()
        self.lib.pbrt_hip_host_compose(_ptr(a[0], C.c_float), _ptr(a[1], C.c_float), _ptr(b[0], C.c_float), _ptr(b[1], C.c_float), _ptr(m, C.c_float), _ptr(mi, C.c_float))
        return m, mi

    def screen_window(self, xres, yres):
        s = np.zeros(4, np.float32)
        self.lib.pbrt_hip_host_screen_window(xres, yres, _ptr(s, C.c_float))
        return s

    def perspective_raster_to_camera(self, fov, xres, yres, screen=None):
        if screen is None:
            screen = self.screen_window(xres, yres)
        m = self._m()
        self.lib.pbrt_hip_host_perspective_raster_to_camera(C.c_float(fov), xres, yres, _ptr(_f32(screen), C.c_float), _ptr(m, C.c_float))
        return m

    def orthographic_raster_to_camera(self, xres, yres, screen=None):
        if screen is None:
            screen = self.screen_window(xres, yres)
        m = self._m()
        self.lib.pbrt_hip_host_orthographic_raster_to_camera(xres, yres, _ptr(_f32(screen), C.c_float), _ptr(m, C.c_float))
        return m

    def film_box(self, xres, yres, crop_window=(0.0, 1.0, 0.0, 1.0), radius=(0.5, 0.5)):
        cb, sb, table = np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(256, np.float32)
        self.lib.pbrt_hip_host_film_box(xres, yres, _ptr(_f32(crop_window), C.c_float), _ptr(_f32(radius), C.c_float), _ptr(cb, C.c_int), _ptr(table, C.c_float), _ptr(sb, C.c_int))
        return cb, table, sb

    FILTER_KINDS = {"box": 0, "gaussian": 1, "mitchell": 2, "sinc": 3, "triangle": 4}

    def film_filter(self, kind, xres, yres, radius, params=(0.0, 0.0), crop_window=(0.0, 1.0, 0.0, 1.0)):
        """Film::new for any filter of filters/src (kind: name or 0..4) -> (cropped bounds, 16x16 table, sample bounds)."""
        k = self.FILTER_KINDS[kind] if isinstance(kind, str) else int(kind)
        cb, sb, table = np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(256, np.float32)
        rc = self.lib.pbrt_hip_host_film_filter(k, _ptr(_f32(params), C.c_float), xres, yres, _ptr(_f32(crop_window), C.c_float), _ptr(_f32(radius), C.c_float),
                                                _ptr(cb, C.c_int), _ptr(table, C.c_float), _ptr(sb, C.c_int))
        if rc != 0:
            raise PbrtHipError(ERR_INVALID_ARG, f"film_filter: unknown filter kind {kind}")
        return cb, table, sb

    def invert(self, m):
        out = self._m()
        self.lib.pbrt_hip_host_invert(_ptr(_f32(m), C.c_float), _ptr(out, C.c_float))
        return out

    def transform_vectors(self, m, v):
        v = _f32(v, (-1, 3)); out = np.empty_like(v)
        self.lib.pbrt_hip_host_transform_vectors(_ptr(_f32(m), C.c_float), _ptr(v, C.c_float), _ptr(out, C.c_float), len(v))
        return out

    def transform_normals(self, m_inv, n):
        n = _f32(n, (-1, 3)); out = np.empty_like(n)
        self.lib.pbrt_hip_host_transform_normals(_ptr(_f32(m_inv), C.c_float), _ptr(n, C.c_float), _ptr(out, C.c_float), len(n))
        return out

    def swaps_handedness(self, m):
        return bool(self.lib.pbrt_hip_host_swaps_handedness(_ptr(_f32(m), C.c_float)))

    def distant_direction(self, l2w, frm, to):
        w = np.zeros(3, np.float32)
        self.lib.pbrt_hip_host_distant_direction(_ptr(_f32(l2w), C.c_float), _ptr(_f32(frm), C.c_float), _ptr(_f32(to), C.c_float), _ptr(w, C.c_float))
        return w

    def spot(self, ctm, frm, to, cone_angle=30.0, cone_delta=5.0):
        """SpotLight parameters -> (light_to_world, world_to_light, cos_total_width, cos_falloff_start)."""
        l2w, w2l, c = self._m(), self._m(), np.zeros(2, np.float32)
        self.lib.pbrt_hip_host_spot(_ptr(_f32(ctm[0]), C.c_float), _ptr(_f32(ctm[1]), C.c_float), _ptr(_f32(frm), C.c_float), _ptr(_f32(to), C.c_float),
                                    C.c_float(cone_angle), C.c_float(cone_delta), _ptr(l2w, C.c_float), _ptr(w2l, C.c_float), _ptr(c, C.c_float))
        return l2w, w2l, float(c[0]), float(c[1])

    def point_position(self, l2w, l2w_inv, frm):
        p = np.zeros(3, np.float32)
        self.lib.pbrt_hip_host_point_position(_ptr(_f32(l2w), C.c_float), _ptr(_f32(l2w_inv), C.c_float), _ptr(_f32(frm), C.c_float), _ptr(p, C.c_float))
        return p

    def transform_points(self, m, pts):
        pts = _f32(pts, (-1, 3)); out = np.empty_like(pts)
        self.lib.pbrt_hip_host_transform_points(_ptr(_f32(m), C.c_float), _ptr(pts, C.c_float), _ptr(out, C.c_float), len(pts))
        return out

    def gen_random_tris(self, n_tris, seed):
        P = np.empty((3 * n_tris, 3), np.float32)
        idx = np.empty(3 * n_tris, np.uint32)
        self.lib.pbrt_hip_host_gen_random_tris(n_tris, seed, _ptr(P, C.c_float), _ptr(idx, C.c_uint32))
        return P, idx


IDENTITY = np.eye(4, dtype=np.float32).reshape(16)


class Scene:
    """One captured scene on one device (PbrtHipScene*).  Not re-entrant, like the C handle."""

    def __init__(self, binding: Binding | None = None, device: int = 0, devices=None):
        """device: one GPU.  devices: a list of ordinals -> ONE handle driving all of them (pbrt_hip_scene_create_multi; an ordinal may repeat)."""
        self.b = binding or default_binding()
        if devices is not None:
            arr = np.ascontiguousarray(devices, dtype=np.int32)
            self.h = self.b.fn("scene_create_multi")(_ptr(arr, C.c_int), len(arr))
        else:
            self.h = self.b.fn("scene_create")(device)
        if not self.h:
            msg = self.b.fn("last_error")(None)
            raise PbrtHipError(ERR_NO_DEVICE, (msg or b"scene_create failed").decode())
        self.film_shape = None
        self._keep = []

    def close(self):
        if getattr(self, "h", None):
            self.b.fn("scene_destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def last_error(self) -> str:
        """pbrt_hip_last_error: the text of the handle's last failed call (or a warning a successful call left), "" when there is none."""
        return (self.b.fn("last_error")(self.h) or b"").decode()

    def _chk(self, rc):
        if rc != OK:
            msg = self.b.fn("last_error")(self.h)
            raise PbrtHipError(rc, (msg or b"").decode())

    # ---- capture -------------------------------------------------------------------------------------------------
    def add_material_matte(self, kd=(0.5, 0.5, 0.5), sigma=0.0) -> int:
        out = C.c_uint32(0)
        self._chk(self.b.fn("add_material_matte")(self.h, _ptr(_f32(kd), C.c_float), C.c_float(sigma), C.byref(out)))
        return out.value

    def _mat(self, name, *args):
        mid = C.c_uint32()
        self._chk(self.b.fn(name)(self.h, *args, C.byref(mid)))
        return mid.value

    @staticmethod
    def _rgb(v):
        return _ptr(_f32(v), C.c_float)

    def add_material_none(self) -> int:
        return self._mat("add_material_none")

    def add_material_mirror(self, kr=(0.9, 0.9, 0.9)) -> int:
        return self._mat("add_material_mirror", self._rgb(kr))

    def add_material_plastic(self, kd=(0.25, 0.25, 0.25), ks=(0.25, 0.25, 0.25), roughness=0.1, remap_roughness=True) -> int:
        return self._mat("add_material_plastic", self._rgb(kd), self._rgb(ks), C.c_float(roughness), int(remap_roughness))

    def add_material_glass(self, kr=(1, 1, 1), kt=(1, 1, 1), uroughness=0.0, vroughness=0.0, eta=1.5, remap_roughness=True) -> int:
        return self._mat("add_material_glass", self._rgb(kr), self._rgb(kt), C.c_float(uroughness), C.c_float(vroughness), C.c_float(eta), int(remap_roughness))

    def add_material_metal(self, eta, k, uroughness=0.01, vroughness=0.01, remap_roughness=True) -> int:
        return self._mat("add_material_metal", self._rgb(eta), self._rgb(k), C.c_float(uroughness), C.c_float(vroughness), int(remap_roughness))

    def add_material_uber(self, kd=(0.25, 0.25, 0.25), ks=(0.25, 0.25, 0.25), kr=(0, 0, 0), kt=(0, 0, 0), opacity=(1, 1, 1), uroughness=0.1, vroughness=0.1,
                          eta=1.5, remap_roughness=True) -> int:
        return self._mat("add_material_uber", self._rgb(kd), self._rgb(ks), self._rgb(kr), self._rgb(kt), self._rgb(opacity), C.c_float(uroughness),
                         C.c_float(vroughness), C.c_float(eta), int(remap_roughness))

    def add_material_substrate(self, kd=(0.5, 0.5, 0.5), ks=(0.5, 0.5, 0.5), uroughness=0.1, vroughness=0.1, remap_roughness=True) -> int:
        return self._mat("add_material_substrate", self._rgb(kd), self._rgb(ks), C.c_float(uroughness), C.c_float(vroughness), int(remap_roughness))

    def add_material_translucent(self, kd=(0.25,) * 3, ks=(0.25,) * 3, reflect=(0.5,) * 3, transmit=(0.5,) * 3, roughness=0.1, remap_roughness=True) -> int:
        return self._mat("add_material_translucent", self._rgb(kd), self._rgb(ks), self._rgb(reflect), self._rgb(transmit), C.c_float(roughness), int(remap_roughness))

    def add_material_mix(self, material1, material2, amount=(0.5, 0.5, 0.5)) -> int:
        return self._mat("add_material_mix", int(material1), int(material2), self._rgb(amount))

    def add_mesh(self, P, indices, material, N=None, S=None, UV=None, first_area_light=-1, reverse_orientation=False,
                 swaps_handedness=False, alpha=1.0, shadow_alpha=1.0):
        P = _f32(P, (-1, 3)); idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        N = _f32(N, (-1, 3)) if N is not None else None
        S = _f32(S, (-1, 3)) if S is not None else None
        UV = _f32(UV, (-1, 2)) if UV is not None else None
        flags = (1 if reverse_orientation else 0) | (2 if swaps_handedness else 0)
        self._chk(self.b.fn("add_mesh")(self.h, _ptr(P, C.c_float), len(P), _ptr(idx, C.c_uint32), len(idx) // 3, _ptr(N, C.c_float),
                                        _ptr(S, C.c_float), _ptr(UV, C.c_float), material, first_area_light, flags, C.c_float(alpha), C.c_float(shadow_alpha)))

    # Quadric shapes (shapes/src/{sphere,hyperboloid,cylinder,cone,paraboloid,disk}.rs).  object_to_world is handed over as the reference's Transform holds it: the matrix
    # AND its inverse.  Each takes one slot of the primitive list, in call order with the meshes' triangles.
    def add_sphere(self, object_to_world, world_to_object, radius=1.0, z_min=None, z_max=None, phi_max=360.0, material=0, reverse_orientation=False):
        z_min = -radius if z_min is None else z_min
        z_max = radius if z_max is None else z_max
        self._chk(self.b.fn("add_sphere")(self.h, _ptr(_f32(object_to_world), C.c_float), _ptr(_f32(world_to_object), C.c_float), C.c_float(radius), C.c_float(z_min),
                                          C.c_float(z_max), C.c_float(phi_max), material, 1 if reverse_orientation else 0))

    def add_sphere_light(self, object_to_world, world_to_object, radius=1.0, z_min=None, z_max=None, phi_max=360.0, material=0, reverse_orientation=False, L=(1, 1, 1),
                         two_sided=False):
        """add_sphere plus the DiffuseAreaLight whose shape is that sphere (radiance L): the light joins the scene's lights in call order.  Rendered by render_whitted only."""
        z_min = -radius if z_min is None else z_min
        z_max = radius if z_max is None else z_max
        self._chk(self.b.fn("add_sphere_light")(self.h, _ptr(_f32(object_to_world), C.c_float), _ptr(_f32(world_to_object), C.c_float), C.c_float(radius), C.c_float(z_min),
                                                C.c_float(z_max), C.c_float(phi_max), material, 1 if reverse_orientation else 0, _ptr(_f32(L), C.c_float), 1 if two_sided else 0))

    def add_hyperboloid(self, object_to_world, world_to_object, p1, p2, phi_max=360.0, material=0, reverse_orientation=False):
        self._chk(self.b.fn("add_hyperboloid")(self.h, _ptr(_f32(object_to_world), C.c_float), _ptr(_f32(world_to_object), C.c_float), _ptr(_f32(p1), C.c_float),
                                               _ptr(_f32(p2), C.c_float), C.c_float(phi_max), material, 1 if reverse_orientation else 0))

    QUADRIC_KINDS = {"cylinder": 0, "cone": 1, "paraboloid": 2, "disk": 3}

    def add_quadric(self, kind, object_to_world, world_to_object, radius, a, b, phi_max=360.0, material=0, reverse_orientation=False):
        """kind: "cylinder" (a, b = zmin, zmax) | "cone" (a = height) | "paraboloid" (a, b = zmin, zmax) | "disk" (a = height, b = innerradius), or its number"""
        k = self.QUADRIC_KINDS[kind] if isinstance(kind, str) else int(kind)
        self._chk(self.b.fn("add_quadric")(self.h, k, _ptr(_f32(object_to_world), C.c_float), _ptr(_f32(world_to_object), C.c_float), C.c_float(radius), C.c_float(a),
                                           C.c_float(b), C.c_float(phi_max), material, 1 if reverse_orientation else 0))

    def add_quadric_light(self, kind, object_to_world, world_to_object, radius, a, b, phi_max=360.0, material=0, reverse_orientation=False, L=(1, 1, 1), two_sided=False):
        """add_quadric for a "cylinder" or a "disk" plus the DiffuseAreaLight whose shape it is (pbrt_hip_add_quadric_light): the light joins the scene's lights in call order.
        Rendered by render_path (no switch) and render_whitted.  "cone" and "paraboloid" are refused: the reference's Shape::sample for them is todo!()."""
        k = self.QUADRIC_KINDS[kind] if isinstance(kind, str) else int(kind)
        self._chk(self.b.fn("add_quadric_light")(self.h, k, _ptr(_f32(object_to_world), C.c_float), _ptr(_f32(world_to_object), C.c_float), C.c_float(radius), C.c_float(a),
                                                 C.c_float(b), C.c_float(phi_max), material, 1 if reverse_orientation else 0, _ptr(_f32(L), C.c_float), 1 if two_sided else 0))

    CURVE_TYPES = {"flat": 0, "cylinder": 1, "ribbon": 2}

    def add_curve(self, object_to_world, world_to_object, curve_type, cp, width, n=None, split_depth=3, material=0, reverse_orientation=False):
        """Curve::create_segments (shapes/src/curve.rs:105-140, pbrt_hip_add_curve): one cubic Bezier curve, control points cp (4,3) in object space, end widths
        width (2,), type "flat" | "cylinder" | "ribbon" (or its number), a ribbon's end normals n (2,3).  Takes 2^split_depth consecutive slots of the primitive list; a hit
        on a segment reports b0 = u, b1 = v."""
        k = self.CURVE_TYPES[curve_type] if isinstance(curve_type, str) else int(curve_type)
        nn = None if n is None else _f32(n, (6,))
        self._chk(self.b.fn("add_curve")(self.h, _ptr(_f32(object_to_world), C.c_float), _ptr(_f32(world_to_object), C.c_float), k, _ptr(_f32(cp, (12,)), C.c_float),
                                         _ptr(_f32(width, (2,)), C.c_float), _ptr(nn, C.c_float), int(split_depth), material, 1 if reverse_orientation else 0))

    CURVE_PROBE_STRIDE = 20

    def curve_probe(self, prim, rays, shadow=False):
        """curve_test, then curve_surface, of the curve segment in primitive slot `prim` on explicit rays, each with its own t_max (pbrt_hip_curve_probe_batch), a probe for the
        parity tests.  Returns (n,20): hit flag, t, u, v, then world-space p, p_error, dpdu, dpdv, n (one pad word).  shadow=True: Curve::intersect_p's decision in column 0 alone."""
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        out = np.zeros((len(rays), self.CURVE_PROBE_STRIDE), np.float32)
        self._chk(self.b.fn("curve_probe_batch")(self.h, prim, 1 if shadow else 0, len(rays), rays.ctypes.data, _ptr(out, C.c_float)))
        return out

    def loopsubdiv_mesh(self, P, indices, n_levels=3, object_to_world=None, world_to_object=None, counts_only=False):
        """LoopSubDiv::subdivide (shapes/src/loopsubdiv.rs:321-659, pbrt_hip_loopsubdiv_mesh): the control mesh P (n,3), indices refined n_levels times on the device, pushed to
        the limit surface, with the normals s x t, moved to world space by object_to_world and its inverse (None: object space).  Returns (P (V,3), N (V,3), indices (3 F 4^L,));
        counts_only=True validates only and returns (V, F 4^L), no device work."""
        P = _f32(P, (-1, 3)); idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        m = None if object_to_world is None else _f32(object_to_world, (16,))
        mi = None if world_to_object is None else _f32(world_to_object, (16,))
        nv, nt = C.c_uint32(0), C.c_uint32(0)
        call = self.b.fn("loopsubdiv_mesh")
        head = (self.h, _ptr(m, C.c_float), _ptr(mi, C.c_float), _ptr(P, C.c_float) if len(P) else None, len(P), _ptr(idx, C.c_uint32) if len(idx) else None, len(idx), int(n_levels),
                C.byref(nv), C.byref(nt))
        self._chk(call(*head, None, None, None))
        if counts_only:
            return nv.value, nt.value
        oP, oN, oI = np.empty((nv.value, 3), np.float32), np.empty((nv.value, 3), np.float32), np.empty(3 * nt.value, np.uint32)
        self._chk(call(*head, _ptr(oP, C.c_float), _ptr(oN, C.c_float), _ptr(oI, C.c_uint32)))
        return oP, oN, oI

    def add_loopsubdiv(self, P, indices, n_levels=3, material=0, object_to_world=None, world_to_object=None, first_area_light=-1, reverse_orientation=False,
                       swaps_handedness=False, alpha=1.0, shadow_alpha=1.0):
        """pbrt_hip_add_loopsubdiv: loopsubdiv_mesh followed by exactly what add_mesh does with its P, N and indices; an area light needs one light per OUTPUT triangle
        (add_light_diffuse_area(L, n_tris=F 4^L), the count loopsubdiv_mesh(.., counts_only=True) gives)."""
        P = _f32(P, (-1, 3)); idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        m = None if object_to_world is None else _f32(object_to_world, (16,))
        mi = None if world_to_object is None else _f32(world_to_object, (16,))
        flags = (1 if reverse_orientation else 0) | (2 if swaps_handedness else 0)
        self._chk(self.b.fn("add_loopsubdiv")(self.h, _ptr(m, C.c_float), _ptr(mi, C.c_float), _ptr(P, C.c_float) if len(P) else None, len(P), _ptr(idx, C.c_uint32) if len(idx) else None,
                                              len(idx), int(n_levels), material, first_area_light, flags, C.c_float(alpha), C.c_float(shadow_alpha)))

    def object_begin(self) -> int:
        """ObjectBegin (api/src/lib.rs:911-925): meshes added until object_end() belong to the returned object."""
        oid = C.c_uint32()
        self._chk(self.b.fn("object_begin")(self.h, C.byref(oid)))
        return oid.value

    def object_end(self):
        self._chk(self.b.fn("object_end")(self.h))

    def add_instance(self, object_id, instance_to_world, world_to_instance):
        """ObjectInstance (lib.rs:942-1000): one TransformedPrimitive in the scene's primitive list."""
        self._chk(self.b.fn("add_instance")(self.h, object_id, _ptr(_f32(instance_to_world), C.c_float), _ptr(_f32(world_to_instance), C.c_float)))

    def add_light_infinite(self, L=(1, 1, 1), light_to_world=None, world_to_light=None):
        l2w = _f32(light_to_world if light_to_world is not None else IDENTITY)
        w2l = _f32(world_to_light if world_to_light is not None else IDENTITY)
        self._chk(self.b.fn("add_light_infinite")(self.h, _ptr(_f32(L), C.c_float), _ptr(l2w, C.c_float), _ptr(w2l, C.c_float)))

    def add_light_infinite_map(self, L, image, light_to_world=None, world_to_light=None):
        """InfiniteAreaLight with a radiance map: image (H, W, 3) float32 as an image reader returns it (top row first)."""
        img = np.ascontiguousarray(image, dtype=np.float32)
        l2w = _f32(light_to_world if light_to_world is not None else IDENTITY)
        w2l = _f32(world_to_light if world_to_light is not None else IDENTITY)
        self._chk(self.b.fn("add_light_infinite_map")(self.h, _ptr(_f32(L), C.c_float), img.shape[1], img.shape[0], _ptr(img, C.c_float), _ptr(l2w, C.c_float), _ptr(w2l, C.c_float)))

    def add_light_distant(self, L, w_light_world):
        self._chk(self.b.fn("add_light_distant")(self.h, _ptr(_f32(L), C.c_float), _ptr(_f32(w_light_world), C.c_float)))

    def add_light_point(self, I, p_world):
        self._chk(self.b.fn("add_light_point")(self.h, _ptr(_f32(I), C.c_float), _ptr(_f32(p_world), C.c_float)))

    def add_light_spot(self, I, light_to_world, world_to_light, cos_total_width, cos_falloff_start):
        self._chk(self.b.fn("add_light_spot")(self.h, _ptr(_f32(I), C.c_float), _ptr(_f32(light_to_world), C.c_float), _ptr(_f32(world_to_light), C.c_float),
                                              C.c_float(cos_total_width), C.c_float(cos_falloff_start)))

    def add_light_projection(self, I, light_to_world, world_to_light, fov, image=None):
        """ProjectionLight: image (H, W, 3) float32, top row first, or None (white inside the frustum)."""
        img = None if image is None else np.ascontiguousarray(image, dtype=np.float32)
        self._chk(self.b.fn("add_light_projection")(self.h, _ptr(_f32(I), C.c_float), _ptr(_f32(light_to_world), C.c_float), _ptr(_f32(world_to_light), C.c_float), C.c_float(fov),
                                                    0 if img is None else img.shape[1], 0 if img is None else img.shape[0], None if img is None else _ptr(img, C.c_float)))

    def add_light_goniometric(self, I, light_to_world, world_to_light, image=None):
        """GonioPhotometricLight: image (H, W, 3) float32 indexed by (phi / 2 pi, theta / pi), or None (a point light)."""
        img = None if image is None else np.ascontiguousarray(image, dtype=np.float32)
        self._chk(self.b.fn("add_light_goniometric")(self.h, _ptr(_f32(I), C.c_float), _ptr(_f32(light_to_world), C.c_float), _ptr(_f32(world_to_light), C.c_float),
                                                     0 if img is None else img.shape[1], 0 if img is None else img.shape[0], None if img is None else _ptr(img, C.c_float)))

    def add_light_diffuse_area(self, L, n_tris, two_sided=False) -> int:
        out = C.c_uint32(0)
        self._chk(self.b.fn("add_light_diffuse_area")(self.h, _ptr(_f32(L), C.c_float), 1 if two_sided else 0, n_tris, C.byref(out)))
        return out.value

    def set_camera_perspective(self, raster_to_camera, camera_to_world, lens_radius=0.0, focal_distance=1e6, shutter_open=0.0, shutter_close=1.0):
        self._chk(self.b.fn("set_camera_perspective")(self.h, _ptr(_f32(raster_to_camera), C.c_float), _ptr(_f32(camera_to_world), C.c_float),
                                                      C.c_float(lens_radius), C.c_float(focal_distance), C.c_float(shutter_open), C.c_float(shutter_close)))

    def set_camera_orthographic(self, raster_to_camera, camera_to_world, lens_radius=0.0, focal_distance=1e6, shutter_open=0.0, shutter_close=1.0):
        self._chk(self.b.fn("set_camera_orthographic")(self.h, _ptr(_f32(raster_to_camera), C.c_float), _ptr(_f32(camera_to_world), C.c_float),
                                                       C.c_float(lens_radius), C.c_float(focal_distance), C.c_float(shutter_open), C.c_float(shutter_close)))

    def set_camera_environment(self, camera_to_world, xres, yres, shutter_open=0.0, shutter_close=1.0):
        self._chk(self.b.fn("set_camera_environment")(self.h, _ptr(_f32(camera_to_world), C.c_float), int(xres), int(yres), C.c_float(shutter_open), C.c_float(shutter_close)))

    def set_film(self, xres, yres, cropped_bounds, radius, table, scale=1.0, max_sample_luminance=float("inf")):
        cb = np.ascontiguousarray(cropped_bounds, dtype=np.int32)
        self._chk(self.b.fn("set_film")(self.h, xres, yres, _ptr(cb, C.c_int), _ptr(_f32(radius), C.c_float), _ptr(_f32(table), C.c_float),
                                        C.c_float(scale), C.c_float(max_sample_luminance)))
        self.film_shape = (int(cb[3] - cb[1]), int(cb[2] - cb[0]))
        self.cropped_bounds = cb

    def set_sampler(self, kind, spp, sample_bounds, sample_at_pixel_center=False):
        sb = np.ascontiguousarray(sample_bounds, dtype=np.int32)
        self._chk(self.b.fn("set_sampler")(self.h, kind, spp, _ptr(sb, C.c_int), 1 if sample_at_pixel_center else 0))
        self.sample_bounds = sb

    def set_sobol_tables(self, m32, vdc, vdc_inv):
        """Generator matrices for the Sobol sampler (data tables the host owns; the library embeds none)."""
        m32 = np.ascontiguousarray(m32, dtype=np.uint32); vdc = np.ascontiguousarray(vdc, dtype=np.uint64); vdci = np.ascontiguousarray(vdc_inv, dtype=np.uint64)
        assert len(vdc) == len(vdci)
        self._chk(self.b.fn("set_sobol_tables")(self.h, _ptr(m32, C.c_uint32), len(m32), _ptr(vdc, C.c_uint64), _ptr(vdci, C.c_uint64), len(vdc)))

    def build_accel_device(self, split_method=1, max_prims_in_node=4):
        """The SAH (0) or HLBVH (1) tree constructed on the GPU: same tree as build_accel(split_method, ..)."""
        self._chk(self.b.fn("build_accel_device")(self.h, split_method, max_prims_in_node))

    def build_accel_device_shapes(self, split_method=0, max_prims_in_node=4):
        """build_accel_device, except that the SAH tree (0) of a scene with quadric shapes is built on the GPU as well."""
        self._chk(self.b.fn("build_accel_device_shapes")(self.h, split_method, max_prims_in_node))

    def build_accel(self, split_method=0, max_prims_in_node=4):
        self._chk(self.b.fn("build_accel")(self.h, split_method, max_prims_in_node))

    def build_accel_best(self, split_method=0, max_prims_in_node=4):
        """build_accel_device where it applies (SAH / HLBVH trees, scenes with object instances included; not EqualCounts), build_accel_device_shapes for the SAH tree of a scene with
        quadrics, which build_accel_device refuses, build_accel elsewhere: the same tree either way."""
        if split_method in (0, 1) and self.b.has("build_accel_device"):
            try:
                return self.build_accel_device(split_method, max_prims_in_node)
            except PbrtHipError as e:
                if e.code != ERR_UNSUPPORTED:
                    raise
            if split_method == 0 and self.b.has("build_accel_device_shapes"):
                try:
                    return self.build_accel_device_shapes(split_method, max_prims_in_node)
                except PbrtHipError as e:
                    if e.code != ERR_UNSUPPORTED:
                        raise
        self.build_accel(split_method, max_prims_in_node)

    def world_bound(self):
        out = np.zeros(6, np.float32)
        self._chk(self.b.fn("world_bound")(self.h, _ptr(out, C.c_float)))
        return out

    # ---- hot path ------------------------------------------------------------------------------------------------
    def intersect_batch(self, rays):
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        hits = np.zeros(len(rays), HIT_DTYPE)
        self._chk(self.b.fn("intersect_batch")(self.h, rays.ctypes.data, hits.ctypes.data, len(rays)))
        return hits

    def occluded_batch(self, rays):
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        out = np.zeros(len(rays), np.uint8)
        self._chk(self.b.fn("occluded_batch")(self.h, rays.ctypes.data, out.ctypes.data, len(rays)))
        return out

    def intersect_batch_device(self, d_rays_ptr, d_hits_ptr, n):
        ms = C.c_float(0)
        self._chk(self.b.fn("intersect_batch_device")(self.h, d_rays_ptr, d_hits_ptr, n, C.byref(ms)))
        return ms.value

    def occluded_batch_device(self, d_rays_ptr, d_out_ptr, n):
        ms = C.c_float(0)
        self._chk(self.b.fn("occluded_batch_device")(self.h, d_rays_ptr, d_out_ptr, n, C.byref(ms)))
        return ms.value

    # ---- textures (include/pbrt_hip.h "textures") ------------------------------------------------------------------------------
    WRAP = {"repeat": 0, "black": 1, "clamp": 2}

    def add_mipmap(self, image, as_float=False, scale=1.0, gamma=False, trilinear=False, wrap="repeat", max_anisotropy=8.0):
        """image: (H, W, 3) float32 as an image reader returns it (top row first).  Returns the mipmap id."""
        img = np.ascontiguousarray(image, dtype=np.float32)
        assert img.ndim == 3 and img.shape[2] == 3
        out = C.c_uint32(0)
        self._chk(self.b.fn("add_mipmap")(self.h, img.shape[1], img.shape[0], _ptr(img, C.c_float), 1 if as_float else 0, C.c_float(scale), 1 if gamma else 0,
                                          0 if trilinear else 1, self.WRAP[wrap], C.c_float(max_anisotropy), C.byref(out)))
        return out.value

    def add_texture_constant(self, value):
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(value, np.float32), (3,)), dtype=np.float32)
        out = C.c_uint32(0); self._chk(self.b.fn("add_texture_constant")(self.h, _ptr(v, C.c_float), C.byref(out))); return out.value

    def add_texture_scale(self, t1, t2):
        out = C.c_uint32(0); self._chk(self.b.fn("add_texture_scale")(self.h, t1, t2, C.byref(out))); return out.value

    def add_texture_mix(self, t1, t2, amount):
        out = C.c_uint32(0); self._chk(self.b.fn("add_texture_mix")(self.h, t1, t2, amount, C.byref(out))); return out.value

    def add_texture_imagemap(self, mipmap, su=1.0, sv=1.0, du=0.0, dv=0.0):
        out = C.c_uint32(0)
        self._chk(self.b.fn("add_texture_imagemap")(self.h, mipmap, C.c_float(su), C.c_float(sv), C.c_float(du), C.c_float(dv), C.byref(out))); return out.value

    def add_texture_checkerboard(self, t1, t2, su=1.0, sv=1.0, du=0.0, dv=0.0, aa="closedform"):
        out = C.c_uint32(0)
        self._chk(self.b.fn("add_texture_checkerboard")(self.h, t1, t2, C.c_float(su), C.c_float(sv), C.c_float(du), C.c_float(dv), 0 if aa == "none" else 1, C.byref(out)))
        return out.value

    def add_texture_uv(self, su=1.0, sv=1.0, du=0.0, dv=0.0):
        out = C.c_uint32(0); self._chk(self.b.fn("add_texture_uv")(self.h, C.c_float(su), C.c_float(sv), C.c_float(du), C.c_float(dv), C.byref(out))); return out.value

    def add_texture_bilerp(self, v00, v01, v10, v11, su=1.0, sv=1.0, du=0.0, dv=0.0):
        vs = [np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float32), (3,)), dtype=np.float32) for v in (v00, v01, v10, v11)]
        out = C.c_uint32(0)
        self._chk(self.b.fn("add_texture_bilerp")(self.h, *[_ptr(v, C.c_float) for v in vs], C.c_float(su), C.c_float(sv), C.c_float(du), C.c_float(dv), C.byref(out)))
        return out.value

    def add_texture_dots(self, inside, outside, su=1.0, sv=1.0, du=0.0, dv=0.0):
        out = C.c_uint32(0)
        self._chk(self.b.fn("add_texture_dots")(self.h, inside, outside, C.c_float(su), C.c_float(sv), C.c_float(du), C.c_float(dv), C.byref(out))); return out.value

    def add_texture_fbm(self, m=IDENTITY, omega=0.5, octaves=8, wrinkled=False):
        out = C.c_uint32(0)
        self._chk(self.b.fn("add_texture_wrinkled" if wrinkled else "add_texture_fbm")(self.h, _ptr(_f32(m), C.c_float), C.c_float(omega), octaves, C.byref(out))); return out.value

    def add_texture_windy(self, m=IDENTITY):
        out = C.c_uint32(0); self._chk(self.b.fn("add_texture_windy")(self.h, _ptr(_f32(m), C.c_float), C.byref(out))); return out.value

    def add_texture_marble(self, m=IDENTITY, omega=0.5, octaves=8, scale=1.0, variation=0.2):
        out = C.c_uint32(0)
        self._chk(self.b.fn("add_texture_marble")(self.h, _ptr(_f32(m), C.c_float), C.c_float(omega), octaves, C.c_float(scale), C.c_float(variation), C.byref(out))); return out.value

    def add_texture_checkerboard3d(self, t1, t2, m=IDENTITY):
        out = C.c_uint32(0); self._chk(self.b.fn("add_texture_checkerboard3d")(self.h, t1, t2, _ptr(_f32(m), C.c_float), C.byref(out))); return out.value

    def set_texture_mapping(self, texture, kind, params):
        """kind "spherical" | "cylindrical" (params = world_to_texture, 16 floats) | "planar" (params = v1, v2, udelta, vdelta: 8 floats)"""
        k = {"spherical": 1, "cylindrical": 2, "planar": 3}[kind]
        prm = np.ascontiguousarray(np.asarray(params, np.float32).reshape(-1), dtype=np.float32)
        assert len(prm) == (8 if k == 3 else 16)
        self._chk(self.b.fn("set_texture_mapping")(self.h, texture, k, _ptr(prm, C.c_float)))

    def add_material_matte_tex(self, kd_texture, sigma=0.0):
        out = C.c_uint32(0); self._chk(self.b.fn("add_material_matte_tex")(self.h, kd_texture, C.c_float(sigma), C.byref(out))); return out.value

    PARAM = {"Kd": 0, "Ks": 1, "Kr": 2, "Kt": 3, "opacity": 4, "amount": 5, "eta": 6, "k": 7, "reflect": 8, "transmit": 9}

    def set_material_texture(self, material, param, texture):
        """param: "Kd" | "Ks" | "Kr" | "Kt" | "opacity" (uber) | "amount" (mix) | "eta" | "k" (metal) | "reflect" | "transmit" (translucent) — that parameter of `material` becomes `texture`, evaluated per hit."""
        self._chk(self.b.fn("set_material_texture")(self.h, material, self.PARAM[param], texture))

    def set_last_mesh_alpha_textures(self, alpha=None, shadow_alpha=None):
        """Float textures for the `alpha` / `shadowalpha` masks of the mesh added last (None keeps the constant)."""
        none = 0xFFFFFFFF
        self._chk(self.b.fn("set_last_mesh_alpha_textures")(self.h, none if alpha is None else alpha, none if shadow_alpha is None else shadow_alpha))

    FPARAM = {"sigma": 0, "uroughness": 1, "vroughness": 2, "index": 3}

    def set_material_float_texture(self, material, fparam, texture):
        """fparam: "sigma" (matte) | "uroughness" | "vroughness" | "roughness" (= both) | "index" (glass, uber) — that scalar of `material` becomes the float texture, evaluated per hit."""
        for f in (("uroughness", "vroughness") if fparam == "roughness" else (fparam,)):
            self._chk(self.b.fn("set_material_float_texture")(self.h, material, self.FPARAM[f], texture))

    def set_material_bump(self, material, texture):
        """Material::bump with the float texture `texture` as displacement map."""
        self._chk(self.b.fn("set_material_bump")(self.h, material, texture))

    def texture_eval(self, texture, uv, derivs=None, p=None, dpdx=None, dpdy=None, nodiff=False):
        """Evaluates `texture` at uv (n,2) with (du/dx, dv/dx, du/dy, dv/dy) (n,4) and, for the 3D textures, the hit point p (n,3) with dp/dx, dp/dy;
        returns (n,3).  A probe for the parity tests.  nodiff=True: the product's evaluator for contexts without differentials
        (pbrt_hip_texture_eval_batch_nodiff), which ignores the derivatives."""
        uv = np.asarray(uv, np.float32).reshape(-1, 2)
        z3 = np.zeros((len(uv), 3), np.float32)
        d = np.zeros((len(uv), 4), np.float32) if derivs is None else np.asarray(derivs, np.float32).reshape(-1, 4)
        cols = [uv, d] + [z3 if a is None else np.asarray(a, np.float32).reshape(-1, 3) for a in (p, dpdx, dpdy)]
        inp = np.ascontiguousarray(np.concatenate(cols, axis=1), dtype=np.float32)
        out = np.zeros((len(uv), 3), np.float32)
        self._chk(self.b.fn("texture_eval_batch_nodiff" if nodiff else "texture_eval_batch")(self.h, texture, len(uv), _ptr(inp, C.c_float), _ptr(out, C.c_float)))
        return out

    def bsdf_probe_batch(self, material, op, wo, wi, u, flags, frame=None, path=0):
        """The BSDF of `material` on explicit inputs (pbrt_hip_bsdf_probe_batch), a probe for the parity tests: wo, wi (n,3), u (n,2), flags (n,), frame = (ns, ng, dpdu) or
        None for the canonical one.  Returns (n,8): op 0 -> f rgb, pdf; op 1 -> sample_f's f rgb, pdf, wi xyz, sampled type; op 2 -> num_components, lobe count, eta.
        path 1: the one-lobe matte BSDF."""
        wo = _f32(wo, (-1, 3)); wi = _f32(wi, (-1, 3)); u = _f32(u, (-1, 2))
        flags = np.ascontiguousarray(flags, dtype=np.uint32).reshape(-1)
        n = len(wo)
        assert len(wi) == n and len(u) == n and len(flags) == n
        fr = None if frame is None else _f32(frame, (9,))
        out = np.zeros((n, 8), np.float32)
        self._chk(self.b.fn("bsdf_probe_batch")(self.h, material, op, path, n, _ptr(wo, C.c_float), _ptr(wi, C.c_float), _ptr(u, C.c_float), _ptr(flags, C.c_uint32),
                                                _ptr(fr, C.c_float), _ptr(out, C.c_float)))
        return out

    def sampler_value_batch(self, xy, sample, dim, use_lds=False):
        """The configured sampler's value per (pixel, sample number, dimension) (pbrt_hip_sampler_value_batch), a probe for the parity tests.  use_lds: read the first 54
        Halton dimensions from the LDS copy of their tables, as the shade pass does."""
        xy = np.ascontiguousarray(xy, dtype=np.int32).reshape(-1, 2)
        sample = np.ascontiguousarray(sample, dtype=np.uint32).reshape(-1); dim = np.ascontiguousarray(dim, dtype=np.uint32).reshape(-1)
        n = len(xy)
        assert len(sample) == n and len(dim) == n
        out = np.zeros(n, np.float32)
        self._chk(self.b.fn("sampler_value_batch")(self.h, n, _ptr(xy, C.c_int), _ptr(sample, C.c_uint32), _ptr(dim, C.c_uint32), 1 if use_lds else 0, _ptr(out, C.c_float)))
        return out

    LIGHT_PROBE_STRIDE = 28

    def _light_probe(self, fn, head, ref, u, wi):
        """What the two light probes share: ref (n,10), u (n,2) or 0.5s, wi (n,3) or +z, and the zeroed (n,28) result, around the call fn(handle, *head, n, ref, u, wi, out)."""
        ref = _f32(ref, (-1, 10)); n = len(ref)
        u = _f32(u, (-1, 2)) if u is not None else np.full((n, 2), 0.5, np.float32)
        wi = _f32(wi, (-1, 3)) if wi is not None else np.tile(np.array([0, 0, 1], np.float32), (n, 1))
        assert len(u) == n and len(wi) == n
        out = np.zeros((n, self.LIGHT_PROBE_STRIDE), np.float32)
        self._chk(self.b.fn(fn)(self.h, *head, n, _ptr(ref, C.c_float), _ptr(u, C.c_float), _ptr(wi, C.c_float), _ptr(out, C.c_float)))
        return out

    def light_probe_batch(self, light, op, ref, u=None, wi=None, variant=0):
        """Light number `light` on explicit reference points (pbrt_hip_light_probe_batch), a probe for the parity tests: ref (n,10) = p, p_error, n, time; u (n,2); wi (n,3).
        Returns (n,28): op 0 -> sample_li's wi, pdf, radiance, valid, far point / error / normal, shadow ray origin / direction / t_max; op 1 -> pdf_li; op 2 -> le.
        variant 0 / 1: the code of scenes with / without textures; 2: the Whitted light loop's sample_li (spherical lights)."""
        return self._light_probe("light_probe_batch", (light, op, variant), ref, u, wi)

    def sphere_light_probe_batch(self, light, op, ref, u=None, wi=None):
        """A spherical, disk or cylinder area light as the path integrator's sphere-light shade pass calls it (pbrt_hip_sphere_light_probe_batch): op 0 -> sample_li, op 1 -> pdf_li.  Inputs and the
        (n,28) output are light_probe_batch's."""
        return self._light_probe("sphere_light_probe_batch", (light, op), ref, u, wi)

    def spatial_probe_begin(self):
        """Set the spatial light distribution's tables up as a light_strategy=2 render does (pbrt_hip_spatial_probe_begin) -> ((nx, ny, nz), pool capacity in voxels)."""
        nv = np.zeros(3, np.int32); cap = np.zeros(1, np.uint32)
        self._chk(self.b.fn("spatial_probe_begin")(self.h, _ptr(nv, C.c_int), _ptr(cap, C.c_uint32)))
        return (int(nv[0]), int(nv[1]), int(nv[2])), int(cap[0])

    def spatial_probe_batch(self, p, u, strategy=2):
        """The light pick at explicit points (pbrt_hip_spatial_probe_batch): p (n,3), u (n,).  strategy 2: claim pass, distribution pass and pick on the tables of
        spatial_probe_begin, which stay between calls; 0 / 1: the pick on the scene-wide uniform / power table.
        Returns (pi (n,3) int32 — zeros under 0 / 1 —, light (n,) uint32, pick_pdf (n,) float32, counters (4,) uint32 = claimed, computed, pool-exhausted flag, blocks)."""
        p = _f32(p, (-1, 3)); n = len(p)
        u = _f32(u, (-1,))
        assert len(u) == n
        pi = np.zeros((n, 3), np.int32); light = np.zeros(n, np.uint32); pdf = np.zeros(n, np.float32); ctr = np.zeros(4, np.uint32)
        self._chk(self.b.fn("spatial_probe_batch")(self.h, n, _ptr(p, C.c_float), _ptr(u, C.c_float), strategy, _ptr(pi, C.c_int32), _ptr(light, C.c_uint32), _ptr(pdf, C.c_float),
                                                   _ptr(ctr, C.c_uint32)))
        return pi, light, pdf, ctr

    def spatial_probe_voxel(self, pi, n_lights):
        """(func (n_lights,), cdf (n_lights + 1,), func_int) of a voxel a spatial_probe_batch computed (pbrt_hip_spatial_probe_voxel); n_lights: the scene's number of lights."""
        n = int(n_lights)
        pi = np.ascontiguousarray(pi, np.int32)
        func = np.zeros(n, np.float32); cdf = np.zeros(n + 1, np.float32); fi = np.zeros(1, np.float32)
        self._chk(self.b.fn("spatial_probe_voxel")(self.h, _ptr(pi, C.c_int), _ptr(func, C.c_float), _ptr(cdf, C.c_float), _ptr(fi, C.c_float)))
        return func, cdf, fi[0]

    SURFACE_PROBE_AUX, SURFACE_PROBE_STRIDE = 48, 40

    def surface_probe_batch(self, op, rays, hits, aux, variant=1, texture=0, camera_ray=False):
        """The hit-to-interaction code on explicit hits (pbrt_hip_surface_probe_batch), a probe for the parity tests: rays (n,) RAY_DTYPE in world space; hits (n,) HIT_DTYPE as
        intersect_batch wrote them, t and b0..b2 then set freely; aux (n,48) = p_film, lens, wi, hp, hp_error, hn and op 4's differentials.  op 0 the interaction, 1 the texture
        context and shading dn/du, dn/dv, 2 Material::bump with `texture`, 3 spawn_ray / spawn_ray_to_hit, 4 the specular ray differentials.  variant 0 make_surface_hit (by prim),
        1 make_surface_hit_any (leaf record, instances), 2 make_surface_hit_q (scenes with quadrics).  Returns (n,40) float32; include/pbrt_hip.h gives the slots."""
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE); hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE); n = len(rays)
        aux = _f32(aux, (-1, self.SURFACE_PROBE_AUX))
        assert len(hits) == n and len(aux) == n
        out = np.zeros((n, self.SURFACE_PROBE_STRIDE), np.float32)
        self._chk(self.b.fn("surface_probe_batch")(self.h, op, variant, texture, 1 if camera_ray else 0, n, rays.ctypes.data, hits.ctypes.data, _ptr(aux, C.c_float), _ptr(out, C.c_float)))
        return out

    def texture_probe_batch(self, texture, contexts, variant=0):
        """`texture` at explicit contexts (n,15) = u v du/dx dv/dx du/dy dv/dy p dp/dx dp/dy (pbrt_hip_texture_probe_batch), a probe for the parity tests.  variant 0 / 1: the
        general evaluator with / without differentials; 2 / 3: the evaluator of constant / image / scale / mix programs with / without; 4: the lean alpha test's (red channel in
        column 0).  Returns (n,3)."""
        ctx = _f32(contexts, (-1, 15)); n = len(ctx)
        out = np.zeros((n, 3), np.float32)
        self._chk(self.b.fn("texture_probe_batch")(self.h, texture, variant, n, _ptr(ctx, C.c_float), _ptr(out, C.c_float)))
        return out

    def bump_probe_batch(self, texture, inputs, variant=0):
        """Material::bump with `texture` as displacement on explicit inputs (n,33) = the 15 context floats, then n, ns, dpdu_s, dpdv_s, dndu, dndv (pbrt_hip_bump_probe_batch).
        Returns (n,6): the new shading normal and shading dp/du.  variant 0 .. 3 as in texture_probe_batch."""
        inp = _f32(inputs, (-1, 33)); n = len(inp)
        out = np.zeros((n, 6), np.float32)
        self._chk(self.b.fn("bump_probe_batch")(self.h, texture, variant, n, _ptr(inp, C.c_float), _ptr(out, C.c_float)))
        return out

    def traverse_probe(self, mode, rays_cl=None, rays_sh=None, order=None, n_heads=1, head_chunk=49152, blocks=1):
        """The traversal kernel on an explicit queue (pbrt_hip_traverse_probe).  mode 0: rays_cl, 1: rays_sh, 2: both in one launch.  Returns (hits, occluded).  An entry of
        `order` with bit 31 set marks that closest-hit ray as an escape query (mode 2, eligible scenes): its record says only whether it hit anything."""
        rays_cl = np.ascontiguousarray(rays_cl if rays_cl is not None else [], dtype=RAY_DTYPE)
        rays_sh = np.ascontiguousarray(rays_sh if rays_sh is not None else [], dtype=RAY_DTYPE)
        hits = np.zeros(len(rays_cl), HIT_DTYPE); occ = np.zeros(len(rays_sh), np.uint8)
        if order is not None:
            order = np.ascontiguousarray(order, dtype=np.uint32)
            assert len(order) == len(rays_cl) + len(rays_sh)
        ptr = lambda a: a.ctypes.data if a is not None and len(a) else None
        self._chk(self.b.fn("traverse_probe")(self.h, mode, ptr(rays_cl), len(rays_cl), ptr(rays_sh), len(rays_sh), order.ctypes.data if order is not None else None,
                                              n_heads, head_chunk, blocks, ptr(hits), ptr(occ)))
        return hits, occ

    def film_probe_layout(self, tile_size=16, tile_part=0, tile_parts=1):
        """What film_probe's arrays are laid out by (pbrt_hip_film_probe_layout): (pixels (n_px, 2) int32 of this part's pixel list, tile pixel bounds (n_tiles, 4) int32,
        (slot_w, slot_h) of a tile's slot in the tile buffer)."""
        out = (C.c_uint64 * 4)()
        self._chk(self.b.fn("film_probe_layout")(self.h, tile_size, tile_part, tile_parts, out, None, None))
        px = np.zeros((int(out[0]), 2), np.int32); pb = np.zeros((int(out[1]), 4), np.int32)
        self._chk(self.b.fn("film_probe_layout")(self.h, tile_size, tile_part, tile_parts, out, _ptr(px, C.c_int) if len(px) else None, _ptr(pb, C.c_int) if len(pb) else None))
        return px, pb, (int(out[2]), int(out[3]))

    def _film_probe_tile_floats(self, tile_size, tile_part, tile_parts):
        return self.tile_buffer_floats(tile_size, tile_part, tile_parts)

    def film_probe(self, L, p_film, tile_size=16, tile_part=0, tile_parts=1, d_tile_buffer_ptr=None, film=True, tiles=False):
        """The film pass and the merge on explicit camera samples (pbrt_hip_film_probe): L (spp, n_px, 3) and p_film (spp, n_px, 2) in the order of film_probe_layout's pixel
        list, a NaN p_film x meaning no sample.  Returns (xyz, weight, tile buffer): the film of this part's tiles alone (None, None with film=False or a caller's device
        buffer) and a host copy of the part's tile buffer (None without tiles=True)."""
        L = _f32(L); pf = _f32(p_film)
        assert L.ndim == 3 and pf.ndim == 3 and L.shape[:2] == pf.shape[:2] and L.shape[2] == 3 and pf.shape[2] == 2
        xyz = wt = buf = None
        if film and d_tile_buffer_ptr is None:
            h, w = self._film_hw()
            xyz = np.zeros((h, w, 3), np.float32); wt = np.zeros((h, w), np.float32)
        if tiles:
            buf = np.zeros(self._film_probe_tile_floats(tile_size, tile_part, tile_parts), np.float32)
        n = L.shape[1]
        self._chk(self.b.fn("film_probe")(self.h, tile_size, tile_part, tile_parts, n, _ptr(L, C.c_float) if L.size else None, _ptr(pf, C.c_float) if pf.size else None,
                                          d_tile_buffer_ptr, _ptr(xyz, C.c_float), _ptr(wt, C.c_float), _ptr(buf, C.c_float) if buf is not None and buf.size else None))
        return xyz, wt, buf

    def mipmap_pyramid(self, mipmap):
        """The pyramid the host built: list of (h, w, 3) float32 arrays, finest first (row 0 = t 0 = the image's bottom row)."""
        n = C.c_int(0); wh = (C.c_int * 64)()
        self._chk(self.b.fn("mipmap_levels")(self.h, mipmap, C.byref(n), wh))
        levels = []
        for i in range(n.value):
            a = np.zeros((wh[2 * i + 1], wh[2 * i], 3), np.float32)
            self._chk(self.b.fn("mipmap_level_texels")(self.h, mipmap, i, _ptr(a, C.c_float)))
            levels.append(a)
        return levels

    def set_traversal_counting(self, on):
        """Measurement aid (include/pbrt_hip.h): traversal launches also tally nodes / triangle tests / rays.  Never timed."""
        self._chk(self.b.fn("set_traversal_counting")(self.h, 1 if on else 0))

    def traversal_counts(self):
        """{closest: nodes_passed, tri_tests, rays, ref_node_visits; any_hit: the same} since the last call (resets the tallies)."""
        c = (C.c_uint64 * 8)()
        self._chk(self.b.fn("get_traversal_counts")(self.h, c))
        return {"closest": {"nodes_passed": int(c[0]), "tri_tests": int(c[1]), "rays": int(c[2]), "ref_node_visits": int(c[2]) + 2 * int(c[0])},
                "any_hit": {"nodes_passed": int(c[3]), "tri_tests": int(c[4]), "rays": int(c[5]), "ref_node_visits": int(c[6])},
                "culled_pops": int(c[7])}

    def devices(self):
        out = np.zeros(64, np.int32)
        n = self.b.fn("scene_devices")(self.h, _ptr(out, C.c_int), 64)
        return [int(v) for v in out[:n]]

    def selftest_rccl_gather(self, n_floats=1 << 20):
        wrong = C.c_uint64(0)
        self._chk(self.b.fn("selftest_rccl_gather")(self.h, n_floats, C.byref(wrong)))
        return int(wrong.value)

    def accel_stats(self):
        """Sizes of the built acceleration structure in the device layout (measurement aid)."""
        c = (C.c_uint64 * 8)()
        self._chk(self.b.fn("accel_stats")(self.h, c))
        return {"interior_nodes": int(c[0]), "leaf_records": int(c[1]), "node_bytes": int(c[2]), "leaf_record_bytes": int(c[3]), "leaves": int(c[4]),
                "depth": int(c[5]), "max_leaf_prims": int(c[6]), "build_seconds": int(c[7]) * 1e-6}

    def accel_copy(self):
        """(nodes (n, 16) uint32, leaf records (m, 12) uint32): the built structure in the device layout, copied from wherever it lives (test aid)."""
        st = self.accel_stats()
        nodes = np.zeros((max(st["interior_nodes"], 1), 16), np.uint32); recs = np.zeros((max(st["leaf_records"], 1), 12), np.uint32)
        self._chk(self.b.fn("accel_copy")(self.h, nodes.ctypes.data, st["interior_nodes"], recs.ctypes.data, st["leaf_records"]))
        return nodes[:st["interior_nodes"]], recs[:st["leaf_records"]]

    def _film_hw(self):
        if self.film_shape is None:
            raise PbrtHipError(ERR_STATE, "set_film must be called before rendering")
        return self.film_shape

    def render_path(self, max_depth=5, rr_threshold=1.0, light_strategy=2, pixel_bounds=None, tile_size=16, tile_part=0, tile_parts=1, out=None):
        """out = (xyz, weight) arrays to fill instead of fresh ones (see merge_tiles_device)."""
        h, w = self._film_hw()
        if out is not None:
            xyz, wt = out
            assert xyz.shape == (h, w, 3) and wt.shape == (h, w) and xyz.dtype == np.float32 and wt.dtype == np.float32 and xyz.flags.c_contiguous and wt.flags.c_contiguous
        else:
            xyz = np.zeros((h, w, 3), np.float32); wt = np.zeros((h, w), np.float32)
        pb = np.ascontiguousarray(pixel_bounds if pixel_bounds is not None else self.sample_bounds, dtype=np.int32)
        st = Stats()
        self._chk(self.b.fn("render_path")(self.h, max_depth, C.c_float(rr_threshold), light_strategy, _ptr(pb, C.c_int), tile_size, tile_part, tile_parts,
                                           _ptr(xyz, C.c_float), _ptr(wt, C.c_float), C.byref(st)))
        return xyz, wt, st

    def render_whitted(self, max_depth=5, pixel_bounds=None, tile_size=16, tile_part=0, tile_parts=1):
        """WhittedIntegrator (pbrt_hip_render_whitted): the same film, tiles and return value as render_path."""
        h, w = self._film_hw()
        xyz = np.zeros((h, w, 3), np.float32); wt = np.zeros((h, w), np.float32)
        pb = np.ascontiguousarray(pixel_bounds if pixel_bounds is not None else self.sample_bounds, dtype=np.int32)
        st = Stats()
        self._chk(self.b.fn("render_whitted")(self.h, max_depth, _ptr(pb, C.c_int), tile_size, tile_part, tile_parts, _ptr(xyz, C.c_float), _ptr(wt, C.c_float), C.byref(st)))
        return xyz, wt, st

    def render_whitted_devices(self, max_depth=5, pixel_bounds=None, tile_size=16, tile_part=0, tile_parts=1):
        """render_whitted on a handle over any number of devices (pbrt_hip_render_whitted_devices): the handle's tiles dealt round-robin to its devices, gathered on the first
        and merged in tile order.  On a one-device handle it is render_whitted."""
        h, w = self._film_hw()
        xyz = np.zeros((h, w, 3), np.float32); wt = np.zeros((h, w), np.float32)
        pb = np.ascontiguousarray(pixel_bounds if pixel_bounds is not None else self.sample_bounds, dtype=np.int32)
        st = Stats()
        self._chk(self.b.fn("render_whitted_devices")(self.h, max_depth, _ptr(pb, C.c_int), tile_size, tile_part, tile_parts, _ptr(xyz, C.c_float), _ptr(wt, C.c_float), C.byref(st)))
        return xyz, wt, st

    @staticmethod
    def _direct_strategy(strategy):
        """"all" / "one" (or the C ABI's 0 / 1) -> the C ABI's int; anything else goes through for the library to refuse."""
        return {"all": 0, "one": 1}.get(strategy, strategy)

    def render_direct(self, strategy="all", max_depth=5, pixel_bounds=None, tile_size=16, tile_part=0, tile_parts=1):
        """DirectLightingIntegrator (pbrt_hip_render_direct), strategy "all" or "one": the same film, tiles and return value as render_whitted."""
        h, w = self._film_hw()
        xyz = np.zeros((h, w, 3), np.float32); wt = np.zeros((h, w), np.float32)
        pb = np.ascontiguousarray(pixel_bounds if pixel_bounds is not None else self.sample_bounds, dtype=np.int32)
        st = Stats()
        self._chk(self.b.fn("render_direct")(self.h, self._direct_strategy(strategy), max_depth, _ptr(pb, C.c_int), tile_size, tile_part, tile_parts,
                                             _ptr(xyz, C.c_float), _ptr(wt, C.c_float), C.byref(st)))
        return xyz, wt, st

    def render_direct_devices(self, strategy="all", max_depth=5, pixel_bounds=None, tile_size=16, tile_part=0, tile_parts=1):
        """render_direct on a handle over any number of devices (pbrt_hip_render_direct_devices), as render_whitted_devices is for render_whitted."""
        h, w = self._film_hw()
        xyz = np.zeros((h, w, 3), np.float32); wt = np.zeros((h, w), np.float32)
        pb = np.ascontiguousarray(pixel_bounds if pixel_bounds is not None else self.sample_bounds, dtype=np.int32)
        st = Stats()
        self._chk(self.b.fn("render_direct_devices")(self.h, self._direct_strategy(strategy), max_depth, _ptr(pb, C.c_int), tile_size, tile_part, tile_parts,
                                                     _ptr(xyz, C.c_float), _ptr(wt, C.c_float), C.byref(st)))
        return xyz, wt, st

    def set_sample_record_budget(self, nbytes=0):
        """Bound on the bytes of sample records resident at once (pbrt_hip_set_sample_record_budget): the frame renders in bands of whole tiles, bit for bit the
        one-band film.  0 = automatic.  Holds until changed."""
        self._chk(self.b.fn("set_sample_record_budget")(self.h, int(nbytes)))

    def set_path_sphere_lights(self, on=True):
        """Let render_path / render_path_tiles_device sample spherical area lights (pbrt_hip_set_path_sphere_lights) instead of refusing such a scene.  Off by default;
        holds until changed."""
        self._chk(self.b.fn("set_path_sphere_lights")(self.h, 1 if on else 0))

    def render_footprint(self):
        """What the last render came to (pbrt_hip_get_render_footprint)."""
        c = (C.c_uint64 * 8)()
        self._chk(self.b.fn("get_render_footprint")(self.h, c))
        return {"bands": int(c[0]), "band_tiles": int(c[1]), "record_bytes": int(c[2]), "record_budget": int(c[3]), "chunk_paths": int(c[4]), "chunk_bytes": int(c[5])}

    def mis_escape(self):
        """Did the last render_path trace the BSDF-sampled MIS ray as an escape query (pbrt_hip_get_mis_escape)?"""
        v = C.c_int(0)
        self._chk(self.b.fn("get_mis_escape")(self.h, C.byref(v)))
        return bool(v.value)

    def film_to_rgb(self, xyz, weight):
        rgb = np.zeros_like(xyz)
        self._chk(self.b.fn("film_to_rgb")(self.h, _ptr(_f32(xyz), C.c_float), _ptr(_f32(weight), C.c_float), _ptr(rgb, C.c_float)))
        return rgb

    def generate_camera_rays(self, pixel_bounds, sample_index):
        pb = np.ascontiguousarray(pixel_bounds, dtype=np.int32)
        n = int((pb[2] - pb[0]) * (pb[3] - pb[1]))
        rays = np.zeros(n, RAY_DTYPE); pf = np.zeros((n, 2), np.float32)
        self._chk(self.b.fn("generate_camera_rays")(self.h, _ptr(pb, C.c_int), sample_index, rays.ctypes.data, _ptr(pf, C.c_float)))
        return rays, pf

    def tile_buffer_floats(self, tile_size, tile_part, tile_parts):
        out = C.c_uint64(0)
        self._chk(self.b.fn("tile_buffer_floats")(self.h, tile_size, tile_part, tile_parts, C.byref(out)))
        return out.value

    def render_path_tiles_device(self, d_tile_buffer_ptr, max_depth=5, rr_threshold=1.0, light_strategy=2, pixel_bounds=None, tile_size=16, tile_part=0, tile_parts=1):
        pb = np.ascontiguousarray(pixel_bounds if pixel_bounds is not None else self.sample_bounds, dtype=np.int32)
        st = Stats()
        self._chk(self.b.fn("render_path_tiles_device")(self.h, max_depth, C.c_float(rr_threshold), light_strategy, _ptr(pb, C.c_int), tile_size, tile_part, tile_parts,
                                                        d_tile_buffer_ptr, C.byref(st)))
        return st

    def render_whitted_tiles_device(self, d_tile_buffer_ptr, max_depth=5, pixel_bounds=None, tile_size=16, tile_part=0, tile_parts=1):
        """The Whitted integrator's rank form (pbrt_hip_render_whitted_tiles_device): this part's FilmTiles into a device buffer of tile_buffer_floats floats."""
        pb = np.ascontiguousarray(pixel_bounds if pixel_bounds is not None else self.sample_bounds, dtype=np.int32)
        st = Stats()
        self._chk(self.b.fn("render_whitted_tiles_device")(self.h, max_depth, _ptr(pb, C.c_int), tile_size, tile_part, tile_parts, d_tile_buffer_ptr, C.byref(st)))
        return st

    def render_direct_tiles_device(self, d_tile_buffer_ptr, strategy="all", max_depth=5, pixel_bounds=None, tile_size=16, tile_part=0, tile_parts=1):
        """The direct-lighting integrator's rank form (pbrt_hip_render_direct_tiles_device): this part's FilmTiles into a device buffer of tile_buffer_floats floats."""
        pb = np.ascontiguousarray(pixel_bounds if pixel_bounds is not None else self.sample_bounds, dtype=np.int32)
        st = Stats()
        self._chk(self.b.fn("render_direct_tiles_device")(self.h, self._direct_strategy(strategy), max_depth, _ptr(pb, C.c_int), tile_size, tile_part, tile_parts,
                                                          d_tile_buffer_ptr, C.byref(st)))
        return st

    def merge_tiles_device(self, d_ptrs, tile_size=16, out=None):
        """out = (xyz (h, w, 3) float32, weight (h, w) float32) to fill instead of fresh arrays — page-locked ones (e.g. torch.empty(.., pin_memory=True).numpy())
        make the read-back of a large film a DMA transfer instead of a staged copy into freshly faulted pages."""
        h, w = self._film_hw()
        if out is not None:
            xyz, wt = out
            assert xyz.shape == (h, w, 3) and wt.shape == (h, w) and xyz.dtype == np.float32 and wt.dtype == np.float32 and xyz.flags.c_contiguous and wt.flags.c_contiguous
        else:
            xyz = np.zeros((h, w, 3), np.float32); wt = np.zeros((h, w), np.float32)
        arr = (C.c_void_p * len(d_ptrs))(*d_ptrs)
        self._chk(self.b.fn("merge_tiles_device")(self.h, tile_size, len(d_ptrs), arr, _ptr(xyz, C.c_float), _ptr(wt, C.c_float)))
        return xyz, wt


def read_ply(path):
    """Vertices and triangles of a PLY file as shapes/src/plymesh.rs:21-249 reads them: `x y z` of element vertex (any other vertex property is skipped here), faces
    `vertex_indices` / `vertex_index` of 3 or 4 (a quad a b c d -> a b c, d a c); ascii and binary, either endianness.  Returns (P float32 (n, 3), idx uint32 (3 n_tris,))."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header") + len(b"end_header")
    end = data.index(b"\n", end) + 1
    header = data[:end].decode("ascii", "replace").split("\n")
    fmt = None; elements = []
    for line in header:
        t = line.split()
        if not t: continue
        if t[0] == "format": fmt = t[1]
        elif t[0] == "element": elements.append({"name": t[1], "n": int(t[2]), "props": []})
        elif t[0] == "property" and elements:
            if t[1] == "list": elements[-1]["props"].append(("list", t[2], t[3], t[4]))
            else: elements[-1]["props"].append(("scalar", t[1], t[2]))
    types = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4",
             "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}
    P = None; tris = []
    if fmt == "ascii":
        tok = data[end:].split(); pos = 0
        for e in elements:
            if e["name"] == "vertex":
                names = [p[2] for p in e["props"]]; w = len(names)
                a = np.array(tok[pos:pos + w * e["n"]], dtype=np.float64).reshape(e["n"], w); pos += w * e["n"]
                P = np.stack([a[:, names.index(c)] for c in "xyz"], axis=1).astype(np.float32)
            else:
                for _ in range(e["n"]):
                    for pr in e["props"]:
                        if pr[0] == "list":
                            k = int(tok[pos]); v = [int(x) for x in tok[pos + 1:pos + 1 + k]]; pos += 1 + k
                            if e["name"] == "face" and pr[3] in ("vertex_indices", "vertex_index"): tris.append(v)
                        else: pos += 1
    else:
        bo = "<" if fmt == "binary_little_endian" else ">"
        off = end
        for e in elements:
            if all(p[0] == "scalar" for p in e["props"]):
                dt = np.dtype([(p[2], bo + types[p[1]]) for p in e["props"]])
                a = np.frombuffer(data, dt, e["n"], off); off += dt.itemsize * e["n"]
                if e["name"] == "vertex": P = np.stack([a[c] for c in "xyz"], axis=1).astype(np.float32)
            else:
                if e["name"] == "face" and len(e["props"]) == 1:   # the common case: one list per face; try the fixed-size fast paths first
                    _, ct, it, nm = e["props"][0]; cdt = np.dtype(bo + types[ct]); idt = np.dtype(bo + types[it])
                    done = False
                    for k in (3, 4):
                        rec = np.dtype([("n", cdt), ("v", idt, (k,))])
                        if off + rec.itemsize * e["n"] <= len(data):
                            a = np.frombuffer(data, rec, e["n"], off)
                            if (a["n"] == k).all():
                                if nm in ("vertex_indices", "vertex_index"): tris = a["v"].astype(np.int64)
                                off += rec.itemsize * e["n"]; done = True; break
                    if done: continue
                for _ in range(e["n"]):
                    for pr in e["props"]:
                        if pr[0] == "list":
                            cdt = np.dtype(bo + types[pr[1]]); idt = np.dtype(bo + types[pr[2]])
                            k = int(np.frombuffer(data, cdt, 1, off)[0]); off += cdt.itemsize
                            v = np.frombuffer(data, idt, k, off).astype(np.int64).tolist(); off += idt.itemsize * k
                            if e["name"] == "face" and pr[3] in ("vertex_indices", "vertex_index"): tris.append(v)
                        else: off += np.dtype(types[pr[1]]).itemsize
    if P is None: raise ValueError(f"{path}: no vertex element")
    if isinstance(tris, np.ndarray):
        idx = tris.reshape(-1, 3) if tris.shape[1] == 3 else np.concatenate([tris[:, [0, 1, 2]], tris[:, [3, 0, 2]]], axis=1).reshape(-1, 3)
    else:
        out = []
        for v in tris:
            if len(v) == 3: out.append(v)
            elif len(v) == 4: out.append([v[0], v[1], v[2]]); out.append([v[3], v[0], v[2]])   # plymesh.rs:228-236
        idx = np.array(out, np.int64).reshape(-1, 3)
    return np.ascontiguousarray(P), np.ascontiguousarray(idx.reshape(-1), dtype=np.uint32)


@dataclass
class SceneSpec:
    """The synthetic measurement scene of BASELINE.md §3 / SURVEY §8d, as plain data, so that the same description can
    be captured into any Binding (product or, in tests, the oracle)."""
    n_tris: int = 1000
    seed: int = 1
    xres: int = 64
    yres: int = 64
    spp: int = 4
    max_depth: int = 5
    fov: float = 40.0
    kd: tuple = (0.5, 0.5, 0.5)
    sigma: float = 0.0
    env_L: tuple = (1.0, 1.0, 1.0)
    material: str = "matte"   # matte | plastic | glass | metal | uber: the material of every triangle (headline workload: matte)
    eye: tuple = (0.0, -4.0, 0.0)
    look: tuple = (0.0, 0.0, 0.0)
    up: tuple = (0.0, 0.0, 1.0)
    crop_window: tuple = (0.0, 1.0, 0.0, 1.0)   # Film "cropwindow" x0 x1 y0 y1 (fractions of the full resolution)


def capture_spec(spec: SceneSpec, scene: Scene, host: Host, geometry=None, instances: int = 0, device_build: bool = False):
    """LookAt 0 -4 0  0 0 0  0 0 1 / perspective fov 40 / box filter / halton / matte 0.5 / infinite L=1.
    instances = K > 0: the triangles form ONE object placed K times (ObjectInstance) on a jittered lattice inside the unit
    cube, each copy scaled by K^(-1/3) and rotated — K x n_tris instanced triangles behind a two-level BVH."""
    P, idx = geometry if geometry is not None else host.gen_random_tris(spec.n_tris, spec.seed)
    if spec.material == "matte":
        mat = scene.add_material_matte(spec.kd, spec.sigma)
    elif spec.material == "plastic":
        mat = scene.add_material_plastic(spec.kd, (0.25, 0.25, 0.25), 0.1, True)
    elif spec.material == "glass":
        mat = scene.add_material_glass((1, 1, 1), (1, 1, 1), 0.0, 0.0, 1.5, True)
    elif spec.material == "metal":
        mat = scene.add_material_metal((0.2, 0.92, 1.1), (3.9, 2.45, 2.14), 0.05, 0.05, True)
    elif spec.material == "uber":
        mat = scene.add_material_uber(spec.kd, (0.25, 0.25, 0.25), (0.1, 0.1, 0.1), (0.1, 0.1, 0.1), (0.9, 0.9, 0.9), 0.1, 0.1, 1.5, True)
    elif spec.material == "textured":  # MatteMaterial whose Kd is a 1024 x 1024 image map (EWA, repeat); triangles use the default uv (0,0) (1,0) (1,1)
        img = np.random.default_rng(spec.seed + 7).uniform(0.1, 0.9, (1024, 1024, 3)).astype(np.float32)
        mat = scene.add_material_matte_tex(scene.add_texture_imagemap(scene.add_mipmap(img)), spec.sigma)
    elif spec.material == "mixed":
        mat = None
    else:
        raise ValueError(spec.material)
    if spec.env_L is not None:
        scene.add_light_infinite(spec.env_L)
    if mat is None:  # five materials over five equal slices of the triangle list (spatially interleaved: the triangles are random)
        mats = [scene.add_material_matte(spec.kd, spec.sigma), scene.add_material_plastic(spec.kd, (0.25, 0.25, 0.25), 0.1, True),
                scene.add_material_glass((1, 1, 1), (1, 1, 1), 0.0, 0.0, 1.5, True), scene.add_material_metal((0.2, 0.92, 1.1), (3.9, 2.45, 2.14), 0.05, 0.05, True),
                scene.add_material_uber(spec.kd, (0.25, 0.25, 0.25), (0.1, 0.1, 0.1), (0.1, 0.1, 0.1), (0.9, 0.9, 0.9), 0.1, 0.1, 1.5, True)]
        nt = len(idx) // 3
        for k, m in enumerate(mats):
            t0, t1 = nt * k // 5, nt * (k + 1) // 5
            scene.add_mesh(P[3 * t0:3 * t1], idx[3 * t0:3 * t1] - 3 * t0, m)
    elif instances > 0:
        ob = scene.object_begin(); scene.add_mesh(P, idx, mat); scene.object_end()
        side = int(np.ceil(instances ** (1.0 / 3.0)))
        rng = np.random.default_rng(spec.seed + 1000)
        ident = (IDENTITY, IDENTITY)
        sc = 1.0 / side
        for k in range(instances):
            i, j, l = k % side, (k // side) % side, k // (side * side)
            c = (np.array([i, j, l], np.float64) + 0.5) / side * 2.0 - 1.0 + rng.uniform(-0.2, 0.2, 3) / side
            t = host.compose(host.compose(host.compose(ident, host.translate(c)), host.rotate(float(rng.uniform(0, 360)), rng.normal(size=3) + 1e-3)),
                             host.scale([sc, sc, sc]))
            scene.add_instance(ob, t[0], t[1])
    else:
        scene.add_mesh(P, idx, mat)
    w2c, c2w = host.look_at(spec.eye, spec.look, spec.up)
    r2c = host.perspective_raster_to_camera(spec.fov, spec.xres, spec.yres)
    scene.set_camera_perspective(r2c, c2w)
    cb, table, sb = host.film_box(spec.xres, spec.yres, crop_window=spec.crop_window)
    scene.set_film(spec.xres, spec.yres, cb, (0.5, 0.5), table)
    scene.set_sampler(0, spec.spp, sb)
    if device_build: scene.build_accel_device(0, 4)   # the same tree(s), made on the GPU and left there (csrc/bvh_sah_device.hip)
    else: scene.build_accel(0, 4)
    return P, idx
