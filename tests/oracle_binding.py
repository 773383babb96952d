"""Test-side loader for the CPU oracle (oracle/liboracle.so).  Only tests/, smoke() and bench.py's cpu_baseline leg
may import this."""
import ctypes as C
import os
import subprocess

import numpy as np

import pbrt_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
ORACLE_LIB = os.path.join(ORACLE_DIR, "liboracle.so")


class TraversalStats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("nodes_visited", C.c_uint64), ("tri_tests", C.c_uint64)]


_binding = None


def build_oracle():
    srcs = [os.path.join(ORACLE_DIR, f) for f in os.listdir(ORACLE_DIR) if f.endswith((".cpp", ".hpp"))]   # every source: a header left out would leave a stale library
    if not os.path.exists(ORACLE_LIB) or any(os.path.getmtime(s) > os.path.getmtime(ORACLE_LIB) for s in srcs):
        subprocess.check_call(["make", "-C", ORACLE_DIR, "-s"])


def oracle_binding():
    global _binding
    if _binding is None:
        build_oracle()
        b = pbrt_hip.Binding(ORACLE_LIB, "oracle_")
        L = b.lib
        vp = C.c_void_p
        L.oracle_intersect_batch_stats.argtypes = [vp, vp, vp, C.c_uint64, C.POINTER(TraversalStats), C.c_int]
        L.oracle_occluded_batch_stats.argtypes = [vp, vp, vp, C.c_uint64, C.POINTER(TraversalStats), C.c_int]
        L.oracle_render_path_ex.argtypes = [vp, C.c_int, C.c_float, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float),
                                            C.POINTER(C.c_float), C.POINTER(pbrt_hip.Stats), C.c_int, C.c_int, C.POINTER(C.c_uint64)]
        L.oracle_record_rays.argtypes = [vp, C.c_uint64]
        L.oracle_recorded_count.argtypes = [vp, C.c_int]
        L.oracle_recorded_count.restype = C.c_uint64
        L.oracle_recorded_rays.argtypes = [vp, C.c_int, vp]
        L.oracle_bvh_node_count.argtypes = [vp]
        L.oracle_bvh_node_count.restype = C.c_uint64
        L.oracle_bvh_nodes.argtypes = [vp, vp]
        L.oracle_bvh_ordered_prims.argtypes = [vp, vp]
        L.oracle_radical_inverse.restype = C.c_float
        L.oracle_radical_inverse.argtypes = [C.c_int, C.c_uint64]
        L.oracle_scrambled_radical_inverse.restype = C.c_float
        L.oracle_scrambled_radical_inverse.argtypes = [C.c_int, C.c_uint64]
        L.oracle_sampler_value.restype = C.c_float
        L.oracle_sampler_value.argtypes = [vp, C.c_int, C.c_int, C.c_uint32, C.c_uint32]
        L.oracle_prime.restype = C.c_uint32
        L.oracle_prime_sum.restype = C.c_uint32
        L.oracle_rng_u32.argtypes = [C.c_uint64, C.c_int, vp, C.c_int]
        L.oracle_halton_perm.argtypes = [C.c_int, vp]
        L.oracle_geom_op.argtypes = [C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.oracle_set_libm_mode.argtypes = [C.c_int]
        fp = C.POINTER(C.c_float)
        L.oracle_bsdf_probe.argtypes = [vp, C.c_uint32, C.c_int, fp, fp, fp, C.c_int, fp]
        L.oracle_spatial_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.oracle_spatial_voxel.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.oracle_spatial_lookup_batch.argtypes = [vp, C.c_uint64, fp, fp, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_uint32), fp, C.POINTER(C.c_int)]
        L.oracle_texture_probe_work.argtypes = [vp, C.c_uint32, C.c_uint64, fp, C.POINTER(C.c_uint64)]
        L.oracle_ray_stats_batch.argtypes = [vp, vp, C.c_uint64, C.c_int, vp]
        _binding = b
    return _binding


class OracleScene(pbrt_hip.Scene):
    """pbrt_hip.Scene driven against liboracle.so, plus the oracle-only extras.  The batch probes (bsdf_probe_batch, sampler_value_batch, light_probe_batch, texture_probe_batch,
    bump_probe_batch) are the inherited methods: oracle_bsdf_probe_batch / oracle_sampler_value_batch / oracle_light_probe_batch / oracle_texture_probe_batch /
    oracle_bump_probe_batch have the product's signatures."""

    def __init__(self):
        super().__init__(oracle_binding(), 0)

    def intersect_batch_stats(self, rays, threads=0):
        rays = np.ascontiguousarray(rays, dtype=pbrt_hip.RAY_DTYPE)
        hits = np.zeros(len(rays), pbrt_hip.HIT_DTYPE)
        st = TraversalStats()
        self._chk(self.b.lib.oracle_intersect_batch_stats(self.h, rays.ctypes.data, hits.ctypes.data, len(rays), C.byref(st), threads))
        return hits, st

    def occluded_batch_stats(self, rays, threads=0):
        rays = np.ascontiguousarray(rays, dtype=pbrt_hip.RAY_DTYPE)
        out = np.zeros(len(rays), np.uint8)
        st = TraversalStats()
        self._chk(self.b.lib.oracle_occluded_batch_stats(self.h, rays.ctypes.data, out.ctypes.data, len(rays), C.byref(st), threads))
        return out, st

    RAY_STATS_DTYPE = np.dtype([("dev_peak", "<u4"), ("dev_peak_scene", "<u4"), ("dev_peak_count", "<u4"), ("ref_peak", "<u4"), ("alpha_candidates", "<u4"), ("inst_entered", "<u4"),
                                ("leaf_seq", "<u4"), ("nodes_visited", "<u4"), ("tri_tests", "<u4"), ("found", "<u4")])
    # leaf_seq bits (oracle_scene.hpp, ORC_SEQ_*)
    SEQ_INST_THEN_PRIM, SEQ_PRIM_THEN_INST, SEQ_INST_LAST, SEQ_INST_NOT_LAST, SEQ_INST_SINGLE, SEQ_INST_ROOT_LEAF, SEQ_INST_TREE, SEQ_QUADRIC_WITH_INST = 1, 2, 4, 8, 16, 32, 64, 128
    SEQ_HIT_IN_INST_THEN_NEARER, SEQ_ALPHA_LAST, SEQ_ALPHA_NOT_LAST = 256, 512, 1024

    def ray_stats_batch(self, rays, any_hit=False):
        """Per ray, the counters of the oracle's walk (oracle_ray_stats_batch): the stack height the device would reach (dev_peak: scene-level and object-level entries together,
        dev_peak_scene: scene level alone, dev_peak_count: an any-hit ray under the counting rows), the reference's own to_visit peak, alpha-mask candidates, instances entered,
        the SEQ_* bits of the leaf-record sequences met, nodes visited, primitive tests, and whether it hit."""
        rays = np.ascontiguousarray(rays, dtype=pbrt_hip.RAY_DTYPE)
        out = np.zeros(len(rays), self.RAY_STATS_DTYPE)
        self._chk(self.b.lib.oracle_ray_stats_batch(self.h, rays.ctypes.data, len(rays), 1 if any_hit else 0, out.ctypes.data))
        return out

    def render_path_ex(self, max_depth=5, rr_threshold=1.0, light_strategy=2, pixel_bounds=None, tile_size=16, tile_part=0, tile_parts=1, threads=0,
                       count_traversal=False):
        h, w = self.film_shape
        xyz = np.zeros((h, w, 3), np.float32); wt = np.zeros((h, w), np.float32)
        pb = np.ascontiguousarray(pixel_bounds if pixel_bounds is not None else self.sample_bounds, dtype=np.int32)
        st = pbrt_hip.Stats(); nvnt = (C.c_uint64 * 4)()
        self._chk(self.b.lib.oracle_render_path_ex(self.h, max_depth, C.c_float(rr_threshold), light_strategy, pb.ctypes.data_as(C.POINTER(C.c_int)), tile_size,
                                                  tile_part, tile_parts, xyz.ctypes.data_as(C.POINTER(C.c_float)), wt.ctypes.data_as(C.POINTER(C.c_float)),
                                                  C.byref(st), threads, 1 if count_traversal else 0, nvnt))
        return xyz, wt, st, list(nvnt)

    def _film_probe_tile_floats(self, tile_size, tile_part, tile_parts):
        out = (C.c_uint64 * 4)()
        self._chk(self.b.fn("film_probe_layout")(self.h, tile_size, tile_part, tile_parts, out, None, None))
        return int(out[2])

    def film_probe_tiles(self, L, p_film, tile_size=16, tile_part=0, tile_parts=1):
        """oracle_film_probe: (xyz, weight, tiles) with tiles = this part's FilmTiles in increasing index, each (pixel bounds (4,), sums (h, w, 4): contribution rgb, weight sum).
        film_probe / film_probe_layout themselves are the inherited methods; the layout's third entry is (floats of all tiles packed, 0) here."""
        xyz, wt, buf = self.film_probe(L, p_film, tile_size, tile_part, tile_parts, tiles=True)
        _, pbs, _ = self.film_probe_layout(tile_size, tile_part, tile_parts)
        tiles, o = [], 0
        for pb in pbs:
            w, h = max(int(pb[2] - pb[0]), 0), max(int(pb[3] - pb[1]), 0)
            tiles.append((pb.copy(), buf[o:o + 4 * w * h].reshape(h, w, 4))); o += 4 * w * h
        assert o == len(buf)
        return xyz, wt, tiles

    def bsdf_probe(self, material, op, wo=(0, 0, 1), wi=(0, 0, 1), u=(0.5, 0.5), flags=31):
        """BSDF of `material` in the canonical frame: op 0 -> (f rgb, pdf), op 1 -> sample_f (f rgb, pdf, wi xyz, type), op 2 -> counts."""
        out = np.zeros(8, np.float32)
        f = lambda a: np.ascontiguousarray(a, dtype=np.float32).ctypes.data_as(C.POINTER(C.c_float))
        self._chk(self.b.lib.oracle_bsdf_probe(self.h, material, op, f(wo), f(wi), f(u), flags, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def texture_probe_work(self, texture, contexts):
        """per probe (n,2): the footprint texels MIPMap::ewa visits and the noise_3d calls of the evaluation with differentials (oracle_texture_probe_work)"""
        ctx = np.ascontiguousarray(contexts, dtype=np.float32).reshape(-1, 15)
        out = np.zeros((len(ctx), 2), np.uint64)
        self._chk(self.b.lib.oracle_texture_probe_work(self.h, texture, len(ctx), ctx.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def spatial_stats(self):
        """(voxel resolution xyz, distributions created) of the last spatial render."""
        out = (C.c_uint64 * 4)()
        self._chk(self.b.lib.oracle_spatial_stats(self.h, out))
        return tuple(out[:3]), int(out[3])

    def spatial_voxel(self, pi, n_lights):
        """compute_distribution for voxel pi: (func[n], cdf[n+1], func_int)."""
        func = np.zeros(n_lights, np.float32); cdf = np.zeros(n_lights + 1, np.float32); fi = C.c_float()
        pi = np.ascontiguousarray(pi, dtype=np.int32)
        self._chk(self.b.lib.oracle_spatial_voxel(self.h, pi.ctypes.data_as(C.POINTER(C.c_int)), func.ctypes.data_as(C.POINTER(C.c_float)),
                                                 cdf.ctypes.data_as(C.POINTER(C.c_float)), C.byref(fi)))
        return func, cdf, fi.value

    def spatial_lookup_batch(self, p, u, strategy=2):
        """uniform_sample_one_light's pick at explicit points (oracle_spatial_lookup_batch): p (n,3), u (n,).  strategy 2: lookup's voxel, compute_distribution (once per voxel
        within the call), sample_discrete(u); 0 / 1: sample_discrete on the uniform / power distribution.
        Returns (pi (n,3) int32 — zeros under 0 / 1 —, light (n,) uint32, pick_pdf (n,) float32, voxel resolution (3,) — zeros under 0 / 1)."""
        p = np.ascontiguousarray(p, np.float32).reshape(-1, 3); n = len(p)
        u = np.ascontiguousarray(u, np.float32).reshape(-1)
        assert len(u) == n
        pi = np.zeros((n, 3), np.int32); light = np.zeros(n, np.uint32); pdf = np.zeros(n, np.float32); nv = np.zeros(3, np.int32)
        fp = C.POINTER(C.c_float)
        self._chk(self.b.lib.oracle_spatial_lookup_batch(self.h, n, p.ctypes.data_as(fp), u.ctypes.data_as(fp), strategy, pi.ctypes.data_as(C.POINTER(C.c_int32)),
                                                        light.ctypes.data_as(C.POINTER(C.c_uint32)), pdf.ctypes.data_as(fp), nv.ctypes.data_as(C.POINTER(C.c_int))))
        return pi, light, pdf, (int(nv[0]), int(nv[1]), int(nv[2]))

    def record_rays(self, cap):
        self.b.lib.oracle_record_rays(self.h, cap)

    def recorded_rays(self, shadow=False):
        n = self.b.lib.oracle_recorded_count(self.h, 1 if shadow else 0)
        rays = np.zeros(n, pbrt_hip.RAY_DTYPE)
        if n:
            self.b.lib.oracle_recorded_rays(self.h, 1 if shadow else 0, rays.ctypes.data)
        return rays

    def bvh_nodes(self):
        n = self.b.lib.oracle_bvh_node_count(self.h)
        dt = np.dtype([("pmin", "<f4", 3), ("pmax", "<f4", 3), ("offset", "<u4"), ("n_primitives", "<u2"), ("axis", "u1"), ("pad", "u1")])
        nodes = np.zeros(n, dt)
        self.b.lib.oracle_bvh_nodes(self.h, nodes.ctypes.data)
        return nodes


def set_libm_mode(mode):
    oracle_binding().lib.oracle_set_libm_mode(mode)
