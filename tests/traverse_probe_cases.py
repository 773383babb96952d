"""Case sets for the traversal kernel's control logic (csrc/traverse.h) through Scene.traverse_probe, shared by the CPU test that states through the oracle's counters what every set
reaches (test_traverse_probe_cases_cpu.py) and the GPU test that compares every launch with the oracle bit for bit (test_traverse_probe_gpu.py).

A case = one tiny scene (`capture(scene)`, for either binding), a pool of rays laid out in 64-position batches of a stated composition, and the queue shapes of QUEUE_SHAPES: grid,
ray counts, modes, queue heads, head chunks and orders.  A queue shape takes the first n_cl rays of the pool as the closest-hit queue and the first n_sh as the any-hit queue, so one
oracle run per case (`prepared`) serves every launch.  The reference is exact: whatever the queue looks like, a ray's result is the oracle's intersect / intersect_p of that ray.

Ray categories of a pool, checked against the oracle's per-ray counters when the pool is built and again by the CPU test:
  early   the root box is missed (a ray pointing away, t_max = 0, a zero or NaN direction): the lane is done at the refill that loaded it
  walker  visits at least the case's `walk_min` nodes and meets no alpha-masked candidate
  mask    has at least one candidate hit that needs an alpha mask's verdict (the alpha wait phase)
Batch compositions (COMPOSITIONS): all early, one walker among 63 early, refill_min - 1 / refill_min / refill_min + 1 early among walkers for the row's refill_min, all walkers;
the alpha cases instead hold exactly 1, 11, 12, 13 and 64 mask rays per batch, the rest early (the wait ends because no node work is left) or walkers (the waiters stay parked).

The stack fixture (`chain_mesh`): n triangles A_i = (-s_i, -s_i), B_i = (4 s_i, -s_i), C_i = (-s_i, 2 s_i) at z = s_i / 8 with s_i in geometric progression.  Each contains the
boxes of all smaller ones, the centroids (2 s_i / 3, 0) lie in the same progression on x.  With max_prims_in_node = 1 the SAH build peels the largest triangle off at every level
as long as ratio^2 exceeds the triangle count: a chain of n - 1 interior nodes, first child the rest of the chain, second child the peeled leaf.  A ray from the apex region
(origin s_j (ax, ay, -1), direction (1/16, 1/32, 1): positive x, so the chain is the near child) that aims into region j hits both boxes at the n - 1 - j levels above it: the
device's stack reaches exactly that height before the first leaf is met.  Family 0 aims inside triangle j (found at the bottom of the walk, every popped entry is culled), family 1
beside its hypotenuse (inside box j, outside the triangle: the hit is the first popped entry's).  Everything is self-similar; the flat fixture's scales span 2^-31 .. 2^38, where neither the
fourth powers (the degenerate-triangle test's squared cross product) underflow nor the cubes (the error bound of t) overflow: every triangle can be hit.  The instanced fixture puts the same chain, scaled down, in the place of the scene-level chain's innermost triangle: scene-level and object-level entries share one stack.

Out of scope by design: the stack-overflow path (error_flag -> PBRT_HIP_ERR_DEVICE).  No builder produces a tree deep enough within float range to reach the flat cap of 64 or the
shared cap of 128, and the oracle's own stack ends at 64."""
import itertools

import numpy as np

import pbrt_hip
import scenes
import quadric_instance_scenes as QI
from oracle_binding import OracleScene
from quadric_alpha_scenes import libm1, mask_textures

BATCH = 64                     # PH_BATCH
N_BIG = 4 * BATCH * 9 + 1      # 2305: at blocks = 1 every wave refills many times
STRUCTURED = 34                # batches of stated composition; scenes.axis_rays() and walkers fill the pool up to N_BIG
MISS = 0xFFFFFFFF
RESIDENT_LANES = 256 * 6 * 256

# the rows of TravShapes (traverse.h) a case can name: (refill_min, lds_depth); the counting row of every scene is ShapeCount: (12, 12)
ROWS = {"ShapeFlat": (32, 12), "ShapeInst": (12, 11), "ShapeFlatAlphaLean": (12, 12), "ShapeInstAlphaLean": (12, 11), "ShapeAlphaGeneral<false>": (12, 12),
        "ShapeQuadric": (32, 12), "ShapeInstQuadric": (12, 11)}
COUNT_ROW = (12, 12)
ALPHA_MIN = 12


class QueueShape:
    def __init__(self, mode, n_cl, n_sh, order=None, n_heads=1, head_chunk=49152, blocks=1):
        self.mode, self.n_cl, self.n_sh, self.order, self.n_heads, self.head_chunk, self.blocks = mode, n_cl, n_sh, order, n_heads, head_chunk, blocks

    def order_array(self):
        n = self.n_cl + self.n_sh
        if self.order is None: return None
        if self.order == "identity": return np.arange(n, dtype=np.uint32)
        if self.order == "reversed": return np.arange(n, dtype=np.uint32)[::-1].copy()
        if self.order == "random": return np.random.default_rng(1234 + n).permutation(n).astype(np.uint32)
        assert self.order == "interleave"   # the two queues' positions in turn, the longer one's rest behind
        a, b = np.arange(self.n_cl, dtype=np.uint32), np.arange(self.n_cl, n, dtype=np.uint32)
        k = min(len(a), len(b))
        return np.concatenate([np.stack([a[:k], b[:k]], 1).reshape(-1), a[k:], b[k:]]).astype(np.uint32)

    def __repr__(self):
        return f"mode{self.mode}-cl{self.n_cl}-sh{self.n_sh}-{self.order or 'noorder'}-h{self.n_heads}x{self.head_chunk}-b{self.blocks}"


def _queue_shapes():
    Q, S = QueueShape, []
    for blocks in (1, 2, 3, 8 + 1):
        for n in (0, 1, 63, 64, 65, N_BIG):
            S.append(Q(0, n, 0, blocks=blocks))
    for n, blocks in ((0, 1), (1, 1), (65, 2), (N_BIG, 1), (N_BIG, 3)):
        S.append(Q(1, 0, n, blocks=blocks))
    # mixed: an empty closest-hit queue, an empty any-hit queue, both empty, both odd
    for blocks in (1, 3):
        S += [Q(2, 0, 65, blocks=blocks), Q(2, 65, 0, blocks=blocks), Q(2, 0, 0, blocks=blocks), Q(2, 1025, 1023, blocks=blocks), Q(2, 63, N_BIG, blocks=blocks)]
    # queue heads: heads dry from the start, an exact multiple of a round of chunks, one ray into a new chunk, more than one chunk per head with a last chunk that is not full
    for h, c in itertools.product((2, 8), (64, 128)):
        for n in sorted({c - 27, h * c - 37, h * c, h * c + 1, min(2 * h * c, N_BIG - 1), min(2 * h * c + 1, N_BIG), N_BIG}):
            S.append(Q(0, n, 0, n_heads=h, head_chunk=c, blocks=2 if n < 1000 else 3))
        S.append(Q(2, h * c // 2 + 1, h * c // 2, n_heads=h, head_chunk=c, blocks=8 + 1))
        S.append(Q(1, 0, h * c + 1, n_heads=h, head_chunk=c, blocks=1))
    for h in (2, 8):
        S += [Q(0, N_BIG, 0, n_heads=h, head_chunk=49152, blocks=8 + 1), Q(2, 100, 99, n_heads=h, head_chunk=49152, blocks=1)]
    S.append(Q(0, N_BIG, 0, n_heads=1, head_chunk=64, blocks=2))
    # orders
    for order in ("identity", "reversed", "random"):
        S += [Q(0, N_BIG, 0, order=order, blocks=1), Q(1, 0, 1025, order=order, blocks=2), Q(0, 1025, 0, order=order, n_heads=8, head_chunk=64, blocks=3)]
    for order in ("reversed", "random", "interleave"):
        S += [Q(2, 1025, 1023, order=order, blocks=1), Q(2, 1025, 1023, order=order, n_heads=8, head_chunk=128, blocks=3), Q(2, 65, 7, order=order, blocks=1)]
    return S


QUEUE_SHAPES = _queue_shapes()
# the full grid with one head and no order: must equal intersect_batch / occluded_batch, which run the same launch with the grid shrunk to the ray count
FULL_GRID_SHAPES = [(0, N_BIG), (1, N_BIG), (0, 65)]


# ---- rays -------------------------------------------------------------------------------------------------------------------------------------------------------------
def rays_from(o, d, t_max=np.inf):
    o = np.asarray(o, np.float32).reshape(-1, 3); d = np.asarray(d, np.float32).reshape(-1, 3)
    n = max(len(o), len(d))
    r = np.zeros(n, pbrt_hip.RAY_DTYPE)
    r["o"] = o; r["d"] = d; r["t_max"] = t_max
    return r


def early_candidates(bound):
    """rays that miss the root box `bound` (lo xyz, hi xyz), for every reason a lane can be done at its refill"""
    lo, hi = np.asarray(bound[:3], np.float64), np.asarray(bound[3:], np.float64)
    ext = np.maximum(hi - lo, 1e-3)
    g = np.random.default_rng(5)
    out = []
    for k in range(12):
        o = hi + ext * (0.25 + 0.5 * k) * g.uniform(0.5, 1.0, 3)
        out.append(rays_from(o, g.uniform(0.1, 1.0, 3)))                        # beyond the far corner, pointing away
        out.append(rays_from(o, (lo + hi) / 2 - o, t_max=0.0))                  # aimed at the box, t_max = 0
    o = hi + ext
    out += [rays_from(o, (0.0, 0.0, 0.0)), rays_from(o, (-0.0, 0.0, -0.0)), rays_from(o, (np.nan, np.nan, np.nan)), rays_from(o, (np.nan, 1.0, 0.0)),
            rays_from(lo - ext, (-1.0, -0.0, 0.0)), rays_from(lo - ext, (0.0, -1.0, 0.0)), rays_from(o, (lo + hi) / 2 - o, t_max=-1.0)]
    return np.concatenate(out)


COMPOSITIONS = ("all early", "one walker", "refill_min - 1 early", "refill_min early", "refill_min + 1 early", "all walkers")
ALPHA_COUNTS = (1, 11, 12, 13, 64)


def batch_plan(case):
    """per structured batch {category: count}"""
    plan = []
    for b in range(STRUCTURED):
        if case.alpha:
            k = ALPHA_COUNTS[b % 5]
            plan.append({"mask": k, ("early" if (b // 5) % 2 == 0 else "walker"): BATCH - k})
        else:
            rm = ROWS[case.row][0] if (b // 6) % 2 == 0 else COUNT_ROW[0]   # the timed row's threshold and the counting row's in turn
            e = {0: BATCH, 1: BATCH - 1, 2: rm - 1, 3: rm, 4: rm + 1, 5: 0}[b % 6]
            plan.append({"early": e, "walker": BATCH - e})
    return plan


def classify(case, st):
    """the category of every ray from the oracle's counters (ray_stats_batch), "" where it has none"""
    cat = np.full(len(st), "", dtype="U8")
    cat[(st["nodes_visited"] >= case.walk_min) & (st["alpha_candidates"] == 0)] = "walker"
    cat[st["alpha_candidates"] > 0] = "mask"
    cat[(st["nodes_visited"] <= 1) & (st["found"] == 0)] = "early"
    return cat


# ---- the stack fixture ------------------------------------------------------------------------------------------------------------------------------------------------
CHAIN_DIR = (1.0 / 16, 1.0 / 32, 1.0)
CHAIN_AIMS = ((-0.5, -0.5), (3.5, 1.5))   # family 0: inside triangle j; family 1: inside its box, beyond the hypotenuse


def chain_scales(n, ratio, top_exp):
    return np.float64(2.0) ** top_exp / np.float64(ratio) ** np.arange(n - 1, -1, -1)


def chain_mesh(s):
    s = np.asarray(s, np.float64)
    P = np.zeros((len(s), 3, 3)); z = s / 8
    P[:, 0] = np.stack([-s, -s, z], 1); P[:, 1] = np.stack([4 * s, -s, z], 1); P[:, 2] = np.stack([-s, 2 * s, z], 1)
    return P.reshape(-1, 3).astype(np.float32), np.arange(3 * len(s), dtype=np.uint32)


def chain_rays(s, family):
    s = np.asarray(s, np.float64)
    ax, ay = CHAIN_AIMS[family]
    return rays_from(np.stack([ax * s, ay * s, -s], 1), CHAIN_DIR)


FLAT_CHAIN = dict(n=29, ratio=5.5, top_exp=38)
# instanced: 34 + 34 levels at ratio 5.85 (5.85^2 > 34).  The scene-level chain spans 2^60 .. 2^-24, the object — the same construction with its top at 2^38 in object space,
# scaled by 2^-63 into the place of the scene-level chain's innermost triangle — 2^-25 .. 2^-109 in world space: a ray's origin stays a normal float.  To get both trees into the
# float range the scene-level chain goes above 2^42: there the triangle test's error bound (a product of three coordinates) overflows to infinity and rejects the candidate, on
# either side alike; below 2^-32 the degenerate-triangle test's squared cross product underflows to zero and rejects it.  Those triangles are boxes to walk past and never a
# hit.  The stack heights, which is what this fixture is for, are not affected.
INST_CHAIN = dict(n=34, ratio=5.85, top_exp=60, object_top_exp=38, object_shift=-25)


def inst_chain_parts():
    c = INST_CHAIN
    s_scene = chain_scales(c["n"], c["ratio"], c["top_exp"])
    s_obj = chain_scales(c["n"], c["ratio"], c["object_top_exp"])
    sigma = np.float64(2.0) ** (c["object_shift"] - c["object_top_exp"])  # the object's largest triangle comes to scale 2^object_shift, below s_scene[1]
    return s_scene, s_obj, sigma


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------------------------------
class Case:
    """name, the TravShapes row its scene runs (timed), capture(scene), walker / mask candidates (filtered by the oracle), walk_min, what it claims to reach"""

    def __init__(self, name, row, capture, walkers, masks=None, walk_min=5, claims=None):
        self.name, self.row, self.capture, self.walkers, self.masks, self.walk_min = name, row, capture, walkers, masks, walk_min
        self.alpha = masks is not None
        self.claims = claims or {}


def _mat(s):
    return s.add_material_matte((0.5, 0.5, 0.5))


def case_flat(host):
    P, idx = host.gen_random_tris(2000, 11)

    def capture(s):
        s.add_mesh(P, idx, _mat(s)); s.build_accel(0, 4)
    return Case("flat", "ShapeFlat", capture, lambda: scenes.random_rays(1500, 21), walk_min=20)


def case_chain_flat(host):
    s_ = chain_scales(**FLAT_CHAIN)
    P, idx = chain_mesh(s_)

    def capture(s):
        s.add_mesh(P, idx, _mat(s)); s.build_accel(0, 1)
    walkers = lambda: np.concatenate([chain_rays(s_, 0), chain_rays(s_, 1)])
    return Case("chain_flat", "ShapeFlat", capture, walkers, walk_min=1, claims={"chain": FLAT_CHAIN["n"], "peaks": list(range(9, 15)) + [24, FLAT_CHAIN["n"] - 1]})


def case_chain_inst(host):
    s_scene, s_obj, sigma = inst_chain_parts()
    Ps, idxs = chain_mesh(s_scene[1:])     # the innermost place is the instance's
    Po, idxo = chain_mesh(s_obj)
    i2w = np.diag([sigma, sigma, sigma, 1.0]).astype(np.float32).reshape(16)
    w2i = np.diag([1 / sigma, 1 / sigma, 1 / sigma, 1.0]).astype(np.float32).reshape(16)

    def capture(s):
        m = _mat(s)
        ob = s.object_begin(); s.add_mesh(Po, idxo, m); s.object_end()
        s.add_instance(ob, i2w, w2i)
        s.add_mesh(Ps, idxs, m)
        s.build_accel(0, 1)
    walkers = lambda: np.concatenate([chain_rays(s_scene[1:], 0), chain_rays(s_scene[1:], 1), chain_rays(s_obj * sigma, 0), chain_rays(s_obj * sigma, 1)])
    n = INST_CHAIN["n"]
    return Case("chain_inst", "ShapeInst", capture, walkers, walk_min=1,
                claims={"chain": n, "peaks": list(range(9, 15)) + [22, 63, 64, 65, 2 * n - 2], "scene_peak": n - 1})


MASK_QUAD = 1.0   # the masked quad spans [-1, 1]^2 at z = 0, uv = (xy + 1) / 2


def _masked_quad(s, m, mask, z=0.0):
    P = np.array([[-1, -1, z], [1, -1, z], [1, 1, z], [-1, 1, z]], np.float32) * np.float32([MASK_QUAD, MASK_QUAD, 1])
    s.add_mesh(P, [0, 1, 2, 0, 2, 3], m, UV=((P[:, :2] + MASK_QUAD) / (2 * MASK_QUAD)).astype(np.float32))
    s.set_last_mesh_alpha_textures(*mask_textures(s, mask, shadow=True))


def _quad_rays(n, seed, shift=(0.0, 0.0, 0.0)):
    """rays straight and obliquely through the masked quad, spread over its texels"""
    g = np.random.default_rng(seed)
    tgt = np.concatenate([g.uniform(-0.98, 0.98, (n, 2)) * MASK_QUAD, np.zeros((n, 1))], 1) + np.asarray(shift)
    d = np.concatenate([g.uniform(-0.3, 0.3, (n, 2)), -np.ones((n, 1))], 1)
    return rays_from(tgt - d * 2.0, d)


def case_alpha(host, mask):
    Pw, iw = host.gen_random_tris(1500, 13)
    Pw = Pw + np.float32([6.0, 0.0, 0.0])   # the deep walker mesh, beside the quad

    def capture(s):
        m = _mat(s)
        s.add_mesh(Pw, iw, m)
        _masked_quad(s, m, mask)
        s.add_mesh(np.array([[-1, -1, -1.5], [1, -1, -1.5], [0, 1, -1.5]], np.float32), [0, 1, 2], m)   # an opaque triangle behind the quad: what a ray through a hole finds
        s.build_accel(0, 4)

    def walkers():
        r = scenes.random_rays(1500, 23)
        r["o"] += np.float32([6.0, 0.0, 0.0])
        return r
    row = "ShapeFlatAlphaLean" if mask == "imagemap" else "ShapeAlphaGeneral<false>"
    return Case("alpha_" + mask, row, capture, walkers, masks=lambda: _quad_rays(900, 31), walk_min=20, claims={"alpha_last": True, "alpha_not_last": True})


def _proj():
    m = np.eye(4, dtype=np.float64); m[:3, 3] = [1.5, -4.0, 0.25]; m[0, 0] = 1.25; m[3] = [0.03, -0.02, 0.01, 1.2]
    return m.astype(np.float32).reshape(16), np.linalg.inv(m).astype(np.float32).reshape(16)


def _xl(host, t, rot=None):
    a = host.compose(QI.I4, host.translate(t))
    return host.compose(a, host.rotate(*rot)) if rot else a


INST_SPOTS = {"one": (-4.0, 0.0, 0.0), "leaf": (-4.0, 4.0, 0.0), "tree": (0.0, 0.0, 0.0), "tree2": (4.0, 0.5, 0.0), "pairA": (0.0, 4.0, 0.0), "pairB": (4.0, 4.0, 0.0), "masked": (-4.0, -4.0, 0.0)}


def case_instances(host, max_prims, masked=False):
    """a single-primitive object, an object whose aggregate is one leaf, a multi-level object (twice, once under a rotation), a projective instance, and two places where an
    instance and a scene-level triangle lie on top of each other so that one leaf holds both (directive order instance, triangle and triangle, instance); masked: plus an object
    that holds an alpha-masked quad (ShapeInstAlphaLean)"""
    P, idx = host.gen_random_tris(300, 5)
    tri = lambda at, k=1.0: (np.array([[-1.0, -0.9, 0.05], [1.1, -0.8, -0.05], [0.0, 1.2, 0.0]], np.float32) * np.float32(k) + np.float32(at))
    # three triangles almost on top of each other: no SAH split beats the leaf, so the object's aggregate is its root leaf — and, at scene level, an instance and two such
    # triangles share one leaf
    small = np.concatenate([tri((0.0, 0.0, 0.03 * k), 1.0 - 0.02 * k) for k in range(3)])
    proj = _proj()

    def capture(s):
        m = _mat(s)
        tree = s.object_begin(); s.add_mesh(P, idx, m); s.object_end()
        one = s.object_begin(); s.add_mesh(tri((0.0, 0.0, 0.0), 0.97), [0, 1, 2], m); s.object_end()
        leaf = s.object_begin(); s.add_mesh(small, np.arange(9, dtype=np.uint32), m); s.object_end()
        if masked:
            mo = s.object_begin(); _masked_quad(s, m, "imagemap"); s.add_mesh(P[:60], idx[:60], m); s.object_end()
        S = INST_SPOTS
        s.add_instance(one, *_xl(host, S["one"]))
        s.add_instance(leaf, *_xl(host, S["leaf"]))
        s.add_instance(tree, *_xl(host, S["tree"]))
        s.add_mesh(tri(S["tree"], 0.4) + np.float32([0, 0, 1.3]), [0, 1, 2], m)            # nearer than anything inside `tree` for a ray from +z
        s.add_instance(tree, *_xl(host, S["tree2"], (40, [0.2, 1, 0.3])))
        up, dn = np.float32([0, 0, 0.04]), np.float32([0, 0, -0.04])
        s.add_instance(one, *_xl(host, S["pairA"])); s.add_mesh(tri(S["pairA"]) + up, [0, 1, 2], m); s.add_mesh(tri(S["pairA"], 0.98) + dn, [0, 1, 2], m)    # instance, then triangles
        s.add_mesh(tri(S["pairB"]) + up, [0, 1, 2], m); s.add_mesh(tri(S["pairB"], 0.98) + dn, [0, 1, 2], m); s.add_instance(leaf, *_xl(host, S["pairB"]))   # triangles, then instance
        s.add_instance(tree, *proj)
        if masked:
            s.add_instance(mo, *_xl(host, S["masked"]))
        s.build_accel(0, max_prims)

    def aimed(n, seed, spots):
        g = np.random.default_rng(seed)
        out = []
        for k, at in enumerate(spots):
            tgt = np.asarray(at) + g.uniform(-0.8, 0.8, (n, 3)) * [1, 1, 0.3]
            d = g.normal(size=(n, 3)); d[:, 2] = -np.abs(d[:, 2]) - 0.5
            if k % 2: d = -d                                    # every other spot from below
            r = rays_from(tgt - d * g.uniform(1.5, 3.0, (n, 1)), d)
            r["t_max"][::5] = np.float32(1.0)                   # a fifth end at their target (inside the object's cloud)
            out.append(r)
        return np.concatenate(out)
    walkers = lambda: np.concatenate([aimed(150, 41, [v for k, v in INST_SPOTS.items() if k != "masked"] + [(1.5 / 1.2, -4.0 / 1.2, 0.25 / 1.2)]), scenes.random_rays(400, 43, bound=5.0)])
    masks = (lambda: _quad_rays(900, 47, INST_SPOTS["masked"])) if masked else None
    row = "ShapeInstAlphaLean" if masked else "ShapeInst"
    seq = ["SEQ_INST_SINGLE", "SEQ_INST_ROOT_LEAF", "SEQ_INST_TREE", "SEQ_INST_THEN_PRIM", "SEQ_PRIM_THEN_INST", "SEQ_INST_LAST", "SEQ_INST_NOT_LAST", "SEQ_HIT_IN_INST_THEN_NEARER"]
    return Case(f"instances_mp{max_prims}" + ("_masked" if masked else ""), row, capture, walkers, masks=masks, walk_min=5, claims={"seq": seq, "occluded_in_inst": True})


def case_inst_quadric(host, instance_first):
    """quadric_instance_scenes.one_leaf: a triangle, two quadrics and two instances in ONE scene-level leaf, in either directive order (ShapeInstQuadric)"""
    def capture(s):
        QI.one_leaf(s, host, instance_first=instance_first)
    return Case("inst_quadric_" + ("inst_first" if instance_first else "tri_first"), "ShapeInstQuadric", capture, lambda: QI.one_leaf_rays(n=1500), walk_min=3,
                claims={"seq": ["SEQ_QUADRIC_WITH_INST", "SEQ_INST_TREE", "SEQ_INST_THEN_PRIM", "SEQ_PRIM_THEN_INST", "SEQ_INST_NOT_LAST" if instance_first else "SEQ_INST_LAST"]})


def case_quadric(host):
    P, idx = host.gen_random_tris(800, 17)

    def capture(s):
        m = _mat(s)
        s.add_mesh(P, idx, m)
        s.add_sphere(*QI.cf_ctm(host, host.translate((0.2, 0.1, 0.0))), 0.5, None, None, 300.0, m, False)
        s.add_quadric("cylinder", *QI.cf_ctm(host, host.translate((-0.5, 0.3, 0.2)), host.rotate(60.0, (1, 1, 0))), 0.3, -0.6, 0.6, 270.0, m, False)
        s.add_quadric("disk", *QI.cf_ctm(host, host.translate((0.4, -0.5, -0.3))), 0.6, 0.0, 0.1, 360.0, m, False)
        s.build_accel(0, 4)
    return Case("quadric", "ShapeQuadric", capture, lambda: scenes.random_rays(1500, 53), walk_min=15)


CASES = {
    "flat": case_flat,
    "chain_flat": case_chain_flat,
    "chain_inst": case_chain_inst,
    "alpha_imagemap": lambda h: case_alpha(h, "imagemap"),
    "alpha_checkerboard": lambda h: case_alpha(h, "checkerboard"),
    "instances_mp4": lambda h: case_instances(h, 4),
    "instances_mp8": lambda h: case_instances(h, 8),
    "instances_mp4_masked": lambda h: case_instances(h, 4, masked=True),
    "inst_quadric_tri_first": lambda h: case_inst_quadric(h, False),
    "inst_quadric_inst_first": lambda h: case_inst_quadric(h, True),
    "quadric": case_quadric,
}
# every row the issue names is the timed row of some case; its counting row runs with set_traversal_counting on
ROWS_NEEDED = ("ShapeFlat", "ShapeInst", "ShapeFlatAlphaLean", "ShapeInstAlphaLean", "ShapeAlphaGeneral<false>", "ShapeQuadric", "ShapeInstQuadric")


class Prepared:
    """a case, its scene on the oracle, the pool and the oracle's answers and counters for it"""
    pass


_prepared = {}


def build_pool(case, orc):
    """-> (pool, category per position or "" outside the structured batches).  Candidates are sorted into categories by the oracle's counters; a batch takes its rays from the
    category lists in turn, at positions shuffled per batch."""
    cands = {"walker": case.walkers(), "early": early_candidates(orc.world_bound())}
    if case.alpha: cands["mask"] = case.masks()
    lists = {}
    for want, rays in cands.items():
        cat = classify(case, orc.ray_stats_batch(rays))
        cat_sh = classify(case, orc.ray_stats_batch(rays, any_hit=True))
        keep = (cat == want) & ((cat_sh == want) | (want == "walker"))   # (an any-hit ray may stop early: a walker is one by its closest-hit walk)
        lists[want] = rays[keep]
        assert len(lists[want]) >= (8 if want == "early" else 30), (case.name, want, len(lists[want]), len(rays))
    nxt = {k: 0 for k in lists}
    pool, cats = [], []
    for b, comp in enumerate(batch_plan(case)):
        rays, cs = [], []
        for cat, cnt in comp.items():
            pick = (nxt[cat] + np.arange(cnt)) % len(lists[cat]); nxt[cat] += cnt
            rays.append(lists[cat][pick]); cs += [cat] * cnt
        perm = np.random.default_rng(100 + b).permutation(BATCH)
        pool.append(np.concatenate(rays)[perm]); cats += list(np.array(cs)[perm])
    axis = scenes.axis_rays()
    n_fill = N_BIG - STRUCTURED * BATCH - len(axis)
    fill = lists["walker"][(nxt["walker"] + np.arange(n_fill)) % len(lists["walker"])]
    pool += [axis, fill]; cats += [""] * (len(axis) + n_fill)
    pool = np.concatenate(pool)
    assert len(pool) == N_BIG
    return pool, np.array(cats)


def prepared(name, host):
    if name in _prepared: return _prepared[name]
    p = Prepared()
    p.case = CASES[name](host)
    with libm1():
        p.orc = OracleScene()
        p.case.capture(p.orc)
        p.pool, p.cats = build_pool(p.case, p.orc)
        p.hits, p.st_cl = p.orc.intersect_batch_stats(p.pool)
        p.occ, p.st_sh = p.orc.occluded_batch_stats(p.pool)
        p.rs_cl = p.orc.ray_stats_batch(p.pool)
        p.rs_sh = p.orc.ray_stats_batch(p.pool, any_hit=True)
    _prepared[name] = p
    return p
