// Ray binning between wavefront rounds ("ray sorting / Morton ordering").
//
// The reference traces one path at a time (sampler_integrator.rs:352-398), so the order in which a round's rays are traced is a free
// choice here: every ray's result goes to its own slot and nothing else depends on who traces it when.  After the first diffuse bounce
// the queues are in path order, i.e. spatially random, and on scenes larger than the caches every node fetch of a ray then misses L2.
// These kernels produce `order`, a permutation of the round's queue positions grouped by the cell of the ray origin (Morton order
// of a 16^3 grid over the scene bound), closest-hit rays first, any-hit rays behind them —
// the traversal kernel walks the queue through it.  Rays are not moved: the kernel that writes a ray (shade) also writes its 4-byte bin key, the two
// passes here read the keys and write 4 B of `order` per ray.  A closest-hit key may carry the escape-query mark (mis_escape.h: PH_SORT_BINS on top of the bin, written by the path
// integrator's shade pass alone): the ray is binned by its cell as every other, and bit 31 of its entry of `order` hands the mark on to the traversal kernel.
//
// A counting sort without global atomics per ray, in two passes over the keys.  Every block owns a contiguous slice of the queue (raysort_plan.h: the same slice in
// both passes).  The first pass histograms the slice in LDS and adds the non-empty bins to the global tallies, one atomic per block and bin; what the atomic
// returns is where the block's share of that bin starts inside the bin, and the block keeps it: one row of `block_share` per block.  A single block scans the
// 8192 tallies.  The second pass starts a cursor per bin at bin_start + block_share in LDS and ranks its rays with LDS atomics, one per run of equal keys in a lane.  (Until the shares were
// kept, the second pass histogrammed its slice again only to claim them with a second round of global atomics: a third read of the keys, a third LDS-atomic pass
// and a second 32 KB LDS array, which held the kernel to two blocks per CU.)  Keys are read 16 bytes per lane and several loads deep (PH_SORT_DEPTH) before the
// first LDS atomic that depends on them: with one 4-byte load in flight per lane the passes were bound by load latency, at 0.9 - 1.5 TB/s.
// The order inside a bin is whatever the atomics give; no result depends on it.  The time of the traversal kernel does, by about 2 %: neighbours in the queue are mostly
// rays of one pixel in one cell, and it pays to leave them neighbours inside a block's share of a bin (raysort_scatter_kernel).  (Tried and dropped: one LDS atomic per distinct key of a wave, found with a
// ballot loop — a wave of the path-ordered queue holds many distinct keys, the loop cost more than the plain atomics: binning 28 -> 70 ms per configs[2] frame.)
#pragma once
#include "raysort_plan.h"
#include "mis_escape.h"
#include "traverse.h"

namespace ph {

#define PH_SORT_DEPTH 4               // 16-byte key loads a lane issues before it uses the first

struct RaySortParams {
    const uint32_t* keys_cl; const uint32_t* keys_sh;   // one key per queue slot, written by the kernel that wrote the ray (ray_sort_key)
    const uint32_t* n_cl; const uint32_t* n_sh;
    uint32_t* order;        // out: [n_cl + n_sh]
    uint32_t* bin_start;    // [PH_SORT_KEYS] tallies -> exclusive starts (scan kernel)
    uint32_t* block_share;  // [gridDim.x][PH_SORT_KEYS] where each block's rays start inside each bin; 0 for a bin the block has no ray in
};
struct RaySortGrid {        // how a ray is binned: by the cell of its origin in a 16^3 grid over the scene bound
    float lo[3], scale[3];  // cell coordinate = (o - lo) * scale in [0, 1)
};

PH_DEV uint32_t part1by2(uint32_t v) {  // 4 bits -> every third bit
    v &= 0xFu;
    v = (v | (v << 4)) & 0xC3u;
    v = (v | (v << 2)) & 0x249u;
    return v;
}

// bin of a ray with origin (ox, oy, oz): the Morton index of its cell; < PH_SORT_BINS
PH_DEV uint32_t ray_sort_key(const RaySortGrid& g, float ox, float oy, float oz) {
    const float fx = (ox - g.lo[0]) * g.scale[0], fy = (oy - g.lo[1]) * g.scale[1], fz = (oz - g.lo[2]) * g.scale[2];
    // NaN / out-of-bound origins land in the border cells: any bin is a correct bin
    const uint32_t cx = (uint32_t)pmini(pmaxi((int)(fx * 16.0f), 0), 15);
    const uint32_t cy = (uint32_t)pmini(pmaxi((int)(fy * 16.0f), 0), 15);
    const uint32_t cz = (uint32_t)pmini(pmaxi((int)(fz * 16.0f), 0), 15);
    return part1by2(cx) | (part1by2(cy) << 1) | (part1by2(cz) << 2);
}
// The keys of one run of a slice (raysort_plan.h), each handed on by exactly one thread of the block with its joint key (key + key_add) and its joint queue position (position
// in the run's array + pos_add): scalar head, 16-byte body, scalar tail.  The body goes PH_SORT_DEPTH vectors per lane at a time while that many are left, all loads issued
// before `fv` sees them (fv(v, i0): v[d] holds the keys of positions i0 + 4 * d * PH_SORT_BLOCK + 0 .. 3), and one vector at a time through `f1(key, position)` after that.
// CL: the run is the closest-hit keys', of which the shade pass may have marked some as escape queries (mis_escape.h): the joint key then carries the mark in bit 31, above
// every bin — raysort_bin drops it, the scatter pass hands it on into `order`.  A key below PH_SORT_BINS (every key of a frame without the query) is its own joint key.
template <bool CL, class FV, class F1>
PH_DEV void raysort_walk_run(const uint32_t* keys, const RaySortRun& r, uint32_t key_add, uint32_t pos_add, FV&& fv, F1&& f1) {
    auto joint = [&](uint32_t k) -> uint32_t { return CL ? mis_escape_joint_key(k) : k + key_add; };
    if (r.head + threadIdx.x < r.body) f1(joint(keys[r.head + threadIdx.x]), r.head + threadIdx.x + pos_add);
    const uint4* body = reinterpret_cast<const uint4*>(keys + r.body);
    const uint32_t n_vec = (r.tail - r.body) >> 2;
    uint32_t j = threadIdx.x;
    for (; j + (PH_SORT_DEPTH - 1) * PH_SORT_BLOCK < n_vec; j += PH_SORT_DEPTH * PH_SORT_BLOCK) {
        uint4 v[PH_SORT_DEPTH];
#pragma unroll
        for (uint32_t d = 0; d < PH_SORT_DEPTH; d++) v[d] = body[j + d * PH_SORT_BLOCK];
        __builtin_amdgcn_sched_barrier(0);   // (left alone, the scheduler sinks each load to just above its first use: one in flight again)
#pragma unroll
        for (uint32_t d = 0; d < PH_SORT_DEPTH; d++) { v[d].x = joint(v[d].x); v[d].y = joint(v[d].y); v[d].z = joint(v[d].z); v[d].w = joint(v[d].w); }
        fv(v, r.body + 4u * j + pos_add);
    }
    for (; j < n_vec; j += PH_SORT_BLOCK) {
        const uint4 v = body[j];
        const uint32_t i = r.body + 4u * j + pos_add;
        f1(joint(v.x), i); f1(joint(v.y), i + 1u); f1(joint(v.z), i + 2u); f1(joint(v.w), i + 3u);
    }
    if (r.tail + threadIdx.x < r.end) f1(joint(keys[r.tail + threadIdx.x]), r.tail + threadIdx.x + pos_add);
}
// every ray of the slice; an any-hit ray's key lies PH_SORT_BINS up, its position n_cl up
template <class FV, class F1>
PH_DEV void raysort_walk_slice(const RaySortParams& p, const RaySortSlice& s, uint32_t n_cl, FV&& fv, F1&& f1) {
    raysort_walk_run<true>(p.keys_cl, s.cl, 0u, 0u, fv, f1);
    raysort_walk_run<false>(p.keys_sh, s.sh, PH_SORT_BINS, n_cl, fv, f1);
}
PH_DEV RaySortSlice raysort_slice(const RaySortParams& p, uint32_t n_cl, uint32_t n_sh) {
    return raysort_plan(n_cl, n_sh, gridDim.x, PH_SORT_BLOCK, PH_SORT_FLOOR, blockIdx.x, (uint32_t)((uintptr_t)p.keys_cl >> 2) & 3u, (uint32_t)((uintptr_t)p.keys_sh >> 2) & 3u);
}
// a key outside the table (the shade pass writes none) must not reach past the LDS array; the mark of an escape query (bit 31 of a joint key) is no part of the bin
PH_DEV uint32_t raysort_bin(uint32_t key) { return key & (PH_SORT_KEYS - 1u); }
PH_DEV uint32_t raysort_mark(uint32_t key) { return key & PH_ORDER_ESCAPE; }

__global__ __launch_bounds__(PH_SORT_BLOCK) void raysort_hist_kernel(RaySortParams p) {
    __shared__ uint32_t h[PH_SORT_KEYS];
    const uint32_t n_cl = *p.n_cl, n_sh = *p.n_sh;
    const RaySortSlice s = raysort_slice(p, n_cl, n_sh);
    if (s.lo >= s.hi) return;
    for (uint32_t k = threadIdx.x; k < PH_SORT_KEYS; k += PH_SORT_BLOCK) h[k] = 0u;
    __syncthreads();
    raysort_walk_slice(p, s, n_cl,
        [&](const uint4 (&v)[PH_SORT_DEPTH], uint32_t) {
#pragma unroll
            for (uint32_t d = 0; d < PH_SORT_DEPTH; d++) {
                atomicAdd(&h[raysort_bin(v[d].x)], 1u); atomicAdd(&h[raysort_bin(v[d].y)], 1u); atomicAdd(&h[raysort_bin(v[d].z)], 1u); atomicAdd(&h[raysort_bin(v[d].w)], 1u);
            }
        },
        [&](uint32_t key, uint32_t) { atomicAdd(&h[raysort_bin(key)], 1u); });
    __syncthreads();
    uint32_t* share = p.block_share + (size_t)blockIdx.x * PH_SORT_KEYS;
    for (uint32_t k = threadIdx.x; k < PH_SORT_KEYS; k += PH_SORT_BLOCK) {
        const uint32_t c = h[k];
        share[k] = c ? atomicAdd(&p.bin_start[k], c) : 0u;
    }
}

// one block: exclusive scan of the PH_SORT_KEYS tallies in place
__global__ __launch_bounds__(1024) void raysort_scan_kernel(RaySortParams p) {
    __shared__ uint32_t part[1024];
    constexpr uint32_t PER = PH_SORT_KEYS / 1024u;
    uint32_t v[PER], sum = 0u;
    for (uint32_t k = 0; k < PER; k++) { v[k] = p.bin_start[threadIdx.x * PER + k]; sum += v[k]; }
    part[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t o = 1; o < 1024u; o <<= 1) {
        const uint32_t add = threadIdx.x >= o ? part[threadIdx.x - o] : 0u;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    uint32_t run = part[threadIdx.x] - sum;
    for (uint32_t k = 0; k < PER; k++) { p.bin_start[threadIdx.x * PER + k] = run; run += v[k]; }
}

__global__ __launch_bounds__(PH_SORT_BLOCK) void raysort_scatter_kernel(RaySortParams p) {
    __shared__ uint32_t base[PH_SORT_KEYS];  // where the slice's next ray of each bin goes in `order`
    const uint32_t n_cl = *p.n_cl, n_sh = *p.n_sh;
    const RaySortSlice s = raysort_slice(p, n_cl, n_sh);
    if (s.lo >= s.hi) return;
    const uint32_t* share = p.block_share + (size_t)blockIdx.x * PH_SORT_KEYS;
    for (uint32_t k = threadIdx.x; k < PH_SORT_KEYS; k += PH_SORT_BLOCK) base[k] = p.bin_start[k] + share[k];
    __syncthreads();
    raysort_walk_slice(p, s, n_cl,
        [&](const uint4 (&v)[PH_SORT_DEPTH], uint32_t i0) {
            // A lane holds four consecutive queue positions.  Equal keys among them take one atomic (at the first of them) and consecutive ranks, in position order: the queue is
            // in path order, the rays of one pixel follow each other and mostly share a cell, and the traversal kernel is faster by 2 % of its time when such rays stay neighbours in
            // `order` (one atomic per key, four passes over the lanes, deals them out four ways: traversal 652 -> 666 ms per configs[2] frame).
            // All ranks first, then all stores: an LDS atomic that returns is as slow as a load, and a store behind each would make them take turns.
            uint4 at[PH_SORT_DEPTH];
#pragma unroll
            for (uint32_t d = 0; d < PH_SORT_DEPTH; d++) {
                const uint32_t x = raysort_bin(v[d].x), y = raysort_bin(v[d].y), z = raysort_bin(v[d].z), w = raysort_bin(v[d].w);
                const uint32_t yx = y == x, zx = z == x, wx = w == x, zy = z == y, wy = w == y, wz = w == z;
                at[d].x = atomicAdd(&base[x], 1u + yx + zx + wx);
                at[d].y = yx ? 0u : atomicAdd(&base[y], 1u + zy + wy);
                at[d].z = (zx | zy) ? 0u : atomicAdd(&base[z], 1u + wz);
                at[d].w = (wx | wy | wz) ? 0u : atomicAdd(&base[w], 1u);
            }
#pragma unroll
            for (uint32_t d = 0; d < PH_SORT_DEPTH; d++) {
                const uint32_t x = raysort_bin(v[d].x), y = raysort_bin(v[d].y), z = raysort_bin(v[d].z), w = raysort_bin(v[d].w);
                const uint32_t yx = y == x, zx = z == x, wx = w == x, zy = z == y, wy = w == y, wz = w == z;
                const uint32_t rx = at[d].x, ry = yx ? rx + 1u : at[d].y;
                const uint32_t rz = zx ? rx + 1u + yx : zy ? ry + 1u : at[d].z;
                const uint32_t rw = wx ? rx + 1u + yx + zx : wy ? ry + 1u + zy : wz ? rz + 1u : at[d].w;
                const uint32_t i = i0 + 4u * d * PH_SORT_BLOCK;
                p.order[rx] = i | raysort_mark(v[d].x); p.order[ry] = (i + 1u) | raysort_mark(v[d].y); p.order[rz] = (i + 2u) | raysort_mark(v[d].z); p.order[rw] = (i + 3u) | raysort_mark(v[d].w);
            }
        },
        [&](uint32_t key, uint32_t i) { p.order[atomicAdd(&base[raysort_bin(key)], 1u)] = i | raysort_mark(key); });
}

}  // namespace ph
