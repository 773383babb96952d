// HLBVH construction on the device: BVHAccel::new with SplitMethod::HLBVH (accelerators/src/bvh/hlbvh.rs:33-449, morton.rs:33-120),
// the same tree the host builder (bvh_build.cpp) and the reference make — including the reference's Morton quirk (quirk B10: the code interleaves the
// low bits of the IEEE BIT PATTERN of the scaled centroid offset, morton.rs:33-39) — so closest hits, ties included, do not depend on where the tree was built.
//
// One build makes a FOREST of trees laid out [scene | object | object ..] (bvh_build.h): the scene's aggregate and, for scenes with object instances, every instanced object's,
// all in the same launches.  A scene without instances is a forest of one tree whose item i is triangle i (no item list, no instances).
//
//   K1  item bounds + every tree's bounds      compute_morton_primitives' inputs (hlbvh.rs:52-60; Triangle::world_bound triangle.rs:427-431); the objects' trees first, then the
//                                              instances' world bounds (transform.rs:552-561), then the scene's tree, which holds them
//   K2  Morton codes, relative to the item's   hlbvh.rs:97-135, morton.rs:33-48, :101-118
//       own tree's bounds
//   K3  stable LSD radix sort, 8-bit digits    morton.rs:50-98 sorts 5 x 6 bits; any stable sort by the 30-bit code gives the same order.  Four passes over the code, then (more
//                                              than one tree) passes over the tree: sorted by (tree, code), every tree in its own range
//   K4  treelets: maximal runs of equal        hlbvh.rs:62-84; run heads counted per block, scanned, written out in order
//       (tree, top 12 code bits)
//   K5  emit_lbvh, one level per launch        hlbvh.rs:199-294 (the treelets of all trees side by side; round 3 — rounds 1 - 2 gave each treelet one thread)
//   --  per tree, on the host: SAH over its    hlbvh.rs:296-432 (bvh_build.cpp: build_upper_sah), where its treelets' nodes and leaf records go, its SAH nodes — and for a real
//       treelet roots                          forest the host builder's node numbering: hlbvh_forest_stitch.h
//   K6  Node64 / TriRec emission               the device layout of scene_types.h; leaves in depth-first order as flatten_bvh_tree leaves them
//
// Inside a treelet emit_lbvh always splits a sorted range into a lower and an upper part, so the depth-first leaf order of a treelet IS the sorted
// order; a tree's leaf order is its treelets' ranges concatenated in the depth-first order of its upper SAH tree.
#include "scene_host.h"
#include "device_build_stage.h"
#include "host_math.h"
#include "hlbvh_forest_stitch.h"
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <thread>

namespace phd {

struct DNode {  // a build node of a treelet: 48 B
    float lo[3]; uint32_t kid0;   // kids: pool indices; leaf: 0xFFFFFFFF
    float hi[3]; uint32_t kid1;
    uint32_t first, count;        // leaf: range of the SORTED primitive list
    uint32_t axis, dense;         // interior: split axis, index among the treelet's interior nodes in creation order
};
#define PHD_NONE 0xFFFFFFFFu

__device__ __forceinline__ float fmn(float a, float b) { return a < b ? a : b; }   // core/src/pbrt/common.rs:81-92 (`<`-based)
__device__ __forceinline__ float fmx(float a, float b) { return a > b ? a : b; }
// order-preserving map float -> uint32 for atomicMin / atomicMax
__device__ __forceinline__ uint32_t f2ord(float f) { const uint32_t u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__host__ __device__ inline float ord2f(uint32_t o) { const uint32_t u = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o; float f; memcpy(&f, &u, 4); return f; }

__device__ __forceinline__ uint32_t left_shift_3(uint32_t x) {  // morton.rs:101-118
    uint32_t v = (x == (1u << 10)) ? x - 1 : x;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
// K3: one pass of a stable least-significant-digit radix sort, 8-bit digits.  Block b owns the contiguous slice [b * per, (b + 1) * per).
#define PHD_RS_BLOCK 256
__global__ __launch_bounds__(PHD_RS_BLOCK) void rs_hist_kernel(const uint32_t* keys, uint32_t n, uint32_t per, int shift, uint32_t* block_hist /*[256][gridDim.x]*/) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t lo = blockIdx.x * per, hi = lo + per < n ? lo + per : n;
    for (uint32_t i = lo + threadIdx.x; i < hi; i += PHD_RS_BLOCK) atomicAdd(&h[(keys[i] >> shift) & 255u], 1u);
    __syncthreads();
    block_hist[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = h[threadIdx.x];
}
// (the scan of the block histograms between the two: exclusive_scan_kernel, device_build_stage.h)
__global__ __launch_bounds__(PHD_RS_BLOCK) void rs_scatter_kernel(const uint32_t* keys, const uint32_t* vals, uint32_t* keys_out, uint32_t* vals_out, uint32_t n, uint32_t per, int shift,
                                                                 const uint32_t* block_base /*scanned [256][gridDim.x]*/) {
    __shared__ uint32_t run[256];                       // where the block's next key of each digit goes
    __shared__ uint32_t cnt[PHD_RS_BLOCK / 64][256];    // this round's keys per wave and digit
    run[threadIdx.x] = block_base[(size_t)threadIdx.x * gridDim.x + blockIdx.x];
    const uint32_t lo = blockIdx.x * per, hi = lo + per < n ? lo + per : n;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t lane_lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    for (uint32_t base = lo; base < hi; base += PHD_RS_BLOCK) {   // rounds of 256 keys, in order: stability
        for (uint32_t w = 0; w < PHD_RS_BLOCK / 64; w++) cnt[w][threadIdx.x] = 0u;
        __syncthreads();
        const uint32_t i = base + threadIdx.x;
        const bool ok = i < hi;
        uint32_t key = 0, val = 0, d = 0;
        if (ok) { key = keys[i]; val = vals[i]; d = (key >> shift) & 255u; }
        // lanes of the wave with the same digit (eight ballots), rank among them
        uint64_t same = __ballot(ok);
        for (int b = 0; b < 8; b++) { const uint64_t m = __ballot((d >> b) & 1u); same &= ((d >> b) & 1u) ? m : ~m; }
        const uint32_t rank = (uint32_t)__popcll(same & lane_lt);
        if (ok && rank == 0u) cnt[wave][d] = (uint32_t)__popcll(same);
        __syncthreads();
        if (ok) {
            uint32_t pos = run[d] + rank;
            for (uint32_t w = 0; w < wave; w++) pos += cnt[w][d];
            keys_out[pos] = key; vals_out[pos] = val;
        }
        __syncthreads();
        uint32_t tot = 0u;
        for (uint32_t w = 0; w < PHD_RS_BLOCK / 64; w++) tot += cnt[w][threadIdx.x];
        run[threadIdx.x] += tot;
        __syncthreads();
    }
}

// K5: emit_lbvh (hlbvh.rs:199-294) for all treelets at once, one LEVEL of the recursion per launch (round 3).  The reference's Morton quirk (B10) leaves a few treelets with
// millions of primitives; one thread per treelet — rounds 1 - 2 — spent 0.3 s of a 10 M-triangle build walking those alone.  emit_lbvh only ever cuts a sorted range in two
// at the first index whose code differs in the current bit, so a node is known by its range: every node of a level is decided independently (skip the bits that do not
// split, leaf or binary search), and what the recursion's order decides — the interior nodes' creation (pre-order) numbers, the boxes — follows from two more sweeps over the
// levels: bottom-up the boxes and the number of interior nodes below each node, top-down `dense` = the parent's number + 1 (+ the first child's subtree for the second child).
// A node's pool slot is a function of its range (interior: 2 x its split position; leaf: 2 x its first position + 1; a treelet's root: 2 x the treelet's first position,
// where f_roots_kernel looks for it), so no slot counter is shared and slot j belongs to the treelet of position j / 2 (f_convert_kernel).
struct TreeletInfo { uint32_t first, n, interior, leaves, max_leaf, depth, pad[2]; };
struct EmitItem { uint32_t first, n, slot_of_parent, tree; int bit; uint32_t which, self, pad; };   // which: 0 / 1 = first / second child, 2 = a treelet's root
#define PHD_MAX_LEVELS 20   // a split consumes at least one of the 18 code bits below the treelet key: 19 levels at most

// one level: every item decides leaf / split, writes its node, tells its parent where it lives and appends its two children to the next level
__global__ __launch_bounds__(256) void emit_level_kernel(EmitItem* items, const uint32_t* lvl, int level, uint32_t* n_items, const uint32_t* codes, uint32_t max_prims, DNode* pool, uint32_t* leaf_last,
                                                         TreeletInfo* info) {
    const uint32_t i = lvl[level] + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= lvl[level + 1]) return;
    EmitItem it = items[i];
    int bit = it.bit;
    bool leaf = false;
    for (;;) {
        if (bit == -1 || it.n < max_prims) { leaf = true; break; }
        const uint32_t mask = 1u << bit;
        if ((codes[it.first] & mask) != (codes[it.first + it.n - 1] & mask)) break;
        bit--;   // no split on this bit
    }
    uint32_t hi = 0;
    if (!leaf) {   // hlbvh.rs:253-268: first index whose bit differs from the first primitive's
        const uint32_t mask = 1u << bit;
        uint32_t lo = 0; hi = it.n - 1;
        while (lo + 1 != hi) {
            const uint32_t mid = (lo + hi) / 2;
            if ((codes[it.first + lo] & mask) == (codes[it.first + mid] & mask)) lo = mid; else hi = mid;
        }
    }
    const uint32_t self = it.which == 2u ? 2u * it.first : (leaf ? 2u * it.first + 1u : 2u * (it.first + hi));
    items[i].self = self; items[i].bit = leaf ? -2 : bit;   // (-2: a leaf, for the two sweeps that follow)
    if (it.which == 0u) pool[it.slot_of_parent].kid0 = self; else if (it.which == 1u) pool[it.slot_of_parent].kid1 = self;
    DNode& nd = pool[self];
    if (leaf) {
        nd.kid0 = nd.kid1 = PHD_NONE; nd.first = it.first; nd.count = it.n; nd.axis = 0; nd.dense = 0;
        leaf_last[it.first + it.n - 1] = 1u;
        atomicAdd(&info[it.tree].leaves, 1u); atomicMax(&info[it.tree].max_leaf, it.n); atomicMax(&info[it.tree].depth, (uint32_t)level + 1u);
        return;
    }
    nd.count = 0; nd.first = 0; nd.axis = (uint32_t)(bit % 3); nd.dense = 0;
    const uint32_t at = atomicAdd(n_items, 2u);
    items[at] = EmitItem{it.first, hi, self, it.tree, bit - 1, 0u, 0u, 0u};
    items[at + 1u] = EmitItem{it.first + hi, it.n - hi, self, it.tree, bit - 1, 1u, 0u, 0u};
}
__global__ void emit_close_level_kernel(uint32_t* lvl, int level, const uint32_t* n_items) { if (threadIdx.x == 0 && blockIdx.x == 0) lvl[level + 2] = *n_items; }
// bottom-up: boxes, and in `first` of an interior node the number of interior nodes of its subtree
__global__ __launch_bounds__(256) void emit_up_kernel(const EmitItem* items, const uint32_t* lvl, int level, const uint32_t* ids, const float* blo, const float* bhi, DNode* pool) {
    const uint32_t i = lvl[level] + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= lvl[level + 1]) return;
    const EmitItem it = items[i];
    DNode& nd = pool[it.self];
    if (it.bit == -2) {
        float lo[3], hi[3];
        for (uint32_t k = 0; k < it.n; k++) {
            const size_t id = ids[it.first + k];
            for (int q = 0; q < 3; q++) {
                const float l = blo[3 * id + q], h = bhi[3 * id + q];
                lo[q] = k == 0 ? l : fmn(lo[q], l); hi[q] = k == 0 ? h : fmx(hi[q], h);
            }
        }
        for (int q = 0; q < 3; q++) { nd.lo[q] = lo[q]; nd.hi[q] = hi[q]; }
        return;
    }
    const DNode& a = pool[nd.kid0]; const DNode& b = pool[nd.kid1];
    for (int q = 0; q < 3; q++) { nd.lo[q] = fmn(a.lo[q], b.lo[q]); nd.hi[q] = fmx(a.hi[q], b.hi[q]); }
    nd.first = 1u + (a.kid0 == PHD_NONE ? 0u : a.first) + (b.kid0 == PHD_NONE ? 0u : b.first);
}
// top-down: the creation numbers of the recursion (a node, then its whole first subtree, then the second)
__global__ __launch_bounds__(256) void emit_down_kernel(const EmitItem* items, const uint32_t* lvl, int level, DNode* pool, TreeletInfo* info) {
    const uint32_t i = lvl[level] + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= lvl[level + 1]) return;
    const EmitItem it = items[i];
    if (it.bit == -2) return;
    DNode& nd = pool[it.self];
    if (it.which == 2u) { nd.dense = 0u; info[it.tree].interior = nd.first; }
    DNode& a = pool[nd.kid0]; DNode& b = pool[nd.kid1];
    const uint32_t below_a = a.kid0 == PHD_NONE ? 0u : a.first;
    if (a.kid0 != PHD_NONE) a.dense = nd.dense + 1u;
    if (b.kid0 != PHD_NONE) b.dense = nd.dense + 1u + below_a;
}

// A POSITION of the item list belongs to the same tree before and after the sort (the sort is by (tree, code) and the items start grouped by tree), so one table says which.
__global__ __launch_bounds__(256) void f_tree_of_kernel(const uint32_t* tree_start, uint32_t n_trees, uint32_t n, uint32_t* tree_of) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t lo = 0, hi = n_trees;   // the last tree whose start is <= i
    while (lo + 1 < hi) { const uint32_t mid = (lo + hi) >> 1; if (tree_start[mid] <= i) lo = mid; else hi = mid; }
    tree_of[i] = lo;
}
// K1: bounds of the items at positions [i0, i1) (a primitive slot, or PH_ITEM_INST | k with the bound inst_bounds[6k ..]; no item list: item i is slot i) and, per tree, the union of them.
// A slot holds a triangle or, where prim_quadric[slot] = 1 + q, a quadric whose bound quad_bounds[6q ..] the caller computed (bvh_build.cpp:421-423); its index triple is never followed.
// prim_quadric is null in a scene without quadrics.
__global__ __launch_bounds__(256) void f_bounds_kernel(const float* P, const uint32_t* idx, const uint32_t* items, const float* inst_bounds, const uint32_t* prim_quadric, const float* quad_bounds,
                                                       const uint32_t* tree_of, uint32_t i0, uint32_t i1, float* blo, float* bhi, uint32_t* tb /*[n_trees][6]: ord(min xyz), ord(max xyz)*/) {
    const uint32_t first = i0 + blockIdx.x * blockDim.x, i = first + threadIdx.x;
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    const bool ok = i < i1;
    if (ok) {
        const uint32_t item = items ? items[i] : i;
        const uint32_t quad = (prim_quadric && !(item & PH_ITEM_INST)) ? prim_quadric[item] : 0u;
        if (item & PH_ITEM_INST) {
            const float* bb = inst_bounds + 6 * (size_t)(item & ~PH_ITEM_INST);
            for (int k = 0; k < 3; k++) { lo[k] = bb[k]; hi[k] = bb[3 + k]; }
        } else if (quad) {
            const float* bb = quad_bounds + 6 * (size_t)(quad - 1u);
            for (int k = 0; k < 3; k++) { lo[k] = bb[k]; hi[k] = bb[3 + k]; }
        } else {
            const float* a = P + 3 * (size_t)idx[3 * (size_t)item];
            const float* b = P + 3 * (size_t)idx[3 * (size_t)item + 1];
            const float* c = P + 3 * (size_t)idx[3 * (size_t)item + 2];
            for (int k = 0; k < 3; k++) { lo[k] = fmn(fmn(a[k], b[k]), c[k]); hi[k] = fmx(fmx(a[k], b[k]), c[k]); }
        }
        for (int k = 0; k < 3; k++) { blo[3 * (size_t)i + k] = lo[k]; bhi[3 * (size_t)i + k] = hi[k]; }
    }
    const uint32_t last = first + blockDim.x - 1u < i1 ? first + blockDim.x - 1u : i1 - 1u;
    const uint32_t t_first = tree_of[first], t_last = tree_of[last];   // (first < i1 for every block of the grid)
    if (t_first == t_last) {   // the whole block in one tree: reduce in LDS first (the same for every thread of the block)
        __shared__ uint32_t sm[6];
        if (threadIdx.x < 3) { sm[threadIdx.x] = 0xFFFFFFFFu; sm[3 + threadIdx.x] = 0u; }
        __syncthreads();
        if (ok) for (int k = 0; k < 3; k++) { atomicMin(&sm[k], f2ord(lo[k])); atomicMax(&sm[3 + k], f2ord(hi[k])); }
        __syncthreads();
        if (threadIdx.x < 3) { atomicMin(&tb[6 * (size_t)t_first + threadIdx.x], sm[threadIdx.x]); atomicMax(&tb[6 * (size_t)t_first + 3 + threadIdx.x], sm[3 + threadIdx.x]); }
    } else if (ok) {
        uint32_t* g = tb + 6 * (size_t)tree_of[i];
        for (int k = 0; k < 3; k++) { atomicMin(&g[k], f2ord(lo[k])); atomicMax(&g[3 + k], f2ord(hi[k])); }
    }
}
// TransformedPrimitive::world_bound of every instance: Transform::transform_bounds (transform.rs:552-561) of its object's tree bounds — phost::transform_bounds, expression by expression
__global__ __launch_bounds__(256) void f_inst_bounds_kernel(const uint32_t* tb, const uint32_t* inst_tree, const float* i2w, uint32_t n_inst, float* inst_bounds) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_inst) return;
    const float* m = i2w + 16 * (size_t)k;
    const uint32_t* g = tb + 6 * (size_t)inst_tree[k];
    float lo[3], hi[3], ob[6];
    for (int a = 0; a < 3; a++) { lo[a] = ord2f(g[a]); hi[a] = ord2f(g[3 + a]); ob[a] = ob[3 + a] = 0.0f; }
    for (int c = 0; c < 8; c++) {   // corners in the reference's order: lll hll lhl llh lhh hhl hlh hhh
        const bool hx = c == 1 || c == 5 || c == 6 || c == 7, hy = c == 2 || c == 4 || c == 5 || c == 7, hz = c == 3 || c == 4 || c == 6 || c == 7;
        const float x = hx ? hi[0] : lo[0], y = hy ? hi[1] : lo[1], z = hz ? hi[2] : lo[2];
        const float xp = m[0] * x + m[1] * y + m[2] * z + m[3], yp = m[4] * x + m[5] * y + m[6] * z + m[7];
        const float zp = m[8] * x + m[9] * y + m[10] * z + m[11], wp = m[12] * x + m[13] * y + m[14] * z + m[15];
        float q[3];
        if (wp == 1.0f) { q[0] = xp; q[1] = yp; q[2] = zp; } else { const float inv = 1.0f / wp; q[0] = inv * xp; q[1] = inv * yp; q[2] = inv * zp; }
        for (int a = 0; a < 3; a++) {
            if (c == 0) { ob[a] = ob[3 + a] = q[a]; }
            else { ob[a] = ob[a] < q[a] ? ob[a] : q[a]; ob[3 + a] = ob[3 + a] > q[a] ? ob[3 + a] : q[a]; }
        }
    }
    for (int a = 0; a < 6; a++) inst_bounds[6 * (size_t)k + a] = ob[a];
}
// K2: a code is relative to the bounds of its own tree.  vals = the item's position before the sort.
__global__ __launch_bounds__(256) void f_morton_kernel(const float* blo, const float* bhi, uint32_t n, const uint32_t* tb, const uint32_t* tree_of, uint32_t* codes, uint32_t* codes_keep, uint32_t* ids) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* g = tb + 6 * (size_t)tree_of[i];
    uint32_t c[3];
    for (int k = 0; k < 3; k++) {
        const float glo = ord2f(g[k]), ghi = ord2f(g[3 + k]);
        const float ctr = 0.5f * (blo[3 * (size_t)i + k] + bhi[3 * (size_t)i + k]);
        float o = ctr - glo;
        if (ghi > glo) o = o / (ghi - glo);
        c[k] = left_shift_3(__float_as_uint(o * 1024.0f));
    }
    const uint32_t code = (c[2] << 2) | (c[1] << 1) | c[0];
    codes[i] = code; codes_keep[i] = code; ids[i] = i;
}
// K3: after the passes over the code, passes over the tree of every item (keys = that tree) bring each tree's items back to its own range, in code order
__global__ __launch_bounds__(256) void f_lookup_kernel(const uint32_t* ids, const uint32_t* table, uint32_t n, uint32_t* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = table[ids[i]];
}
// K4: a treelet is a maximal run of equal (tree, top 12 code bits).  Count the run heads per block, scan, write them out in order.
__device__ __forceinline__ bool f_is_head(const uint32_t* codes, const uint32_t* tree_of, uint32_t i) { return i == 0u || tree_of[i] != tree_of[i - 1u] || (codes[i] >> 18) != (codes[i - 1u] >> 18); }
__global__ __launch_bounds__(256) void f_heads_count_kernel(const uint32_t* codes, const uint32_t* tree_of, uint32_t n, uint32_t* block_counts) {
    __shared__ uint32_t wave_n[4];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool head = i < n && f_is_head(codes, tree_of, i);
    const uint64_t m = __ballot(head);
    if ((threadIdx.x & 63u) == 0u) wave_n[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0u) block_counts[blockIdx.x] = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
}
__global__ __launch_bounds__(256) void f_heads_write_kernel(const uint32_t* codes, const uint32_t* tree_of, uint32_t n, const uint32_t* block_base /*scanned*/, uint32_t n_treelets, uint32_t* tl_first /*n_treelets + 1*/,
                                                            uint32_t* tl_of_pos) {
    __shared__ uint32_t wave_n[4];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool head = i < n && f_is_head(codes, tree_of, i);
    const uint64_t m = __ballot(head);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0u) wave_n[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (i >= n) return;
    uint32_t at = block_base[blockIdx.x] + (uint32_t)__popcll(m & (lane == 0u ? 0ull : (~0ull >> (64u - lane))));   // heads before this position
    for (uint32_t w = 0; w < wave; w++) at += wave_n[w];
    if (head) { if (at < n_treelets) tl_first[at] = i; tl_of_pos[i] = at; } else tl_of_pos[i] = at - 1u;   // (position 0 is a head: at >= 1 here)
    if (i == 0u) tl_first[n_treelets] = n;
}
__global__ __launch_bounds__(256) void f_emit_roots_kernel(const uint32_t* tl_first, uint32_t n_treelets, EmitItem* items, uint32_t* lvl, uint32_t* n_items, TreeletInfo* info) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0) { lvl[0] = 0u; lvl[1] = n_treelets; *n_items = n_treelets; }
    if (t >= n_treelets) return;
    const uint32_t first = tl_first[t], cnt = tl_first[t + 1u] - first;
    items[t] = EmitItem{first, cnt, PHD_NONE, t, 29 - 12, 2u, 0u, 0u};
    info[t] = TreeletInfo{first, cnt, 0u, 0u, 0u, 0u, {0u, 0u}};
}
// the treelet roots' boxes, side by side for one read-back
__global__ __launch_bounds__(256) void f_roots_kernel(const DNode* pool, const uint32_t* tl_first, uint32_t n_treelets, float* rb /*6 per treelet*/) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_treelets) return;
    const DNode& r = pool[2 * (size_t)tl_first[t]];
    for (int k = 0; k < 3; k++) { rb[6 * (size_t)t + k] = r.lo[k]; rb[6 * (size_t)t + 3 + k] = r.hi[k]; }
}
// K6a: every interior build node of every treelet -> its Node64 (both children's boxes, child references in the final numbering); one thread per pool slot (a slot belongs to the treelet of position slot / 2)
__global__ __launch_bounds__(256) void f_convert_kernel(const DNode* pool, uint32_t n, const uint32_t* tl_of_pos, const uint32_t* tl_first, const uint32_t* tl_dense_base, const uint32_t* tl_out_base, Node64* nodes) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= 2u * n) return;
    const DNode nd = pool[j];
    if (nd.kid0 == PHD_NONE) return;   // a leaf, or a slot no treelet used (the pool is cleared to 0xFF first)
    const uint32_t t = tl_of_pos[j >> 1], T0 = tl_first[t];
    const DNode a = pool[nd.kid0], b = pool[nd.kid1];
    auto ref = [&](const DNode& c) { return c.kid0 == PHD_NONE ? (PH_LEAF_BIT | (tl_out_base[t] + (c.first - T0))) : tl_dense_base[t] + c.dense; };
    Node64 o;
    o.x0[0] = a.lo[0]; o.x0[1] = a.hi[0]; o.y0[0] = a.lo[1]; o.y0[1] = a.hi[1]; o.z0[0] = a.lo[2]; o.z0[1] = a.hi[2];
    o.x1[0] = b.lo[0]; o.x1[1] = b.hi[0]; o.y1[0] = b.lo[1]; o.y1[1] = b.hi[1]; o.z1[0] = b.lo[2]; o.z1[1] = b.hi[2];
    o.c0 = ref(a); o.c1 = ref(b); o.axis = nd.axis; o.pad = 0;
    nodes[tl_dense_base[t] + nd.dense] = o;
}
// K6b: leaf records in the final order; an instance's record is what build_bvh writes (prim, PH_TRI_INSTANCE, the rest zero until the scene is uploaded), and so is a quadric's
// (bvh_build.cpp:451-455: the quadric's index as the bit pattern of p0[0], the slot, PH_TRI_QUADRIC, the slot's flags and mesh, the rest zero)
__global__ __launch_bounds__(256) void f_gather_kernel(const uint32_t* ids, const uint32_t* leaf_last, const uint32_t* tl_of_pos, const uint32_t* tl_first, const uint32_t* tl_out_base, uint32_t n, const uint32_t* items,
                                                       const float* P, const uint32_t* idx, const uint32_t* tri_flags, const uint32_t* tri_mesh, const uint32_t* prim_quadric, TriRec* tris) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t t = tl_of_pos[i];
    const uint32_t q = tl_out_base[t] + (i - tl_first[t]);
    const uint32_t id = items ? items[ids[i]] : ids[i];
    const uint32_t last = leaf_last[i] ? PH_TRI_LAST : 0u;
    const uint32_t quad = (prim_quadric && !(id & PH_ITEM_INST)) ? prim_quadric[id] : 0u;
    TriRec r;
    if (id & PH_ITEM_INST) {
        r.p0[0] = r.p0[1] = r.p0[2] = 0.0f; r.prim = id & ~PH_ITEM_INST;
        r.p1[0] = r.p1[1] = r.p1[2] = 0.0f; r.flags = PH_TRI_INSTANCE | last;
        r.p2[0] = r.p2[1] = r.p2[2] = 0.0f; r.mesh = 0u;
    } else if (quad) {
        r.p0[0] = __uint_as_float(quad - 1u); r.p0[1] = r.p0[2] = 0.0f; r.prim = id;
        r.p1[0] = r.p1[1] = r.p1[2] = 0.0f; r.flags = ((tri_flags ? tri_flags[id] : 0u) & ~PH_TRI_LAST) | PH_TRI_QUADRIC | last;
        r.p2[0] = r.p2[1] = r.p2[2] = 0.0f; r.mesh = tri_mesh ? tri_mesh[id] : 0u;
    } else {
        const float* p0 = P + 3 * (size_t)idx[3 * (size_t)id]; const float* p1 = P + 3 * (size_t)idx[3 * (size_t)id + 1]; const float* p2 = P + 3 * (size_t)idx[3 * (size_t)id + 2];
        r.p0[0] = p0[0]; r.p0[1] = p0[1]; r.p0[2] = p0[2]; r.prim = id;
        r.p1[0] = p1[0]; r.p1[1] = p1[1]; r.p1[2] = p1[2]; r.flags = ((tri_flags ? tri_flags[id] : 0u) & ~PH_TRI_LAST) | last;
        r.p2[0] = p2[0]; r.p2[1] = p2[1]; r.p2[2] = p2[2]; r.mesh = tri_mesh ? tri_mesh[id] : 0u;
    }
    tris[q] = r;
}

}  // namespace phd

namespace phost {

// Builds the HLBVH of `in` on the current device — or, with `forest`, the scene's aggregate and the aggregates of its instanced objects in one go, laid out
// [scene | object | object ..] as build_forest_host lays them out; every kernel runs over all trees at once.  Without `forest` the input is one tree of all its triangles.
// The host waits for the device three times: for the number of treelets, for the treelet roots (the SAH over them, per tree, is the host's: hlbvh_forest_stitch.h) and for the result.
// Returns 0, -1 (bad arguments / device failure, `err` says which), -2 (one of the reference's HLBVH assertions fires on this input).
int build_hlbvh_device(const BuildInput& in, int max_prims_in_node, hipStream_t stream, BuildOutput& out, std::string& err, const ForestSpec* forest, std::vector<ForestTreeOut>* trees_out) {
    out = BuildOutput();
    if (trees_out) trees_out->clear();
    if (check_device_build_input(in, forest, err) != 0) return -1;
    const DeviceBuildItems bi(in, forest);
    const uint32_t n = bi.n, n_trees = bi.n_trees;
    if (n == 0) return 0;
    const uint32_t* tree_start = bi.tree_start(); const uint32_t top_end = bi.top_end(); const size_t n_inst = bi.n_inst();
    const uint32_t max_prims = (uint32_t)(max_prims_in_node & 0xff);   // bvh/mod.rs:357 `as u8`
    // host staging stands before the arena: it outlives the arena's wait for the stream, whichever way the function is left
    std::vector<phd::TreeletInfo> info; std::vector<float> rb; std::vector<StitchTreelet> tl; StitchPlan plan;
    const BuildLaps lap{"build_hlbvh_forest_device n=" + std::to_string(n) + " trees=" + std::to_string(n_trees), stream};
    std::vector<uint32_t> tb_init((size_t)n_trees * 6);
    for (uint32_t t = 0; t < n_trees; t++) for (int k = 0; k < 3; k++) { tb_init[6 * (size_t)t + k] = 0xFFFFFFFFu; tb_init[6 * (size_t)t + 3 + k] = 0u; }
    DeviceArena arena(stream);
    const DeviceBuildInput d = upload_build_input(arena, in, bi);
    uint32_t* tree_of = arena.alloc<uint32_t>(n);
    uint32_t* d_inst_tree = arena.upload(n_inst ? forest->inst_tree : nullptr, n_inst); float* d_i2w = arena.upload(n_inst ? forest->inst_i2w : nullptr, n_inst * 16);
    float* d_inst_bounds = arena.alloc<float>(n_inst * 6);
    float* blo = arena.alloc<float>((size_t)n * 3); float* bhi = arena.alloc<float>((size_t)n * 3);
    uint32_t* tb = arena.upload(tb_init.data(), tb_init.size());
    uint32_t* keys[2] = {arena.alloc<uint32_t>(n), arena.alloc<uint32_t>(n)};
    uint32_t* vals[2] = {arena.alloc<uint32_t>(n), arena.alloc<uint32_t>(n)};
    uint32_t* codes_keep = arena.alloc<uint32_t>(n);
    const uint32_t nb = std::min<uint32_t>(1024u, (n + 2047u) / 2048u), per = (((n + nb - 1u) / nb) + 255u) & ~255u;
    uint32_t* bh = arena.alloc<uint32_t>((size_t)256 * nb);
    const uint32_t n_blocks = (n + 255u) / 256u;
    uint32_t* head_counts = arena.alloc<uint32_t>((size_t)n_blocks + 1);
    uint32_t* tl_of_pos = arena.alloc<uint32_t>(n);
    uint32_t* leaf_last = arena.alloc<uint32_t>(n);
    phd::DNode* pool = arena.alloc<phd::DNode>((size_t)2 * n);
    phd::EmitItem* items = arena.alloc<phd::EmitItem>((size_t)2 * n);
    uint32_t* lvl = arena.alloc<uint32_t>(PHD_MAX_LEVELS + 2); uint32_t* n_items = arena.alloc<uint32_t>(4);
    TriRec* d_tris = arena.alloc<TriRec>(n);
    if (!arena.ok()) { err = "device build: " + arena.why(); return -1; }
    uint32_t nt = 0;
    PH_BUILD_CHECK(hipMemsetAsync(head_counts, 0, ((size_t)n_blocks + 1) * 4, stream));
    PH_BUILD_CHECK(hipMemsetAsync(pool, 0xFF, (size_t)2 * n * sizeof(phd::DNode), stream));
    PH_BUILD_CHECK(hipMemsetAsync(leaf_last, 0, (size_t)n * 4, stream));
    PH_BUILD_CHECK(hipMemsetAsync(lvl, 0, (PHD_MAX_LEVELS + 2) * 4, stream));
    const dim3 g(n_blocks), b(256);
    lap("allocations and uploads");
    hipLaunchKernelGGL(phd::f_tree_of_kernel, g, b, 0, stream, d.tree_start, n_trees, n, tree_of);
    // K1: the objects' trees first — the scene's tree holds TransformedPrimitives, whose bounds are the objects' tree bounds carried to world space
    if (n > top_end) hipLaunchKernelGGL(phd::f_bounds_kernel, dim3((n - top_end + 255u) / 256u), b, 0, stream, d.P, d.idx, d.items, d_inst_bounds, d.prim_quadric, d.quad_bounds, tree_of, top_end, n, blo, bhi, tb);
    if (n_inst) hipLaunchKernelGGL(phd::f_inst_bounds_kernel, dim3((uint32_t)((n_inst + 255u) / 256u)), b, 0, stream, tb, d_inst_tree, d_i2w, (uint32_t)n_inst, d_inst_bounds);
    hipLaunchKernelGGL(phd::f_bounds_kernel, dim3((top_end + 255u) / 256u), b, 0, stream, d.P, d.idx, d.items, d_inst_bounds, d.prim_quadric, d.quad_bounds, tree_of, 0u, top_end, blo, bhi, tb);
    hipLaunchKernelGGL(phd::f_morton_kernel, g, b, 0, stream, blo, bhi, n, tb, tree_of, keys[0], codes_keep, vals[0]);
    int cur = 0;
    auto sort_pass = [&](int shift) {
        hipLaunchKernelGGL(phd::rs_hist_kernel, dim3(nb), dim3(PHD_RS_BLOCK), 0, stream, keys[cur], n, per, shift, bh);
        hipLaunchKernelGGL(exclusive_scan_kernel, dim3(1), dim3(1024), 0, stream, bh, 256u * nb);
        hipLaunchKernelGGL(phd::rs_scatter_kernel, dim3(nb), dim3(PHD_RS_BLOCK), 0, stream, keys[cur], vals[cur], keys[cur ^ 1], vals[cur ^ 1], n, per, shift, bh);
        cur ^= 1;
    };
    for (int pass = 0; pass < 4; pass++) sort_pass(pass * 8);   // K3: by the 30-bit code ..
    if (n_trees > 1) {                                          // .. then by the tree, as many digits as n_trees - 1 has
        hipLaunchKernelGGL(phd::f_lookup_kernel, g, b, 0, stream, vals[cur], tree_of, n, keys[cur]);
        for (int shift = 0; shift < 32 && ((n_trees - 1u) >> shift) != 0u; shift += 8) sort_pass(shift);
        hipLaunchKernelGGL(phd::f_lookup_kernel, g, b, 0, stream, vals[cur], codes_keep, n, keys[cur]);   // the keys were the trees: the codes again, in the sorted order
    }
    uint32_t* ids = vals[cur]; uint32_t* codes = keys[cur];
    // K4: run heads, counted and compacted
    hipLaunchKernelGGL(phd::f_heads_count_kernel, g, b, 0, stream, codes, tree_of, n, head_counts);
    hipLaunchKernelGGL(exclusive_scan_kernel, dim3(1), dim3(1024), 0, stream, head_counts, n_blocks + 1u);
    PH_BUILD_CHECK(hipGetLastError());
    PH_BUILD_CHECK(hipMemcpyAsync(&nt, head_counts + n_blocks, 4, hipMemcpyDeviceToHost, stream));
    PH_BUILD_CHECK(hipStreamSynchronize(stream));
    lap("bounds, codes, sort, heads");
    if (nt == 0 || nt > n) { err = "device build: treelet count out of range"; return -1; }
    uint32_t* d_tl_first = arena.alloc<uint32_t>((size_t)nt + 1); uint32_t* d_tl_dense = arena.alloc<uint32_t>(nt); uint32_t* d_tl_out = arena.alloc<uint32_t>(nt);
    phd::TreeletInfo* d_info = arena.alloc<phd::TreeletInfo>(nt); float* d_rb = arena.alloc<float>((size_t)nt * 6);
    if (!arena.ok()) { err = "device build: " + arena.why(); return -1; }
    const dim3 gt((nt + 255u) / 256u);
    hipLaunchKernelGGL(phd::f_heads_write_kernel, g, b, 0, stream, codes, tree_of, n, head_counts, nt, d_tl_first, tl_of_pos);
    hipLaunchKernelGGL(phd::f_emit_roots_kernel, gt, b, 0, stream, d_tl_first, nt, items, lvl, n_items, d_info);
    {   // K5: emit_lbvh, level by level, over the treelets of all trees
        auto grid_of = [&](int L) { const uint64_t most = std::min<uint64_t>((uint64_t)n, (uint64_t)nt << std::min(L, 24)); return dim3((uint32_t)((most + 255u) / 256u)); };
        for (int L = 0; L < PHD_MAX_LEVELS; L++) {
            hipLaunchKernelGGL(phd::emit_level_kernel, grid_of(L), dim3(256), 0, stream, items, lvl, L, n_items, codes, max_prims, pool, leaf_last, d_info);
            hipLaunchKernelGGL(phd::emit_close_level_kernel, dim3(1), dim3(64), 0, stream, lvl, L, n_items);
        }
        for (int L = PHD_MAX_LEVELS - 1; L >= 0; L--) hipLaunchKernelGGL(phd::emit_up_kernel, grid_of(L), dim3(256), 0, stream, items, lvl, L, ids, blo, bhi, pool);
        for (int L = 0; L < PHD_MAX_LEVELS; L++) hipLaunchKernelGGL(phd::emit_down_kernel, grid_of(L), dim3(256), 0, stream, items, lvl, L, pool, d_info);
    }
    hipLaunchKernelGGL(phd::f_roots_kernel, gt, b, 0, stream, pool, d_tl_first, nt, d_rb);
    PH_BUILD_CHECK(hipGetLastError());
    info.resize(nt); rb.resize(6 * (size_t)nt);
    PH_BUILD_CHECK(hipMemcpyAsync(info.data(), d_info, (size_t)nt * sizeof(phd::TreeletInfo), hipMemcpyDeviceToHost, stream));
    PH_BUILD_CHECK(hipMemcpyAsync(rb.data(), d_rb, (size_t)nt * 24, hipMemcpyDeviceToHost, stream));
    PH_BUILD_CHECK(hipStreamSynchronize(stream));
    lap("treelets");
    tl.resize(nt);
    for (uint32_t t = 0; t < nt; t++) {
        StitchTreelet& q = tl[t];
        q.first = info[t].first; q.n = info[t].n; q.interior = info[t].interior; q.leaves = info[t].leaves; q.max_leaf = info[t].max_leaf; q.depth = info[t].depth;
        for (int k = 0; k < 3; k++) { q.lo[k] = rb[6 * (size_t)t + k]; q.hi[k] = rb[6 * (size_t)t + 3 + k]; }
    }
    const int prc = plan_hlbvh_forest(tl.data(), nt, tree_start, n_trees, plan);
    if (prc == -2) { err = "the reference's HLBVH build asserts on this input (hlbvh.rs:338/356/418)"; return -2; }
    if (prc != 0) { err = "device build: the treelets do not tile the trees"; return -1; }
    lap("SAH over the treelet roots");
    out.interior_nodes = plan.interior_nodes;
    Node64* d_nodes = arena.alloc<Node64>(std::max<size_t>(out.interior_nodes, 1));
    if (!d_nodes) { err = "device build: " + arena.why(); return -1; }
    PH_BUILD_CHECK(hipMemcpyAsync(d_tl_dense, plan.dense_base.data(), (size_t)nt * 4, hipMemcpyHostToDevice, stream));
    PH_BUILD_CHECK(hipMemcpyAsync(d_tl_out, plan.out_base.data(), (size_t)nt * 4, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(phd::f_convert_kernel, dim3((uint32_t)(((uint64_t)2 * n + 255u) / 256u)), b, 0, stream, pool, n, tl_of_pos, d_tl_first, d_tl_dense, d_tl_out, d_nodes);
    hipLaunchKernelGGL(phd::f_gather_kernel, g, b, 0, stream, ids, leaf_last, tl_of_pos, d_tl_first, d_tl_out, n, d.items, d.P, d.idx, d.tri_flags, d.tri_mesh, d.prim_quadric, d_tris);
    PH_BUILD_CHECK(hipGetLastError());
    out.nodes.resize(out.interior_nodes);
    out.tris.resize(n);
    if (out.interior_nodes) PH_BUILD_CHECK(hipMemcpyAsync(out.nodes.data(), d_nodes, out.interior_nodes * sizeof(Node64), hipMemcpyDeviceToHost, stream));
    PH_BUILD_CHECK(hipMemcpyAsync(out.tris.data(), d_tris, (size_t)n * sizeof(TriRec), hipMemcpyDeviceToHost, stream));
    PH_BUILD_CHECK(hipStreamSynchronize(stream));
    lap("nodes, records, downloads");
    place_upper_nodes(plan, out.nodes.data());
    if (forest || in.prim_quadric) {   // a single tree of triangles keeps the kernels' numbering.  A forest takes the host builder's, tree by tree (trees are independent: spread them over a few threads where there is much to do),
                          // and so does the single tree of a scene with quadrics: such a scene's arrays are the host builder's entry by entry, with or without instances
        const uint32_t n_thr = out.interior_nodes >= (1u << 18) ? std::min<uint32_t>(std::min<uint32_t>(16u, std::max(1u, std::thread::hardware_concurrency())), n_trees) : 1u;
        std::vector<uint32_t> cut(n_thr + 1, n_trees);   // cut the trees into runs of about equal node counts
        cut[0] = 0;
        for (uint32_t k = 1, t = 0; k < n_thr; k++) { const uint64_t want = (uint64_t)out.interior_nodes * k / n_thr; while (t < n_trees && plan.node_base[t] < want) t++; cut[k] = t; }
        ThreadGroup th;
        for (uint32_t k = 1; k < n_thr; k++) if (cut[k + 1] > cut[k]) th.run([&plan, &out, a = cut[k], e = cut[k + 1]]() { renumber_like_host(plan, out.nodes.data(), a, e); });
        renumber_like_host(plan, out.nodes.data(), cut[0], cut[1]);
        th.join();
    }
    lap("numbering");
    out.root_ref = plan.trees[0].root_ref;
    for (int k = 0; k < 3; k++) { out.root_lo[k] = plan.trees[0].lo[k]; out.root_hi[k] = plan.trees[0].hi[k]; }
    if (trees_out) *trees_out = plan.trees;
    out.leaf_nodes = plan.leaf_nodes; out.max_leaf_prims = plan.max_leaf_prims; out.max_depth = plan.max_depth;   // over all trees of the forest
    out.total_nodes = out.interior_nodes + out.leaf_nodes;
    out.build_seconds = lap.seconds();
    return 0;
}

}  // namespace phost

// Test / measurement hook with the signature of pbrt_hip_host_build_bvh (host_setup.cpp): the same tree, built on device `device`.
extern "C" int pbrt_hip_device_build_bvh(int device, const float* P, const uint32_t* idx, uint64_t n_tris, int split_method, int max_prims_in_node, uint32_t* out_ordered_prims,
                                         uint32_t* out_leaf_last, void* out_nodes, uint64_t* out_info, float* out_root_bounds, double* out_seconds) {
    return phost::ph_guard(nullptr, "pbrt_hip_device_build_bvh", [&]() -> int {
    if (split_method != 0 && split_method != 1) return -1;
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return -1; }
    phost::BuildInput in{P, idx, (size_t)n_tris, nullptr, nullptr};
    phost::BuildOutput out;
    std::string err;
    const int rc = split_method == 1 ? phost::build_hlbvh_device(in, max_prims_in_node, nullptr, out, err) : phost::build_sah_device(in, max_prims_in_node, nullptr, out, err);
    if (rc && !err.empty()) std::fprintf(stderr, "pbrt_hip_device_build_bvh: %s\n", err.c_str());
    if (rc) return rc;
    for (size_t i = 0; i < out.tris.size(); i++) {
        if (out_ordered_prims) out_ordered_prims[i] = out.tris[i].prim;
        if (out_leaf_last) out_leaf_last[i] = (out.tris[i].flags & PH_TRI_LAST) ? 1u : 0u;
    }
    if (out_nodes && !out.nodes.empty()) std::memcpy(out_nodes, out.nodes.data(), out.nodes.size() * sizeof(Node64));
    if (out_info) { out_info[0] = out.interior_nodes; out_info[1] = out.leaf_nodes; out_info[2] = out.max_leaf_prims; out_info[3] = (uint64_t)out.max_depth; out_info[4] = out.root_ref; }
    if (out_root_bounds) { for (int k = 0; k < 3; k++) { out_root_bounds[k] = out.root_lo[k]; out_root_bounds[3 + k] = out.root_hi[k]; } }
    if (out_seconds) *out_seconds = out.build_seconds;
    return 0;
    });
}
