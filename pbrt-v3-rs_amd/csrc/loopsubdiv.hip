// LoopSubDiv::subdivide on the device (shapes/src/loopsubdiv.rs:402-643).  The control mesh comes from loopsubdiv_host.h; every stage of a level, the push to the limit surface,
// the normals and TriangleMesh::new's move to world space are gathers with one thread per vertex, face or face-edge.  The f32 expression order is the reference's: each sum
// runs along the vertex's ring in the order SDVertex::one_ring walks it, and nothing is fused (-ffp-contract=off).  cos / sin come from the host's table: no device libm runs.
//
// Children are implicit: vertex i's child is i, face i's children are 4 i + 0..3 — the numbers the reference's allocation loops hand out (:409-424).  A new edge vertex is
// V + the rank of its owning face-edge among the owners in (face, edge) order, the order in which the reference's HashMap meets an edge first (:454-483).
#include "loopsubdiv_device.h"
#include "device_build_stage.h"

namespace pls {

constexpr uint32_t CHUNK = 2048u;   // face-edges one block scans: 256 threads x 8

struct Mesh {   // one level, read side or write side
    float* P; int32_t* start_face; uint32_t* vflags;   // per vertex
    int32_t* fv; int32_t* ff;                          // 3 per face
    uint32_t n_verts, n_faces;
};
struct F3 { float x, y, z; };
__device__ inline F3 ldp(const float* P, int32_t i) { return F3{P[3 * i], P[3 * i + 1], P[3 * i + 2]}; }
__device__ inline void stp(float* P, uint32_t i, F3 p) { P[3 * i] = p.x; P[3 * i + 1] = p.y; P[3 * i + 2] = p.z; }
__device__ inline F3 add(F3 a, F3 b) { return F3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ inline F3 sub(F3 a, F3 b) { return F3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline F3 mul(F3 a, float s) { return F3{a.x * s, a.y * s, a.z * s}; }
__device__ inline F3 mul(float s, F3 a) { return F3{s * a.x, s * a.y, s * a.z}; }
__device__ inline int next3(int i) { return i == 2 ? 0 : i + 1; }
__device__ inline int prev3(int i) { return i == 0 ? 2 : i - 1; }
__device__ inline int vnum(const int32_t* v, int32_t vert) { return v[0] == vert ? 0 : v[1] == vert ? 1 : 2; }   // (the host's checks leave no walk that misses its vertex)

// SDVertex::valence (:52-87)
__device__ inline uint32_t valence_of(const Mesh& m, int32_t vi, bool boundary) {
    const int32_t start = m.start_face[vi];
    int32_t f = start;
    uint32_t nf = 1u;
    if (!boundary) {
        while (f != -1) {
            f = m.ff[3 * f + vnum(m.fv + 3 * f, vi)];
            if (f == start) break;
            nf++;
        }
        return nf;
    }
    while (f != -1) {
        f = m.ff[3 * f + vnum(m.fv + 3 * f, vi)];
        if (f != -1) nf++; else break;
    }
    f = start;
    while (f != -1) {
        f = m.ff[3 * f + prev3(vnum(m.fv + 3 * f, vi))];
        if (f != -1) nf++; else break;
    }
    return nf + 1u;
}

// SDVertex::one_ring (:94-129): visit(k, position of the k-th ring vertex) in ring order, positions read from P
template <class Visit> __device__ inline void one_ring(const Mesh& m, const float* P, int32_t vi, bool boundary, Visit visit) {
    const int32_t start = m.start_face[vi];
    uint32_t k = 0u;
    if (!boundary) {
        int32_t f = start;
        do {
            const int j = vnum(m.fv + 3 * f, vi);
            visit(k++, ldp(P, m.fv[3 * f + next3(j)]));
            f = m.ff[3 * f + j];
        } while (f != start && f != -1);   // (-1 cannot come up at an interior vertex; it only guards the loop)
    } else {
        int32_t f = start;
        for (;;) {
            const int32_t f2 = m.ff[3 * f + vnum(m.fv + 3 * f, vi)];
            if (f2 == -1) break;
            f = f2;
        }
        visit(k++, ldp(P, m.fv[3 * f + next3(vnum(m.fv + 3 * f, vi))]));
        do {
            const int j = vnum(m.fv + 3 * f, vi);
            visit(k++, ldp(P, m.fv[3 * f + prev3(j)]));
            f = m.ff[3 * f + prev3(j)];
        } while (f != -1);
    }
}

__device__ inline float beta_of(uint32_t valence) { return valence == 3u ? 3.0f / 16.0f : 3.0f / (8.0f * (float)valence); }          // beta (:695-701)
__device__ inline float loop_gamma(uint32_t valence) { return 1.0f / ((float)valence + 3.0f / (8.0f * beta_of(valence))); }          // loop_gamma (:706-708)

__device__ inline F3 weight_one_ring(const Mesh& m, int32_t vi, float beta) {   // (:717-731)
    const uint32_t valence = valence_of(m, vi, false);
    F3 p = mul(ldp(m.P, vi), 1.0f - (float)valence * beta);
    one_ring(m, m.P, vi, false, [&](uint32_t, F3 q) { p = add(p, mul(q, beta)); });
    return p;
}
__device__ inline F3 weight_boundary(const Mesh& m, int32_t vi, float beta) {   // (:740-754)
    F3 first{0, 0, 0}, last{0, 0, 0};
    one_ring(m, m.P, vi, true, [&](uint32_t k, F3 q) { if (k == 0u) first = q; last = q; });
    F3 p = mul(ldp(m.P, vi), 1.0f - 2.0f * beta);
    p = add(p, mul(first, beta));
    p = add(p, mul(last, beta));
    return p;
}

// even vertices: the position rules (:429-450), the flags the allocation loop copies (:413-416), and the child's start_face (:488-497)
__global__ __launch_bounds__(256) void k_even(Mesh in, Mesh out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= in.n_verts) return;
    const uint32_t fl = in.vflags[i];
    F3 p;
    if (!(fl & ploop::V_BOUNDARY)) p = weight_one_ring(in, (int32_t)i, (fl & ploop::V_REGULAR) ? 1.0f / 16.0f : beta_of(valence_of(in, (int32_t)i, false)));
    else p = weight_boundary(in, (int32_t)i, 1.0f / 8.0f);
    stp(out.P, i, p);
    out.vflags[i] = fl;
    const int32_t sf = in.start_face[i];
    out.start_face[i] = 4 * sf + vnum(in.fv + 3 * sf, (int32_t)i);
}

// face-edge (i, k) owns its edge when it has no neighbour there or its face comes first
__device__ inline uint32_t owner_flag(const Mesh& m, uint32_t e) { const int32_t f2 = m.ff[e]; return (f2 == -1 || (int32_t)(e / 3u) < f2) ? 1u : 0u; }

// prefix sum of the owner flags, in the pattern of the SAH builder's k_flags / exclusive_scan_kernel / k_scan_write (bvh_sah_device.hip): flags and chunk sums, the chunk sums scanned
// by one block (device_build_stage.h), the flags replaced by their exclusive prefix
__global__ __launch_bounds__(256) void k_owner_flags(Mesh m, uint32_t* scan, uint32_t* chunk_sums) {
    __shared__ uint32_t part[4];
    const uint32_t n = 3u * m.n_faces, base = blockIdx.x * CHUNK, lim = base + CHUNK < n ? base + CHUNK : n;
    uint32_t sum = 0u;
    for (uint32_t e = base + threadIdx.x; e < lim; e += 256u) { const uint32_t f = owner_flag(m, e); scan[e] = f; sum += f; }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o);
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) chunk_sums[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}
__global__ __launch_bounds__(256) void k_scan_write(uint32_t* scan, uint32_t n, const uint32_t* chunk_base) {
    __shared__ uint32_t part[256];
    const uint32_t base = blockIdx.x * CHUNK;
    const uint32_t per = CHUNK / 256u, first = base + threadIdx.x * per;
    uint32_t f[CHUNK / 256u];
    uint32_t sum = 0u;
    for (uint32_t j = 0; j < per; j++) { f[j] = first + j < n ? scan[first + j] : 0u; sum += f[j]; }
    part[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t o = 1; o < 256u; o <<= 1) {
        const uint32_t add = threadIdx.x >= o ? part[threadIdx.x - o] : 0u;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    uint32_t run = chunk_base[blockIdx.x] + part[threadIdx.x] - sum;
    for (uint32_t j = 0; j < per; j++) if (first + j < n) { scan[first + j] = run; run += f[j]; }
}

// SDFace::other_vert (:289-296)
__device__ inline int32_t other_vert(const int32_t* v, int32_t v0, int32_t v1) { return (v[0] != v0 && v[0] != v1) ? v[0] : (v[1] != v0 && v[1] != v1) ? v[1] : v[2]; }

// odd vertices (:453-483): the owner of an edge writes its vertex
__global__ __launch_bounds__(256) void k_edge_verts(Mesh in, Mesh out, const uint32_t* scan) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= 3u * in.n_faces || !owner_flag(in, e)) return;
    const uint32_t i = e / 3u; const int k = (int)(e - 3u * i);
    const uint32_t nv = in.n_verts + scan[e];
    const int32_t a = in.fv[3 * i + k], b = in.fv[3 * i + next3(k)];
    const int32_t v0 = a < b ? a : b, v1 = a < b ? b : a;   // SDEdge::new orders its endpoints (:173-179)
    const int32_t f2 = in.ff[e];
    F3 p;
    if (f2 == -1) p = add(mul(0.5f, ldp(in.P, v0)), mul(0.5f, ldp(in.P, v1)));
    else {
        const F3 ov = ldp(in.P, other_vert(in.fv + 3 * i, v0, v1)), fk_ov = ldp(in.P, other_vert(in.fv + 3 * f2, v0, v1));
        p = add(add(add(mul(3.0f / 8.0f, ldp(in.P, v0)), mul(3.0f / 8.0f, ldp(in.P, v1))), mul(1.0f / 8.0f, ov)), mul(1.0f / 8.0f, fk_ov));
    }
    stp(out.P, nv, p);
    out.vflags[nv] = ploop::V_REGULAR | (f2 == -1 ? ploop::V_BOUNDARY : 0u);
    out.start_face[nv] = 4 * (int32_t)i + 3;
}

// the new vertex on edge k of face i: the owner's number; the other side finds it through its neighbour's matching edge (which runs the other way, so it starts at our end)
__device__ inline int32_t edge_vertex(const Mesh& m, const uint32_t* scan, uint32_t i, int k) {
    uint32_t e = 3u * i + (uint32_t)k;
    if (!owner_flag(m, e)) {
        const int32_t f2 = m.ff[e];
        e = 3u * (uint32_t)f2 + (uint32_t)vnum(m.fv + 3 * f2, m.fv[3 * i + next3(k)]);
    }
    return (int32_t)(m.n_verts + scan[e]);
}

// child faces: neighbour pointers (:500-534) and vertex pointers (:537-563), each child computing its own six fields
__global__ __launch_bounds__(256) void k_child_faces(Mesh in, Mesh out, const uint32_t* scan) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= 4u * in.n_faces) return;
    const uint32_t i = t >> 2; const int c = (int)(t & 3u);
    const int32_t* v = in.fv + 3 * i; const int32_t* f = in.ff + 3 * i;
    int32_t cv[3], cf[3];
    if (c == 3) {
        for (int j = 0; j < 3; j++) { cv[j] = edge_vertex(in, scan, i, j); cf[j] = 4 * (int32_t)i + next3(j); }
    } else {
        const int j = c, nj = next3(j), pj = prev3(j);
        cv[j] = v[j];
        cv[nj] = edge_vertex(in, scan, i, j);
        cv[pj] = edge_vertex(in, scan, i, pj);
        cf[nj] = 4 * (int32_t)i + 3;
        const int32_t fa = f[j], fb = f[pj];
        cf[j] = fa != -1 ? 4 * fa + vnum(in.fv + 3 * fa, v[j]) : -1;
        cf[pj] = fb != -1 ? 4 * fb + vnum(in.fv + 3 * fb, v[j]) : -1;
    }
    for (int j = 0; j < 3; j++) { out.fv[3 * t + j] = cv[j]; out.ff[3 * t + j] = cf[j]; }
}

// limit positions (:571-593), into a second buffer
__global__ __launch_bounds__(256) void k_limit(Mesh m, float* p_limit) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= m.n_verts) return;
    F3 p;
    if (m.vflags[i] & ploop::V_BOUNDARY) p = weight_boundary(m, (int32_t)i, 1.0f / 5.0f);
    else p = weight_one_ring(m, (int32_t)i, loop_gamma(valence_of(m, (int32_t)i, false)));
    stp(p_limit, i, p);
}

// normals from the ring of LIMIT positions (:596-634): ns = s x t, not normalised
__global__ __launch_bounds__(256) void k_normals(Mesh m, const float* p_limit, const float* trig, const int32_t* interior_off, const int32_t* boundary_off, uint32_t n_off, float* N) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= m.n_verts) return;
    const bool boundary = (m.vflags[i] & ploop::V_BOUNDARY) != 0u;
    const uint32_t valence = valence_of(m, (int32_t)i, boundary);
    F3 s{0.0f, 0.0f, 0.0f}, t{0.0f, 0.0f, 0.0f};
    // a valence the host's table lacks cannot come up (valence never grows; new vertices have 6 or 4): the test only keeps a read inside the table
    const int32_t off = valence < n_off ? (boundary ? (valence > 4u ? boundary_off[valence] : 0) : interior_off[valence]) : -1;
    if (off < 0) { stp(N, i, F3{0.0f, 0.0f, 0.0f}); return; }
    if (!boundary) {
        const float* cs = trig + off;
        one_ring(m, p_limit, (int32_t)i, false, [&](uint32_t j, F3 q) { s = add(s, mul(cs[2u * j], q)); t = add(t, mul(cs[2u * j + 1u], q)); });
    } else {
        // the ring's first four positions and its last: the walk of one_ring with its first steps written out, so that the five stay in registers (as an array indexed by
        // the ring position they went to LDS, as selects on it to scratch: profiles/loopsubdiv_kernel_resources.md)
        F3 r0{0, 0, 0}, r1 = r0, r2 = r0, r3 = r0, last = r0;
        {
            int32_t f = m.start_face[i];
            for (;;) {
                const int32_t f2 = m.ff[3 * f + vnum(m.fv + 3 * f, (int32_t)i)];
                if (f2 == -1) break;
                f = f2;
            }
            r0 = ldp(p_limit, m.fv[3 * f + next3(vnum(m.fv + 3 * f, (int32_t)i))]);
            auto step = [&](F3& dst) {   // the ring's next position, and on to the previous face
                const int j = vnum(m.fv + 3 * f, (int32_t)i);
                dst = ldp(p_limit, m.fv[3 * f + prev3(j)]);
                last = dst;
                f = m.ff[3 * f + prev3(j)];
            };
            step(r1);
            if (f != -1) step(r2);
            if (f != -1) step(r3);
            while (f != -1) { F3 q; step(q); }
        }
        const F3 vp = ldp(p_limit, (int32_t)i);
        s = sub(last, r0);
        if (valence == 2u) t = sub(add(r0, r1), mul(2.0f, vp));
        else if (valence == 3u) t = sub(r1, vp);
        else if (valence == 4u) t = sub(sub(add(add(mul(-1.0f, r0), mul(2.0f, r1)), mul(2.0f, r2)), mul(1.0f, r3)), mul(2.0f, vp));
        else {
            const float* tb = trig + off;
            const float sin_theta = tb[0], cos_theta = tb[1];
            t = mul(sin_theta, add(r0, last));
            one_ring(m, p_limit, (int32_t)i, true, [&](uint32_t k, F3 q) {
                if (k >= 1u && k + 1u < valence) { const float wt = (2.0f * cos_theta - 2.0f) * tb[1u + k]; t = add(t, mul(wt, q)); }
            });
            t = F3{-t.x, -t.y, -t.z};
        }
    }
    stp(N, i, F3{(s.y * t.z) - (s.z * t.y), (s.z * t.x) - (s.x * t.z), (s.x * t.y) - (s.y * t.x)});
}

struct M16 { float m[16]; };
// TriangleMesh::new (triangle.rs:93-96): transform_point by the matrix, transform_normal by the inverse's transpose, in the expression order of
// pbrt_hip_host_transform_points / _normals (host_setup.cpp), the host path of a trianglemesh
__global__ __launch_bounds__(256) void k_world(uint32_t n, M16 a, M16 ai, float* P, float* N) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    {
        const float x = P[3 * i], y = P[3 * i + 1], z = P[3 * i + 2];
        const float xp = a.m[0] * x + a.m[1] * y + a.m[2] * z + a.m[3];
        const float yp = a.m[4] * x + a.m[5] * y + a.m[6] * z + a.m[7];
        const float zp = a.m[8] * x + a.m[9] * y + a.m[10] * z + a.m[11];
        const float wp = a.m[12] * x + a.m[13] * y + a.m[14] * z + a.m[15];
        if (wp == 1.0f) { P[3 * i] = xp; P[3 * i + 1] = yp; P[3 * i + 2] = zp; }
        else { const float inv = 1.0f / wp; P[3 * i] = inv * xp; P[3 * i + 1] = inv * yp; P[3 * i + 2] = inv * zp; }
    }
    {
        const float x = N[3 * i], y = N[3 * i + 1], z = N[3 * i + 2];
        N[3 * i] = ai.m[0] * x + ai.m[4] * y + ai.m[8] * z;
        N[3 * i + 1] = ai.m[1] * x + ai.m[5] * y + ai.m[9] * z;
        N[3 * i + 2] = ai.m[2] * x + ai.m[6] * y + ai.m[10] * z;
    }
}

}  // namespace pls

namespace phost {

int loopsubdiv_device(const ploop::Control& c, const float* P, int n_levels, const float* o2w_m, const float* o2w_minv, hipStream_t stream, float* out_P, float* out_N,
                      uint32_t* out_idx, std::string& err) {
    using namespace pls;
    const size_t nv = (size_t)c.out_verts, nf = (size_t)c.out_faces;
    const size_t max_edges3 = 3 * (n_levels > 0 ? nf / 4 : nf);   // the face-edges of the last level's input
    const uint32_t max_chunks = (uint32_t)((max_edges3 + CHUNK - 1) / CHUNK);
    DeviceArena arena(stream);
    Mesh lv[2];
    for (int k = 0; k < 2; k++) {
        lv[k].P = arena.alloc<float>(nv * 3); lv[k].start_face = arena.alloc<int32_t>(nv); lv[k].vflags = arena.alloc<uint32_t>(nv);
        lv[k].fv = arena.alloc<int32_t>(nf * 3); lv[k].ff = arena.alloc<int32_t>(nf * 3);
        lv[k].n_verts = 0; lv[k].n_faces = 0;
    }
    uint32_t* scan = arena.alloc<uint32_t>(max_edges3);
    uint32_t* chunk_sums = arena.alloc<uint32_t>((size_t)max_chunks);
    float* d_N = arena.alloc<float>(nv * 3);
    float* d_trig = arena.upload(c.trig.data(), c.trig.size());
    int32_t* d_ioff = arena.upload(c.interior_off.data(), c.interior_off.size());
    int32_t* d_boff = arena.upload(c.boundary_off.data(), c.boundary_off.size());
    const bool prof = build_profile_on();   // the kernels' time, uploads and downloads excluded, to stderr
    DeviceEvent ev0, ev1;
    if (!arena.ok()) { err = arena.why(); return -1; }
    const dim3 b(256);
    int cur = 0;
    uint64_t V = c.n_verts, E = c.n_edges, F = c.n_faces;
    if (prof) { PH_BUILD_CHECK(hipEventCreate(&ev0.e)); PH_BUILD_CHECK(hipEventCreate(&ev1.e)); }
    PH_BUILD_CHECK(hipMemcpyAsync(lv[0].P, P, V * 12, hipMemcpyHostToDevice, stream));
    PH_BUILD_CHECK(hipMemcpyAsync(lv[0].start_face, c.start_face.data(), V * 4, hipMemcpyHostToDevice, stream));
    PH_BUILD_CHECK(hipMemcpyAsync(lv[0].vflags, c.vflags.data(), V * 4, hipMemcpyHostToDevice, stream));
    PH_BUILD_CHECK(hipMemcpyAsync(lv[0].fv, c.fv.data(), F * 12, hipMemcpyHostToDevice, stream));
    PH_BUILD_CHECK(hipMemcpyAsync(lv[0].ff, c.ff.data(), F * 12, hipMemcpyHostToDevice, stream));
    if (prof) PH_BUILD_CHECK(hipEventRecord(ev0.e, stream));
    for (int l = 0; l < n_levels; l++) {
        Mesh& in = lv[cur]; Mesh& out = lv[cur ^ 1];
        in.n_verts = (uint32_t)V; in.n_faces = (uint32_t)F;
        const uint32_t n_fe = 3u * (uint32_t)F, n_chunks = (n_fe + CHUNK - 1u) / CHUNK;
        hipLaunchKernelGGL(k_even, dim3(((uint32_t)V + 255u) / 256u), b, 0, stream, in, out);
        hipLaunchKernelGGL(k_owner_flags, dim3(n_chunks), b, 0, stream, in, scan, chunk_sums);
        hipLaunchKernelGGL(exclusive_scan_kernel, dim3(1), dim3(1024), 0, stream, chunk_sums, n_chunks);
        hipLaunchKernelGGL(k_scan_write, dim3(n_chunks), b, 0, stream, scan, n_fe, chunk_sums);
        hipLaunchKernelGGL(k_edge_verts, dim3((n_fe + 255u) / 256u), b, 0, stream, in, out, scan);
        hipLaunchKernelGGL(k_child_faces, dim3((4u * (uint32_t)F + 255u) / 256u), b, 0, stream, in, out, scan);
        PH_BUILD_CHECK(hipGetLastError());
        const uint64_t nV = V + E, nE = 2 * E + 3 * F, nF = 4 * F;
        V = nV; E = nE; F = nF;
        cur ^= 1;
    }
    if (V != c.out_verts || F != c.out_faces) { err = "level counts disagree with the control mesh's"; return -1; }
    Mesh& m = lv[cur];
    m.n_verts = (uint32_t)V; m.n_faces = (uint32_t)F;
    float* p_limit = lv[cur ^ 1].P;   // the other level's positions are done with
    const dim3 per_vert(((uint32_t)V + 255u) / 256u);
    hipLaunchKernelGGL(k_limit, per_vert, b, 0, stream, m, p_limit);
    hipLaunchKernelGGL(k_normals, per_vert, b, 0, stream, m, (const float*)p_limit, (const float*)d_trig, (const int32_t*)d_ioff, (const int32_t*)d_boff, (uint32_t)c.interior_off.size(), d_N);
    if (o2w_m) {
        M16 a, ai;
        for (int k = 0; k < 16; k++) { a.m[k] = o2w_m[k]; ai.m[k] = o2w_minv[k]; }
        hipLaunchKernelGGL(k_world, per_vert, b, 0, stream, (uint32_t)V, a, ai, p_limit, d_N);
    }
    PH_BUILD_CHECK(hipGetLastError());
    if (prof) PH_BUILD_CHECK(hipEventRecord(ev1.e, stream));
    PH_BUILD_CHECK(hipMemcpyAsync(out_P, p_limit, V * 12, hipMemcpyDeviceToHost, stream));
    PH_BUILD_CHECK(hipMemcpyAsync(out_N, d_N, V * 12, hipMemcpyDeviceToHost, stream));
    PH_BUILD_CHECK(hipMemcpyAsync(out_idx, m.fv, F * 12, hipMemcpyDeviceToHost, stream));   // face.v[0..3] in face order (:639-643); no index is negative
    PH_BUILD_CHECK(hipStreamSynchronize(stream));
    if (prof) {
        float ms = 0.0f;
        PH_BUILD_CHECK(hipEventElapsedTime(&ms, ev0.e, ev1.e));
        std::fprintf(stderr, "loopsubdiv_device faces=%u levels=%d triangles=%llu: kernels %.3f ms\n", c.n_faces, n_levels, (unsigned long long)c.out_faces, ms);
    }
    return 0;   // (the arena waits for the stream before its buffers go, on every way out)
}

}  // namespace phost
