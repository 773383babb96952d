// Test hooks (include/pbrt_hip.h: pbrt_hip_bsdf_probe_batch, pbrt_hip_sampler_value_batch): the device's BSDF and sampler code on explicit inputs.
// Each kernel only unpacks its arguments and calls the PH_DEV functions the render kernels call (pt_device.h, bsdf_general.h, wf_device.h); no formula lives here.
#define PH_OUTLINE_MATH 1
#include "scene_host.h"
#include "pt_device.h"
#include "bsdf_general.h"
#include "wf_device.h"
#include <cstring>

namespace ph {

struct ProbeFrame { float ns[3], ng[3], ss[3]; };
#define PH_PROBE_BLOCK 128

// GEN = true: GBsdf as shade_kernel<true> makes it (make_gbsdf); GEN = false: the one-lobe Bsdf of shade_kernel<false> (make_bsdf), which has no flags and no sampled type:
// the host admits only flags the lobe matches, and a sample that succeeded reports the lobe's type as BsdfOps<false>::sample_all does
template <bool GEN>
__global__ __launch_bounds__(PH_PROBE_BLOCK) void bsdf_probe_kernel(DeviceScene sc, uint32_t material, int op, uint32_t n, const float* wo_in, const float* wi_in, const float* u_in,
                                                                   const uint32_t* flags_in, ProbeFrame fr, float* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    SurfHit si;
    si.p = mk3(0.0f, 0.0f, 0.0f); si.p_error = si.p; si.wo = si.p; si.time = 0.0f; si.prim = 0u;
    si.ns = ld3(fr.ns); si.n = ld3(fr.ng); si.dpdu_s = ld3(fr.ss);
    const f3 wo = ld3(wo_in + 3 * (size_t)i), wi = ld3(wi_in + 3 * (size_t)i);
    const f2 u = mk2(u_in[2 * (size_t)i], u_in[2 * (size_t)i + 1]);
    const uint32_t flags = flags_in[i];
    float* o = out + 8 * (size_t)i;
    for (int k = 0; k < 8; k++) o[k] = 0.0f;
    if (GEN) {
        const GBsdf b = make_gbsdf(sc, si, material);
        if (op == 0) {
            const spec f = bsdf_f(b, wo, wi, flags);
            o[0] = f.r; o[1] = f.g; o[2] = f.b; o[3] = bsdf_pdf(b, wo, wi, flags);
        } else if (op == 1) {
            spec f; float pdf; f3 w; uint32_t st;
            bsdf_sample_f(b, wo, u, flags, f, pdf, w, st);
            o[0] = f.r; o[1] = f.g; o[2] = f.b; o[3] = pdf; o[4] = w.x; o[5] = w.y; o[6] = w.z; o[7] = (float)st;
        } else {
            o[0] = (float)bsdf_num_components(b, flags); o[1] = (float)b.n; o[2] = b.eta;
        }
    } else {
        const Bsdf b = make_bsdf(sc, si, material);
        if (op == 0) {
            const spec f = bsdf_f(b, wo, wi);
            o[0] = f.r; o[1] = f.g; o[2] = f.b; o[3] = bsdf_pdf(b, wo, wi);
        } else if (op == 1) {
            spec f; float pdf; f3 w;
            bsdf_sample_f(b, wo, u, f, pdf, w);
            o[0] = f.r; o[1] = f.g; o[2] = f.b; o[3] = pdf; o[4] = w.x; o[5] = w.y; o[6] = w.z; o[7] = pdf == 0.0f ? 0.0f : (float)(BX_REFL | BX_DIFF);
        } else {
            o[0] = b.has_bxdf ? 1.0f : 0.0f; o[1] = o[0]; o[2] = 1.0f;
        }
    }
}

// cursor_for + sampler_dim as the render kernels pair them; use_lds: the block stages the first PH_LDS_DIMS Halton dimensions like shade_kernel does
__global__ __launch_bounds__(256) void sampler_value_kernel(DeviceScene sc, SamplerRec sp, uint32_t n, const int* xy, const uint32_t* sample, const uint32_t* dim, int use_lds, float* out) {
    __shared__ HaltonLds halton_lds;
    const HaltonLds* hl = nullptr;
    if (use_lds && sp.kind == 0) { halton_lds_fill(&halton_lds, sc); hl = &halton_lds; }
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const SamplerCursor c = cursor_for(sc, sp, xy[2 * (size_t)i], xy[2 * (size_t)i + 1], sample[i], dim[i], hl);
    out[i] = sampler_dim(sc, sp, c, c.dim);
}

}  // namespace ph

using namespace phost;

namespace {
// one scratch allocation per call, split into 256-byte aligned parts; freed by the caller's guard
struct Scratch {
    void* p = nullptr;
    ~Scratch() { if (p) (void)hipFree(p); }
};
size_t up256(size_t v) { return (v + 255u) & ~(size_t)255u; }
bool material_reads_a_texture(const MaterialRec& m) {
    return m.textured || m.kd_tex1 || m.bump_tex1 || m.sigma_tex1 || m.opacity_tex1 || m.amount_tex1 || m.rt_mode || m.refl_tex1 || m.trans_tex1 || m.index_tex1;
}
}  // namespace

extern "C" {

int pbrt_hip_bsdf_probe_batch(PbrtHipScene* s, uint32_t material, int op, int path, uint64_t n, const float* wo, const float* wi, const float* u, const uint32_t* flags, const float* frame,
                              float* out) {
    return ph_guard(s, "pbrt_hip_bsdf_probe_batch", [&]() -> int {
    if (!s || (n && (!wo || !wi || !u || !flags || !out))) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "bsdf_probe_batch: null argument");
    if (material >= s->materials.size()) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "bsdf_probe_batch: unknown material");
    if (op < 0 || op > 2 || path < 0 || path > 1) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "bsdf_probe_batch: op must be 0, 1 or 2 and path 0 or 1");
    if (n > 0xFFFFFFFFull) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "bsdf_probe_batch: too many probes");
    const MaterialRec& m = s->materials[material];
    if (material_reads_a_texture(m)) return set_err(s, PBRT_HIP_ERR_UNSUPPORTED, "bsdf_probe_batch: the material takes a parameter from a texture (its BSDF differs from hit to hit)");
    if (path == 1) {
        if (s->material_params[material].made_as != 6) return set_err(s, PBRT_HIP_ERR_UNSUPPORTED, "bsdf_probe_batch: path 1 is the one-lobe BSDF of MatteMaterial; this material is not matte");
        for (uint64_t i = 0; i < n; i++)
            if ((flags[i] & 5u) != 5u) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "bsdf_probe_batch: path 1 has no flags; every flags[i] must hold REFLECTION | DIFFUSE");
    }
    if (n == 0) return PBRT_HIP_OK;
    ph::ProbeFrame fr = {{0.0f, 0.0f, 1.0f}, {0.0f, 0.0f, 1.0f}, {1.0f, 0.0f, 0.0f}};
    if (frame) { std::memcpy(fr.ns, frame, 12); std::memcpy(fr.ng, frame + 3, 12); std::memcpy(fr.ss, frame + 6, 12); }
    PH_CHECK(s, hipSetDevice(s->device));
    int rc;
    if ((rc = upload_scene(s))) return rc;   // materials and lobes; an empty accelerator is fine
    const size_t o_wo = 0, o_wi = o_wo + up256(n * 12), o_u = o_wi + up256(n * 12), o_fl = o_u + up256(n * 8), o_out = o_fl + up256(n * 4), total = o_out + up256(n * 32);
    Scratch sx;
    PH_CHECK(s, hipMalloc(&sx.p, total));
    char* d = static_cast<char*>(sx.p);
    PH_CHECK(s, hipMemcpyAsync(d + o_wo, wo, n * 12, hipMemcpyHostToDevice, s->stream));
    PH_CHECK(s, hipMemcpyAsync(d + o_wi, wi, n * 12, hipMemcpyHostToDevice, s->stream));
    PH_CHECK(s, hipMemcpyAsync(d + o_u, u, n * 8, hipMemcpyHostToDevice, s->stream));
    PH_CHECK(s, hipMemcpyAsync(d + o_fl, flags, n * 4, hipMemcpyHostToDevice, s->stream));
    const dim3 grid((uint32_t)((n + PH_PROBE_BLOCK - 1) / PH_PROBE_BLOCK)), block(PH_PROBE_BLOCK);
    if (path == 0)
        hipLaunchKernelGGL(ph::bsdf_probe_kernel<true>, grid, block, 0, s->stream, s->ds, material, op, (uint32_t)n, (const float*)(d + o_wo), (const float*)(d + o_wi), (const float*)(d + o_u),
                           (const uint32_t*)(d + o_fl), fr, (float*)(d + o_out));
    else
        hipLaunchKernelGGL(ph::bsdf_probe_kernel<false>, grid, block, 0, s->stream, s->ds, material, op, (uint32_t)n, (const float*)(d + o_wo), (const float*)(d + o_wi), (const float*)(d + o_u),
                           (const uint32_t*)(d + o_fl), fr, (float*)(d + o_out));
    PH_CHECK(s, hipGetLastError());
    PH_CHECK(s, hipMemcpyAsync(out, d + o_out, n * 32, hipMemcpyDeviceToHost, s->stream));
    PH_CHECK(s, hipStreamSynchronize(s->stream));
    return PBRT_HIP_OK;
    });
}

int pbrt_hip_sampler_value_batch(PbrtHipScene* s, uint64_t n, const int* xy, const uint32_t* sample, const uint32_t* dim, int use_lds, float* out) {
    return ph_guard(s, "pbrt_hip_sampler_value_batch", [&]() -> int {
    if (!s || (n && (!xy || !sample || !dim || !out))) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "sampler_value_batch: null argument");
    if (!s->have_sampler) return set_err(s, PBRT_HIP_ERR_STATE, "sampler_value_batch: set_sampler first");
    if (n > 0xFFFFFFFFull) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "sampler_value_batch: too many values");
    const SamplerRec& sp = s->sampler;
    if (sp.kind == 0) {
        for (uint64_t i = 0; i < n; i++)
            if (dim[i] >= 1000u) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "sampler_value_batch: the Halton tables hold 1000 dimensions (PRIME_TABLE_SIZE)");
    } else {
        if (s->sobol32.empty()) return set_err(s, PBRT_HIP_ERR_STATE, "sampler_value_batch: sobol tables not set");
        const int m = sp.log2_resolution;
        const uint64_t n_dims = s->sobol32.size() / 52;
        if (m > (int)(s->vdc.size() / 52) || m > 26) return set_err(s, PBRT_HIP_ERR_UNSUPPORTED, "sampler_value_batch: sample-bounds resolution exceeds the Sobol tables given");
        for (uint64_t i = 0; i < n; i++) {
            if (dim[i] >= n_dims) return set_err(s, PBRT_HIP_ERR_UNSUPPORTED, "sampler_value_batch: dimension beyond the Sobol tables given");
            // the index of (pixel, sample) must stay below 2^52, the columns a generator matrix has: sample < 2^(52 - 2m), pixel inside the power-of-two square
            if (2 * m > 20 && ((uint64_t)sample[i] >> (52 - 2 * m)) != 0) return set_err(s, PBRT_HIP_ERR_UNSUPPORTED, "sampler_value_batch: sample number beyond the 52 columns of the Sobol matrices");
            const int64_t dx = (int64_t)xy[2 * i] - sp.bounds[0], dy = (int64_t)xy[2 * i + 1] - sp.bounds[1];
            if (dx < 0 || dy < 0 || dx >= sp.resolution || dy >= sp.resolution) return set_err(s, PBRT_HIP_ERR_INVALID_ARG, "sampler_value_batch: pixel outside the Sobol sampler's square");
        }
    }
    if (n == 0) return PBRT_HIP_OK;
    PH_CHECK(s, hipSetDevice(s->device));
    int rc;
    if ((rc = upload_scene(s))) return rc;   // the sampler tables; an empty accelerator is fine
    const size_t o_xy = 0, o_s = o_xy + up256(n * 8), o_d = o_s + up256(n * 4), o_out = o_d + up256(n * 4), total = o_out + up256(n * 4);
    Scratch sx;
    PH_CHECK(s, hipMalloc(&sx.p, total));
    char* d = static_cast<char*>(sx.p);
    PH_CHECK(s, hipMemcpyAsync(d + o_xy, xy, n * 8, hipMemcpyHostToDevice, s->stream));
    PH_CHECK(s, hipMemcpyAsync(d + o_s, sample, n * 4, hipMemcpyHostToDevice, s->stream));
    PH_CHECK(s, hipMemcpyAsync(d + o_d, dim, n * 4, hipMemcpyHostToDevice, s->stream));
    hipLaunchKernelGGL(ph::sampler_value_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s->stream, s->ds, s->sampler, (uint32_t)n, (const int*)(d + o_xy), (const uint32_t*)(d + o_s),
                       (const uint32_t*)(d + o_d), use_lds ? 1 : 0, (float*)(d + o_out));
    PH_CHECK(s, hipGetLastError());
    PH_CHECK(s, hipMemcpyAsync(out, d + o_out, n * 4, hipMemcpyDeviceToHost, s->stream));
    PH_CHECK(s, hipStreamSynchronize(s->stream));
    return PBRT_HIP_OK;
    });
}

}  // extern "C"
