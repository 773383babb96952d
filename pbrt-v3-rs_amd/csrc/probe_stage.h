// The device side of one probe call (probe.hip): its inputs, outputs and work buffers, each made by the one call that states its type and its element count.
//     ProbeStage st(s);
//     const float* d_in = st.in(in, n * 15);  float* d_out = st.out(out, n * 3);
//     if (!st.ok()) return st.finish();
//     hipLaunchKernelGGL(..., d_in, d_out);
//     return st.finish();
// The parts are a DeviceArena's over s->stream, one allocation each (hipMalloc aligns to 256 bytes and more): every return, early or not, waits for the stream before the buffers go.
// Host arrays handed to in() must outlive the stage (declare them first).
#pragma once
#include "device_arena.h"
#include "scene_host.h"

namespace phost {

class ProbeStage {
public:
    explicit ProbeStage(PbrtHipScene* s) : s_(s), arena_(s->stream) {}
    // `count` elements copied up from `src`, the copy queued at once; no copy from a null `src` or of nothing, the pointer is a valid allocation all the same
    template <class T> const T* in(const T* src, size_t count) { return src ? arena_.upload(src, count) : arena_.alloc<T>(count); }
    // `count` elements that finish() copies down to `dst`, or that stay on the device under a null `dst`; `fill` (a byte, none if negative) is queued at once
    template <class T> T* out(T* dst, size_t count, int fill = -1) {
        T* p = work<T>(count, fill);
        if (p && dst && count) outs_.push_back({dst, p, count * sizeof(T)});
        return p;
    }
    // finish() also copies down `count` elements of a device array that is not the stage's (the film probe's tiles)
    template <class T> void fetch(T* dst, const T* d_src, size_t count) { if (count) outs_.push_back({dst, d_src, count * sizeof(T)}); }
    template <class T> T* work(size_t count, int fill = -1) {
        T* p = arena_.alloc<T>(count);
        if (p && count && fill >= 0 && !rc_) rc_ = check(hipMemsetAsync(p, fill, count * sizeof(T), s_->stream), "hipMemsetAsync (probe stage)");
        return p;
    }
    bool ok() const { return arena_.ok() && !rc_; }   // false: a part is missing, launch nothing and return finish()
    // the launches' error state, the downloads and the wait for the stream; the status of the first failure since construction (hip_fail's codes and text)
    int finish() {
        if (!arena_.ok()) return set_err(s_, arena_.error() == hipErrorOutOfMemory ? PBRT_HIP_ERR_OOM : PBRT_HIP_ERR_DEVICE, arena_.why());
        if (rc_) return rc_;
        if ((rc_ = check(hipGetLastError(), "hipGetLastError (probe launch)"))) return rc_;
        for (const Out& o : outs_)
            if ((rc_ = check(hipMemcpyAsync(o.dst, o.src, o.bytes, hipMemcpyDeviceToHost, s_->stream), "hipMemcpyAsync (download)"))) return rc_;
        outs_.clear();
        return rc_ = check(hipStreamSynchronize(s_->stream), "hipStreamSynchronize");
    }
private:
    struct Out { void* dst; const void* src; size_t bytes; };
    int check(hipError_t e, const char* call) { return e == hipSuccess ? PBRT_HIP_OK : hip_fail(s_, e, call); }
    PbrtHipScene* s_; DeviceArena arena_; std::vector<Out> outs_; int rc_ = PBRT_HIP_OK;
};

}  // namespace phost
