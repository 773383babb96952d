// Device scratch that lives as long as one call: what the device-side builders (device_build_stage.h) and the probes' staging (probe_stage.h) allocate from.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <vector>

namespace phost {

// Device scratch of one build or probe.  alloc and upload never throw: a failure gives null and is kept in why() / error() (the first one), so a caller allocates everything it knows the
// size of and asks ok() once.  The destructor waits for the stream (nothing of the call is in flight when the buffers go) and frees whatever was not released to the caller.
class DeviceArena {
public:
    explicit DeviceArena(hipStream_t stream) : stream_(stream) {}
    DeviceArena(const DeviceArena&) = delete; DeviceArena& operator=(const DeviceArena&) = delete;
    ~DeviceArena() { if (!owned_.empty()) (void)hipStreamSynchronize(stream_); for (void* p : owned_) if (p) (void)hipFree(p); }
    template <class T> T* alloc(size_t count) { void* p = nullptr; if (failed(hipMalloc(&p, count ? count * sizeof(T) : 16), "hipMalloc")) return nullptr; owned_.push_back(p); return static_cast<T*>(p); }
    template <class T> T* upload(const T* src, size_t count) {   // alloc, and the copy queued on the stream; the caller keeps `src` alive past this arena (declare it first)
        T* p = alloc<T>(count);
        if (p && count) (void)failed(hipMemcpyAsync(p, src, count * sizeof(T), hipMemcpyHostToDevice, stream_), "hipMemcpyAsync (upload)");
        return p;
    }
    bool ok() const { return why_.empty(); }
    const std::string& why() const { return why_; }   // "<the HIP call>: <its error string>"
    hipError_t error() const { return error_; }       // the same failure as HIP named it; hipSuccess while ok()
    template <class T> T* release(T* p) { for (void*& q : owned_) if (q == (void*)p) q = nullptr; return p; }   // handed to the caller, who frees it
private:
    bool failed(hipError_t e, const char* call) { if (e == hipSuccess) return false; (void)hipGetLastError(); if (why_.empty()) { why_ = std::string(call) + ": " + hipGetErrorString(e); error_ = e; } return true; }
    hipStream_t stream_; std::vector<void*> owned_; std::string why_; hipError_t error_ = hipSuccess;
};

}  // namespace phost
