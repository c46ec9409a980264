// device_owned.h -- the owners of what the host side allocates on or for the device, and how a host function refuses.  Whatever is
// allocated is a member (or a local) of one of the three move-only types below, so no destroy function lists memory or events: a
// handle is synchronised, then deleted, with its device current.  Streams have no owner type: the engine's are pooled and never
// destroyed (engine_internal.h, StreamSet), the two other handles have one each and must synchronise it before they destroy it.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <type_traits>

#include "../../include/roft_engine.h"

namespace roft {
namespace host {

// sets the calling thread's error string (roft_last_error_string) and returns `code` (engine.hip)
int fail(int code, const std::string& msg);


#define HIP_TRY(expr)                                                                                      \
    do {                                                                                                   \
        hipError_t _e = (expr);                                                                            \
        if (_e != hipSuccess)                                                                              \
            return fail(ROFT_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e));               \
    } while (0)
#define TRY(call) do { if (int _rc = (call)) return _rc; } while (0)   // (a call that has set the error string itself)

// "Is device d there?"  When it is not: the runtime's stale error is dropped (it is not the next call's) and the call is refused
// with the caller's text.
inline int require_device(int d, const char* refusal)
{
    int n = 0;
    if (hipGetDeviceCount(&n) == hipSuccess && d < n) return ROFT_OK;
    (void)hipGetLastError();
    return fail(ROFT_ERR_DEVICE, refusal);
}

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept { swap(o); }   // (move-only: one owner frees the memory; what `this` held goes with `o`)
    DevBuf& operator=(DevBuf&& o) noexcept { swap(o); return *this; }
    void swap(DevBuf& o) { std::swap(p, o.p); std::swap(n, o.n); }
    ~DevBuf() { release(); }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    hipError_t ensure(size_t count, bool zero = false)
    {
        if (count <= n && p) return hipSuccess;
        release();
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(count, 1) * sizeof(T));
        if (e != hipSuccess) { p = nullptr; return e; }
        n = count;
        if (zero) e = hipMemset(p, 0, std::max<size_t>(count, 1) * sizeof(T));
        return e;
    }
};

// pinned host memory (hipHostMalloc with the caller's flags): staging blocks, landing blocks, words a kernel writes
template <class T>
struct PinnedBuf {
    T* p = nullptr;
    size_t n = 0;
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf&& o) noexcept { swap(o); }
    PinnedBuf& operator=(PinnedBuf&& o) noexcept { swap(o); return *this; }
    void swap(PinnedBuf& o) { std::swap(p, o.p); std::swap(n, o.n); }
    ~PinnedBuf() { release(); }
    void release()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        n = 0;
    }
    hipError_t ensure(size_t count, unsigned flags = hipHostMallocDefault)
    {
        if (count <= n && p) return hipSuccess;
        release();
        const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(count, 1) * sizeof(T), flags);
        if (e != hipSuccess) p = nullptr; else n = count;
        return e;
    }
};

// a HIP event: null until the first create() (later ones keep it); reads as the hipEvent_t it holds wherever one is enqueued, waited
// for or timed
struct Event {
    hipEvent_t ev = nullptr;
    Event() = default;
    Event(Event&& o) noexcept { std::swap(ev, o.ev); }
    Event& operator=(Event&& o) noexcept { std::swap(ev, o.ev); return *this; }
    ~Event() { if (ev) (void)hipEventDestroy(ev); }
    hipError_t create(unsigned flags = hipEventDefault) { return ev ? hipSuccess : hipEventCreateWithFlags(&ev, flags); }
    operator hipEvent_t() const { return ev; }
};

// The round trip of a one-shot operator on HOST buffers: the inputs up, `run(inputs on the device, the product's place)` -- which
// enqueues on the null stream, or waits for what it enqueued elsewhere; what it returns but ROFT_OK is a refusal it has worded --
// the launch checked, the product down.
struct HostInput { const void* src; size_t bytes; };
template <size_t N, class F>
int host_round_trip(const HostInput (&in)[N], void* out, size_t out_bytes, F&& run)
{
    DevBuf<unsigned char> d_in[N], d_out;
    for (size_t i = 0; i < N; ++i) {
        HIP_TRY(d_in[i].ensure(in[i].bytes));
        HIP_TRY(hipMemcpy(d_in[i].p, in[i].src, in[i].bytes, hipMemcpyHostToDevice));
    }
    HIP_TRY(d_out.ensure(out_bytes));
    TRY(run(d_in, d_out.p));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d_out.p, out_bytes, hipMemcpyDeviceToHost));
    return ROFT_OK;
}

static_assert(!std::is_copy_constructible<DevBuf<float>>::value && !std::is_copy_constructible<PinnedBuf<float>>::value &&
                  !std::is_copy_constructible<Event>::value,
              "one owner releases what it holds");

}  // namespace host
}  // namespace roft
