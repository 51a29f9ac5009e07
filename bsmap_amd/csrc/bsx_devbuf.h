// bsx_devbuf.h — owners of what the host code of libbsx.so holds on a device: memory, events, streams.  Each frees what it holds when it goes out of scope or
// with the handle it is a member of (the handle's destroy function makes the device current first), so a fail path is a plain `return`.  Host translation
// units include this beside bsx_internal.h; no kernel sees it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

// Device memory.  A failed allocation leaves it empty and returns HIP's error, for HIP_TRY or a message of the caller's own.  Where a T * is expected the
// buffer itself will do (null while empty); a kernel launch, which deduces its argument types, takes `.p`.
template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;  // bytes
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { reset(); }
    operator T *() const { return p; }
    void reset() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }   // frees
    T *detach() { T *q = p; p = nullptr; cap = 0; return q; }         // hands the memory to a raw owner (the members of bsx_ref)
    // at least `bytes` of it; a buffer that is large enough stays (with its contents), a smaller one is replaced (without them)
    hipError_t reserve(size_t bytes)
    {
        if (p && bytes <= cap) return hipSuccess;
        reset();
        const hipError_t e = hipMalloc((void **)&p, bytes ? bytes : 1);
        if (e != hipSuccess) { (void)hipGetLastError(); p = nullptr; return e; }
        cap = bytes;
        return hipSuccess;
    }
    // `bytes` of zeroes, ready when it returns; on `stream`, so that it does not wait for the null stream
    hipError_t zeroed(size_t bytes, hipStream_t stream)
    {
        hipError_t e = reserve(bytes);
        if (e == hipSuccess) e = hipMemsetAsync(p, 0, bytes, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) reset();
        return e;
    }
};

// (movable: pools of them grow in a std::vector)
struct DevEvent {
    hipEvent_t ev = nullptr;
    DevEvent() = default;
    DevEvent(const DevEvent &) = delete;
    DevEvent &operator=(const DevEvent &) = delete;
    DevEvent(DevEvent &&o) noexcept : ev(o.ev) { o.ev = nullptr; }
    ~DevEvent() { reset(); }
    operator hipEvent_t() const { return ev; }
    void reset() { if (ev) (void)hipEventDestroy(ev); ev = nullptr; }
    hipError_t create(unsigned flags = 0) { reset(); return flags ? hipEventCreateWithFlags(&ev, flags) : hipEventCreate(&ev); }
};

// (destroyed as it is: its owner synchronises it first where work may still be queued)
struct DevStream {
    hipStream_t s = nullptr;
    DevStream() = default;
    DevStream(const DevStream &) = delete;
    DevStream &operator=(const DevStream &) = delete;
    ~DevStream() { reset(); }
    operator hipStream_t() const { return s; }
    void reset() { if (s) (void)hipStreamDestroy(s); s = nullptr; }
    hipError_t create(unsigned flags) { reset(); return hipStreamCreateWithFlags(&s, flags); }
    hipError_t create(unsigned flags, int priority) { reset(); return hipStreamCreateWithPriority(&s, flags, priority); }
};
