// rtw_devbuf.h — the one owner of a device allocation: every buffer of a context (rtw_hip.hip rtw_ctx) and every per-call scratch
// buffer is a DevBuf. Host code over the runtime's C API alone (no device code in here, in the style of the *_plan.h headers), so
// tests/native/devbuf_check.cpp holds it with g++ and the sanitizers over stand-ins for the three runtime functions it calls.
#pragma once
#include <hip/hip_runtime_api.h>

namespace rtwk {

// A pointer and a capacity. The capacity's unit is the caller's (pixels, probes, elements, bytes): grow() compares in it and allocates
// in bytes. hipMalloc and hipFree on purpose: hipFree waits for the device, so a buffer may be grown while other streams of the
// context still have work queued.
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {  // (frees what it held)
        if (this != &o) { release(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
        return *this;
    }
    ~DevBuf() { release(); }

    // At least `need` units, `bytes` large when it has to be made anew; nothing happens when need <= cap(). drain: the stream whose
    // pending work may still read the old buffer and is waited for before that is freed, or null where every use has been waited
    // for. A failed allocation leaves the pointer null and the capacity 0, and its error is returned.
    hipError_t grow(size_t need, size_t bytes, const hipStream_t* drain = nullptr) {
        if (need <= cap_) return hipSuccess;
        if (drain) {
            const hipError_t e = hipStreamSynchronize(*drain);
            if (e != hipSuccess) return e;
        }
        release();
        const hipError_t e = hipMalloc(&p_, bytes);
        if (e != hipSuccess) { p_ = nullptr; return e; }
        cap_ = need;
        return hipSuccess;
    }
    void release() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr; cap_ = 0;
    }

    template <class T> T* as() const { return static_cast<T*>(p_); }
    size_t cap() const { return cap_; }
    explicit operator bool() const { return p_ != nullptr; }

private:
    void* p_ = nullptr;
    size_t cap_ = 0;
};

}  // namespace rtwk
