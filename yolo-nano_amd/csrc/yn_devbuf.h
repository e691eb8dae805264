// yn_devbuf.h — the one owner of device and pinned host memory: every hipMalloc / hipFree / hipHostMalloc / hipHostFree of the library
// is in this file (tests/test_capi_cpu.py).  A long-lived object holds DevBuf / PinnedBuf members and needs no free list: deleting it
// with its device current releases them.  tests/test_devbuf_cpu.py drives the type on the host with a malloc-backed policy.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <utility>

namespace ynk {

// blocks and bytes held through HipDeviceAlloc, process-wide (yn_live_device_memory)
inline std::atomic<int64_t> g_live_blocks{0}, g_live_bytes{0};

// An allocator policy: alloc() returns 0 and a block, or an error code (a hipError_t here) and nothing; release() takes the byte count alloc()
// was given and ignores errors (as every destroy path does); copy(), needed by the keeping growth only, returns once the bytes have arrived and
// `s` is drained, also for 0 bytes.
struct HipDeviceAlloc {
    static int alloc(void** p, size_t bytes)
    {
        const hipError_t r = hipMalloc(p, bytes);
        if (r != hipSuccess) { *p = nullptr; return (int)r; }
        g_live_blocks += 1; g_live_bytes += (int64_t)bytes;
        return 0;
    }
    static void release(void* p, size_t bytes)
    {
        (void)hipFree(p);
        g_live_blocks -= 1; g_live_bytes -= (int64_t)bytes;
    }
    static int copy(void* dst, const void* src, size_t bytes, hipStream_t s)
    {
        hipError_t r = bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s) : hipSuccess;
        if (r == hipSuccess) r = hipStreamSynchronize(s);
        return (int)r;
    }
};

template <unsigned Flags>
struct HipPinnedAlloc {
    static int alloc(void** p, size_t bytes)
    {
        const hipError_t r = hipHostMalloc(p, bytes, Flags);
        if (r != hipSuccess) *p = nullptr;
        return (int)r;
    }
    static void release(void* p, size_t) { (void)hipHostFree(p); }
};

// Owns one block of cap() elements of T.  After ANY return, failure included, it is {nullptr, 0} or a live block of cap() elements.
// The growth calls return 0 or the allocator's error code and set *moved (when given, never cleared) if get() changed: a caller that has
// captured the address in a graph drops the graph then, also on the way out of a failure.
// `first` is the growth rule of the call site: 0 = exactly `need` elements; else the capacity (`first` when empty) doubled until it holds `need`.
template <typename T, typename Alloc = HipDeviceAlloc>
class DevBuf {
    T* p_ = nullptr;
    size_t cap_ = 0;

    static size_t grown(size_t cap, size_t need, size_t first)
    {
        if (!first) return need;
        size_t nc = cap ? cap : first;
        while (nc < need) nc *= 2;
        return nc;
    }

public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
        return *this;
    }
    ~DevBuf() { reset(); }

    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t cap() const { return cap_; }

    void reset()
    {
        if (p_) Alloc::release(p_, cap_ * sizeof(T));
        p_ = nullptr; cap_ = 0;
    }

    // at least `need` elements, contents dropped: the old block goes first, so the peak is one block
    int reserve(size_t need, size_t first = 0, bool* moved = nullptr)
    {
        if (need <= cap_) return 0;
        const size_t nc = grown(cap_, need, first);
        if (p_ && moved) *moved = true;
        reset();
        void* q = nullptr;
        const int r = Alloc::alloc(&q, nc * sizeof(T));
        if (r) return r;
        p_ = static_cast<T*>(q); cap_ = nc;
        if (moved) *moved = true;
        return 0;
    }

    // at least `need` elements, the first `used` kept: copied on `s`, which is drained before the old block goes.  On failure the old
    // block and its contents stay and the new one is released.
    int reserve_keep(size_t need, size_t used, hipStream_t s, size_t first = 0, bool* moved = nullptr)
    {
        if (need <= cap_) return 0;
        DevBuf n;
        int r = n.reserve(grown(cap_, need, first));
        if (!r) r = Alloc::copy(n.p_, p_, used * sizeof(T), s);
        if (r) return r;
        *this = std::move(n);
        if (moved) *moved = true;
        return 0;
    }
};

template <typename T, unsigned Flags = hipHostMallocDefault>
using PinnedBuf = DevBuf<T, HipPinnedAlloc<Flags>>;

}  // namespace ynk
