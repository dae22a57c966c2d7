// psgpu_buf.h — the owners of the library's device, pinned, stream and event handles (host only).
// Every hipMalloc / hipHostMalloc, every stream and every event of the library is made, and
// freed or destroyed, here.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <utility>

namespace psgpu {

// Device bytes currently held through DevBuf, process-wide (psgpu_debug_device_bytes).
inline std::atomic<uint64_t> g_deviceBytes{0};

// How reserve sizes a new allocation: ByHalf for buffers that grow run after run (at least half
// again the old capacity), Exact where the caller's expression already carries the slack.
enum class Growth { ByHalf, Exact };

// One hipMalloc allocation of `cap` elements.  An object lives in a heap context that its
// destroy function deletes, never in static storage: no free runs after the runtime shut down.
template <typename T>
struct DevBuf {
    T* ptr = nullptr;
    size_t cap = 0;  // elements

    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : ptr(std::exchange(o.ptr, nullptr)), cap(std::exchange(o.cap, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            ptr = std::exchange(o.ptr, nullptr);
            cap = std::exchange(o.cap, 0);
        }
        return *this;
    }
    ~DevBuf() { release(); }
    operator T*() const { return ptr; }

    // Room for `need` elements; a buffer that has to grow loses its contents.  *fresh: a new
    // allocation was made.  On failure the buffer is empty.
    hipError_t reserve(size_t need, Growth g, bool* fresh = nullptr) {
        if (fresh) *fresh = false;
        if (need <= cap && ptr) return hipSuccess;
        const size_t n = std::max<size_t>(g == Growth::ByHalf ? std::max(need, cap + cap / 2) : need, 1);
        release();
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&ptr), n * sizeof(T));
        if (e != hipSuccess) {
            ptr = nullptr;
            return e;
        }
        cap = n;
        g_deviceBytes += n * sizeof(T);
        if (fresh) *fresh = true;
        return hipSuccess;
    }
    void release() {
        if (ptr) {
            (void)hipFree(ptr);
            g_deviceBytes -= cap * sizeof(T);
        }
        ptr = nullptr;
        cap = 0;
    }
};

// The same over hipHostMalloc(flags); not counted in g_deviceBytes.
template <typename T>
struct PinnedBuf {
    T* ptr = nullptr;
    size_t cap = 0;  // elements

    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    PinnedBuf(PinnedBuf&& o) noexcept : ptr(std::exchange(o.ptr, nullptr)), cap(std::exchange(o.cap, 0)) {}
    PinnedBuf& operator=(PinnedBuf&& o) noexcept {
        if (this != &o) {
            release();
            ptr = std::exchange(o.ptr, nullptr);
            cap = std::exchange(o.cap, 0);
        }
        return *this;
    }
    ~PinnedBuf() { release(); }
    operator T*() const { return ptr; }
    T* operator->() const { return ptr; }

    // Exactly `need` elements (at least one), unless that many are held already.
    hipError_t reserve(size_t need, unsigned flags) {
        if (need <= cap && ptr) return hipSuccess;
        release();
        const size_t n = std::max<size_t>(need, 1);
        const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&ptr), n * sizeof(T), flags);
        if (e != hipSuccess) {
            ptr = nullptr;
            return e;
        }
        cap = n;
        return hipSuccess;
    }
    void release() {
        if (ptr) (void)hipHostFree(ptr);
        ptr = nullptr;
        cap = 0;
    }
};

// One stream, one event.  create() is a no-op while the handle is held; the same rule as DevBuf:
// in a heap context, never static.  reset() wants the handle's device current.
struct Stream {
    hipStream_t h = nullptr;

    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    Stream(Stream&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
    Stream& operator=(Stream&& o) noexcept {
        if (this != &o) {
            reset();
            h = std::exchange(o.h, nullptr);
        }
        return *this;
    }
    ~Stream() { reset(); }
    operator hipStream_t() const { return h; }

    hipError_t create(unsigned flags) {
        if (h) return hipSuccess;
        const hipError_t e = hipStreamCreateWithFlags(&h, flags);
        if (e != hipSuccess) h = nullptr;
        return e;
    }
    void reset() {
        if (h) (void)hipStreamDestroy(h);
        h = nullptr;
    }
};

struct Event {
    hipEvent_t h = nullptr;

    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    Event(Event&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
    Event& operator=(Event&& o) noexcept {
        if (this != &o) {
            reset();
            h = std::exchange(o.h, nullptr);
        }
        return *this;
    }
    ~Event() { reset(); }
    operator hipEvent_t() const { return h; }

    hipError_t create(unsigned flags = hipEventDefault) {  // (hipEventCreate is these flags)
        if (h) return hipSuccess;
        const hipError_t e = hipEventCreateWithFlags(&h, flags);
        if (e != hipSuccess) h = nullptr;
        return e;
    }
    void reset() {
        if (h) (void)hipEventDestroy(h);
        h = nullptr;
    }
};

// `count` elements of `size` bytes to the host, if the caller wants them and there are any.
inline hipError_t download_if(void* dst, const void* src, size_t count, size_t size) {
    return dst && count ? hipMemcpy(dst, src, count * size, hipMemcpyDeviceToHost) : hipSuccess;
}

}  // namespace psgpu
