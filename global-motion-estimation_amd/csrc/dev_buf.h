// The one owner of device memory in libgme_hip.so: every hipMalloc and hipFree of the library is in this file (but for the
// upload lane's staging block, gme_api.hip).  Needs the HIP runtime API and the error codes only, so a host compiler
// builds it alone (tests/native/dev_buf_check.cpp).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>

#include <initializer_list>

#include "../../include/gme_hip.h"

void gme_set_error(const char* fmt, ...);

// A device block of `cap` elements of T, freed with its owner.  Converts to the plain pointer the launchers take.
template <typename T>
struct DevBuf {
    T* ptr = nullptr;
    size_t cap = 0;               // elements

    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : ptr(o.ptr), cap(o.cap) { o.ptr = nullptr; o.cap = 0; }      // movable, not copyable
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) { reset(); ptr = o.ptr; cap = o.cap; o.ptr = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { reset(); }

    T* get() const { return ptr; }
    operator T*() const { return ptr; }
    template <typename U>
    explicit operator U*() const { return (U*)ptr; }      // a cast reinterprets, as it does on the plain pointer

    void reset()
    {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        cap = 0;
    }

    // Room for n elements.  Grows only, and frees the old block first (peak memory never holds both): the contents are
    // lost when it grows, and work in flight that reads the old block must be waited for by the caller.  A failed
    // allocation leaves the buffer empty; a size past size_t is refused before the allocator is called at all, so the
    // buffer stays as it is.
    int ensure(size_t n, const char* what)
    {
        if (n <= cap) return GME_OK;
        if (n > (size_t)-1 / sizeof(T)) {
            gme_set_error("out of device memory (%zu elements of %zu bytes of %s)", n, sizeof(T), what);
            return GME_ERR_NOMEM;
        }
        reset();
        if (hipMalloc((void**)&ptr, n * sizeof(T)) != hipSuccess) {
            ptr = nullptr;
            gme_set_error("out of device memory (%zu bytes of %s)", n * sizeof(T), what);
            return GME_ERR_NOMEM;
        }
        cap = n;
        return GME_OK;
    }
};

// One member of a group of buffers that are sized together.
struct DevBufWant {
    int (*ensure)(void* buf, size_t n, const char* what);
    void (*reset)(void* buf);
    void* buf;
    size_t n;
    template <typename T>
    DevBufWant(DevBuf<T>& b, size_t n_)
        : ensure([](void* p, size_t n, const char* what) { return ((DevBuf<T>*)p)->ensure(n, what); }),
          reset([](void* p) { ((DevBuf<T>*)p)->reset(); }), buf(&b), n(n_) {}
};

// All or nothing: every member ends up large enough, or every member is empty.
inline int dev_ensure_all(const char* what, std::initializer_list<DevBufWant> group)
{
    for (const DevBufWant& w : group) {
        const int rc = w.ensure(w.buf, w.n, what);
        if (rc) {
            for (const DevBufWant& v : group) v.reset(v.buf);
            return rc;
        }
    }
    return GME_OK;
}
