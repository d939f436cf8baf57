// Owners of device memory.  Every device block of the library comes from the block pool (brx_devpool.hip) through one of
// the two types here; host-only code can include this header (it needs no HIP compiler).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <utility>
#include <vector>

#include "../../include/brx.h"

namespace brx {

void set_error(const char *fmt, ...);
hipError_t dev_alloc(void **out, size_t bytes);
hipError_t dev_free(void *p);

// Owns one device block from the pool; movable, not copyable.  Converts to T* so that reads and launch argument lists
// look as they do with a raw pointer.
template <typename T> class DevBuf {
  public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept { swap(o); }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) {
            reset();
            swap(o);
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    T *get() const { return p_; }
    operator T *() const { return p_; }
    uint64_t bytes() const { return bytes_; }
    uint64_t cap() const { return bytes_ / sizeof(T); } // elements

    // At least `need` elements; contents are NOT kept across a growth.  Within capacity: no call into the pool.  A growth
    // frees the old block, then asks the pool for (need + headroom) * sizeof(T) bytes.  When that fails: set_error with
    // `what` and the byte count, BRX_ERR_NOMEM, and the buffer is empty (null, capacity 0).
    int reserve(uint64_t need, uint64_t headroom, const char *what)
    {
        return reserve_bytes(need * sizeof(T), headroom * sizeof(T), what);
    }
    // the same for the owners that size a workspace in bytes (a headroom in bytes need not be a whole number of elements)
    int reserve_bytes(uint64_t need, uint64_t headroom, const char *what)
    {
        if (p_ && need <= bytes_)
            return BRX_OK;
        reset();
        const uint64_t want = need + headroom;
        void *p = nullptr;
        const hipError_t e = dev_alloc(&p, want);
        if (e != hipSuccess) {
            set_error("hipMalloc(%llu B, %s): HIP error %d", (unsigned long long)want, what, (int)e);
            return BRX_ERR_NOMEM;
        }
        p_ = (T *)p;
        bytes_ = want;
        return BRX_OK;
    }
    void reset() // free now
    {
        if (p_)
            (void)dev_free(p_);
        p_ = nullptr;
        bytes_ = 0;
    }
    // hand-over to an owner outside (it frees with dev_free), and from one: `cap` elements
    T *release()
    {
        T *p = p_;
        p_ = nullptr;
        bytes_ = 0;
        return p;
    }
    void adopt(T *p, uint64_t cap)
    {
        reset();
        p_ = p;
        bytes_ = p ? cap * sizeof(T) : 0;
    }
    void swap(DevBuf &o)
    {
        std::swap(p_, o.p_);
        std::swap(bytes_, o.bytes_);
    }

  private:
    T *p_ = nullptr;
    uint64_t bytes_ = 0;
};

// device blocks of one call; released when the call returns
struct DevScratch {
    std::vector<DevBuf<uint8_t>> blocks;
    template <typename T> int get(T **out, uint64_t n)
    {
        DevBuf<uint8_t> b;
        const int st = b.reserve_bytes((n ? n : 1) * sizeof(T), 0, "scratch of one call");
        *out = (T *)b.get();
        if (st == BRX_OK)
            blocks.push_back(std::move(b));
        return st;
    }
};

} // namespace brx
