// What the files of keys share (brx_keyfile.hip: key files; brx_kmertext.hip: k-mer text): the block scan their kernels
// place things with, and the piece machinery of the host paths -- a stream passes through two page-locked pieces of
// BRX_KEYFILE_SLICE_KB KiB (default 8192, at least 4), one being filled or drained by the fd while the other is copied.
#pragma once
#include "brx_internal.hpp"

#include <chrono>

namespace brx {

#if defined(__HIPCC__)
static __device__ __forceinline__ unsigned long long wave_incl_scan(unsigned long long x, uint32_t lane)
{
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long y = __shfl_up(x, o);
        if (lane >= (uint32_t)o)
            x += y;
    }
    return x;
}

// exclusive prefix of x over the 256 threads of the block, *total = their sum; sh holds 4 entries
static __device__ __forceinline__ unsigned long long block_excl_scan(unsigned long long x, unsigned long long *sh, unsigned long long *total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long inc = wave_incl_scan(x, lane);
    __syncthreads(); // (sh may still be read from the trip before)
    if (lane == 63u)
        sh[wave] = inc;
    __syncthreads();
    unsigned long long off = 0;
    for (uint32_t w = 0; w < wave; w++)
        off += sh[w];
    *total = sh[0] + sh[1] + sh[2] + sh[3];
    return off + inc - x;
}
#endif

typedef std::chrono::steady_clock Clock;
inline uint64_t ns_since(Clock::time_point t0) { return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(Clock::now() - t0).count(); }

// bytes of a piece (brx_keyfile.hip)
size_t slice_bytes();
// all n bytes to the fd / until `want` bytes or the end of the stream, *got = bytes read; an I/O error is BRX_ERR_ARG
int write_all(int fd, const uint8_t *p, size_t n);
int read_upto(int fd, uint8_t *p, size_t want, size_t *got);

struct PinnedPair {
    uint8_t *p[2] = {nullptr, nullptr};
    ~PinnedPair()
    {
        host_buf_release(p[0]);
        host_buf_release(p[1]);
    }
    int get(size_t bytes)
    {
        for (int i = 0; i < 2; i++)
            if (!(p[i] = (uint8_t *)host_buf_acquire(bytes))) {
                set_error("key file: no host memory for a piece of %llu bytes", (unsigned long long)bytes);
                return BRX_ERR_NOMEM;
            }
        return BRX_OK;
    }
};

struct EventPair {
    hipEvent_t e[2] = {nullptr, nullptr};
    ~EventPair()
    {
        for (int i = 0; i < 2; i++)
            if (e[i])
                (void)hipEventDestroy(e[i]);
    }
    int make()
    {
        for (int i = 0; i < 2; i++)
            BRX_HIP(hipEventCreateWithFlags(&e[i], hipEventDisableTiming));
        return BRX_OK;
    }
};

} // namespace brx
