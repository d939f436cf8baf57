// Lookups in a count list (include/brx.h "count lists"): the bucket directory over its sorted keys, and the entries that
// answer from it.  No counterpart in the reference.
//
// A list of n ascending keys below 2^(2k-1) and a directory of 2^d buckets, shift = (2k-1) - d:
//   dir[b] = number of keys < (b << shift), b = 0 .. 2^d, so dir[2^d] = n and bucket b is keys[dir[b] .. dir[b + 1]).
// d is the smallest with 16 * 2^d >= n, capped at min(2k-1, 30): 16 keys -- one 128-byte request -- per bucket in the
// mean, 8 bytes of offset per bucket, n/2 bytes beside the list's 9n.  br_amd/countops.py states it in numpy (directory,
// auto_log2_buckets, lookup).
// The build is one launch, a thread per bucket (and one more for dir[2^d]): a lower-bound search over the whole list for
// the bucket's first border, then a galloping search from there for its end, which costs a step or two where the bucket
// is of the mean size and stays logarithmic where the list skews.  Every thread writes its own dir[b] and nothing else but
// a wave-reduced atomic max of the bucket sizes; no thread reads what another wrote, no workgroup waits for another.
// The lookups themselves are abund_count<SRC_LIST> of brx_abundance.hip.
#include <shared_mutex>

#include "brx_internal.hpp"

using namespace brx;

namespace {

typedef unsigned long long u64;

// first index in [lo, hi) whose key is >= x (hi if none)
__device__ __forceinline__ uint64_t lower_bound(const uint64_t *__restrict__ keys, uint64_t lo, uint64_t hi, uint64_t x)
{
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < x)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void list_dir_kernel(const uint64_t *__restrict__ keys, uint64_t n, uint32_t shift, uint64_t n_buckets,
                                                       uint64_t *__restrict__ dir, u64 *__restrict__ d_fullest)
{
    const uint64_t b = (uint64_t)blockIdx.x * 256ull + threadIdx.x;
    uint64_t size = 0;
    if (b < n_buckets) {
        const uint64_t first = lower_bound(keys, 0, n, b << shift);
        // the end of the bucket: gallop from its start ((b + 1) << shift <= 2^(2k-1) <= 2^61: no overflow)
        const uint64_t border = (b + 1ull) << shift;
        uint64_t step = 16, lo = first, hi = first;
        for (;;) {
            hi = n - lo < step ? n : lo + step; // candidate end, <= n
            if (hi == n || keys[hi - 1] >= border)
                break;
            lo = hi; // keys[hi - 1] < border: the end lies at or behind hi
            step <<= 1;
        }
        size = lower_bound(keys, lo, hi, border) - first;
        dir[b] = first;
    } else if (b == n_buckets) {
        dir[b] = n;
    }
    for (int d = 32; d > 0; d >>= 1) {
        const uint64_t o = (uint64_t)__shfl_xor((long long)size, d);
        size = o > size ? o : size;
    }
    if ((threadIdx.x & 63u) == 0u && size)
        atomicMax(d_fullest, (u64)size);
}

int max_log2(int k) { return 2 * k - 1 < 30 ? 2 * k - 1 : 30; }

int auto_log2(uint64_t n, int k)
{
    int d = 0;
    while (d < max_log2(k) && (16ull << d) < n)
        d++;
    return d;
}

// the caller holds lk_mu (shared is enough)
int refuse_unprepared(const char *me, const brx_counts *l)
{
    set_error("%s: the count list has no lookup directory (k=%d, %llu entries): build it first with brx_counts_lookup_prepare", me, l->k,
              (u64)l->n);
    return BRX_ERR_UNSUPPORTED;
}

ListView view_of(const brx_counts *l)
{
    ListView v;
    v.k = l->k;
    v.keys = l->d_keys;
    v.cnts = l->d_cnts;
    v.dir = l->d_dir;
    v.shift = (uint32_t)(2 * l->k - 1 - l->lk_log2);
    v.n = l->n;
    return v;
}

// the body of both batch entries; the caller holds lk_mu shared and has seen a directory
int list_abund_locked(const brx_counts *l, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads, uint64_t total_bases,
                      uint8_t abundance, uint8_t *d_profile, uint32_t *d_hist, brx_abund_stats_t *d_stats, hipStream_t s)
{
    bool done = false;
    BRX_TRY(abund_empty_batch(n_reads, total_bases, d_profile, d_hist, d_stats, s, &done));
    return done ? BRX_OK
                : abund_batch_list(view_of(l), d_bases, d_offsets, n_reads, total_bases, abundance, d_profile, d_hist, d_stats, s);
}

} // namespace

extern "C" {

int brx_counts_lookup_prepare(brx_counts_t *l, int log2_buckets)
{
    const char *me = "brx_counts_lookup_prepare";
    BRX_TRY(list_ok(me, l));
    if (!(l->k & 1) || l->k < 5 || l->k > 31) {
        set_error("%s: count lists hold the keys of odd k from 5 to 31 (k=%d)", me, l->k);
        return BRX_ERR_UNSUPPORTED;
    }
    if (log2_buckets > max_log2(l->k)) {
        set_error("%s: log2_buckets=%d, at most min(2k-1, 30) = %d at k=%d (negative: chosen from the entries)", me, log2_buckets,
                  max_log2(l->k), l->k);
        return BRX_ERR_ARG;
    }
    const int d = log2_buckets < 0 ? auto_log2(l->n, l->k) : log2_buckets;
    std::unique_lock<std::shared_mutex> g(l->lk_mu);
    if (l->lk_log2 == d)
        return BRX_OK;
    BRX_TRY(use_device(l->device));
    l->lk_log2 = -1;
    l->lk_fullest = 0;
    l->d_dir.reset(); // (another d: not both directories at once)
    const uint64_t n_buckets = 1ull << d;
    BRX_TRY(l->d_dir.reserve(n_buckets + 1, 0, "lookup directory of a count list"));
    DevScratch ws; // (declared before the stream: the stream is synchronised before the scratch goes back)
    u64 *d_fullest = nullptr;
    BRX_TRY(ws.get(&d_fullest, 1));
    OwnStream own;
    BRX_HIP(hipStreamCreateWithFlags(&own.s, hipStreamNonBlocking));
    BRX_HIP(hipMemsetAsync(d_fullest, 0, 8, own.s));
    {
        KernelTimer kt("list_dir", own.s);
        list_dir_kernel<<<(uint32_t)((n_buckets + 1 + 255) / 256), 256, 0, own.s>>>(l->d_keys, l->n, (uint32_t)(2 * l->k - 1 - d), n_buckets,
                                                                                   l->d_dir, d_fullest);
        BRX_HIP(hipGetLastError());
    }
    u64 fullest = 0;
    BRX_HIP(hipMemcpyAsync(&fullest, d_fullest, 8, hipMemcpyDeviceToHost, own.s));
    const hipError_t e = hipStreamSynchronize(own.s);
    if (e != hipSuccess) {
        l->d_dir.reset();
        set_error("%s: %s", me, hipGetErrorString(e));
        return BRX_ERR_HIP;
    }
    l->lk_fullest = fullest;
    l->lk_log2 = d;
    return BRX_OK;
}

int brx_counts_lookup_info(const brx_counts_t *l, uint64_t *info4)
{
    const char *me = "brx_counts_lookup_info";
    BRX_TRY(list_ok(me, l));
    if (!info4) {
        set_error("%s: null info4", me);
        return BRX_ERR_ARG;
    }
    std::shared_lock<std::shared_mutex> g(l->lk_mu);
    const bool ready = l->lk_log2 >= 0;
    info4[0] = ready ? 1 : 0;
    info4[1] = ready ? (uint64_t)l->lk_log2 : 0;
    info4[2] = ready ? ((1ull << l->lk_log2) + 1) * 8 : 0;
    info4[3] = ready ? l->lk_fullest : 0;
    return BRX_OK;
}

int brx_counts_lookup_directory(const brx_counts_t *l, void **d_dir, uint64_t *entries)
{
    const char *me = "brx_counts_lookup_directory";
    BRX_TRY(list_ok(me, l));
    if (!d_dir || !entries) {
        set_error("%s: null output", me);
        return BRX_ERR_ARG;
    }
    std::shared_lock<std::shared_mutex> g(l->lk_mu);
    if (l->lk_log2 < 0)
        return refuse_unprepared(me, l);
    *d_dir = (void *)l->d_dir.get();
    *entries = (1ull << l->lk_log2) + 1;
    return BRX_OK;
}

int brx_counts_lookup_drop(brx_counts_t *l)
{
    BRX_TRY(list_ok("brx_counts_lookup_drop", l));
    std::unique_lock<std::shared_mutex> g(l->lk_mu);
    l->lk_log2 = -1;
    l->lk_fullest = 0;
    l->d_dir.reset();
    return BRX_OK;
}

int brx_counts_abundance_batch_device(const brx_counts_t *l, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads,
                                      uint64_t total_bases, uint8_t abundance, uint8_t *d_profile, uint32_t *d_hist,
                                      brx_abund_stats_t *d_stats, void *stream)
{
    const char *me = "brx_counts_abundance_batch_device";
    BRX_TRY(list_ok(me, l));
    std::shared_lock<std::shared_mutex> g(l->lk_mu);
    if (l->lk_log2 < 0)
        return refuse_unprepared(me, l);
    BRX_TRY(check_batch_args(me, d_bases, d_offsets, n_reads, total_bases));
    BRX_TRY(use_device(l->device));
    return list_abund_locked(l, d_bases, d_offsets, n_reads, total_bases, abundance, d_profile, d_hist, d_stats, (hipStream_t)stream);
}

int brx_counts_abundance_batch(const brx_counts_t *l, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads, uint8_t abundance,
                               uint8_t *profile, uint32_t *hist, brx_abund_stats_t *stats)
{
    const char *me = "brx_counts_abundance_batch";
    BRX_TRY(list_ok(me, l));
    if (n_reads && !offsets) {
        set_error("%s: null offsets", me);
        return BRX_ERR_ARG;
    }
    const uint64_t total = n_reads ? offsets[n_reads] : 0;
    std::shared_lock<std::shared_mutex> g(l->lk_mu);
    if (l->lk_log2 < 0)
        return refuse_unprepared(me, l);
    BRX_TRY(check_batch_args(me, bases, offsets, n_reads, total));
    BRX_TRY(check_offsets(me, offsets, n_reads));
    BRX_TRY(use_device(l->device));
    if (!n_reads || (!profile && !hist && !stats))
        return BRX_OK;
    DevScratch sc;
    uint8_t *d_bases = nullptr, *d_profile = nullptr;
    uint64_t *d_off = nullptr;
    uint32_t *d_hist = nullptr;
    brx_abund_stats_t *d_stats = nullptr;
    BRX_TRY(sc.get(&d_bases, total));
    BRX_TRY(sc.get(&d_off, (uint64_t)n_reads + 1));
    if (profile)
        BRX_TRY(sc.get(&d_profile, total));
    if (hist)
        BRX_TRY(sc.get(&d_hist, (uint64_t)n_reads * 256ull));
    if (stats)
        BRX_TRY(sc.get(&d_stats, n_reads));
    OwnStream own;
    BRX_HIP(hipStreamCreateWithFlags(&own.s, hipStreamNonBlocking));
    hipStream_t s = own.s;
    auto run = [&]() -> int {
        if (total)
            BRX_HIP(hipMemcpyAsync(d_bases, bases, total, hipMemcpyHostToDevice, s));
        BRX_HIP(hipMemcpyAsync(d_off, offsets, ((uint64_t)n_reads + 1) * 8, hipMemcpyHostToDevice, s));
        BRX_TRY(list_abund_locked(l, d_bases, d_off, n_reads, total, abundance, d_profile, d_hist, d_stats, s));
        if (profile && total)
            BRX_HIP(hipMemcpyAsync(profile, d_profile, total, hipMemcpyDeviceToHost, s));
        if (hist)
            BRX_HIP(hipMemcpyAsync(hist, d_hist, (uint64_t)n_reads * 1024ull, hipMemcpyDeviceToHost, s));
        if (stats)
            BRX_HIP(hipMemcpyAsync(stats, d_stats, (uint64_t)n_reads * sizeof(brx_abund_stats_t), hipMemcpyDeviceToHost, s));
        return BRX_OK;
    };
    const int st = run();
    const hipError_t e = hipStreamSynchronize(s); // the blocks are freed below: nothing may still be running
    if (st == BRX_OK && e != hipSuccess) {
        set_error("%s: %s", me, hipGetErrorString(e));
        return BRX_ERR_HIP;
    }
    return st;
}

int brx_counts_get_counts(const brx_counts_t *l, const uint64_t *forward_kmers, uint32_t n, uint8_t *out)
{
    const char *me = "brx_counts_get_counts";
    BRX_TRY(list_ok(me, l));
    std::shared_lock<std::shared_mutex> g(l->lk_mu);
    if (l->lk_log2 < 0)
        return refuse_unprepared(me, l);
    if ((!forward_kmers || !out) && n) {
        set_error("%s: null k-mers / out", me);
        return BRX_ERR_ARG;
    }
    BRX_TRY(use_device(l->device));
    if (!n)
        return BRX_OK;
    DevScratch sc;
    uint64_t *d_k = nullptr;
    uint8_t *d_o = nullptr;
    BRX_TRY(sc.get(&d_k, n));
    BRX_TRY(sc.get(&d_o, n));
    OwnStream own;
    BRX_HIP(hipStreamCreateWithFlags(&own.s, hipStreamNonBlocking));
    hipStream_t s = own.s;
    auto run = [&]() -> int {
        BRX_HIP(hipMemcpyAsync(d_k, forward_kmers, (uint64_t)n * 8, hipMemcpyHostToDevice, s));
        BRX_TRY(abund_get_counts_list(view_of(l), d_k, n, d_o, s));
        BRX_HIP(hipMemcpyAsync(out, d_o, n, hipMemcpyDeviceToHost, s));
        return BRX_OK;
    };
    const int st = run();
    const hipError_t e = hipStreamSynchronize(s);
    if (st == BRX_OK && e != hipSuccess) {
        set_error("%s: %s", me, hipGetErrorString(e));
        return BRX_ERR_HIP;
    }
    return st;
}

} // extern "C"
