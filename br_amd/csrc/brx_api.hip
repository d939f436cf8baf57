// Diagnostics, device selection and the per-kernel event timers of libbrx.so; the C entries of the abundance calls.
#include "brx_internal.hpp"

#include <stdio.h>
#include <stdlib.h>
#include <chrono>
#include <string.h>
#include <map>

namespace brx {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int use_device(int device)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        set_error("no usable HIP device (hipGetDeviceCount: %s); libbrx has no CPU fallback",
                  e == hipSuccess ? "0 devices" : hipGetErrorString(e));
        return BRX_ERR_NODEVICE;
    }
    if (device < 0 || device >= n) {
        set_error("device %d out of range (0..%d)", device, n - 1);
        return BRX_ERR_ARG;
    }
    BRX_HIP(hipSetDevice(device));
    return BRX_OK;
}

int check_batch_args(const char *what, const void *bases, const uint64_t *offsets, uint32_t n_reads, uint64_t total_bases)
{
    if ((n_reads && !offsets) || (total_bases && !bases)) {
        set_error("%s: null bases / offsets for %u reads, %llu bases", what, n_reads, (unsigned long long)total_bases);
        return BRX_ERR_ARG;
    }
    if (total_bases && !n_reads) {
        set_error("%s: %llu bases in no reads", what, (unsigned long long)total_bases);
        return BRX_ERR_ARG;
    }
    return BRX_OK;
}

int check_offsets(const char *what, const uint64_t *offsets, uint32_t n_reads, bool strand_rule)
{
    const uint64_t longest = strand_rule ? 0xfffffffeull : 0xfffffff0ull;
    for (uint32_t r = 0; r < n_reads; r++)
        if (offsets[r + 1] < offsets[r] || offsets[r + 1] - offsets[r] > longest || (!strand_rule && r == 0 && offsets[0] != 0)) {
            if (strand_rule)
                set_error("%s: offsets must not decrease and a read holds fewer than 2^32 - 1 bases (read %u)", what, r);
            else
                set_error("%s: offsets must start at 0 and not decrease; a read holds fewer than 2^32 - 16 bases (read %u)", what, r);
            return BRX_ERR_ARG;
        }
    return BRX_OK;
}

void trace_stage(hipStream_t s, const char *what)
{
    static const bool on = [] { const char *e = getenv("BRX_TRACE"); return e && *e && *e != '0'; }();
    if (!on)
        return;
    static const auto t0 = std::chrono::steady_clock::now();
    const hipError_t e = hipStreamSynchronize(s);
    fprintf(stderr, "[brx %9.3f s] %s%s%s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), what,
            e == hipSuccess ? "" : " -> ", e == hipSuccess ? "" : hipGetErrorString(e));
    fflush(stderr);
}

// ---- timers ---------------------------------------------------------------------------------
struct TimerSlot {
    std::string name;
    double total_ms = 0;
    uint64_t launches = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

static std::mutex g_tmu;
static bool g_prof_on = false;
static std::vector<TimerSlot> g_slots;
static std::vector<hipEvent_t> g_pool;

static int slot_of(const char *name)
{
    for (size_t i = 0; i < g_slots.size(); i++)
        if (g_slots[i].name == name)
            return (int)i;
    g_slots.emplace_back();
    g_slots.back().name = name;
    return (int)g_slots.size() - 1;
}

static hipEvent_t get_event()
{
    if (!g_pool.empty()) {
        hipEvent_t e = g_pool.back();
        g_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess)
        return nullptr;
    return e;
}

static void resolve(TimerSlot &s)
{
    for (auto &p : s.pending) {
        float ms = 0;
        if (hipEventSynchronize(p.second) == hipSuccess && hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) {
            s.total_ms += ms;
            s.launches++;
        } else {
            // (events of a timer whose stream is gone by now, e.g. a finished pipeline's: the runtime keeps the failed
            // query as the thread's last error, and the next launch that asks hipGetLastError would take it for its own)
            (void)hipGetLastError();
        }
        g_pool.push_back(p.first);
        g_pool.push_back(p.second);
    }
    s.pending.clear();
}

KernelTimer::KernelTimer(const char *name, hipStream_t s) : slot_(-1), s_(s), start_(nullptr), stop_(nullptr), on_(false)
{
    std::lock_guard<std::mutex> g(g_tmu);
    if (!g_prof_on)
        return;
    slot_ = slot_of(name);
    start_ = get_event();
    stop_ = get_event();
    if (!start_ || !stop_)
        return;
    on_ = hipEventRecord(start_, s_) == hipSuccess;
}

KernelTimer::~KernelTimer()
{
    if (!on_)
        return;
    (void)hipEventRecord(stop_, s_);
    std::lock_guard<std::mutex> g(g_tmu);
    g_slots[slot_].pending.emplace_back(start_, stop_);
}

// ---- page-locked host buffers: what the host-buffer entry points hand back, and what callers may fill ---------------
// A copy between HBM and PAGEABLE host memory goes through the runtime's own bounce buffers at 6-10 GB/s: 82 MB each
// way per 8192-record batch was 2/3 of brx_chain_correct_batch's 31 ms (tools/host_rate.py, round 2).  Page-locked memory
// moves at PCIe speed and asynchronously; hipHostMalloc itself costs milliseconds, so the blocks are pooled: a block
// released by brx_buf_free / brx_host_free is kept (up to BRX_HOSTPOOL_GB) for the next batch.
namespace {
struct HostBlock {
    void *p;
    size_t cap;
    bool used;
};
std::mutex g_hostpool_mu;
std::vector<HostBlock> g_hostpool;
// idle page-locked bytes kept for reuse (BRX_HOSTPOOL_GB, default 4): three chains in flight with 32768-record batches
// hold ~2 GiB of blocks between them -- at the first 1 GiB limit every batch paid a hipHostMalloc of its 328 MB output
// again (67 ms per batch instead of 25: profiles/r4h_bench_n1.json records_32768 before the change)
size_t pool_keep()
{
    static const size_t v = [] {
        const char *e = getenv("BRX_HOSTPOOL_GB");
        const double gb = e && *e ? atof(e) : 4.0;
        return gb <= 0 ? (size_t)0 : (size_t)(gb * (double)(1ull << 30));
    }();
    return v;
}
}

void *host_buf_acquire(size_t bytes)
{
    {
        std::lock_guard<std::mutex> g(g_hostpool_mu);
        int best = -1;
        for (int i = 0; i < (int)g_hostpool.size(); i++)
            if (!g_hostpool[i].used && g_hostpool[i].cap >= bytes && g_hostpool[i].cap <= 2 * bytes + (1u << 20) &&
                (best < 0 || g_hostpool[i].cap < g_hostpool[best].cap))
                best = i;
        if (best >= 0) {
            g_hostpool[best].used = true;
            return g_hostpool[best].p;
        }
    }
    void *p = nullptr;
    const size_t cap = bytes + bytes / 8 + 4096; // batches of a stream differ by a few percent: let the next one fit
    if (hipHostMalloc(&p, cap, hipHostMallocDefault) != hipSuccess || !p) {
        // no GPU runtime / no lockable memory left: plain memory still works, only slower
        p = malloc(bytes);
        return p;
    }
    std::lock_guard<std::mutex> g(g_hostpool_mu);
    g_hostpool.push_back(HostBlock{p, cap, true});
    return p;
}

void host_buf_release(void *p)
{
    if (!p)
        return;
    void *drop = nullptr;
    {
        std::lock_guard<std::mutex> g(g_hostpool_mu);
        size_t idle = 0;
        int at = -1;
        for (int i = 0; i < (int)g_hostpool.size(); i++) {
            if (g_hostpool[i].p == p)
                at = i;
            else if (!g_hostpool[i].used)
                idle += g_hostpool[i].cap;
        }
        if (at < 0) { // not one of ours: it came from malloc
            drop = nullptr;
        } else if (idle + g_hostpool[at].cap > pool_keep()) {
            drop = g_hostpool[at].p;
            g_hostpool.erase(g_hostpool.begin() + at);
            (void)hipHostFree(drop);
            return;
        } else {
            g_hostpool[at].used = false;
            return;
        }
    }
    free(p);
}

bool host_buf_is_pinned(const void *p)
{
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError(); // (an ordinary malloc'ed pointer: the query fails and leaves a sticky-looking error behind)
        return false;
    }
    return at.type == hipMemoryTypeHost;
}

} // namespace brx

using namespace brx;

extern "C" {

const char *brx_strerror(int status)
{
    switch (status) {
    case BRX_OK: return "ok";
    case BRX_ERR_ARG: return "bad argument";
    case BRX_ERR_NOMEM: return "out of memory";
    case BRX_ERR_HIP: return "HIP runtime error";
    case BRX_ERR_NODEVICE: return "no usable GPU (no CPU fallback)";
    case BRX_ERR_FORMAT: return "malformed input";
    case BRX_ERR_UNSUPPORTED: return "not implemented";
    case BRX_ERR_OVERFLOW: return "output buffer too small";
    default: return "unknown status";
    }
}

const char *brx_last_error(void) { return g_err; }

int brx_version(void) { return 100; }

int brx_device_count(int *n)
{
    if (!n)
        return BRX_ERR_ARG;
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        c = 0;
    }
    *n = c;
    return BRX_OK;
}

int brx_profile_enable(int on)
{
    std::lock_guard<std::mutex> g(g_tmu);
    g_prof_on = on != 0;
    return BRX_OK;
}

int brx_profile_reset(void)
{
    std::lock_guard<std::mutex> g(g_tmu);
    for (auto &s : g_slots) {
        resolve(s);
        s.total_ms = 0;
        s.launches = 0;
    }
    return BRX_OK;
}

int brx_profile_get(const char *kernel, double *total_ms, uint64_t *launches)
{
    if (!kernel)
        return BRX_ERR_ARG;
    std::lock_guard<std::mutex> g(g_tmu);
    for (auto &s : g_slots)
        if (s.name == kernel) {
            resolve(s);
            if (total_ms)
                *total_ms = s.total_ms;
            if (launches)
                *launches = s.launches;
            return BRX_OK;
        }
    if (total_ms)
        *total_ms = 0;
    if (launches)
        *launches = 0;
    return BRX_OK;
}

int brx_profile_names(char *buf, size_t cap)
{
    if (!buf || cap == 0)
        return BRX_ERR_ARG;
    std::lock_guard<std::mutex> g(g_tmu);
    std::string s;
    for (auto &t : g_slots) {
        if (!s.empty())
            s += ",";
        s += t.name;
    }
    snprintf(buf, cap, "%s", s.c_str());
    return BRX_OK;
}

// ---- abundance (include/brx.h "abundance"; the kernels are in brx_abundance.hip) ---------------------------------------
static int abund_check(const char *what, const brx_counter_t *c, const void *bases, const uint64_t *offsets, uint32_t n_reads,
                       uint64_t total_bases)
{
    if (!c) {
        set_error("%s: null counter", what);
        return BRX_ERR_ARG;
    }
    if (c->strategy == BRX_COUNT_SORTED && !part_lookup_ready(c))
        return abund_refuse_partitioned(what, c->k);
    return check_batch_args(what, bases, offsets, n_reads, total_bases);
}

// the body of both batch entries; the caller holds c->mu
static int abund_batch_locked(brx_counter_t *c, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads, uint64_t total_bases,
                              uint8_t abundance, uint8_t *d_profile, uint32_t *d_hist, brx_abund_stats_t *d_stats, hipStream_t s)
{
    bool done = false;
    BRX_TRY(abund_empty_batch(n_reads, total_bases, d_profile, d_hist, d_stats, s, &done));
    return done ? BRX_OK : abund_batch(c, d_bases, d_offsets, n_reads, total_bases, abundance, d_profile, d_hist, d_stats, s);
}

int brx_counter_abundance_batch_device(brx_counter_t *c, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads,
                                       uint64_t total_bases, uint8_t abundance, uint8_t *d_profile, uint32_t *d_hist,
                                       brx_abund_stats_t *d_stats, void *stream)
{
    BRX_TRY(abund_check("brx_counter_abundance_batch_device", c, d_bases, d_offsets, n_reads, total_bases));
    BRX_TRY(use_device(c->device));
    std::lock_guard<std::mutex> g(c->mu);
    BRX_TRY(abund_batch_locked(c, d_bases, d_offsets, n_reads, total_bases, abundance, d_profile, d_hist, d_stats, (hipStream_t)stream));
    BRX_HIP(counter_mark(c, (hipStream_t)stream)); // (the counts are still being read on `stream`)
    return BRX_OK;
}

int brx_counter_abundance_batch(brx_counter_t *c, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                                uint8_t abundance, uint8_t *profile, uint32_t *hist, brx_abund_stats_t *stats)
{
    const char *me = "brx_counter_abundance_batch";
    if (n_reads && !offsets) {
        set_error("%s: null offsets", me);
        return BRX_ERR_ARG;
    }
    const uint64_t total = n_reads ? offsets[n_reads] : 0;
    BRX_TRY(abund_check(me, c, bases, offsets, n_reads, total));
    BRX_TRY(check_offsets(me, offsets, n_reads));
    BRX_TRY(use_device(c->device));
    if (!n_reads || (!profile && !hist && !stats))
        return BRX_OK;
    std::lock_guard<std::mutex> g(c->mu);
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
    hipStream_t s = c->stream;
    BRX_HIP(counter_join(c, c->stream));
    auto run = [&]() -> int {
        if (total)
            BRX_HIP(hipMemcpyAsync(d_bases, bases, total, hipMemcpyHostToDevice, s));
        BRX_HIP(hipMemcpyAsync(d_off, offsets, ((uint64_t)n_reads + 1) * 8, hipMemcpyHostToDevice, s));
        BRX_TRY(abund_batch_locked(c, d_bases, d_off, n_reads, total, abundance, d_profile, d_hist, d_stats, s));
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

int brx_counter_get_counts(brx_counter_t *c, const uint64_t *forward_kmers, uint32_t n, uint8_t *out)
{
    const char *me = "brx_counter_get_counts";
    BRX_TRY(abund_check(me, c, nullptr, nullptr, 0, 0));
    if ((!forward_kmers || !out) && n) {
        set_error("%s: null k-mers / out", me);
        return BRX_ERR_ARG;
    }
    BRX_TRY(use_device(c->device));
    if (!n)
        return BRX_OK;
    std::lock_guard<std::mutex> g(c->mu);
    DevScratch sc;
    uint64_t *d_k = nullptr;
    uint8_t *d_o = nullptr;
    BRX_TRY(sc.get(&d_k, n));
    BRX_TRY(sc.get(&d_o, n));
    hipStream_t s = c->stream;
    BRX_HIP(counter_join(c, c->stream));
    auto run = [&]() -> int {
        BRX_HIP(hipMemcpyAsync(d_k, forward_kmers, (uint64_t)n * 8, hipMemcpyHostToDevice, s));
        BRX_TRY(abund_get_counts(c, d_k, n, d_o, s));
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

int brx_counter_lookup_prepare(brx_counter_t *c, void *stream)
{
    if (!c) {
        set_error("brx_counter_lookup_prepare: null counter");
        return BRX_ERR_ARG;
    }
    if (c->strategy != BRX_COUNT_SORTED)
        return BRX_OK; // dense / table: the counts are where a lookup reads them
    BRX_TRY(use_device(c->device));
    std::lock_guard<std::mutex> g(c->mu);
    return part_lookup_prepare(c, (hipStream_t)stream);
}

int brx_counter_lookup_state(brx_counter_t *c, int *state)
{
    if (!c || !state) {
        set_error("brx_counter_lookup_state: null counter / state");
        return BRX_ERR_ARG;
    }
    std::lock_guard<std::mutex> g(c->mu);
    *state = c->strategy != BRX_COUNT_SORTED || part_lookup_ready(c) ? 1 : 0;
    return BRX_OK;
}

int brx_counter_lookup_drop(brx_counter_t *c)
{
    if (!c) {
        set_error("brx_counter_lookup_drop: null counter");
        return BRX_ERR_ARG;
    }
    if (c->strategy != BRX_COUNT_SORTED)
        return BRX_OK;
    BRX_TRY(use_device(c->device));
    std::lock_guard<std::mutex> g(c->mu);
    part_lookup_drop(c);
    return BRX_OK;
}

void brx_buf_free(void *p) { brx::host_buf_release(p); }

void *brx_host_alloc(size_t bytes) { return brx::host_buf_acquire(bytes ? bytes : 1); }

void brx_host_free(void *p) { brx::host_buf_release(p); }
void brx_devpool_trim(void) { brx::dev_pool_trim(); }
uint64_t brx_devpool_bytes(void) { return (uint64_t)brx::dev_pool_bytes(); }

} // extern "C"
