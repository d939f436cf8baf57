// Probe index of a solid set: build + test entry points (layout and probe in brx_index.hpp).
#include "brx_internal.hpp"
#include "brx_index.hpp"

#include <stdio.h>
#include <stdlib.h>

#include <rocprim/device/device_radix_sort.hpp>

using namespace brx;

namespace {

// the line a key's minimizer addresses (key = canonical >> 1, as the key lists hold it)
__device__ __forceinline__ uint32_t key_home_line(uint64_t h, uint32_t line_shift, uint32_t m, uint32_t w, int k)
{
    const uint64_t canon = (h << 1) | (uint64_t)(popc64(h) & 1); // even popcount (brx_kmer.hpp)
    return index_line_of(minimizer_of(canon, revcomp(canon, k), m, w), line_shift);
}

// one key per thread: claim a slot of the key's line; a full line is flagged as overflowed and the key is
// left to the bit vector (CHAIN = false) or goes on to the next line (CHAIN = true: sparse sets)
// `cont_lines` (with the number of keys in *n_dev, at most n): the keys whose chain left its region in index_lines_kernel
// go on at the line given there; they were counted, and left their signature, before they left
template <bool CHAIN>
__global__ __launch_bounds__(256) void index_insert_kernel(const uint64_t *__restrict__ keys, uint64_t n, uint64_t *__restrict__ lines,
                                                           uint32_t line_shift, uint32_t m, uint32_t w, int k,
                                                           unsigned long long *__restrict__ n_overflow, uint32_t *__restrict__ line_bits,
                                                           const uint32_t *__restrict__ cont_lines = nullptr,
                                                           const unsigned long long *__restrict__ n_dev = nullptr)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t line_mask = 0xffffffffu >> line_shift;
    uint32_t lost = 0;
    if (n_dev && *n_dev < n)
        n = *n_dev;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t h = keys[i];
        uint32_t line = cont_lines ? cont_lines[i] : key_home_line(h, line_shift, m, w, k);
        bool counted = cont_lines != nullptr;
        // a chained walk visits at most every line once (the host checks that the table has room for its keys;
        // this bound keeps a mis-sized table from spinning the GPU for ever: the key is then simply lost and counted)
        for (uint32_t walked = 0; walked <= line_mask; walked++) {
            unsigned long long *L = reinterpret_cast<unsigned long long *>(lines) + (uint64_t)line * 8ull;
            const unsigned long long seen = __hip_atomic_load(L + 7, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            uint32_t slot = IDX_SLOTS;
            if ((uint32_t)seen < (uint32_t)IDX_SLOTS) // full lines are not counted further: the counter stays small
                slot = (uint32_t)atomicAdd(L + 7, 1ull);
            if (slot < (uint32_t)IDX_SLOTS) {
                L[slot] = h + 1ull;
                if (slot == 0u) // the line's first key: mark the line as occupied (brx_index.hpp: line_bits)
                    atomicOr(line_bits + (line >> 5), 1u << (line & 31u));
                break;
            }
            {   // flag the line; at the key's home line also leave the key's signature bit
                const unsigned long long want = (unsigned long long)IDX_OVERFLOW | (counted ? 0ull : (unsigned long long)idx_sig_bit(h + 1ull));
                if ((seen & want) != want)
                    atomicOr(L + 7, want);
            }
            if (!counted) {
                lost++;
                counted = true;
            }
            if (!CHAIN)
                break;
            line = (line + 1u) & line_mask; // the table has more slots than keys: this ends
        }
    }
    for (int d = 32; d > 0; d >>= 1)
        lost += __shfl_down(lost, d);
    if ((threadIdx.x & 63) == 0 && lost)
        atomicAdd(n_overflow, (unsigned long long)lost);
}

// ---- the build by regions: keys ordered by region, every region's lines put together in LDS and written once -----------
// A region is a run of 2^region_log consecutive lines (a smaller table is one region).
#ifndef BRX_INDEX_REGION_LOG
#define BRX_INDEX_REGION_LOG 10 // 1024 lines: 64 KiB of LDS, two blocks per CU
#endif
#ifndef BRX_INDEX_LINES_THREADS
#define BRX_INDEX_LINES_THREADS 512
#endif
#ifndef BRX_INDEX_ORDER_PAIRS
#define BRX_INDEX_ORDER_PAIRS 0 // 1: (region, key) pairs also where the region fits above the key (the measured comparison)
#endif
#ifndef BRX_INDEX_NT_STORE
#define BRX_INDEX_NT_STORE 1 // the lines go out with non-temporal stores: nobody reads them before the table is whole (0.455 against 0.494 ms)
#endif
constexpr uint32_t IDX_REGION_LOG = BRX_INDEX_REGION_LOG;
constexpr uint32_t IDX_LINES_THREADS = BRX_INDEX_LINES_THREADS;
static_assert(IDX_REGION_LOG >= 6 && IDX_REGION_LOG <= 11, "a region's image must fit the LDS of a CU");
static_assert(IDX_LINES_THREADS % 64 == 0 && IDX_LINES_THREADS <= 1024, "whole waves");

// What the sort orders by: the region of every key's home line.  Where the key's 2k - 1 bits leave room in the word, the
// region goes on top of the key (`packed`, key_bits up) and the sort moves one 8-byte word per key; else it is a 32-bit
// sort key of its own (`region_of`) and the key travels as the pair's value, 12 bytes per key.
__global__ __launch_bounds__(256) void index_region_of_kernel(const uint64_t *__restrict__ keys, uint32_t n, uint32_t line_shift, uint32_t m,
                                                              uint32_t w, int k, uint32_t region_log, uint32_t *__restrict__ region_of,
                                                              uint64_t *__restrict__ packed, uint32_t key_bits)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t h = keys[i];
        const uint32_t region = key_home_line(h, line_shift, m, w, k) >> region_log;
        if (packed)
            packed[i] = ((uint64_t)region << key_bits) | (h & ((1ull << key_bits) - 1ull));
        else
            region_of[i] = region;
    }
}

// first[r] = index of the first key of region r in the sorted list, first[n_regions] = n (neither list: one region)
__global__ __launch_bounds__(256) void index_region_first_kernel(const uint32_t *__restrict__ sorted, const uint64_t *__restrict__ packed,
                                                                 uint32_t key_bits, uint32_t n, uint32_t n_regions,
                                                                 uint32_t *__restrict__ first)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    auto region_at = [&](uint64_t i) { return packed ? (uint32_t)(packed[i] >> key_bits) : (sorted ? sorted[i] : 0u); };
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += stride) {
        const uint32_t lo = i == 0 ? 0u : region_at(i - 1) + 1u;
        uint32_t hi = i == n ? n_regions : region_at(i);
        if (hi > n_regions) // (cannot be: a line number has log2(lines) bits)
            hi = n_regions;
        for (uint32_t r = lo; r <= hi; r++)
            first[r] = (uint32_t)i;
    }
}

// One block per region at a time.  index_insert_kernel's algorithm against the region's image in LDS, then the image
// goes out in 16-byte stores and the region's occupancy bits with it: every byte of the table, of the bits and of the
// spare bytes behind them is written exactly once, and nothing is read.  A chain that walks out of its region is handed to
// index_insert_kernel<true> (cont_keys / cont_lines), which runs when the whole table stands.
template <bool CHAIN>
__global__ __launch_bounds__(IDX_LINES_THREADS) void index_lines_kernel(const uint64_t *__restrict__ keys, uint64_t key_mask,
                                                                        const uint32_t *__restrict__ first, uint32_t n_regions, uint32_t region_log, uint64_t *__restrict__ lines,
                                                                        uint32_t line_shift, uint32_t m, uint32_t w, int k,
                                                                        unsigned long long *__restrict__ n_overflow,
                                                                        uint32_t *__restrict__ line_bits, uint64_t *__restrict__ cont_keys,
                                                                        uint32_t *__restrict__ cont_lines, unsigned long long *__restrict__ n_cont,
                                                                        uint64_t cont_cap)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long img[]; // 8 words per line of the region
    const uint32_t rlines = 1u << region_log;
    const uint32_t line_mask = 0xffffffffu >> line_shift;
    uint4 *img4 = reinterpret_cast<uint4 *>(img);
    uint32_t lost = 0;
    for (uint32_t r = blockIdx.x; r < n_regions; r += gridDim.x) {
        for (uint32_t i = threadIdx.x; i < rlines * 4u; i += IDX_LINES_THREADS)
            img4[i] = make_uint4(0u, 0u, 0u, 0u);
        __syncthreads();
        const uint32_t base = r << region_log;
        const uint32_t end = first[r + 1];
        for (uint32_t i = first[r] + threadIdx.x; i < end; i += IDX_LINES_THREADS) {
            const uint64_t h = keys[i] & key_mask; // (the ordered list may carry the region above the key)
            uint32_t ll = (key_home_line(h, line_shift, m, w, k) - base) & (rlines - 1u); // (the mask: never outside the image)
            bool counted = false;
            for (;;) {
                unsigned long long *L = img + ll * 8u;
                const unsigned long long seen = __hip_atomic_load(L + 7, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                uint32_t slot = IDX_SLOTS;
                if ((uint32_t)seen < (uint32_t)IDX_SLOTS)
                    slot = (uint32_t)__hip_atomic_fetch_add(L + 7, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (slot < (uint32_t)IDX_SLOTS) {
                    L[slot] = h + 1ull;
                    break;
                }
                {
                    const unsigned long long want = (unsigned long long)IDX_OVERFLOW | (counted ? 0ull : (unsigned long long)idx_sig_bit(h + 1ull));
                    if ((seen & want) != want)
                        (void)__hip_atomic_fetch_or(L + 7, want, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                if (!counted) {
                    lost++;
                    counted = true;
                }
                if (!CHAIN)
                    break;
                if (++ll == rlines) { // the chain leaves the region (the last line of the table goes on at line 0)
                    const unsigned long long at = atomicAdd(n_cont, 1ull);
                    if (at < cont_cap) { // (more than the list holds: the host sees the count and builds the old way)
                        cont_keys[at] = h;
                        cont_lines[at] = (base + rlines) & line_mask;
                    }
                    break;
                }
            }
        }
        __syncthreads();
        uint4 *out = reinterpret_cast<uint4 *>(lines + (uint64_t)base * 8ull);
        for (uint32_t i = threadIdx.x; i < rlines * 4u; i += IDX_LINES_THREADS) {
#if BRX_INDEX_NT_STORE
            typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
            __builtin_nontemporal_store(reinterpret_cast<const u32x4 *>(img4)[i], reinterpret_cast<u32x4 *>(out) + i);
#else
            out[i] = img4[i];
#endif
        }
        // occupancy bits, one per line that holds a key: a wave's ballot is the bits of 64 lines
        if (rlines >= 64u) {
            for (uint32_t l = threadIdx.x; l < rlines; l += IDX_LINES_THREADS) { // (wave-uniform trip count)
                const unsigned long long b = __ballot((uint32_t)img[l * 8u + 7u] != 0u);
                if ((threadIdx.x & 63u) == 0u)
                    reinterpret_cast<unsigned long long *>(line_bits)[(base + l) >> 6] = b;
            }
        } else if (threadIdx.x < 64u) { // a table of 16 or 32 lines (it is its only region)
            const unsigned long long b = __ballot(threadIdx.x < rlines && (uint32_t)img[(threadIdx.x & (rlines - 1u)) * 8u + 7u] != 0u);
            if (threadIdx.x == 0u) {
                if (rlines == 32u)
                    line_bits[0] = (uint32_t)b;
                else
                    reinterpret_cast<uint16_t *>(line_bits)[0] = (uint16_t)b;
            }
        }
        if (r == n_regions - 1u && threadIdx.x < 64u) // the 64 spare bytes behind the bits
            reinterpret_cast<uint8_t *>(line_bits)[(((uint64_t)line_mask + 1ull) >> 3) + threadIdx.x] = 0;
        __syncthreads(); // the image is zeroed again for the block's next region
    }
    for (int d = 32; d > 0; d >>= 1)
        lost += __shfl_down(lost, d);
    if ((threadIdx.x & 63) == 0 && lost)
        atomicAdd(n_overflow, (unsigned long long)lost);
}

__global__ void index_get_kernel(IdxView v, const uint32_t *__restrict__ bits, const uint64_t *__restrict__ kmers, uint32_t n, int k,
                                 uint8_t *__restrict__ out, unsigned long long *__restrict__ n_fallback)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const uint64_t fwd = kmers[i] & kmask(k);
    int home = 0;
    out[i] = set_get<true, LINE_BITS_NEVER, true>(v, bits, fwd, k, &home) ? 1 : 0;
    if (home == 2) // the home line could not say: the bit vector or the chain did
        atomicAdd(n_fallback, 1ull);
}

// moves every key of one table into another (growing an insert-built set)
__global__ __launch_bounds__(256) void table_rehash_kernel(KeySource old, int k, uint64_t *__restrict__ lines, uint32_t line_shift, uint32_t m,
                                                           uint32_t w)
{
    for_each_key(old, [&](uint64_t h) { (void)table_find_or_insert(lines, line_shift, m, w, k, (h << 1) | (uint64_t)(popc64(h) & 1)); });
}

// ORs the keys of a list or of a table into a bit vector (materialising a lazy one; brx_set_or_keys_device)
__global__ __launch_bounds__(256) void or_keys_kernel(KeySource src, uint32_t *__restrict__ bits, uint64_t nbits)
{
    for_each_key(src, [&](uint64_t h) { if (h < nbits) atomicOr(bits + (h >> 5), 1u << (h & 31u)); });
}

int env_int(const char *name, int dflt)
{
    const char *e = getenv(name);
    return (e && *e) ? atoi(e) : dflt;
}

} // namespace

namespace brx {

// (the occupancy bits lie behind the lines, in the same allocation)
SetView set_view(const brx_set *set, bool line_bits, bool any_index)
{
    SetView v{no_bits(set) ? nullptr : set->d_bits.get(), IdxView{nullptr, 0, 0, 0}};
    if (set->idx_valid && (any_index || index_wanted(set->k) || no_bits(set)))
        v.idx = IdxView{set->d_lines, 32u - set->idx_log_lines, set->idx_m, (uint32_t)set->k - set->idx_m + 1u,
                        line_bits && set->idx_linebits ? (const uint32_t *)(set->d_lines + (8ull << set->idx_log_lines)) : nullptr};
    return v;
}

// who holds the keys (brx_internal.hpp: SetKeys): the list's counter read once, the rule asked once
int set_keys_locked(const brx_set *set, hipStream_t s, SetKeys *out)
{
    *out = SetKeys{};
    out->list_cap = set->d_keylist.cap();
    if (set->keylist_valid) {
        BRX_TRY(use_device(set->device));
        unsigned long long nl = 0;
        BRX_HIP(hipMemcpyAsync(&nl, set->d_keylist_n, 8, hipMemcpyDeviceToHost, s));
        BRX_HIP(hipStreamSynchronize(s));
        out->listed_n = nl;
    }
    out->holder = set_holder(set->sparse, set->bits_stale, set->keylist_valid, out->listed_n, out->list_cap, set->idx_valid, set->idx_exact,
                             set->d_lines.get() != nullptr);
    if (out->holder == SetHolder::KeyList)
        out->src = list_source(set->d_keylist, out->listed_n);
    else if (out->holder == SetHolder::Table)
        out->src = table_source(set->d_lines, 1ull << set->idx_log_lines);
    else if (out->holder == SetHolder::Bits)
        out->src = bits_source(set->d_bits, set->nwords);
    out->sorted = out->holder == SetHolder::KeyList && set->keylist_sorted;
    out->table_keys = set->idx_keys;
    return BRX_OK;
}

int set_keys(const brx_set *set, hipStream_t s, SetKeys *out)
{
    std::lock_guard<std::mutex> g(const_cast<brx_set *>(set)->idx_mu);
    return set_keys_locked(set, s, out);
}

// the keys of a set, whatever holds it, into d_out, in the holder's order; a lazy bit vector stays lazy.  *sorted (may be
// null): the keys are known to ascend strictly -- they are a key list that says so.  The copy is left queued on `s`.
int set_list_keys(const brx_set *set, hipStream_t s, DevBuf<uint64_t> &d_out, uint64_t *n_out, bool *sorted)
{
    d_out.reset();
    *n_out = 0;
    {
        std::lock_guard<std::mutex> g(const_cast<brx_set *>(set)->idx_mu);
        SetKeys keys;
        const int st = set_keys_locked(set, s, &keys);
        if (sorted)
            *sorted = keys.sorted;
        BRX_TRY(st);
        if (keys.holder == SetHolder::KeyList) {
            if (keys.src.n) {
                BRX_TRY(d_out.reserve(keys.src.n, 0, "keys of the set"));
                KernelTimer kt("key_list", s);
                BRX_HIP(hipMemcpyAsync(d_out, keys.src.keys, keys.src.n * 8, hipMemcpyDeviceToDevice, s));
            }
            *n_out = keys.src.n;
            return BRX_OK;
        }
        if (keys.holder == SetHolder::None) {
            set_error("brx_set_save_fd: the set has neither a bit vector, nor a key list, nor a table");
            return BRX_ERR_UNSUPPORTED;
        }
        if (keys.holder == SetHolder::Table) {
            const uint64_t cap = keys.table_keys;
            if (!cap)
                return BRX_OK;
            DevBuf<unsigned long long> d_n;
            BRX_TRY(d_n.reserve(1, 0, "keys of the set"));
            BRX_HIP(hipMemsetAsync(d_n, 0, 8, s));
            BRX_TRY(d_out.reserve(cap, 0, "keys of the set"));
            BRX_TRY(table_list(keys.src.lines, nullptr, keys.src.n_entries, 1u, d_out, nullptr, cap, d_n, s));
            unsigned long long got = 0;
            BRX_HIP(hipMemcpyAsync(&got, d_n, 8, hipMemcpyDeviceToHost, s));
            BRX_HIP(hipStreamSynchronize(s));
            if (got != cap) {
                set_error("brx_set_save_fd: %llu keys in the table of a set of %llu", got, (unsigned long long)cap);
                return BRX_ERR_HIP;
            }
            *n_out = got;
            return BRX_OK;
        }
    }
    KernelTimer kt("key_list", s);
    return keys_from_bits(set, s, d_out, n_out);
}

bool index_wanted(int k)
{
    if (sparse_k(k))
        return true; // nothing else to probe

    // below k = 15 the whole bitset (<= 4 MiB at k = 13) lives in every XCD's L2 and a plain probe is cheaper
    // (BRX_INDEX_MIN_K lowers the threshold: the parity tests run every corrector through the index at small k)
    return (k & 1) && k >= env_int("BRX_INDEX_MIN_K", 15) && k >= 5 && env_int("BRX_INDEX", 1) != 0;
}

// smallest odd m whose 4^m / 2 canonical m-mers outnumber the keys 16 to 1 (a minimizer shared by many
// genome positions piles all their k-mers into one line), at least 2 windows
int index_auto_m(int k, uint64_t n_keys)
{
    int m = 3;
    while (m < IDX_AUTO_MAX_M && (1ull << (2 * m - 1)) < 16ull * n_keys)
        m += 2;
    // beyond 2^25 keys even the 15-mers (2^29 canonical ones) are fewer than 16 per key: 16-mers (the longest a 32-bit
    // window holds; no masking in the probe either).  Measured at 0.96 G keys (k = 19): 34 % of the keys overflow their
    // line with m = 15, 14 % with m = 16, and a correction pass takes 231 ms instead of 428 (2^28 lines both).
    if (m == IDX_AUTO_MAX_M && (1ull << (2 * IDX_AUTO_MAX_M - 1)) < 16ull * n_keys && k - IDX_MAX_M + 1 >= 3)
        return IDX_MAX_M;
    if (m > k - 2)
        m = k - 2;
    if (!(m & 1))
        m--;
    return m < 3 ? 3 : m;
}

// The build by regions, queued on `s`: order the keys by the region of their home line, put every region's lines
// together in LDS (index_lines_kernel), then place the few keys whose chain left its region.  `done` stays false, and
// nothing is queued, when the scratch (16 bytes per key for the word that is sorted and the ordered list, 24 where the
// region does not fit above the key; the sort's own workspace) cannot be had.  `scratch` must live until the stream
// has run all this.  d_counts[0] gets the keys turned away by their home line, d_counts[1] the keys that left their
// region: above `cont_cap` the list did not hold them all and the table is incomplete.
// An error return may leave kernels queued that use `scratch` and d_counts: the caller waits for the stream before it
// lets go of them.
static int index_build_regions(const uint64_t *d_keys, uint64_t n, uint64_t *d_lines, int log_lines, uint32_t m, uint32_t w, int k, bool chain,
                               unsigned long long *d_counts, hipStream_t s, DevBuf<uint8_t> &scratch, bool &done, uint64_t &cont_cap)
{
    done = false;
    if (n >= (1ull << 31))
        return BRX_OK; // 32-bit positions in the ordered list
    const uint32_t line_shift = 32u - (uint32_t)log_lines;
    const uint32_t region_log = (uint32_t)log_lines < IDX_REGION_LOG ? (uint32_t)log_lines : IDX_REGION_LOG;
    const uint32_t sort_bits = (uint32_t)log_lines - region_log;
    const uint32_t n_regions = 1u << sort_bits;
    const uint64_t n_lines = 1ull << log_lines;
    cont_cap = chain ? n / 8ull + 4096ull : 0ull;

    const bool ordered = sort_bits && n;
    const uint32_t key_bits = 2u * (uint32_t)k - 1u;
    const bool pack = ordered && key_bits + sort_bits <= 64u && !BRX_INDEX_ORDER_PAIRS;
    size_t sort_bytes = 0;
    if (pack)
        BRX_HIP(rocprim::radix_sort_keys(nullptr, sort_bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t)n, key_bits,
                                         key_bits + sort_bits, s));
    else if (ordered)
        BRX_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr, d_keys, (uint64_t *)nullptr,
                                          (uint32_t)n, 0u, sort_bits, s));
    auto up = [](uint64_t b) { return (b + 255ull) & ~255ull; };
    const uint64_t o_first = 0, o_ckeys = o_first + up(((uint64_t)n_regions + 1ull) * 4ull), o_clines = o_ckeys + up(cont_cap * 8ull),
                   o_sorted = o_clines + up(cont_cap * 4ull), o_rin = o_sorted + up(ordered ? n * 8ull : 0ull),
                   o_rout = o_rin + up(!ordered ? 0ull : pack ? n * 8ull : n * 4ull), o_tmp = o_rout + up(ordered && !pack ? n * 4ull : 0ull),
                   total = o_tmp + up(sort_bytes);
    {
        // BRX_INDEX_SCRATCH_PAD_GB (tests): ask for that much more than needed, so that the runtime really refuses the block
        const uint64_t pad = (uint64_t)env_int("BRX_INDEX_SCRATCH_PAD_GB", 0) << 30;
        void *p = nullptr;
        if (dev_alloc(&p, total + pad) != hipSuccess) {
            // not an error of this call: the build goes the old way.  The runtime keeps the refusal as the thread's last error
            // until somebody reads it, and the next launch that asks hipGetLastError would take it for its own.
            (void)hipGetLastError();
            return BRX_OK;
        }
        scratch.adopt((uint8_t *)p, total + pad);
    }
    uint32_t *const first = (uint32_t *)(scratch + o_first);
    uint64_t *const cont_keys = (uint64_t *)(scratch + o_ckeys);
    uint32_t *const cont_lines = (uint32_t *)(scratch + o_clines);
    uint64_t *const sorted = (uint64_t *)(scratch + o_sorted);
    uint32_t *const rin = (uint32_t *)(scratch + o_rin), *const rout = (uint32_t *)(scratch + o_rout);
    uint32_t *const line_bits = (uint32_t *)(d_lines + n_lines * 8ull);
    {
        KernelTimer t("index_sort", s);
        if (ordered) {
            uint32_t blocks = (uint32_t)((n + 255) / 256);
            index_region_of_kernel<<<blocks > 4096u ? 4096u : blocks, 256, 0, s>>>(d_keys, (uint32_t)n, line_shift, m, w, k, region_log, rin,
                                                                                   pack ? (uint64_t *)rin : nullptr, key_bits);
            BRX_HIP(hipGetLastError());
            if (pack) // (`rin` has 8 bytes per key then, and the ordered words land in `sorted`)
                BRX_HIP(rocprim::radix_sort_keys(scratch + o_tmp, sort_bytes, (const uint64_t *)rin, sorted, (uint32_t)n, key_bits,
                                                 key_bits + sort_bits, s));
            else
                BRX_HIP(rocprim::radix_sort_pairs(scratch + o_tmp, sort_bytes, (const uint32_t *)rin, rout, d_keys, sorted, (uint32_t)n, 0u,
                                                  sort_bits, s));
        }
        uint32_t blocks = (uint32_t)((n + 256) / 256);
        index_region_first_kernel<<<blocks > 4096u ? 4096u : blocks, 256, 0, s>>>(ordered && !pack ? rout : nullptr, pack ? sorted : nullptr,
                                                                                  key_bits, (uint32_t)n, n_regions, first);
        BRX_HIP(hipGetLastError());
    }
    {
        KernelTimer t("index_lines", s);
        const uint32_t lds = 64u << region_log;
        const uint32_t grid = n_regions < 2048u ? n_regions : 2048u;
        const uint64_t *const in = ordered ? sorted : d_keys;
        const uint64_t key_mask = pack ? (1ull << key_bits) - 1ull : ~0ull;
        if (lds > 65536u) {
            BRX_HIP(hipFuncSetAttribute((const void *)index_lines_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            BRX_HIP(hipFuncSetAttribute((const void *)index_lines_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        }
        if (chain)
            index_lines_kernel<true><<<grid, IDX_LINES_THREADS, lds, s>>>(in, key_mask, first, n_regions, region_log, d_lines, line_shift, m, w, k, d_counts,
                                                                         line_bits, cont_keys, cont_lines, d_counts + 1, cont_cap);
        else
            index_lines_kernel<false><<<grid, IDX_LINES_THREADS, lds, s>>>(in, key_mask, first, n_regions, region_log, d_lines, line_shift, m, w, k, d_counts,
                                                                          line_bits, nullptr, nullptr, d_counts + 1, 0);
        BRX_HIP(hipGetLastError());
    }
    if (chain && n) {
        KernelTimer t("index_insert", s);
        const uint64_t blocks = (cont_cap + 255) / 256;
        index_insert_kernel<true><<<(int)(blocks > 1024 ? 1024 : blocks), 256, 0, s>>>(cont_keys, cont_cap, d_lines, line_shift, m, w, k, d_counts,
                                                                                       line_bits, cont_lines, d_counts + 1);
        BRX_HIP(hipGetLastError());
    }
    done = true;
    return BRX_OK;
}

static int index_build_locked(brx_set *set, const uint64_t *d_keys, uint64_t n, int m, int log_lines, hipStream_t s)
{
    const int k = set->k;
    if (!(k & 1) || k < 5 || k > 31) {
        set_error("probe index needs odd 5 <= k <= 31 (k=%d)", k);
        return BRX_ERR_UNSUPPORTED;
    }
    BRX_TRY(use_device(set->device));
    if (m <= 0)
        m = env_int("BRX_INDEX_M", 0);
    if (m <= 0)
        m = index_auto_m(k, n);
    if ((!(m & 1) && m != 16) || m < 3 || m > IDX_MAX_M || k - m + 1 < 2) {
        set_error("probe index: minimizer length %d must be odd (or 16), 3..%d and shorter than the %d-mer", m, IDX_MAX_M, k);
        return BRX_ERR_ARG;
    }
    if (log_lines <= 0)
        log_lines = env_int("BRX_INDEX_LOG_LINES", 0);
    if (log_lines <= 0) {
        // about one key per 7-slot line: a minimizer brings up to k-m+1 keys at once, and a line that
        // overflows costs its probes a second round
        log_lines = 10;
        while (log_lines < 29 && (1ull << log_lines) < n + n / 2) // (2^29 lines = 32 GiB; 0.96 G keys: 166 ms per pass against 231 at 2^28)
            log_lines++;
    }
    while (no_bits(set) && log_lines < 30 && (7ull << log_lines) < n + n / 4)
        log_lines++; // a chained table must have room for every key
    if (log_lines < 4 || log_lines > 30) {
        set_error("probe index: log2(lines)=%d out of range 4..30", log_lines);
        return BRX_ERR_ARG;
    }
    if (no_bits(set) && (7ull << log_lines) < n + n / 4) {
        // a chained table that cannot hold its keys would send index_insert_kernel<true> round the table for ever
        set_error("set without bit vector: %llu solid k-mers do not fit a chained table of 2^%d lines (7 slots each)",
                  (unsigned long long)n, log_lines);
        return BRX_ERR_NOMEM;
    }
    set->idx_valid = false;
    set->idx_gen++;
    const uint64_t n_lines = 1ull << log_lines;
    if (set->lines_alloc < n_lines) {
        set->d_lines.reset();
        set->lines_alloc = 0;
        BRX_TRY(set->d_lines.reserve_bytes(n_lines * 64ull + n_lines / 8ull + 64ull, 0, "probe index")); // lines + occupancy bits
        set->lines_alloc = n_lines;
    }
    DevBuf<unsigned long long> d_ovf; // [0] keys turned away by their home line, [1] keys whose chain left its region
    BRX_TRY(d_ovf.reserve(2, 0, "probe index build"));
    BRX_HIP(hipMemsetAsync(d_ovf, 0, 16, s));
    uint32_t *const line_bits = (uint32_t *)(set->d_lines + n_lines * 8ull);
    const uint32_t line_shift = 32u - (uint32_t)log_lines, w = (uint32_t)(k - m + 1);
    unsigned long long ovf[2] = {0, 0};
    bool by_regions = false;
    uint64_t cont_cap = 0;
    DevBuf<uint8_t> scratch; // (freed behind the synchronisation below)
    const bool want_regions = env_int("BRX_INDEX_BUILD", 1) != 0;
    if (want_regions) {
        const int st = index_build_regions(d_keys, n, set->d_lines, log_lines, (uint32_t)m, w, k, no_bits(set), d_ovf, s, scratch, by_regions, cont_cap);
        if (st != BRX_OK) {
            (void)hipStreamSynchronize(s); // (kernels already queued may still use `scratch` and d_ovf)
            return st;
        }
    }
    if (by_regions) {
        BRX_HIP(hipMemcpyAsync(ovf, d_ovf, 16, hipMemcpyDeviceToHost, s));
        BRX_HIP(hipStreamSynchronize(s));
        if (ovf[1] > cont_cap) { // more chains left their regions than the list holds: the table lacks those keys
            by_regions = false;
            BRX_HIP(hipMemsetAsync(d_ovf, 0, 16, s));
        } else if (env_int("BRX_INDEX_TRACE", 0)) {
            fprintf(stderr, "brx index build: 2^%d lines, %llu keys, %llu turned away by their home line, %llu left their region\n",
                    log_lines, (unsigned long long)n, ovf[0], ovf[1]);
        }
    }
    if (!by_regions) { // BRX_INDEX_BUILD=0, or no scratch for the ordered keys: clear the table, then one key at a time
        {
            KernelTimer t("index_zero", s);
            BRX_HIP(hipMemsetAsync(set->d_lines, 0, n_lines * 64ull + n_lines / 8ull + 64ull, s));
        }
        if (n) {
            KernelTimer t("index_insert", s);
            uint64_t blocks = (n + 255) / 256;
            if (blocks > 256 * 16)
                blocks = 256 * 16;
            if (no_bits(set))
                index_insert_kernel<true><<<(int)blocks, 256, 0, s>>>(d_keys, n, set->d_lines, line_shift, (uint32_t)m, w, k, d_ovf, line_bits);
            else
                index_insert_kernel<false><<<(int)blocks, 256, 0, s>>>(d_keys, n, set->d_lines, line_shift, (uint32_t)m, w, k, d_ovf, line_bits);
            BRX_HIP(hipGetLastError());
        }
        BRX_HIP(hipMemcpyAsync(ovf, d_ovf, 8, hipMemcpyDeviceToHost, s));
        BRX_HIP(hipStreamSynchronize(s));
    }
    set->idx_log_lines = (uint32_t)log_lines;
    set->idx_m = (uint32_t)m;
    set->idx_keys = n;
    set->idx_overflow_keys = ovf[0];
    index_mark(set, no_bits(set), false, true); // closed; this build filled the occupancy bits behind the lines
    return BRX_OK;
}

int index_build_from_keys(brx_set *set, const uint64_t *d_keys, uint64_t n, int m, int log_lines, hipStream_t s)
{
    std::lock_guard<std::mutex> g(set->idx_mu);
    return index_build_locked(set, d_keys, n, m, log_lines, s);
}

// presence-only insertion into a sparse set (the table IS the set; kept at most ~half full, regrown by rehashing)
int index_insert_reads(brx_set *set, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads, uint64_t total_bases,
                       hipStream_t s)
{
    const int k = set->k;
    if (!set->sparse || !(k & 1) || k < 5 || k > 31) {
        set_error("k-mer insertion into a sparse set needs an odd 5 <= k <= 31 (k=%d%s)", k, set->sparse ? "" : ", set is not sparse");
        return BRX_ERR_UNSUPPORTED;
    }
    BRX_TRY(use_device(set->device));
    std::lock_guard<std::mutex> g(set->idx_mu);
    if (set->idx_valid && !set->idx_open) {
        set_error("the set was built by counting; k-mers cannot be added to it");
        return BRX_ERR_UNSUPPORTED;
    }
    if (!set->idx_valid) { // the empty set
        set->idx_keys = 0;
        set->idx_overflow_keys = 0;
    }
    const uint64_t need = set->idx_keys + total_bases; // every k-mer of the batch could be new
    const bool have = set->idx_valid && set->d_lines;
    if (!have || (7ull << set->idx_log_lines) < 2ull * need) {
        int log_lines = 12;
        while (log_lines < 30 && (7ull << log_lines) < 3ull * need)
            log_lines++;
        if ((7ull << log_lines) < need + need / 4) {
            set_error("sparse set: %llu k-mers do not fit the largest table", (unsigned long long)need);
            return BRX_ERR_NOMEM;
        }
        int m = env_int("BRX_INDEX_M", 0);
        if (m <= 0)
            m = index_auto_m(k, need);
        if ((!(m & 1) && m != 16) || m < 3 || m > IDX_MAX_M || m > k - 1) {
            set_error("probe index: bad minimizer length %d for k=%d", m, k);
            return BRX_ERR_ARG;
        }
        DevBuf<uint64_t> nl;
        BRX_TRY(nl.reserve_bytes((64ull << log_lines) + ((1ull << log_lines) >> 3) + 64ull, 0, "sparse set table")); // (+ room for occupancy bits)
        BRX_HIP(hipMemsetAsync(nl, 0, 64ull << log_lines, s));
        if (have && set->idx_keys) {
            KernelTimer t("index_rehash", s);
            table_rehash_kernel<<<256 * 8, 256, 0, s>>>(table_source(set->d_lines, 1ull << set->idx_log_lines), k, nl, 32u - (uint32_t)log_lines,
                                                        (uint32_t)m, (uint32_t)(k - m + 1));
        }
        BRX_HIP(hipStreamSynchronize(s));
        set->d_lines = std::move(nl);
        set->lines_alloc = 1ull << log_lines;
        set->idx_log_lines = (uint32_t)log_lines;
        set->idx_m = (uint32_t)m;
    }
    DevBuf<unsigned long long> d_new;
    BRX_TRY(d_new.reserve(1, 0, "sparse set insert"));
    BRX_HIP(hipMemsetAsync(d_new, 0, 8, s));
    if (n_reads) {
        KernelTimer t("index_insert_reads", s);
        BRX_TRY(flat_presence_insert(d_bases, d_offsets, n_reads, total_bases, k, nullptr, set->d_lines, 32u - set->idx_log_lines,
                                     set->idx_m, d_new, s));
    }
    unsigned long long added = 0;
    BRX_HIP(hipMemcpyAsync(&added, d_new, 8, hipMemcpyDeviceToHost, s));
    BRX_HIP(hipStreamSynchronize(s));
    set->idx_keys += added;
    index_mark(set, true, true, false); // open; filled k-mer by k-mer: no occupancy bits
    keylist_mark(set, false); // the table is the set now
    return BRX_OK;
}

int ensure_bits(const brx_set *cset, hipStream_t s, const char *what)
{
    brx_set *set = const_cast<brx_set *>(cset);
    if (set->sparse) {
        set_error("%s needs the bit vector; a sparse set (k=%d) has none", what, set->k);
        return BRX_ERR_UNSUPPORTED;
    }
    if (!set->bits_stale)
        return BRX_OK;
    BRX_TRY(use_device(set->device));
    std::lock_guard<std::mutex> g(set->idx_mu);
    if (!set->bits_stale)
        return BRX_OK;
    SetKeys keys;
    BRX_TRY(set_keys_locked(set, s, &keys));
    if (keys.holder == SetHolder::None) {
        set_error("%s: the set has neither bits, key list nor an exact index", what);
        return BRX_ERR_ARG;
    }
    KernelTimer t("bits_materialise", s);
    BRX_HIP(hipMemsetAsync(set->d_bits, 0, set->nwords * 4, s));
    or_keys_kernel<<<keys.holder == SetHolder::KeyList ? 256 * 8 : 256 * 16, 256, 0, s>>>(keys.src, set->d_bits, set->nwords * 32);
    BRX_HIP(hipGetLastError());
    BRX_HIP(hipStreamSynchronize(s));
    bits_mark(set, true);
    return BRX_OK;
}

int index_ensure(const brx_set *cset, hipStream_t s)
{
    brx_set *set = const_cast<brx_set *>(cset);
    if (!index_wanted(set->k) && !no_bits(set))
        return BRX_OK;
    // several chains may share the set (one per host thread): exactly one of them builds, the others wait
    // here and find the index valid -- a second build would wipe lines the first chain's kernels are reading
    std::lock_guard<std::mutex> g(set->idx_mu);
    if (set->idx_valid || set->idx_declined)
        return BRX_OK;
    BRX_TRY(use_device(set->device));
    SetKeys keys;
    BRX_TRY(set_keys_locked(set, s, &keys));
    uint64_t n = 0;
    BRX_TRY(keys_count(set, keys, s, &n));
    if (no_bits(set) && keys.holder != SetHolder::KeyList) { // (no table either: the set has no index)
        set_error("set without bit vector and without a complete key list (%llu solid k-mers counted, room for %llu)", (unsigned long long)n,
                  (unsigned long long)keys.list_cap);
        return BRX_ERR_NOMEM;
    }
    if (!no_bits(set) && set->k - index_auto_m(set->k, n) + 1 < 3 && env_int("BRX_INDEX_M", 0) <= 0) {
        // so many keys that a safe minimizer is (nearly) the k-mer itself: neighbours would not share lines
        set->idx_declined = true;
        return BRX_OK;
    }
    if (keys.holder == SetHolder::KeyList)
        return index_build_locked(set, keys.src.keys, n, 0, 0, s);
    DevBuf<uint64_t> d_keys;
    uint64_t got = 0;
    BRX_TRY(keys_from_bits(set, s, d_keys, &got, 0, &n));
    return index_build_locked(set, d_keys, got, 0, 0, s);
}

} // namespace brx

extern "C" {

int brx_set_index_build(brx_set_t *set, int m, int log2_lines, void *stream)
{
    if (!set)
        return BRX_ERR_ARG;
    BRX_TRY(use_device(set->device));
    DevBuf<uint64_t> d_keys;
    uint64_t got = 0;
    BRX_TRY(keys_from_bits(set, (hipStream_t)stream, d_keys, &got)); // (a lazy vector is written first)
    return index_build_from_keys(set, d_keys, got, m, log2_lines, (hipStream_t)stream);
}

int brx_set_index_build_from_keys_device(brx_set_t *set, const uint64_t *d_keys, uint64_t n, int m, int log2_lines, void *stream)
{
    if (!set || (!d_keys && n))
        return BRX_ERR_ARG;
    int st = index_build_from_keys(set, d_keys, n, m, log2_lines, (hipStream_t)stream);
    if (st == BRX_OK && no_bits(set) && d_keys != set->d_keylist)
        keylist_mark(set, false); // without a bit vector the list just given IS the set now (multi-GPU exchange)
    return st;
}

int brx_set_or_keys_device(brx_set_t *set, const uint64_t *d_keys, uint64_t n, void *stream)
{
    if (!set || (!d_keys && n))
        return BRX_ERR_ARG;
    BRX_TRY(ensure_bits(set, nullptr, "or_keys (use brx_set_index_build_from_keys_device)"));
    BRX_TRY(use_device(set->device));
    if (!n)
        return BRX_OK;
    index_invalidate(set);
    hipStream_t s = (hipStream_t)stream;
    {
        KernelTimer t("or_keys", s);
        const uint64_t blocks = (n + 255) / 256;
        or_keys_kernel<<<(int)(blocks < 256 * 8 ? blocks : 256 * 8), 256, 0, s>>>(list_source(d_keys, n), set->d_bits, set->nwords * 32);
    }
    BRX_HIP(hipGetLastError());
    return BRX_OK;
}

int brx_set_keylist_device(const brx_set_t *set, void **d_keys, uint64_t *n, void *stream)
{
    if (!set || !d_keys || !n)
        return BRX_ERR_ARG;
    *d_keys = nullptr;
    *n = 0;
    SetKeys keys;
    BRX_TRY(set_keys(set, (hipStream_t)stream, &keys));
    if (keys.holder == SetHolder::KeyList) {
        *d_keys = const_cast<uint64_t *>(keys.src.keys);
        *n = keys.src.n;
    }
    return BRX_OK;
}

// ---- fingerprint: the same three numbers for the same SET, whatever holds it ------------------------------------------
namespace {
__device__ __forceinline__ void fp_add(unsigned long long *out, unsigned long long n, unsigned long long s1, unsigned long long s2)
{
    // wave sums by DPP-free shuffles, then one atomic per wave and number
    for (int o = 32; o > 0; o >>= 1) {
        n += __shfl_down(n, o);
        s1 += __shfl_down(s1, o);
        s2 += __shfl_down(s2, o);
    }
    if ((threadIdx.x & 63) == 0 && n) {
        atomicAdd(out + 0, n);
        atomicAdd(out + 1, s1);
        atomicAdd(out + 2, s2);
    }
}
__global__ __launch_bounds__(256) void fp_kernel(KeySource src, unsigned long long *out)
{
    unsigned long long c = 0, s1 = 0, s2 = 0;
    for_each_key(src, [&](uint64_t h) { c++, s1 += h, s2 += h * h; });
    fp_add(out, c, s1, s2);
}
} // namespace

int brx_set_fingerprint(const brx_set_t *set, uint64_t *out3, void *stream)
{
    if (!set || !out3)
        return BRX_ERR_ARG;
    BRX_TRY(use_device(set->device));
    hipStream_t s = (hipStream_t)stream;
    DevBuf<unsigned long long> d;
    BRX_TRY(d.reserve(3, 0, "fingerprint"));
    BRX_HIP(hipMemsetAsync(d, 0, 24, s));
    SetKeys keys;
    BRX_TRY(set_keys(set, s, &keys));
    if (keys.holder == SetHolder::None) {
        set_error("fingerprint: the set has neither a bit vector, nor a key list, nor a table");
        return BRX_ERR_UNSUPPORTED;
    }
    fp_kernel<<<keys.holder == SetHolder::KeyList ? 2048 : 4096, 256, 0, s>>>(keys.src, d);
    BRX_HIP(hipGetLastError());
    unsigned long long h[3] = {0, 0, 0};
    BRX_HIP(hipMemcpyAsync(h, d, 24, hipMemcpyDeviceToHost, s));
    BRX_HIP(hipStreamSynchronize(s));
    out3[0] = h[0];
    out3[1] = h[1];
    out3[2] = h[2];
    return BRX_OK;
}

int brx_set_index_drop(brx_set_t *set)
{
    if (!set)
        return BRX_ERR_ARG;
    std::lock_guard<std::mutex> g(set->idx_mu);
    set->idx_valid = false;
    set->idx_gen++;
    (void)use_device(set->device);
    set->d_lines.reset();
    set->lines_alloc = 0;
    return BRX_OK;
}

int brx_set_index_info(const brx_set_t *set, uint64_t *info8)
{
    if (!set || !info8)
        return BRX_ERR_ARG;
    for (int i = 0; i < 8; i++)
        info8[i] = 0;
    info8[0] = set->idx_valid ? 1 : 0;
    info8[6] = (index_wanted(set->k) || no_bits(set)) ? 1 : 0;
    info8[7] = set->keylist_valid ? 1 : 0;
    if (set->idx_valid) {
        info8[1] = set->idx_m;
        info8[2] = set->idx_log_lines;
        info8[3] = set->idx_keys;
        info8[4] = set->idx_overflow_keys;
        info8[5] = (1ull << set->idx_log_lines) * 64ull;
    }
    return BRX_OK;
}

int brx_set_get_batch_indexed(const brx_set_t *set, const uint64_t *forward_kmers, uint32_t n, uint8_t *out, uint64_t *n_fallback)
{
    if (!set || (!forward_kmers && n) || (!out && n))
        return BRX_ERR_ARG;
    if (!set->idx_valid) {
        set_error("get_batch_indexed: the set has no probe index (brx_set_index_build)");
        return BRX_ERR_ARG;
    }
    BRX_TRY(use_device(set->device));
    if (n_fallback)
        *n_fallback = 0;
    if (!n)
        return BRX_OK;
    DevBuf<uint64_t> d_k;
    DevBuf<uint8_t> d_o;
    DevBuf<unsigned long long> d_f;
    BRX_TRY(d_k.reserve(n, 0, "get_batch_indexed k-mers"));
    BRX_TRY(d_o.reserve(n, 0, "get_batch_indexed answers"));
    BRX_TRY(d_f.reserve(1, 0, "get_batch_indexed"));
    BRX_HIP(hipMemset(d_f, 0, 8));
    BRX_HIP(hipMemcpy(d_k, forward_kmers, (uint64_t)n * 8, hipMemcpyHostToDevice));
    unsigned long long fb = 0;
    const SetView v = set_view(set, false, true);
    index_get_kernel<<<(n + 255) / 256, 256>>>(v.idx, v.bits, d_k, n, set->k, d_o, d_f);
    BRX_HIP(hipMemcpy(out, d_o, n, hipMemcpyDeviceToHost));
    BRX_HIP(hipMemcpy(&fb, d_f, 8, hipMemcpyDeviceToHost));
    if (n_fallback)
        *n_fallback = fb;
    return BRX_OK;
}

} // extern "C"
