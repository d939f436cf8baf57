// Counting table (BRX_COUNT_TABLE): k-mer counts with an abundance threshold for every odd k up to 31.
//
// The dense counter is a 2^(2k-1)-byte table (k <= 19) and the partitioned counter carries 32-bit keys (k <= 21); this
// one counts into the chained 64-byte-line table that sparse sets are made of (brx_index.hpp: 7 keys per line, addressed
// by the k-mer's minimizer, chained into the next line), with one u32 counter per slot in an array of its own beside the
// lines -- counts[line * 8 + slot] -- so that the line format and every probe stay what they are.
//
//   count    flat_count_kernel (brx_partbuild.hip, beside flat_insert_kernel<true>): find or claim the k-mer's slot with
//            one 64-bit CAS, then one atomic add on the slot's counter unless it has reached 255 (table_count_bump).
//   regrow   the table is kept at most about half full (keys so far + bases of the next batch against 7 slots per line,
//            as index_insert_reads does): a larger one is allocated and table_rehash_counts_kernel moves every key with
//            min(255, its count).
//   finish   table_select_kernel: one pass over the slots, keys with min(255, count) > abundance compacted in the wave
//            (one global atomic per wave) into the destination's key list -- the closed set the partitioned finish
//            leaves at k = 21: the probe index is built from the list on first use.  A set with a bit vector (k <= 19)
//            gets its bits written in the same pass.
//   spectrum table_spectrum_kernel: bins 1..255 from the counters.
//   slice    brx_counter_set_slice: only the k-mers one part of P owns are counted (flat_count_slice_kernel compacts them in
//            LDS so that full waves walk), and the table is sized for them (tab_add_batch_slice: flat_slice_census_kernel
//            counts the batch's k-mers of the part when the bound below does not fit).  Everything else reads the table.
//
// The exact number of distinct keys lives on the device (d_nkeys) and is read back -- one synchronisation of the stream
// -- only when the bound "keys known + bases counted since" no longer fits under the load limit, and by finish.
#include "brx_internal.hpp"
#include "brx_index.hpp"

using namespace brx;

namespace brx {

struct TabState {
    DevBuf<uint64_t> d_lines;      // 8 u64 per line
    DevBuf<uint32_t> d_counts;     // 8 u32 per line (entry 7 unused)
    uint32_t log_lines = 0, m = 0;
    DevBuf<unsigned long long> d_nkeys; // distinct keys in the table
    uint64_t keys_known = 0;       // d_nkeys when it was last read back
    uint64_t pending = 0;          // bases counted since: at most that many more keys
    uint64_t bases_total = 0;      // bases counted in all: at most that many occurrences
    uint64_t peak_bytes = 0;       // lines + counters held at once (both tables during a regrow)
    // after brx_exchange_table_merge: the table holds the k-mers this rank owns, with the counts of the whole job; nothing
    // more can be counted into it until the counter is reset (merged_world 0: an ordinary counter)
    int merged_world = 0, merged_rank = 0;
    // after brx_counter_load_fd of a file that kept only counts >= floor: the k-mers seen fewer times are unknown, so
    // nothing can be added and no set with a threshold below floor - 1 can be finished until the counter is reset
    uint8_t floor = 1;
    // brx_counter_set_slice: the counter counts only the k-mers `part` of `parts` owns (table_owner_of); parts 1: all of them.
    // d_slice, allocated with the first slice: [0, 4) what brx_counter_slice_stats reports, [4, 6) the sizing pass's answer
    uint32_t part = 0, parts = 1;
    DevBuf<unsigned long long> d_slice;
    uint64_t seen_unwalked = 0;    // valid k-mers of the batches that held none of the part: no count kernel ran for them
};

} // namespace brx

namespace {

constexpr int TAB_MIN_LOG_LINES = 12, TAB_MAX_LOG_LINES = 30;

// moves every key of one counting table into another, with its count
__global__ __launch_bounds__(256) void table_rehash_counts_kernel(const uint64_t *__restrict__ old_lines, const uint32_t *__restrict__ old_counts,
                                                                  uint64_t n_old_slots, int k, uint64_t *__restrict__ lines,
                                                                  uint32_t *__restrict__ counts, uint32_t line_shift, uint32_t m, uint32_t w)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_old_slots; i += stride) {
        const uint64_t v = table_slot_key(old_lines, i);
        if (v) {
            const uint64_t h = v - 1ull;
            bool fresh;
            const uint64_t slot = table_find_or_claim(lines, line_shift, m, w, k, (h << 1) | (uint64_t)(popc64(h) & 1), fresh);
            table_count_bump(counts + slot, table_count_read(old_counts[i])); // (a key sits in the old table once)
        }
    }
}

// keys with min(255, count) > abundance: listed (LIST), their bits set (bits != nullptr).  A wave takes 64 consecutive
// slots per trip (n_slots is a multiple of 64), counts its keepers with a ballot and asks for their places with one atomic.
template <bool LIST>
__global__ __launch_bounds__(256) void table_select_kernel(const uint64_t *__restrict__ lines, const uint32_t *__restrict__ counts,
                                                           uint64_t n_slots, uint32_t abundance, uint64_t *__restrict__ out, uint64_t cap,
                                                           unsigned long long *__restrict__ n_out, uint32_t *__restrict__ bits, uint64_t nbits)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += stride) {
        const uint64_t v = table_slot_key(lines, i);
        const bool keep = v && table_count_read(counts[i]) > abundance;
        if (keep && bits && v - 1ull < nbits)
            atomicOr(bits + ((v - 1ull) >> 5), 1u << ((v - 1ull) & 31u));
        if (LIST) {
            const unsigned long long mask = __ballot(keep);
            if (mask) { // wave-uniform, and every lane of the wave is here: n_slots and the stride are multiples of 256
                unsigned long long first = 0;
                if (lane == 0u)
                    first = atomicAdd(n_out, (unsigned long long)__popcll(mask));
                first = __shfl(first, 0);
                const uint64_t pos = first + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
                if (keep && pos < cap)
                    out[pos] = v - 1ull;
            }
        }
    }
}

__global__ __launch_bounds__(256) void table_spectrum_kernel(const uint64_t *__restrict__ lines, const uint32_t *__restrict__ counts,
                                                             uint64_t n_slots, unsigned long long *__restrict__ hist)
{
    __shared__ unsigned long long h[256];
    h[threadIdx.x] = 0ull;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += stride)
        if (table_slot_key(lines, i))
            atomicAdd(&h[table_count_read(counts[i])], 1ull);
    __syncthreads();
    if (h[threadIdx.x])
        atomicAdd(hist + threadIdx.x, h[threadIdx.x]);
}

// ---- the table side of the multi-GPU merge (brx_exchange_table_merge) ---------------------------------------------------
// Both owner kernels stream the slots as table_select_kernel does: 64 consecutive slots per wave trip, entry 7 of a line
// skipped, every lane of the wave in every trip (n_slots and the stride are multiples of 256).  A trip walks the owners
// present among its 64 slots -- the first lane not served yet names one, a ballot finds the lanes that share it -- and
// that leader alone adds the popcount: one atomic per wave and owner present, never one per entry.

// entries per owner into hist[world]
__global__ __launch_bounds__(256) void table_owner_hist_kernel(const uint64_t *__restrict__ lines, uint64_t n_slots, uint32_t world,
                                                               unsigned long long *__restrict__ hist)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += stride) {
        const uint64_t v = table_slot_key(lines, i);
        const uint32_t own = v ? table_owner_of(v - 1ull, world) : 0xffffffffu;
        unsigned long long todo = __ballot(v != 0ull);
        while (todo) { // wave-uniform
            const uint32_t leader = (uint32_t)__ffsll(todo) - 1u;
            const uint32_t o = __shfl(own, leader);
            const unsigned long long same = __ballot(own == o);
            if (lane == leader && o < world)
                atomicAdd(hist + o, (unsigned long long)__popcll(same));
            todo &= ~same;
        }
    }
}

// every entry into its owner's region of (keys, cnts): region r is [off[r], off[r + 1]), cursor[r] starts at off[r]
__global__ __launch_bounds__(256) void table_owner_split_kernel(const uint64_t *__restrict__ lines, const uint32_t *__restrict__ counts,
                                                                uint64_t n_slots, uint32_t world, const uint64_t *__restrict__ off,
                                                                unsigned long long *__restrict__ cursor, uint64_t *__restrict__ keys,
                                                                uint8_t *__restrict__ cnts)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += stride) {
        const uint64_t v = table_slot_key(lines, i);
        const uint32_t own = v ? table_owner_of(v - 1ull, world) : 0xffffffffu;
        const uint32_t cnt = v ? table_count_read(counts[i]) : 0u;
        unsigned long long todo = __ballot(v != 0ull);
        while (todo) { // wave-uniform
            const uint32_t leader = (uint32_t)__ffsll(todo) - 1u;
            const uint32_t o = __shfl(own, leader);
            const unsigned long long same = __ballot(own == o);
            unsigned long long first = 0;
            if (lane == leader && o < world)
                first = atomicAdd(cursor + o, (unsigned long long)__popcll(same));
            first = __shfl(first, leader);
            if (own == o && o < world) {
                const uint64_t pos = first + (uint64_t)__popcll(same & ((1ull << lane) - 1ull));
                if (pos < off[o + 1u]) { // (the histogram pass sized the region: always, unless the table changed in between)
                    keys[pos] = v - 1ull;
                    cnts[pos] = (uint8_t)cnt;
                }
            }
            todo &= ~same;
        }
    }
}

// the rehash kernel with (key, count) arrays as its source: a key may come once per source rank, its counts add up to
// 255.  n_new: keys this launch put in; n_sum: the counts it added (a bound on the occurrences behind the table)
__global__ __launch_bounds__(256) void table_merge_kernel(const uint64_t *__restrict__ keys, const uint8_t *__restrict__ cnts, uint64_t n, int k,
                                                          uint64_t key_limit, uint64_t *__restrict__ lines, uint32_t *__restrict__ counts,
                                                          uint32_t line_shift, uint32_t m, uint32_t w, unsigned long long *__restrict__ n_new,
                                                          unsigned long long *__restrict__ n_sum)
{
    uint32_t added = 0;
    unsigned long long sum = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t h = keys[i];
        const uint32_t by = cnts[i];
        if (h < key_limit && by) { // (anything else is not an entry of a table of this k)
            bool fresh;
            const uint64_t slot = table_find_or_claim(lines, line_shift, m, w, k, (h << 1) | (uint64_t)(popc64(h) & 1), fresh);
            table_count_bump(counts + slot, by);
            added += fresh ? 1u : 0u;
            sum += by;
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        added += __shfl_down(added, d);
        sum += __shfl_down(sum, d);
    }
    if ((threadIdx.x & 63) == 0 && sum) {
        atomicAdd(n_new, (unsigned long long)added);
        atomicAdd(n_sum, sum);
    }
}

uint32_t slot_grid(uint64_t n_slots) { return read_grid((n_slots + 255ull) / 256ull, 256u * 16u); }

void free_table(TabState *t)
{
    t->d_lines.reset();
    t->d_counts.reset();
    t->log_lines = 0;
}

// brings keys_known up to date (synchronises `s`)
int read_keys(TabState *t, hipStream_t s)
{
    unsigned long long n = 0;
    BRX_HIP(hipMemcpyAsync(&n, t->d_nkeys, 8, hipMemcpyDeviceToHost, s));
    BRX_HIP(hipStreamSynchronize(s));
    t->keys_known = n;
    t->pending = 0;
    return BRX_OK;
}

// true: a table of 2^log_lines lines stays at most half full with `need` keys
inline bool fits_half(uint32_t log_lines, uint64_t need) { return (7ull << log_lines) >= 2ull * need; }

// a table for `need` keys (an upper bound), the counted keys carried over
int regrow(brx_counter *c, uint64_t need, hipStream_t s)
{
    TabState *t = c->tab;
    const int k = c->k;
    int log_lines = TAB_MIN_LOG_LINES;
    while (log_lines < TAB_MAX_LOG_LINES && (7ull << log_lines) < 3ull * need)
        log_lines++;
    if ((7ull << log_lines) < need + need / 4) {
        // more keys than slots would send a chain walk round the table for ever: refuse before any kernel runs
        set_error("counting table: %llu k-mers (%llu counted so far + the bases of this batch) do not fit the largest table of 2^%d lines "
                  "(%llu slots)", (unsigned long long)need, (unsigned long long)t->keys_known, TAB_MAX_LOG_LINES,
                  (unsigned long long)(7ull << TAB_MAX_LOG_LINES));
        return BRX_ERR_NOMEM;
    }
    int m = (int)env_u32("BRX_INDEX_M", 0u);
    if (m <= 0)
        m = index_auto_m(k, need);
    if ((!(m & 1) && m != 16) || m < 3 || m > IDX_MAX_M || m > k - 1) {
        set_error("counting table: bad minimizer length %d for k=%d", m, k);
        return BRX_ERR_ARG;
    }
    const uint64_t line_bytes = 64ull << log_lines, count_bytes = 32ull << log_lines;
    DevBuf<uint64_t> nl;
    DevBuf<uint32_t> nc;
    BRX_TRY(nl.reserve_bytes(line_bytes, 0, "counting table lines"));
    BRX_TRY(nc.reserve_bytes(count_bytes, 0, "counting table counters"));
    const uint64_t held = t->d_lines ? (96ull << t->log_lines) : 0ull;
    if (held + line_bytes + count_bytes > t->peak_bytes)
        t->peak_bytes = held + line_bytes + count_bytes;
    {
        KernelTimer z("tab_zero", s);
        BRX_HIP(hipMemsetAsync(nl, 0, line_bytes, s));
        BRX_HIP(hipMemsetAsync(nc, 0, count_bytes, s));
    }
    if (t->d_lines && t->keys_known) {
        KernelTimer r("tab_rehash", s);
        const uint64_t n_old = 8ull << t->log_lines;
        table_rehash_counts_kernel<<<slot_grid(n_old), 256, 0, s>>>(t->d_lines, t->d_counts, n_old, k, nl, nc, 32u - (uint32_t)log_lines,
                                                                    (uint32_t)m, (uint32_t)(k - m + 1));
        BRX_HIP(hipGetLastError());
    }
    BRX_HIP(hipStreamSynchronize(s)); // the old table is freed below
    t->d_lines = std::move(nl);
    t->d_counts = std::move(nc);
    t->log_lines = (uint32_t)log_lines;
    t->m = (uint32_t)m;
    return BRX_OK;
}

} // namespace

namespace brx {

int tab_begin(brx_counter *c)
{
    if (!(c->k & 1) || c->k < 5 || c->k > 31) {
        set_error("table count strategy (BRX_COUNT_TABLE) supports odd 5 <= k <= 31 (got %d)", c->k);
        return BRX_ERR_UNSUPPORTED;
    }
    TabState *t = new TabState();
    c->tab = t;
    BRX_TRY(t->d_nkeys.reserve(1, 0, "counting table key counter"));
    BRX_HIP(zero_now(t->d_nkeys, 8)); // (done on return: the first batch may come on any stream)
    return BRX_OK;
}

void tab_free(brx_counter *c)
{
    delete c->tab;
    c->tab = nullptr;
}

int tab_reset(brx_counter *c, hipStream_t s)
{
    TabState *t = c->tab;
    if (t->d_lines) {
        KernelTimer z("tab_zero", s);
        BRX_HIP(hipMemsetAsync(t->d_lines, 0, 64ull << t->log_lines, s));
        BRX_HIP(hipMemsetAsync(t->d_counts, 0, 32ull << t->log_lines, s));
    }
    BRX_HIP(hipMemsetAsync(t->d_nkeys, 0, 8, s));
    t->keys_known = t->pending = t->bases_total = 0;
    t->merged_world = t->merged_rank = 0;
    t->floor = 1;
    if (t->d_slice)
        BRX_HIP(hipMemsetAsync(t->d_slice, 0, 6 * 8, s));
    t->seen_unwalked = 0; // (the slice itself stays)
    return BRX_OK;
}

// A batch into a sliced counter.  While "every base is a new key" fits the table nothing is asked; when it does not, or
// there is no table, the sizing pass counts the batch's k-mers of the part and the table is sized for the keys known plus
// that number: a P-th of the loose bound, which is what the slice is for.
static int tab_add_batch_slice(brx_counter *c, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads, uint64_t total_bases,
                               hipStream_t s)
{
    TabState *t = c->tab;
    uint64_t bound = total_bases; // k-mers of the part in this batch, at most
    if (!t->d_lines || !fits_half(t->log_lines, t->keys_known + t->pending + total_bases)) {
        BRX_HIP(hipMemsetAsync(t->d_slice + 4, 0, 2 * 8, s));
        {
            KernelTimer kt("tab_census", s);
            BRX_TRY(flat_slice_census(d_bases, d_offsets, n_reads, total_bases, c->k, t->part, t->parts, t->d_slice + 4, s));
        }
        unsigned long long got[2] = {0, 0};
        BRX_HIP(hipMemcpyAsync(got, t->d_slice + 4, 2 * 8, hipMemcpyDeviceToHost, s));
        BRX_TRY(read_keys(t, s)); // (one synchronisation for both)
        bound = got[0];
        if (!bound) { // nothing of the part: no table is made for it, and none is walked
            t->seen_unwalked += got[1];
            return BRX_OK;
        }
        if (!t->d_lines || !fits_half(t->log_lines, t->keys_known + bound))
            BRX_TRY(regrow(c, t->keys_known + bound, s));
    }
    {
        KernelTimer kt("tab_count", s);
        BRX_TRY(flat_table_count_slice(d_bases, d_offsets, n_reads, total_bases, c->k, t->d_lines, t->d_counts, 32u - t->log_lines, t->m,
                                       t->part, t->parts, t->d_nkeys, t->d_slice, s));
    }
    t->pending += bound;
    t->bases_total += bound;
    return BRX_OK;
}

int tab_add_batch(brx_counter *c, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads, uint64_t total_bases, hipStream_t s)
{
    TabState *t = c->tab;
    if (t->merged_world) {
        set_error("counting table: the counter was merged over %d ranks and holds the job's counts of the k-mers rank %d owns; "
                  "brx_counter_reset it before counting again", t->merged_world, t->merged_rank);
        return BRX_ERR_ARG;
    }
    if (t->floor > 1) {
        set_error("counting table: the counter was loaded from a key file that kept only counts from %d up; brx_counter_reset it "
                  "before counting again", (int)t->floor);
        return BRX_ERR_ARG;
    }
    if (!n_reads || !total_bases)
        return BRX_OK;
    if (t->parts > 1u)
        return tab_add_batch_slice(c, d_bases, d_offsets, n_reads, total_bases, s);
    // every k-mer of the batch could be new
    if (!t->d_lines || !fits_half(t->log_lines, t->keys_known + t->pending + total_bases)) {
        if (t->pending)
            BRX_TRY(read_keys(t, s)); // the bound was what did not fit: now the exact number
        if (!t->d_lines || !fits_half(t->log_lines, t->keys_known + total_bases))
            BRX_TRY(regrow(c, t->keys_known + total_bases, s));
    }
    {
        KernelTimer kt("tab_count", s);
        BRX_TRY(flat_table_count(d_bases, d_offsets, n_reads, total_bases, c->k, t->d_lines, t->d_counts, 32u - t->log_lines, t->m,
                                 t->d_nkeys, s));
    }
    t->pending += total_bases;
    t->bases_total += total_bases;
    return BRX_OK;
}

int tab_finish_into(brx_counter *c, uint32_t abundance, hipStream_t s, brx_set *dst)
{
    TabState *t = c->tab;
    if (t->floor > 1 && abundance + 1u < t->floor) {
        set_error("counting table: the counter was loaded from a key file that kept only counts from %d up: a set of the k-mers seen more "
                  "than %u times would miss members (thresholds from %d up can be finished)", (int)t->floor, abundance, (int)t->floor - 1);
        return BRX_ERR_ARG;
    }
    if (t->pending)
        BRX_TRY(read_keys(t, s));
    BRX_TRY(dst->d_keylist_n.reserve(1, 0, "key list counter"));
    BRX_HIP(hipMemsetAsync(dst->d_keylist_n, 0, 8, s));
    if (!dst->sparse) { // the bits are written here, in the same pass (nothing left lazy)
        BRX_HIP(hipMemsetAsync(dst->d_bits, 0, dst->nwords * 4, s));
        bits_mark(dst, true);
    }
    const bool list = dst->sparse || index_wanted(c->k);
    if (t->keys_known && t->d_lines) {
        if (list) {
            // a listed key was seen more than `abundance` times, and is one of the distinct keys
            uint64_t want = t->bases_total / ((uint64_t)abundance + 1ull);
            if (want > t->keys_known)
                want = t->keys_known;
            want += 64;
            BRX_TRY(dst->d_keylist.reserve(want, 0, "solid key list"));
        }
        KernelTimer kt("tab_select", s);
        const uint64_t n_slots = 8ull << t->log_lines;
        if (list)
            table_select_kernel<true><<<slot_grid(n_slots), 256, 0, s>>>(t->d_lines, t->d_counts, n_slots, abundance, dst->d_keylist,
                                                                        dst->d_keylist.cap(), dst->d_keylist_n, dst->sparse ? nullptr : dst->d_bits.get(),
                                                                        dst->nwords * 32);
        else
            table_select_kernel<false><<<slot_grid(n_slots), 256, 0, s>>>(t->d_lines, t->d_counts, n_slots, abundance, nullptr, 0, nullptr,
                                                                         dst->d_bits, dst->nwords * 32);
        BRX_HIP(hipGetLastError());
    }
    keylist_mark(dst, list); // (nothing counted: the empty list)
    trace_stage(s, "table select");
    return BRX_OK;
}

int tab_split_by_owner(brx_counter *c, int world, hipStream_t s, uint64_t **d_keys, uint8_t **d_cnts, uint64_t *per_owner)
{
    TabState *t = c->tab;
    *d_keys = nullptr;
    *d_cnts = nullptr;
    for (int r = 0; r < world; r++)
        per_owner[r] = 0;
    if (t->pending)
        BRX_TRY(read_keys(t, s));
    const uint64_t n = t->d_lines ? t->keys_known : 0ull;
    DevBuf<uint64_t> keys; // handed to the caller at the end
    DevBuf<uint8_t> cnts;
    if (n) {
        const uint64_t n_slots = 8ull << t->log_lines;
        DevScratch ws;
        unsigned long long *d_hist = nullptr, *d_cursor = nullptr;
        uint64_t *d_off = nullptr;
        BRX_TRY(ws.get(&d_hist, (uint64_t)world));
        BRX_TRY(ws.get(&d_cursor, (uint64_t)world));
        BRX_TRY(ws.get(&d_off, (uint64_t)world + 1ull));
        std::vector<uint64_t> off((size_t)world + 1, 0);
        BRX_HIP(hipMemsetAsync(d_hist, 0, (size_t)world * 8, s));
        {
            KernelTimer kt("tab_split", s);
            table_owner_hist_kernel<<<slot_grid(n_slots), 256, 0, s>>>(t->d_lines, n_slots, (uint32_t)world, d_hist);
        }
        BRX_HIP(hipGetLastError());
        BRX_HIP(hipMemcpyAsync(per_owner, d_hist, (size_t)world * 8, hipMemcpyDeviceToHost, s));
        BRX_HIP(hipStreamSynchronize(s));
        for (int r = 0; r < world; r++)
            off[r + 1] = off[r] + per_owner[r];
        if (off[world] != n) {
            set_error("counting table split: %llu entries found, %llu k-mers counted", (unsigned long long)off[world], (unsigned long long)n);
            return BRX_ERR_HIP;
        }
        BRX_TRY(keys.reserve(n, 0, "the table's keys grouped by owner"));
        BRX_TRY(cnts.reserve(n, 0, "the table's counts grouped by owner"));
        if ((96ull << t->log_lines) + n * 9 > t->peak_bytes)
            t->peak_bytes = (96ull << t->log_lines) + n * 9;
        BRX_HIP(hipMemcpyAsync(d_off, off.data(), ((size_t)world + 1) * 8, hipMemcpyHostToDevice, s));
        BRX_HIP(hipMemcpyAsync(d_cursor, d_off, (size_t)world * 8, hipMemcpyDeviceToDevice, s));
        {
            KernelTimer kt("tab_split", s);
            table_owner_split_kernel<<<slot_grid(n_slots), 256, 0, s>>>(t->d_lines, t->d_counts, n_slots, (uint32_t)world, d_off, d_cursor,
                                                                       keys, cnts);
        }
        BRX_HIP(hipGetLastError());
        BRX_HIP(hipStreamSynchronize(s)); // (`off` is a local; the table is freed below)
    }
    free_table(t); // every entry is in the arrays now: never two tables at once
    BRX_HIP(hipMemsetAsync(t->d_nkeys, 0, 8, s));
    t->keys_known = t->pending = t->bases_total = 0;
    *d_keys = keys.release(); // the caller's from here (it adopts them)
    *d_cnts = cnts.release();
    return BRX_OK;
}

int tab_load_pairs(brx_counter *c, const uint64_t *d_keys, const uint8_t *d_cnts, uint64_t n, hipStream_t s)
{
    TabState *t = c->tab;
    if (t->d_lines || t->keys_known || t->pending) {
        set_error("counting table: pairs are loaded into an empty counter");
        return BRX_ERR_ARG;
    }
    if (!n)
        return BRX_OK;
    BRX_TRY(regrow(c, n, s)); // every pair could be a key of its own
    DevScratch ws;
    unsigned long long *d_sum = nullptr;
    BRX_TRY(ws.get(&d_sum, 1));
    BRX_HIP(hipMemsetAsync(d_sum, 0, 8, s));
    {
        KernelTimer kt("tab_merge", s);
        table_merge_kernel<<<read_grid((n + 255ull) / 256ull, 256u * 16u), 256, 0, s>>>(d_keys, d_cnts, n, c->k, set_nbits(c->k), t->d_lines,
                                                                                       t->d_counts, 32u - t->log_lines, t->m,
                                                                                       (uint32_t)c->k - t->m + 1u, t->d_nkeys, d_sum);
        BRX_HIP(hipGetLastError());
    }
    unsigned long long sum = 0;
    BRX_HIP(hipMemcpyAsync(&sum, d_sum, 8, hipMemcpyDeviceToHost, s));
    BRX_TRY(read_keys(t, s));
    t->bases_total = sum; // a key listed by finish has a count above `abundance`: tab_finish_into's bound on the list holds
    return BRX_OK;
}

// tab_load_pairs for a counter that may hold k-mers already (brx_counter_load_fd): the table is regrown for the k-mers
// known plus n, then every pair is found or claimed and its count added up to 255
int tab_merge_pairs(brx_counter *c, const uint64_t *d_keys, const uint8_t *d_cnts, uint64_t n, hipStream_t s)
{
    TabState *t = c->tab;
    if (!n)
        return BRX_OK;
    if (t->pending)
        BRX_TRY(read_keys(t, s));
    if (!t->d_lines || !fits_half(t->log_lines, t->keys_known + n))
        BRX_TRY(regrow(c, t->keys_known + n, s)); // every pair could be a key of its own
    DevScratch ws;
    unsigned long long *d_sum = nullptr;
    BRX_TRY(ws.get(&d_sum, 1));
    BRX_HIP(hipMemsetAsync(d_sum, 0, 8, s));
    {
        KernelTimer kt("tab_merge", s);
        table_merge_kernel<<<read_grid((n + 255ull) / 256ull, 256u * 16u), 256, 0, s>>>(d_keys, d_cnts, n, c->k, set_nbits(c->k), t->d_lines,
                                                                                       t->d_counts, 32u - t->log_lines, t->m,
                                                                                       (uint32_t)c->k - t->m + 1u, t->d_nkeys, d_sum);
        BRX_HIP(hipGetLastError());
    }
    unsigned long long sum = 0;
    BRX_HIP(hipMemcpyAsync(&sum, d_sum, 8, hipMemcpyDeviceToHost, s));
    BRX_TRY(read_keys(t, s));
    t->bases_total += sum; // (the counts in the table add up to no more: tab_finish_into's bound on the list holds)
    return BRX_OK;
}

int tab_set_slice(brx_counter *c, uint32_t part, uint32_t parts)
{
    TabState *t = c->tab;
    if (t->merged_world) {
        set_error("brx_counter_set_slice: the counter holds the k-mers rank %d of a merge over %d ranks owns; brx_counter_reset it first",
                  t->merged_rank, t->merged_world);
        return BRX_ERR_ARG;
    }
    if (t->floor > 1) {
        set_error("brx_counter_set_slice: the counter holds a key file that kept only counts from %d up; brx_counter_reset it first",
                  (int)t->floor);
        return BRX_ERR_ARG;
    }
    if (t->keys_known || t->pending || t->bases_total) {
        set_error("brx_counter_set_slice: the counter holds %s%llu k-mers (%llu occurrences at most); a slice is set on an empty counter: "
                  "brx_counter_reset it first", t->pending ? "at least " : "", (unsigned long long)t->keys_known,
                  (unsigned long long)t->bases_total);
        return BRX_ERR_ARG;
    }
    if (parts > 1u && !t->d_slice) {
        BRX_TRY(t->d_slice.reserve(6, 0, "slice statistics"));
        BRX_HIP(zero_now(t->d_slice, 6 * 8)); // (done on return: the next batch may come on any stream)
    }
    if (t->d_lines) {
        // the zeroing a reset queued (on the caller's stream: its mark; or on the counter's own) ends before the table goes
        if (c->ev_pending.exchange(false))
            BRX_HIP(hipEventSynchronize(c->ev));
        BRX_HIP(hipStreamSynchronize(c->stream));
        free_table(t);
    }
    t->peak_bytes = 0;
    t->seen_unwalked = 0; // (batches that held nothing of the old part left nothing else behind)
    t->part = parts > 1u ? part : 0u;
    t->parts = parts;
    return BRX_OK;
}

bool tab_slice(const brx_counter *c, uint32_t *part, uint32_t *parts)
{
    const TabState *t = c->tab;
    if (part)
        *part = t ? t->part : 0u;
    if (parts)
        *parts = t ? t->parts : 1u;
    return t && t->parts > 1u;
}

int tab_slice_stats(brx_counter *c, uint64_t *stats4, hipStream_t s)
{
    TabState *t = c->tab;
    stats4[0] = stats4[1] = stats4[2] = stats4[3] = 0;
    if (t->parts <= 1u || !t->d_slice)
        return BRX_OK;
    unsigned long long v[4] = {0, 0, 0, 0};
    BRX_HIP(hipMemcpyAsync(v, t->d_slice, 4 * 8, hipMemcpyDeviceToHost, s));
    BRX_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < 4; i++)
        stats4[i] = v[i];
    stats4[0] += t->seen_unwalked;
    return BRX_OK;
}

uint8_t tab_floor(const brx_counter *c) { return c->tab ? c->tab->floor : 1; }

void tab_set_floor(brx_counter *c, uint8_t floor) { c->tab->floor = floor ? floor : 1; }

void tab_set_merged(brx_counter *c, int world, int rank)
{
    c->tab->merged_world = world;
    c->tab->merged_rank = rank;
}

bool tab_merged(const brx_counter *c, int *world, int *rank)
{
    const TabState *t = c->tab;
    if (world)
        *world = t ? t->merged_world : 0;
    if (rank)
        *rank = t ? t->merged_rank : 0;
    return t && t->merged_world != 0;
}

// bins 1..255 of the count spectrum into d_hist (256 x u64, zeroed by the caller); the counter is left as it was
int tab_spectrum(brx_counter *c, hipStream_t s, unsigned long long *d_hist)
{
    TabState *t = c->tab;
    if (!t->d_lines)
        return BRX_OK;
    KernelTimer kt("tab_spectrum", s);
    const uint64_t n_slots = 8ull << t->log_lines;
    table_spectrum_kernel<<<slot_grid(n_slots), 256, 0, s>>>(t->d_lines, t->d_counts, n_slots, d_hist);
    BRX_HIP(hipGetLastError());
    return BRX_OK;
}

// what a read-only lookup needs (brx_abundance.hip); lines == nullptr: nothing counted yet
void tab_view(const brx_counter *c, const uint64_t **lines, const uint32_t **counts, uint32_t *log_lines, uint32_t *m)
{
    const TabState *t = c->tab;
    *lines = t->d_lines;
    *counts = t->d_counts;
    *log_lines = t->log_lines;
    *m = t->m;
}

int tab_info(brx_counter *c, uint64_t *info4, hipStream_t s)
{
    TabState *t = c->tab;
    if (t->pending)
        BRX_TRY(read_keys(t, s));
    info4[0] = t->d_lines ? t->log_lines : 0;
    info4[1] = t->d_lines ? t->m : 0;
    info4[2] = t->keys_known;
    info4[3] = t->peak_bytes;
    return BRX_OK;
}

} // namespace brx
