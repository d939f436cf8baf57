// K-mer abundance of reads: how often the k-mers of a batch were counted.  No counterpart in the reference.
//
// For a read s of n bases and a counter of k-mer length k (include/brx.h, "abundance"):
//   count[i] = the counter's value for the canonical k-mer of s[i..i+k), 0 <= i <= n-k: min(255, occurrences), 0 if never
//              counted (every byte coded by nuc2bit, so a byte that is not ACGT is a base like any other),
//   profile  = one byte per base, count[i] at base i, 0 at the last k-1 bases,
//   hist[v]  = number of i with count[i] == v (256 u32 per read),
//   stats    = kmers, absent = hist[0], above = #(count > abundance), min, lower median, max, sum.
//
// One lookup per k-mer of the batch, asked the way cover_kernel (brx_cover.hip) asks: the batch is cut BY POSITION into a
// work list of tiles (read, first position) built from the offsets, a wave takes a tile of READ_TILE positions (brx_tiles.hpp) and walks
// it 64 neighbouring positions per step, so that neighbours share their table lines.  The k-mers come from the DPP scan
// of brx_correct.hpp, indexed by their LAST base e: count[e-k+1].  A tile needs no look-behind (nothing is carried from
// position to position but the k-mer itself): it starts its scan at its first base with an empty carry, skips the k-1
// incomplete k-mers that gives, and reads k-1 bases past its end for the k-mers that start inside it.
//   table counter  table_lookup_slot (brx_index.hpp): the walk of index_probe_at over the counting table's lines -- whole
//                  line in vector loads, chain followed only while the flag (and at the home line the signature bit)
//                  says so -- then one 4-byte load of the slot's counter, read as min(255, .).
//   dense counter  byte khash(kmer) of the u8 table.
//   partitioned    the count view that brx_counter_lookup_prepare built (brx_partbuild.hip: final_view_kernel): the last
//                  level's bucket h >> 12 holds its distinct keys h & 4095 sorted, at most 4096 of them, then padding;
//                  two neighbouring offsets, a binary search of at most 12 steps, the count byte beside the key.
//   count list     the directory that brx_counts_lookup_prepare built (brx_listlookup.hip): bucket khash >> shift is
//                  keys[dir[b] .. dir[b + 1]), 16 keys in the mean; two neighbouring offsets, a binary search over the whole
//                  bucket however large it is, the count byte beside the key.
// A wave bins its counts into a 256-bin histogram of its own in LDS (one LDS atomic per position) and afterwards adds
// the bins that are not zero to the read's row in global memory: integer atomic adds, so nothing depends on the launch
// geometry or on timing.  abund_stats_kernel, a wave per read, turns the 256 bins into the statistics: a prefix sum over
// the bins finds the median, no sort and no floating point.  The rows are the caller's d_hist, or scratch from the pool.
#include "brx_correct.hpp"
#include "brx_tiles.hpp"

using namespace brx;

namespace {

enum { SRC_NONE = 0, SRC_DENSE = 1, SRC_TABLE = 2, SRC_PART = 3, SRC_LIST = 4 }; // what answers: nothing counted yet, the u8 table, the counting table, a partitioned counter's view, a count list's directory

struct AbundArgs {
    // the counter
    const uint8_t *dense;   // u8 per canonical hash
    const uint64_t *lines;  // counting table
    const uint32_t *counts; // its counters, counts[line * 8 + slot]
    uint32_t line_shift, m, w;
    const uint16_t *vkeys;  // count view of a partitioned counter: sorted low 12 bits per bucket, 0xFFFF behind them
    const uint8_t *vcounts; // min(255, count) beside every key
    const uint64_t *voff;   // bucket b = vkeys[voff[b] .. voff[b + 1])
    const uint64_t *lkeys;  // count list: every key, ascending
    const uint8_t *lcnts;   // the count beside every key
    const uint64_t *ldir;   // bucket b = lkeys[ldir[b] .. ldir[b + 1]), b = key >> lshift
    uint32_t lshift;
    int k;
    uint32_t abundance;
    // the batch
    uint32_t n_reads;
    const uint8_t *bases;
    const uint64_t *offsets;
    TileList tl; // work list (brx_tiles.hpp)
    // outputs, each may be null
    uint8_t *profile;
    uint32_t *hist; // 256 per read
    brx_abund_stats_t *stats;
};

// the counter's value for one forward k-mer
template <int SRC>
__device__ __forceinline__ uint32_t abund_count(const AbundArgs &a, uint64_t km)
{
    if (SRC == SRC_NONE)
        return 0u;
    if (SRC == SRC_DENSE)
        return a.dense[khash(km, a.k)];
    if (SRC == SRC_PART) {
        const uint64_t h = khash(km, a.k);
        const uint32_t key = (uint32_t)h & 4095u;
        const uint64_t s = a.voff[h >> 12], e = a.voff[(h >> 12) + 1];
        uint64_t lo = s, hi = e - s > 4096ull ? s + 4096ull : e; // distinct keys first: never more than 4096 of them
        while (lo < hi) { // first entry >= key (the padding is larger than every key)
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if (a.vkeys[mid] < key)
                lo = mid + 1;
            else
                hi = mid;
        }
        // (lo == s + 4096 only if all 4096 keys are there and smaller, which key <= 4095 rules out)
        return lo < e && a.vkeys[lo] == key ? a.vcounts[lo] : 0u;
    }
    if (SRC == SRC_LIST) {
        const uint64_t h = khash(km, a.k); // < 2^(2k-1), so its bucket is one of the directory's
        const uint64_t b = h >> a.lshift;
        const uint64_t e = a.ldir[b + 1];
        uint64_t lo = a.ldir[b], hi = e;
        while (lo < hi) { // first key >= h of the bucket, whatever its size
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if (a.lkeys[mid] < h)
                lo = mid + 1;
            else
                hi = mid;
        }
        return lo < e && a.lkeys[lo] == h ? a.lcnts[lo] : 0u;
    }
    const uint64_t rc = revcomp(km, a.k);
    const uint64_t key = (((popc64(km) & 1) ? rc : km) >> 1) + 1ull;
    const uint32_t home = index_line_of(minimizer_of(km, rc, a.m, a.w), a.line_shift);
    const uint64_t slot = table_lookup_slot(a.lines, a.line_shift, key, home);
    return slot == TAB_NO_SLOT ? 0u : table_count_read(a.counts[slot]);
}

// A wave per tile.
template <int SRC>
__global__ __launch_bounds__(256) void abund_kernel(AbundArgs a)
{
    __shared__ uint32_t bins[4][256];
    TileView t;
    unsigned long long tile;
    if (!tile_view(a.tl, a.offsets, t, tile))
        return;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t r = t.r, n = t.n, p0 = t.p0, p1 = t.p1;
    const uint64_t o0 = t.o0;
    const int lane = threadIdx.x & 63;
    const uint32_t k = (uint32_t)a.k;
    const uint64_t mask = kmask(a.k);
    const uint8_t *in = a.bases + o0;
    uint32_t *const h = bins[wv];
    if (a.hist) {
#pragma unroll
        for (int j = 0; j < 4; j++)
            h[64 * j + lane] = 0u;
        __builtin_amdgcn_wave_barrier();
    }
    // the k-mers wanted START at p0 .. istop-1 and END at p0+k-1 .. elim-1; the scan begins at base p0
    const uint32_t nk = n >= k ? n - k + 1u : 0u;  // k-mers of the read
    const uint32_t istop = p1 < nk ? p1 : nk;      // first start position that is not this tile's (or is no k-mer)
    const uint32_t elim = istop > p0 ? istop + k - 1u : p0; // (<= n)
    uint64_t carry = 0;
    for (uint32_t eb = p0; eb < elim; eb += 64u) {
        const uint32_t e = eb + (uint32_t)lane;
        const uint8_t c = e < elim ? in[e] : (uint8_t)0;
        const uint64_t km = lane_kmer64_dpp(carry, (c >> 1) & 3u, lane, mask);
        carry = wave_carry(km);
        if (e < elim && e - p0 + 1u >= k) { // the k-mer is whole: it starts at e-k+1 >= p0
            const uint32_t cnt = abund_count<SRC>(a, km);
            if (a.profile)
                a.profile[o0 + (e + 1u - k)] = (uint8_t)cnt;
            if (a.hist)
                atomicAdd(&h[cnt], 1u);
        }
    }
    // the bases of the tile where no k-mer starts: the last k-1 of the read (all of a read shorter than k)
    if (a.profile) {
        const uint32_t z0 = istop > p0 ? istop : p0; // z0 .. p1-1: fewer than k <= 31 bases
        if (z0 + (uint32_t)lane < p1)
            a.profile[o0 + z0 + (uint32_t)lane] = 0;
    }
    if (a.hist) {
        __builtin_amdgcn_wave_barrier();
        uint32_t *row = a.hist + (uint64_t)r * 256ull;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t v = h[64 * j + lane];
            if (v)
                atomicAdd(row + 64 * j + lane, v);
        }
    }
}

__device__ __forceinline__ uint32_t wave_sum32(uint32_t v)
{
    for (int d = 32; d > 0; d >>= 1)
        v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}

// A wave per read: lane l holds bins 4l .. 4l+3.
__global__ __launch_bounds__(256) void abund_stats_kernel(AbundArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (uint32_t r = blockIdx.x * 4u + wv; r < a.n_reads; r += gridDim.x * 4u) {
        const uint32_t *row = a.hist + (uint64_t)r * 256ull + 4u * lane; // (a caller's rows need no more than their own alignment)
        const uint32_t b[4] = {row[0], row[1], row[2], row[3]};
        const uint32_t mine = b[0] + b[1] + b[2] + b[3]; // (a read holds fewer than 2^32 k-mers)
        // inclusive prefix sum of `mine` over the lanes
        uint32_t incl = mine;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
            if ((int)lane >= d)
                incl += up;
        }
        const uint32_t kmers = (uint32_t)__shfl((int)incl, 63);
        uint32_t above = 0;
        unsigned long long sum = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const uint32_t v = 4u * lane + j;
            above += v > a.abundance ? b[j] : 0u;
            sum += (unsigned long long)v * b[j];
        }
        above = wave_sum32(above);
        for (int d = 32; d > 0; d >>= 1)
            sum += (unsigned long long)__shfl_xor((long long)sum, d);
        uint32_t vmin = 0, vmax = 0, vmed = 0;
        if (kmers) { // wave-uniform
            const uint64_t has = __ballot(mine != 0u);
            const uint32_t lo = (uint32_t)__ffsll((unsigned long long)has) - 1u, hi = 63u - (uint32_t)__clzll((long long)has);
            const uint32_t first = b[0] ? 0u : (b[1] ? 1u : (b[2] ? 2u : 3u)), last = b[3] ? 3u : (b[2] ? 2u : (b[1] ? 1u : 0u));
            vmin = (uint32_t)__shfl((int)(4u * lane + first), (int)lo);
            vmax = (uint32_t)__shfl((int)(4u * lane + last), (int)hi);
            // element (kmers-1)/2 of the sorted counts: the smallest v whose bins 0..v hold more than that many
            const uint32_t target = (kmers - 1u) / 2u;
            uint32_t run = incl - mine, med = 0;
            bool found = false;
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                run += b[j];
                if (!found && run > target) {
                    found = true;
                    med = 4u * lane + j;
                }
            }
            const uint64_t fm = __ballot(found);
            vmed = (uint32_t)__shfl((int)med, (int)((uint32_t)__ffsll((unsigned long long)fm) - 1u));
        }
        if (lane == 0u) {
            brx_abund_stats_t st;
            st.kmers = kmers;
            st.absent = kmers ? b[0] : 0u;
            st.above = above;
            st.min = vmin;
            st.median = vmed;
            st.max = vmax;
            st.sum = sum;
            a.stats[r] = st;
        }
    }
}

template <int SRC>
__global__ __launch_bounds__(256) void abund_get_kernel(AbundArgs a, const uint64_t *__restrict__ kmers, uint32_t n, uint8_t *__restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n)
        out[i] = (uint8_t)abund_count<SRC>(a, kmers[i] & kmask(a.k));
}

// how the kernels reach the counter; the table's pointers are read here, i.e. inside the caller's lock
int abund_view(const brx_counter *c, const char *what, AbundArgs &a, int &src)
{
    a.k = c->k;
    if (c->strategy == BRX_COUNT_DENSE) {
        a.dense = reinterpret_cast<const uint8_t *>(c->d_counts.get());
        src = SRC_DENSE;
        return BRX_OK;
    }
    if (c->strategy == BRX_COUNT_TABLE) {
        uint32_t log_lines = 0;
        tab_view(c, &a.lines, &a.counts, &log_lines, &a.m);
        src = a.lines ? SRC_TABLE : SRC_NONE;
        if (a.lines) {
            a.line_shift = 32u - log_lines;
            a.w = (uint32_t)c->k - a.m + 1u;
        }
        return BRX_OK;
    }
    if (c->strategy == BRX_COUNT_SORTED && part_lookup_view(c, &a.vkeys, &a.vcounts, &a.voff)) {
        src = a.vkeys ? SRC_PART : SRC_NONE;
        return BRX_OK;
    }
    if (c->strategy == BRX_COUNT_SORTED)
        return abund_refuse_partitioned(what, c->k); // (the view went between the entry's check and its lock)
    set_error("%s: the counter (strategy %d) holds no counts to look up", what, c->strategy);
    return BRX_ERR_UNSUPPORTED;
}

// the same for a prepared count list; the caller holds its lookup lock shared
void abund_view_list(const ListView &l, AbundArgs &a, int &src)
{
    a.k = l.k;
    a.lkeys = l.keys;
    a.lcnts = l.cnts;
    a.ldir = l.dir;
    a.lshift = l.shift;
    src = l.n ? SRC_LIST : SRC_NONE;
}

// `a` holds the view of what answers (src) and the batch
int abund_enqueue(AbundArgs &a, int src, uint64_t total_bases, DevScratch &sc, hipStream_t s)
{
    const uint32_t n_reads = a.n_reads;
    uint64_t tile_bound = 0;
    BRX_TRY(tile_list_enqueue(a.tl, a.offsets, n_reads, total_bases, "abundance", "abund_tiles", sc, tile_bound, s));
    if (a.stats && !a.hist)
        BRX_TRY(sc.get(&a.hist, (uint64_t)n_reads * 256ull));
    if (a.hist)
        BRX_HIP(hipMemsetAsync(a.hist, 0, (uint64_t)n_reads * 1024ull, s));
    {
        KernelTimer t("abund", s);
        const uint32_t grid = (uint32_t)((tile_bound + 3ull) / 4ull);
        if (src == SRC_TABLE)
            abund_kernel<SRC_TABLE><<<grid, 256, 0, s>>>(a);
        else if (src == SRC_PART)
            abund_kernel<SRC_PART><<<grid, 256, 0, s>>>(a);
        else if (src == SRC_DENSE)
            abund_kernel<SRC_DENSE><<<grid, 256, 0, s>>>(a);
        else if (src == SRC_LIST)
            abund_kernel<SRC_LIST><<<grid, 256, 0, s>>>(a);
        else
            abund_kernel<SRC_NONE><<<grid, 256, 0, s>>>(a);
    }
    if (a.stats) {
        KernelTimer t("abund_stats", s);
        abund_stats_kernel<<<read_grid(((uint64_t)n_reads + 3ull) / 4ull, 4096u), 256, 0, s>>>(a);
    }
    BRX_HIP(hipGetLastError());
    return BRX_OK;
}

} // namespace

namespace brx {

int abund_refuse_partitioned(const char *what, int k)
{
    set_error("%s: a partitioned counter (BRX_COUNT_SORTED) holds sorted keys, no counts to look up; count with BRX_COUNT_TABLE "
              "for an abundance profile at k=%d, or build its count view first with brx_counter_lookup_prepare", what, k);
    return BRX_ERR_UNSUPPORTED;
}

} // namespace brx

namespace {

// the body of abund_batch and abund_batch_list: `a` holds the view of what answers
int abund_run(AbundArgs &a, int src, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads, uint64_t total_bases,
              uint8_t abundance, uint8_t *d_profile, uint32_t *d_hist, brx_abund_stats_t *d_stats, hipStream_t s)
{
    DevScratch sc;
    a.abundance = abundance;
    a.n_reads = n_reads;
    a.bases = d_bases;
    a.offsets = d_offsets;
    a.profile = d_profile;
    a.hist = d_hist;
    a.stats = d_stats;
    int st = abund_enqueue(a, src, total_bases, sc, s);
    // the scratch goes back to the pool when this returns: nothing of the call may still be running then
    const hipError_t e = hipStreamSynchronize(s);
    if (st == BRX_OK && e != hipSuccess) {
        set_error("abundance: %s", hipGetErrorString(e));
        st = BRX_ERR_HIP;
    }
    return st;
}

int abund_get_run(const AbundArgs &a, int src, const uint64_t *d_kmers, uint32_t n, uint8_t *d_out, hipStream_t s)
{
    const uint32_t grid = (n + 255u) / 256u;
    if (src == SRC_TABLE)
        abund_get_kernel<SRC_TABLE><<<grid, 256, 0, s>>>(a, d_kmers, n, d_out);
    else if (src == SRC_PART)
        abund_get_kernel<SRC_PART><<<grid, 256, 0, s>>>(a, d_kmers, n, d_out);
    else if (src == SRC_DENSE)
        abund_get_kernel<SRC_DENSE><<<grid, 256, 0, s>>>(a, d_kmers, n, d_out);
    else if (src == SRC_LIST)
        abund_get_kernel<SRC_LIST><<<grid, 256, 0, s>>>(a, d_kmers, n, d_out);
    else
        abund_get_kernel<SRC_NONE><<<grid, 256, 0, s>>>(a, d_kmers, n, d_out);
    BRX_HIP(hipGetLastError());
    return BRX_OK;
}

} // namespace

namespace brx {

int abund_empty_batch(uint32_t n_reads, uint64_t total_bases, uint8_t *d_profile, uint32_t *d_hist, brx_abund_stats_t *d_stats,
                      hipStream_t s, bool *done)
{
    *done = true;
    if (!n_reads || (!d_profile && !d_hist && !d_stats))
        return BRX_OK;
    if (!total_bases) { // reads without bases: no k-mers, and no kernel
        if (d_hist)
            BRX_HIP(hipMemsetAsync(d_hist, 0, (uint64_t)n_reads * 1024ull, s));
        if (d_stats)
            BRX_HIP(hipMemsetAsync(d_stats, 0, (uint64_t)n_reads * sizeof(brx_abund_stats_t), s));
        BRX_HIP(hipStreamSynchronize(s));
        return BRX_OK;
    }
    *done = false;
    return BRX_OK;
}

int abund_batch(const brx_counter *c, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads, uint64_t total_bases,
                uint8_t abundance, uint8_t *d_profile, uint32_t *d_hist, brx_abund_stats_t *d_stats, hipStream_t s)
{
    AbundArgs a{};
    int src = SRC_NONE;
    BRX_TRY(abund_view(c, "abundance", a, src));
    return abund_run(a, src, d_bases, d_offsets, n_reads, total_bases, abundance, d_profile, d_hist, d_stats, s);
}

int abund_batch_list(const ListView &l, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads, uint64_t total_bases,
                     uint8_t abundance, uint8_t *d_profile, uint32_t *d_hist, brx_abund_stats_t *d_stats, hipStream_t s)
{
    AbundArgs a{};
    int src = SRC_NONE;
    abund_view_list(l, a, src);
    return abund_run(a, src, d_bases, d_offsets, n_reads, total_bases, abundance, d_profile, d_hist, d_stats, s);
}

int abund_get_counts(const brx_counter *c, const uint64_t *d_kmers, uint32_t n, uint8_t *d_out, hipStream_t s)
{
    AbundArgs a{};
    int src = SRC_NONE;
    BRX_TRY(abund_view(c, "get_counts", a, src));
    return abund_get_run(a, src, d_kmers, n, d_out, s);
}

int abund_get_counts_list(const ListView &l, const uint64_t *d_kmers, uint32_t n, uint8_t *d_out, hipStream_t s)
{
    AbundArgs a{};
    int src = SRC_NONE;
    abund_view_list(l, a, src);
    return abund_get_run(a, src, d_kmers, n, d_out, s);
}

} // namespace brx
