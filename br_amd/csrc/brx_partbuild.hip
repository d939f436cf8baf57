// Partitioned set build (BRX_COUNT_SORTED): the same bitset as count -> threshold, without the
// 2^(2k-1)-byte count table.
//
// Reference semantics: pcon Counter<u8>::count_fasta + Solid::from_count (src/main.rs:72-115):
// bit h is set iff min(255, occurrences of canonical hash h) > abundance.
//
// Why: random 1-byte RMWs into a 128 GiB table (k=19) run at the chip's random-request ceiling
// (~50 G requests/s, profiles/r1_probe_bench_calibration.txt) and drag two full passes over the
// table behind them (zeroing + thresholding).  Scattered 4-byte stores hit the same ceiling.  So
// the canonical hashes are PARTITIONED by their high bits, MSD-radix style, with streaming passes
// whose writes are staged through LDS into bucket-contiguous runs, until a bucket's hash range
// (2^12 hashes) fits a per-wavefront LDS counter array:
//
//   hash (2k-1 bits) = [ digit 1 | digit 2 | (digit 3) | low 12 bits ]      digits of <= 9 bits
//   level l   histogram pass (LDS histogram per tile, non-zero bins flushed with global atomics),
//             exclusive scan -> child bucket offsets, scatter pass: tile of 4-8 K keys, LDS
//             histogram + block scan, keys ranked into an LDS staging buffer, one global atomic
//             per (tile, bucket) reserves the run, runs written out with consecutive lanes on
//             consecutive addresses.  Level 1 reads the bases (k-mers are re-derived, never stored
//             whole); the last level writes the low 12 bits as u16.
//   final     one wavefront per fine bucket: u16 LDS counters (2 per word), bucket offsets fetched
//             64 at a time and keys two buckets ahead, count -> min(255,.) > abundance -> the
//             bucket's 512-byte slice of the bitset, written whole (no zeroing pass of the bitset).
//
// Order inside a bucket is irrelevant (we only count): no stable ranking, no per-tile prefix
// matrices.  HBM traffic for k=19: ~30 B per k-mer + one 16 GiB bitset write, instead of 129 B
// per k-mer + 2 x 128 GiB.
#include "brx_internal.hpp"
#include "brx_index.hpp"

#include <stdlib.h>
#include <string.h>
#include <atomic>

using namespace brx;

namespace {

constexpr int F_BITS = 12;      // hashes per fine bucket = 4096 (8 KiB of u16 counters per wave)
constexpr int MAX_LEVELS = 4;
constexpr int MAX_DIGIT_BITS = 9;
// (the scans below keep per-thread partial sums in fixed-size arrays: ln_colscan_kernel tot[2] / run[2] covers 512 digits
// with 256 threads, col_scan_digits_kernel one wave's 16 digits per lane covers 1024)
static_assert(MAX_DIGIT_BITS <= 9, "the digit scans of the partition passes are written for at most 512 digits");

struct Plan {
    int k, nbits, nlev;
    int bits[MAX_LEVELS];        // digit width of each level (may be 0 = pass-through)
    int rem_in[MAX_LEVELS];      // key bits entering the level
    uint64_t nchild[MAX_LEVELS]; // number of buckets after the level
};

Plan make_plan(int k)
{
    Plan p;
    memset(&p, 0, sizeof(p));
    p.k = k;
    p.nbits = 2 * k - 1;
    const int P = p.nbits - F_BITS; // bits to partition away
    p.nlev = (P + MAX_DIGIT_BITS - 1) / MAX_DIGIT_BITS;
    if (p.nlev < 2)
        p.nlev = 2;
    int left = P, rem = p.nbits;
    uint64_t nb = 1;
    for (int l = 0; l < p.nlev; l++) {
        int b = (left + (p.nlev - l) - 1) / (p.nlev - l); // spread evenly, larger digits first
        if (l == 0 && p.nbits - b > 32)
            b = p.nbits - 32;                              // what is left after level 1 travels as u32 keys
        p.bits[l] = b;
        p.rem_in[l] = rem;
        rem -= b;
        left -= b;
        nb <<= b;
        p.nchild[l] = nb;
    }
    return p;
}

// ---- 2-bit packing of a window of bases into LDS -------------------------------------------------------
// word w holds window-local bases 16w..16w+15, first base in the top bits, so a k-mer is a 2k-bit
// field of the big-endian bit string.  pack4: ASCII bytes b0..b3 (b0 at the lowest address) ->
// (c0<<6 | c1<<4 | c2<<2 | c3), c = (b >> 1) & 3.
__device__ __forceinline__ uint32_t pack4(uint32_t w)
{
    uint32_t x = __builtin_bswap32((w >> 1) & 0x03030303u);
    x |= x >> 6;
    return (x | (x >> 12)) & 0xffu;
}

#ifndef BRX_L1_UNROLL
#define BRX_L1_UNROLL 4
#endif
#ifndef BRX_XCD_ITEMS
#define BRX_XCD_ITEMS 1
#endif
// -DBRX_DEBUG_BOUNDS=1 (tools/ab_build.sh): every scatter store of the partition passes is checked against the size of
// its destination; an index outside it is counted in bounds_violations (brx_debug_bounds_violations()) and the store
// is dropped.  For builds that leave phases out to time the rest ("results wrong, time only"): such a build has
// undefined offsets, and on a shared pool an undefined offset must not become a wild store (profiles/r2j_ab_runs.txt,
// ab13).  The shipped build compiles none of it.
#ifndef BRX_DEBUG_BOUNDS
#define BRX_DEBUG_BOUNDS 0
#endif
#if BRX_DEBUG_BOUNDS
__device__ unsigned long long bounds_violations = 0ull;
__device__ __forceinline__ bool store_ok(uint64_t idx, uint64_t cap)
{
    if (idx >= cap) {
        atomicAdd(&bounds_violations, 1ull);
        return false;
    }
    return true;
}
#else
__device__ __forceinline__ bool store_ok(uint64_t, uint64_t) { return true; }
#endif
constexpr bool XCD_ITEMS = BRX_XCD_ITEMS != 0;
constexpr uint32_t L1_TILE = 4096;                    // k-mer start positions per level-1 work item = 16 per thread (round 1: 8192 -> scatter 5.4 ms, 4096 -> 4.3, 2048 -> 5.9 at 1 Gbp; the scatter now stages 16 KB of keys + 10 KB of counters: 5 blocks per CU)
constexpr uint32_t PACK_WORDS = L1_TILE / 16 + 4;     // bases of the tile + k - 1 + slack, 16 per word
constexpr uint32_t BND_WORDS = (L1_TILE + 64) / 32 + 2; // read-boundary bitmap of the same window

// packs bases [g0, g0 + nbases) of the batch into pk[]; bases beyond `total` read as A
__device__ __forceinline__ void pack_window(const uint8_t *__restrict__ bases, uint64_t total, uint64_t g0, uint32_t nbases,
                                            uint32_t *__restrict__ pk)
{
    const uint32_t nwords = (nbases + 15u) / 16u;
    for (uint32_t w = threadIdx.x; w < nwords; w += 256) {
        const uint64_t p = g0 + 16ull * w;
        uint32_t v[4] = {0, 0, 0, 0};
        if (p + 16 <= total) {
            uint4 q;
            __builtin_memcpy(&q, bases + p, 16); // one (possibly unaligned) global_load_dwordx4
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            for (uint32_t j = 0; j < 16; j++)
                if (p + j < total)
                    v[j >> 2] |= (uint32_t)bases[p + j] << (8u * (j & 3u));
        }
        pk[w] = (pack4(v[0]) << 24) | (pack4(v[1]) << 16) | (pack4(v[2]) << 8) | pack4(v[3]);
    }
}

// forward k-mer starting at window-local base `pos`
__device__ __forceinline__ uint64_t kmer_at(const uint32_t *__restrict__ pk, uint32_t pos, int k)
{
    const uint32_t w = pos >> 4, sh = 2u * (pos & 15u);
    const uint64_t hi = ((uint64_t)pk[w] << 32) | pk[w + 1];
    const uint64_t lo = pk[w + 2];
    const uint64_t val = sh ? ((hi << sh) | (lo >> (32u - sh))) : hi;
    return val >> (64 - 2 * k);
}

// ---- which work items a workgroup takes (levels >= 2; level 1 gives a block a contiguous range: l1_range) ------------
// Workgroups are dealt round-robin over the 8 XCDs (blocks b and b + 8 share one: MI355X_MICROARCH.md, Workgroup
// dispatch), and tile t + 1 of a scatter appends each digit's keys right behind tile t's -- 32-byte runs at 8 keys per
// digit.  With the plain grid-stride loop neighbouring tiles sit on different XCDs, so every 128-byte line of the output
// is written in pieces from four L2s that cannot merge them.  Here the blocks that share an XCD take one contiguous
// eighth of the items and walk it side by side, so the pieces of a line meet in one L2 and leave as whole lines.
// Speed only: every item is taken exactly once whatever the placement really is.
struct ItemRange {
    unsigned long long first, end, step;
};
__device__ __forceinline__ ItemRange xcd_items(unsigned long long n_items)
{
    const unsigned long long G = gridDim.x, b = blockIdx.x;
    if (G < 8ull || !XCD_ITEMS)
        return {b, n_items, G};
    const unsigned long long x = b & 7ull, j = b >> 3;
    const unsigned long long R = (n_items + 7ull) >> 3;
    const unsigned long long lo = x * R;
    unsigned long long hi = lo + R;
    if (hi > n_items)
        hi = n_items;
    return {lo + j, hi, (G - x + 7ull) >> 3}; // blocks with label x: x, x + 8, ... < G
}

// ---- level 1: tiles of the flat base stream ---------------------------------------------------------------
// Work item i = k-mer start positions [i*L1_TILE, (i+1)*L1_TILE) of the concatenated batch.  A k-mer is
// valid iff it does not run over a read boundary: bnd[] has a bit for every read START (and for the
// end of the batch) inside the window; position p is valid iff no bit is set in (p, p+k-1].
struct L1Args {
    const uint8_t *bases;
    const uint64_t *offsets; // n_reads + 1 (absolute indices into bases; the flat stream starts at offsets[0])
    uint32_t n_reads;
    uint64_t total;          // bases in the batch
    uint32_t n_items;
    int k, nbits, bits;      // digit = hash >> (nbits - bits)
    uint32_t *matrix;        // [n_items][B] per-tile digit counts (hist): a tile's B counters are one coalesced row
    uint32_t n_ranges;       // ranges of tiles = blocks of the partition kernels (l1_range)
    uint64_t *rsum;          // [n_ranges][B]: keys of digit b in range r (hist), then in the ranges before r (col_scan_columns)
    const uint64_t *coff;    // [B + 1] keys of all digits < b (col_scan_digits)
    uint32_t *keys_out;      // hash with the digit stripped
    uint64_t out_cap;        // entries of keys_out (checked under BRX_DEBUG_BOUNDS)
};

// sh_r0[0] = the first read that starts after the tile's first position, upper_bound(offsets, g0): searched for when
// `search` (17 dependent loads by one thread for 100 000 reads -- about 10 us with everybody else waiting, most of a
// tile's time when every tile did it), otherwise carried over from the tile before, which counts in sh_r0[1] the reads
// that start at or before ITS last position while it marks its boundaries: blocks take their tiles in rising order.
__device__ __forceinline__ void l1_prepare(const L1Args &a, uint32_t item, uint32_t *pk, uint32_t *bnd, uint32_t *sh_r0,
                                           uint32_t &n_here, bool search)
{
    const uint64_t off0 = a.offsets[0];
    const uint64_t g0 = (uint64_t)item * L1_TILE;
    const uint64_t left = a.total - g0;
    n_here = (uint32_t)(left < L1_TILE ? left : L1_TILE);
    const uint32_t win = n_here + (uint32_t)a.k + 32u; // bases needed (+ slack for the 3-word extract)
    pack_window(a.bases + off0, a.total, g0, win, pk);
    for (uint32_t w = threadIdx.x; w < BND_WORDS; w += 256)
        bnd[w] = 0;
    if (threadIdx.x == 0) {
        if (search) {
            uint32_t lo = 0, hi = a.n_reads + 1;
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (a.offsets[mid] - off0 <= g0)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            sh_r0[0] = lo;
        } else {
            sh_r0[0] += sh_r0[1];
        }
        sh_r0[1] = 0;
    }
    __syncthreads();
    const uint64_t lim = g0 + n_here + (uint64_t)a.k; // boundaries at window-local positions <= n_here + k - 1 matter
    uint32_t before_next = 0;
    for (uint32_t r = sh_r0[0] + threadIdx.x; r <= a.n_reads; r += 256) {
        const uint64_t o = a.offsets[r] - off0; // offsets[n_reads] - off0 == total: the batch end is a boundary too
        if (o >= lim)
            break;
        const uint32_t p = (uint32_t)(o - g0);
        atomicOr(&bnd[p >> 5], 1u << (p & 31u));
        before_next += o <= g0 + L1_TILE ? 1u : 0u;
    }
    if (before_next)
        atomicAdd(&sh_r0[1], before_next);
    __syncthreads();
}

// a block's tiles: a contiguous range, taken in rising order.  The partition kernels are launched with one block per range
// (part_add_batch), so the histogram's range sums, the scan and the scatter speak of the same ranges.
__device__ __forceinline__ void l1_range(uint32_t n_items, uint32_t &lo, uint32_t &hi)
{
    lo = (uint32_t)(((uint64_t)blockIdx.x * n_items) / gridDim.x);
    hi = (uint32_t)(((uint64_t)(blockIdx.x + 1) * n_items) / gridDim.x);
}

// The same preparation, one tile ahead.  A tile's global loads -- its bases, the first read offsets behind its start, its
// row of counts -- are round trips to memory with everybody waiting, and a block has only its own four waves to hide
// them behind.  l1_fetch() issues them for a LATER tile into registers and does nothing else: no arithmetic on a loaded
// value lives here (a single subtraction made the compiler wait for every load of the fetch right behind it, vmcnt counts
// in issue order), and offsets[0] comes in as a value read once per kernel.  l1_landed() is the one wait for them and
// l1_consume() is l1_prepare() fed from the registers; a k-mer loop always lies between the fetch and that wait.
struct L1Next {
    uint4 q0, q1;  // 16 bases at window word t, and at word 256 + t (the k + 32 bases behind the tile)
    uint64_t off;  // offsets[r_first + t], as loaded
    uint32_t m[(1u << MAX_DIGIT_BITS) / 256u]; // matrix[item][t + 256 q] (scatter only)
};

__device__ __forceinline__ uint32_t l1_window_words(const L1Args &a, uint32_t item, uint32_t &n_here)
{
    const uint64_t left = a.total - (uint64_t)item * L1_TILE;
    n_here = (uint32_t)(left < L1_TILE ? left : L1_TILE);
    return (n_here + (uint32_t)a.k + 32u + 15u) / 16u; // (+ slack for the 3-word extract)
}

template <bool ROW>
__device__ __forceinline__ void l1_fetch(const L1Args &a, uint64_t off0, uint32_t item, uint32_t r_first, L1Next &nx)
{
    const uint8_t *bases = a.bases + off0;
    const uint64_t g0 = (uint64_t)item * L1_TILE;
    uint32_t n_here;
    const uint32_t nwords = l1_window_words(a, item, n_here);
    const uint64_t p0 = g0 + 16ull * threadIdx.x, p1 = p0 + 16ull * 256ull;
    nx.q0 = make_uint4(0, 0, 0, 0);
    nx.q1 = make_uint4(0, 0, 0, 0);
    if (threadIdx.x < nwords && p0 + 16 <= a.total)
        __builtin_memcpy(&nx.q0, bases + p0, 16); // one (possibly unaligned) global_load_dwordx4
    if (256u + threadIdx.x < nwords && p1 + 16 <= a.total)
        __builtin_memcpy(&nx.q1, bases + p1, 16);
    const uint32_t r = r_first + threadIdx.x;
    nx.off = a.offsets[r <= a.n_reads ? r : a.n_reads];
    if (ROW) {
        const uint32_t B = 1u << a.bits;
#pragma unroll
        for (uint32_t q = 0; q < (1u << MAX_DIGIT_BITS) / 256u; q++) {
            const uint32_t b = threadIdx.x + 256u * q;
            nx.m[q] = b < B ? a.matrix[(uint64_t)item * B + b] : 0u;
        }
    }
}

// One wait for everything l1_fetch loaded, at one place for all lanes.  The compiler waits for a load where its value is
// first used; l1_consume uses most of them under lane conditions (window words, digits < B), the waits would stand inside
// those branches, and behind the join the loads count as possibly still in flight: the next l1_fetch then waits for
// "them" before it overwrites the registers -- with vmcnt(0), which drains the stores the kernel has just issued.
template <bool ROW>
__device__ __forceinline__ void l1_landed(const L1Next &nx)
{
    asm volatile("" ::"v"(nx.q0.x), "v"(nx.q0.y), "v"(nx.q0.z), "v"(nx.q0.w), "v"(nx.q1.x), "v"(nx.q1.y), "v"(nx.q1.z), "v"(nx.q1.w),
                 "v"(nx.off));
    if (ROW) {
#pragma unroll
        for (uint32_t q = 0; q < (1u << MAX_DIGIT_BITS) / 256u; q++)
            asm volatile("" ::"v"(nx.m[q]));
    }
}

__device__ __forceinline__ uint32_t l1_pack16(const L1Args &a, uint64_t off0, const uint4 &q, uint64_t p)
{
    uint32_t v[4] = {q.x, q.y, q.z, q.w};
    if (p + 16 > a.total) { // the batch ends inside these 16 bases (its last tile only): byte by byte, beyond the end reads as A
        const uint8_t *bases = a.bases + off0;
        v[0] = v[1] = v[2] = v[3] = 0;
        for (uint32_t j = 0; j < 16; j++)
            if (p + j < a.total)
                v[j >> 2] |= (uint32_t)bases[p + j] << (8u * (j & 3u));
    }
    return (pack4(v[0]) << 24) | (pack4(v[1]) << 16) | (pack4(v[2]) << 8) | pack4(v[3]);
}

// nx = l1_fetch(item, r_first); r_first = the first read that starts after the tile's first position (searched for at the
// head of a range, afterwards the r_first of the tile before + its sh_r0[1], the reads that start at or before ITS last
// position).  Leaves pk[], bnd[] and sh_r0[1] of `item` behind; the CALLER ends it with a barrier.
// The 256 offsets that came with the fetch nearly always reach past the window: offsets are sorted, so thread 255 can
// tell, and publishes it in sh_r0[2] before the barrier that is here anyway.  Only a window with more than 256 read
// starts goes back to memory (correct, and as slow as it was).
__device__ __forceinline__ void l1_consume(const L1Args &a, uint64_t off0, uint32_t item, const L1Next &nx, uint32_t r_first, uint32_t *pk,
                                           uint32_t *bnd, uint32_t *sh_r0, uint32_t &n_here)
{
    const uint64_t g0 = (uint64_t)item * L1_TILE;
    const uint32_t nwords = l1_window_words(a, item, n_here);
    if (threadIdx.x < nwords)
        pk[threadIdx.x] = l1_pack16(a, off0, nx.q0, g0 + 16ull * threadIdx.x);
    if (256u + threadIdx.x < nwords)
        pk[256u + threadIdx.x] = l1_pack16(a, off0, nx.q1, g0 + 16ull * (256u + threadIdx.x));
    for (uint32_t w = threadIdx.x; w < BND_WORDS; w += 256)
        bnd[w] = 0;
    const uint64_t lim = g0 + n_here + (uint64_t)a.k; // boundaries at window-local positions <= n_here + k - 1 matter
    const uint32_t r = r_first + threadIdx.x;
    const uint64_t o = nx.off - off0; // offsets[n_reads] - off0 == total: the batch end is a boundary too
    const bool mine = r <= a.n_reads && o < lim;
    if (threadIdx.x == 0)
        sh_r0[1] = 0;
    if (threadIdx.x == 255)
        sh_r0[2] = mine ? 1u : 0u; // the window reaches past the offsets that were fetched
    __syncthreads();
    if (mine) {
        uint32_t p = (uint32_t)(o - g0);
        atomicOr(&bnd[p >> 5], 1u << (p & 31u));
        uint32_t before_next = o <= g0 + L1_TILE ? 1u : 0u;
        if (sh_r0[2])
            for (uint32_t r2 = r + 256u; r2 <= a.n_reads; r2 += 256u) {
                const uint64_t o2 = a.offsets[r2] - off0;
                if (o2 >= lim)
                    break;
                p = (uint32_t)(o2 - g0);
                atomicOr(&bnd[p >> 5], 1u << (p & 31u));
                before_next += o2 <= g0 + L1_TILE ? 1u : 0u;
            }
        if (before_next)
            atomicAdd(&sh_r0[1], before_next);
    }
}

// upper_bound(offsets, first position of tile `item`) into sh_r0[0]; ends with a barrier
__device__ __forceinline__ void l1_search(const L1Args &a, uint64_t off0, uint32_t item, uint32_t *sh_r0)
{
    if (threadIdx.x == 0) {
        const uint64_t g0 = (uint64_t)item * L1_TILE;
        uint32_t lo = 0, hi = a.n_reads + 1;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (a.offsets[mid] - off0 <= g0)
                lo = mid + 1;
            else
                hi = mid;
        }
        sh_r0[0] = lo;
    }
    __syncthreads();
}

// true iff no read boundary lies in window-local positions (p, p + k - 1]
__device__ __forceinline__ bool l1_valid(const uint32_t *bnd, uint32_t p, int k)
{
    const uint32_t q = p + 1u; // first position to test, k-1 <= 30 bits
    const uint32_t w = q >> 5, sh = q & 31u;
    const uint64_t two = ((uint64_t)bnd[w + 1] << 32) | bnd[w];
    const uint32_t bits = (uint32_t)(two >> sh) & ((k > 1) ? ((1u << (k - 1)) - 1u) : 0u);
    return bits == 0u;
}

// Every valid k-mer of the tile, rolled: thread t takes window positions 16t .. 16t+15 (L1_TILE = 256 x 16), builds the
// first k-mer and its reverse complement once and then shifts one base in per step -- f(canonical hash) -- instead of
// cutting every k-mer out of pk[] (three LDS reads, a funnel shift, a 64-bit bit reversal) and testing the boundary
// bitmap with two more LDS reads per position.  Both level-1 kernels are bound by the instructions they issue.
static_assert(L1_TILE == 256u * 16u, "l1_for_each_hash: 16 positions per thread");
template <int UNROLL = 4, typename F>
__device__ __forceinline__ void l1_for_each_hash(const uint32_t *__restrict__ pk, const uint32_t *__restrict__ bnd, uint32_t n_here,
                                                 int k, F &&f)
{
    const uint32_t p0 = threadIdx.x * 16u;
    if (p0 >= n_here)
        return;
    const uint32_t w = threadIdx.x; // p0 / 16
    const uint64_t hi = ((uint64_t)pk[w] << 32) | pk[w + 1];
    const uint64_t lo = pk[w + 2];
    const uint64_t mask = kmask(k);
    uint64_t fwd = hi >> (64 - 2 * k);
    uint64_t rc = revcomp(fwd, k);
    // the bases behind the first k-mer, the next one in the top two bits (the 96-bit string hi:lo shifted left by 2k)
    uint64_t next = (hi << (2 * k)) | (2 * k >= 32 ? lo << (2 * k - 32) : lo >> (32 - 2 * k));
    // bit i = a read starts at window position p0 + 1 + i; position p0 + j is valid iff bits j .. j + k - 2 are clear
    const uint32_t q = p0 + 1u, wq = q >> 5, sh = q & 31u;
    uint64_t vb = ((((uint64_t)bnd[wq + 1] << 32) | bnd[wq]) >> sh) | (sh ? (uint64_t)bnd[wq + 2] << (64u - sh) : 0ull);
    const uint64_t vmask = k > 1 ? (1ull << (k - 1)) - 1ull : 0ull;
    const uint32_t left = n_here - p0 < 16u ? n_here - p0 : 16u;
    const int top = 2 * k - 2;
#pragma unroll UNROLL
    for (uint32_t j = 0; j < left; j++) {
        if ((vb & vmask) == 0ull)
            f(((popc64(fwd) & 1) ? rc : fwd) >> 1);
        const uint64_t b = next >> 62;
        next <<= 2;
        vb >>= 1;
        fwd = ((fwd << 2) | b) & mask;
        rc = (rc >> 2) | ((b ^ 2ull) << top);
    }
}

#ifndef BRX_L1HIST_WAVES
#define BRX_L1HIST_WAVES 1 // (1 = the compiler's choice: 76 registers, six waves; tools/ab_build.sh sweeps it)
#endif
constexpr uint32_t L1_OWN = ((1u << MAX_DIGIT_BITS) + 255u) / 256u; // digits per lane: t, t + 256

// One block per range of tiles.  Per tile: the k-mer loop, a barrier, then -- with pk[] and bnd[] dead -- the NEXT tile is
// consumed from the registers its loads went to before that loop, and only then this tile's row of counts is stored and
// the loads of the tile after the next are issued: three barriers per tile, and nothing waits for memory except the wait
// in l1_consume, a k-mer loop behind the loads it waits for.  Each lane also adds up its digits over the range:
// rsum[range][B], from which the scan forms where every range starts (col_scan_* below).
__global__ __launch_bounds__(256, BRX_L1HIST_WAVES) void l1_hist_kernel(L1Args a)
{
    extern __shared__ uint32_t lds[]; // hist[B]
    __shared__ uint32_t pk[PACK_WORDS];
    __shared__ uint32_t bnd[BND_WORDS];
    __shared__ uint32_t sh_r0[3];
    const uint32_t B = 1u << a.bits;
    const int shift = a.nbits - a.bits;
    uint32_t lo, hi;
    l1_range(a.n_items, lo, hi);
    uint64_t rs[L1_OWN];
#pragma unroll
    for (uint32_t q = 0; q < L1_OWN; q++)
        rs[q] = 0;
    if (lo < hi) {
        const uint64_t off0 = a.offsets[0];
        l1_search(a, off0, lo, sh_r0);
        uint32_t r_first = sh_r0[0];
        L1Next nx;
        l1_fetch<false>(a, off0, lo, r_first, nx);
        for (uint32_t b = threadIdx.x; b < B; b += 256)
            lds[b] = 0;
        uint32_t n_here;
        l1_landed<false>(nx);
        l1_consume(a, off0, lo, nx, r_first, pk, bnd, sh_r0, n_here);
        __syncthreads();
        r_first += sh_r0[1];
        l1_fetch<false>(a, off0, lo + 1 < hi ? lo + 1 : lo, r_first, nx);
        for (uint32_t item = lo; item < hi; item++) {
            l1_for_each_hash(pk, bnd, n_here, a.k, [&](uint64_t h) { atomicAdd(&lds[(uint32_t)(h >> shift)], 1u); });
            __syncthreads();
            uint32_t row[L1_OWN];
#pragma unroll
            for (uint32_t q = 0; q < L1_OWN; q++) {
                const uint32_t b = threadIdx.x + 256u * q;
                row[q] = 0;
                if (b < B) {
                    row[q] = lds[b];
                    lds[b] = 0;
                }
            }
            l1_landed<false>(nx); // (in front of the branch: the last tile's fetch below overwrites nx, too)
            if (item + 1 < hi) {
                l1_consume(a, off0, item + 1, nx, r_first, pk, bnd, sh_r0, n_here);
                __syncthreads();
                r_first += sh_r0[1];
            }
#pragma unroll
            for (uint32_t q = 0; q < L1_OWN; q++) {
                const uint32_t b = threadIdx.x + 256u * q;
                if (b < B)
                    a.matrix[(uint64_t)item * B + b] = row[q];
                rs[q] += row[q];
            }
            // (past the end of the range: the last tile once more, into registers nobody reads)
            l1_fetch<false>(a, off0, item + 2 < hi ? item + 2 : hi - 1, r_first, nx);
        }
    }
#pragma unroll
    for (uint32_t q = 0; q < L1_OWN; q++) {
        const uint32_t b = threadIdx.x + 256u * q;
        if (b < B && store_ok((uint64_t)blockIdx.x * B + b, (uint64_t)a.n_ranges * B))
            a.rsum[(uint64_t)blockIdx.x * B + b] = rs[q];
    }
}

// ---- where every range of tiles starts, from the [n_ranges][B] range sums ----------------------------------------------
// The scatter needs, per block, where each digit's keys of its first tile go: (keys of all digits < b) + (keys of digit b
// in the ranges before); from there it follows its own tiles' counts.  The per-tile counts stay tile-major
// (matrix[n_items][B]: a tile reads and writes its B counters as one coalesced row -- digit-major made every tile touch
// B separate cache lines, 0.25 random line accesses per key), but no position per (tile, digit) is formed any more: the
// histogram blocks leave one row of sums per range, one block per digit scans its column in place, one wave scans the
// column totals into the digit offsets, and the scatter adds the two.
// block b: exclusive scan of column b of part[n_rows][B] in place, its total -> coltot[b]
__global__ __launch_bounds__(256) void col_scan_columns_kernel(uint64_t *__restrict__ part, uint32_t n_rows, uint32_t B,
                                                               uint64_t *__restrict__ coltot)
{
    __shared__ uint64_t wsum[4];
    const uint32_t b = blockIdx.x;
    const uint32_t per = (n_rows + 255u) / 256u;
    const uint32_t c0 = threadIdx.x * per;
    uint64_t mine = 0;
    for (uint32_t q = 0; q < per; q++) {
        const uint32_t c = c0 + q;
        if (c < n_rows)
            mine += part[(uint64_t)c * B + b];
    }
    uint64_t incl = mine;
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t t = __shfl_up(incl, d);
        if ((threadIdx.x & 63) >= (unsigned)d)
            incl += t;
    }
    if ((threadIdx.x & 63) == 63)
        wsum[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint64_t base = 0;
    for (uint32_t w = 0; w < (threadIdx.x >> 6); w++)
        base += wsum[w];
    uint64_t run = base + incl - mine;
    for (uint32_t q = 0; q < per; q++) {
        const uint32_t c = c0 + q;
        if (c < n_rows) {
            const uint64_t v = part[(uint64_t)c * B + b];
            part[(uint64_t)c * B + b] = run;
            run += v;
        }
    }
    if (threadIdx.x == 255)
        coltot[b] = base + incl;
}

// one wave: coff[b] = keys of all digits < b, coff[B] = *total = number of keys (B <= 1024)
__global__ __launch_bounds__(64) void col_scan_digits_kernel(const uint64_t *__restrict__ coltot, uint32_t B, uint64_t *__restrict__ coff,
                                                             unsigned long long *__restrict__ total)
{
    uint64_t carry = 0;
    for (uint32_t b0 = 0; b0 < B; b0 += 64) {
        const uint32_t b = b0 + threadIdx.x;
        const uint64_t v = b < B ? coltot[b] : 0;
        uint64_t incl = v;
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t t = __shfl_up(incl, d);
            if (threadIdx.x >= (unsigned)d)
                incl += t;
        }
        if (b < B)
            coff[b] = carry + incl - v;
        carry += __shfl(incl, 63);
    }
    if (threadIdx.x == 0) {
        coff[B] = carry;
        *total = carry;
    }
}

// presence-only insertion over the FLAT base stream (Pcon::from_fasta / Hash::from_fasta): the same tiles and
// read-boundary bitmap as the level-1 partition, so one 250 Mbp record keeps the whole chip busy instead of
// one workgroup.  TABLE = false: atomicOr into the bit vector; TABLE = true: find-or-insert into the chained
// table of a sparse set (n_new counts the k-mers that were not there yet).
template <bool TABLE>
__global__ __launch_bounds__(256) void flat_insert_kernel(L1Args a, uint32_t *__restrict__ bits, uint64_t *__restrict__ lines,
                                                          uint32_t line_shift, uint32_t m, uint32_t w,
                                                          unsigned long long *__restrict__ n_new)
{
    __shared__ uint32_t pk[PACK_WORDS];
    __shared__ uint32_t bnd[BND_WORDS];
    __shared__ uint32_t sh_r0[2];
    uint32_t added = 0;
    uint32_t lo, hi;
    l1_range(a.n_items, lo, hi);
    for (uint32_t item = lo; item < hi; item++) {
        uint32_t n_here;
        l1_prepare(a, item, pk, bnd, sh_r0, n_here, item == lo);
        for (uint32_t p = threadIdx.x; p < n_here; p += 256)
            if (l1_valid(bnd, p, a.k)) {
                const uint64_t kmer = kmer_at(pk, p, a.k);
                if (TABLE) {
                    added += table_find_or_insert(lines, line_shift, m, w, a.k, kmer) ? 1u : 0u;
                } else {
                    const uint64_t h = khash(kmer, a.k);
                    atomicOr(bits + (h >> 5), 1u << (h & 31u));
                }
            }
        __syncthreads();
    }
    if (TABLE) {
        for (int d = 32; d > 0; d >>= 1)
            added += __shfl_down(added, d);
        if ((threadIdx.x & 63) == 0 && added)
            atomicAdd(n_new, (unsigned long long)added);
    }
}

// counting into the chained table (BRX_COUNT_TABLE, brx_counttable.hip): flat_insert_kernel<true>'s walk over the tiles,
// and every valid k-mer then adds one to the counter of the slot that holds it (n_new: keys this launch put in)
__global__ __launch_bounds__(256) void flat_count_kernel(L1Args a, uint64_t *__restrict__ lines, uint32_t *__restrict__ counts,
                                                         uint32_t line_shift, uint32_t m, uint32_t w, unsigned long long *__restrict__ n_new)
{
    __shared__ uint32_t pk[PACK_WORDS];
    __shared__ uint32_t bnd[BND_WORDS];
    __shared__ uint32_t sh_r0[2];
    uint32_t added = 0;
    uint32_t lo, hi;
    l1_range(a.n_items, lo, hi);
    for (uint32_t item = lo; item < hi; item++) {
        uint32_t n_here;
        l1_prepare(a, item, pk, bnd, sh_r0, n_here, item == lo);
        for (uint32_t p = threadIdx.x; p < n_here; p += 256)
            if (l1_valid(bnd, p, a.k)) {
                bool fresh;
                const uint64_t slot = table_find_or_claim(lines, line_shift, m, w, a.k, kmer_at(pk, p, a.k), fresh);
                added += fresh ? 1u : 0u;
                table_count_bump(counts + slot);
            }
        __syncthreads();
    }
    for (int d = 32; d > 0; d >>= 1)
        added += __shfl_down(added, d);
    if ((threadIdx.x & 63) == 0 && added)
        atomicAdd(n_new, (unsigned long long)added);
}

// ---- sliced counting (brx_counter_set_slice): only the k-mers with table_owner_of(hash, parts) == part ----------------
// flat_count_kernel's tiles and rounds of 256 positions.  The walk into the table is a chain of dependent 64-byte probes
// and costs a wave about the same with one lane active as with 64, so a filter in front of it would make each of the
// `parts` sweeps as dear as a whole count.  Instead every wave keeps a ring of SLICE_QUEUE forward k-mers in LDS: a round
// appends the k-mers of the part among its 64 positions (ballot + prefix), and as soon as 64 are queued the wave takes
// them out and walks them with every lane busy.  At most 63 stay behind a walk and a round adds at most 64: 127 < 128,
// so a tile in which every k-mer belongs to the part (a homopolymer read) fits like any other.  The ring lives through
// the tiles of the block's range and only its last, partial content is walked by a partial wave.  A wave's LDS
// instructions execute in order, so its own appends are visible to its own reads without a barrier; the ring is the
// wave's alone.  No block barrier beyond the tile's.
constexpr uint32_t SLICE_QUEUE = 128;

// this lane's position of the round: is its k-mer valid, and the part's (then `kmer` holds it)
__device__ __forceinline__ bool slice_take(const L1Args &a, const uint32_t *pk, const uint32_t *bnd, uint32_t p, uint32_t n_here,
                                           uint32_t part, uint32_t parts, uint64_t &kmer, uint32_t &seen)
{
    if (p >= n_here || !l1_valid(bnd, p, a.k))
        return false;
    seen++;
    kmer = kmer_at(pk, p, a.k);
    return table_owner_of(khash(kmer, a.k), parts) == part;
}

// stats4 (brx_counter_slice_stats): valid k-mers seen, k-mers of the part, wave trips into the walk, waves launched
__global__ __launch_bounds__(256) void flat_count_slice_kernel(L1Args a, uint64_t *__restrict__ lines, uint32_t *__restrict__ counts,
                                                               uint32_t line_shift, uint32_t m, uint32_t w, uint32_t part, uint32_t parts,
                                                               unsigned long long *__restrict__ n_new,
                                                               unsigned long long *__restrict__ stats4)
{
    __shared__ uint32_t pk[PACK_WORDS];
    __shared__ uint32_t bnd[BND_WORDS];
    __shared__ uint32_t sh_r0[2];
    __shared__ uint64_t queue[4][SLICE_QUEUE];
    uint64_t *q = queue[threadIdx.x >> 6];
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t added = 0, seen = 0;
    uint32_t head = 0, queued = 0, trips = 0; // wave-uniform
    unsigned long long walked = 0;            // wave-uniform
    uint32_t lo, hi;
    l1_range(a.n_items, lo, hi);
    for (uint32_t item = lo; item < hi; item++) {
        uint32_t n_here;
        l1_prepare(a, item, pk, bnd, sh_r0, n_here, item == lo);
        for (uint32_t p0 = 0; p0 < n_here; p0 += 256) { // (block-uniform: every lane of the wave is in every round)
            uint64_t kmer = 0;
            const bool mine = slice_take(a, pk, bnd, p0 + threadIdx.x, n_here, part, parts, kmer, seen);
            const unsigned long long mask = __ballot(mine);
            if (mine)
                q[(head + queued + (uint32_t)__popcll(mask & below)) & (SLICE_QUEUE - 1u)] = kmer;
            queued += (uint32_t)__popcll(mask);
            if (queued >= 64u) { // wave-uniform
                __builtin_amdgcn_wave_barrier();
                const uint64_t mer = q[(head + lane) & (SLICE_QUEUE - 1u)];
                __builtin_amdgcn_wave_barrier();
                head = (head + 64u) & (SLICE_QUEUE - 1u);
                queued -= 64u;
                bool fresh;
                const uint64_t slot = table_find_or_claim(lines, line_shift, m, w, a.k, mer, fresh);
                added += fresh ? 1u : 0u;
                table_count_bump(counts + slot);
                walked += 64ull;
                trips++;
            }
        }
        __syncthreads();
    }
    if (queued) { // what is left at the end of the range: the one walk of a partial wave
        __builtin_amdgcn_wave_barrier();
        if (lane < queued) {
            bool fresh;
            const uint64_t slot = table_find_or_claim(lines, line_shift, m, w, a.k, q[(head + lane) & (SLICE_QUEUE - 1u)], fresh);
            added += fresh ? 1u : 0u;
            table_count_bump(counts + slot);
        }
        walked += queued;
        trips++;
    }
    for (int d = 32; d > 0; d >>= 1) {
        added += __shfl_down(added, d);
        seen += __shfl_down(seen, d);
    }
    if (lane == 0u) {
        if (added)
            atomicAdd(n_new, (unsigned long long)added);
        if (seen)
            atomicAdd(stats4 + 0, (unsigned long long)seen);
        if (walked)
            atomicAdd(stats4 + 1, walked);
        if (trips)
            atomicAdd(stats4 + 2, (unsigned long long)trips);
        atomicAdd(stats4 + 3, 1ull);
    }
}

// the sizing pass of a sliced counter: the same tiles and the same owner test without the table.  out2[0] grows by the
// batch's k-mers of the part (occurrences), out2[1] by its valid k-mers
__global__ __launch_bounds__(256) void flat_slice_census_kernel(L1Args a, uint32_t part, uint32_t parts, unsigned long long *__restrict__ out2)
{
    __shared__ uint32_t pk[PACK_WORDS];
    __shared__ uint32_t bnd[BND_WORDS];
    __shared__ uint32_t sh_r0[2];
    uint32_t owned = 0, seen = 0;
    uint32_t lo, hi;
    l1_range(a.n_items, lo, hi);
    for (uint32_t item = lo; item < hi; item++) {
        uint32_t n_here;
        l1_prepare(a, item, pk, bnd, sh_r0, n_here, item == lo);
        for (uint32_t p = threadIdx.x; p < n_here; p += 256) {
            uint64_t kmer;
            owned += slice_take(a, pk, bnd, p, n_here, part, parts, kmer, seen) ? 1u : 0u;
        }
        __syncthreads();
    }
    for (int d = 32; d > 0; d >>= 1) {
        owned += __shfl_down(owned, d);
        seen += __shfl_down(seen, d);
    }
    if ((threadIdx.x & 63) == 0 && seen) {
        atomicAdd(out2 + 0, (unsigned long long)owned);
        atomicAdd(out2 + 1, (unsigned long long)seen);
    }
}

// shared by the scatter kernels: block scan of cntv -> lofs/lcur (all in LDS), in two halves around one barrier so that
// a caller with a barrier of its own there can share it
__device__ __forceinline__ void scan_bins_begin(uint32_t B, const uint32_t *cntv, uint32_t *sh_wsum, uint32_t &mine, uint32_t &incl)
{
    const uint32_t BPT = (B + 255u) / 256u; // bins per thread (1 or 2)
    mine = 0;
    for (uint32_t q = 0; q < BPT; q++) {
        const uint32_t b = threadIdx.x * BPT + q;
        if (b < B)
            mine += cntv[b];
    }
    incl = mine;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(incl, d);
        if ((threadIdx.x & 63) >= (unsigned)d)
            incl += t;
    }
    if ((threadIdx.x & 63) == 63)
        sh_wsum[threadIdx.x >> 6] = incl;
}

__device__ __forceinline__ void scan_bins_end(uint32_t B, const uint32_t *cntv, uint32_t *lofs, uint32_t *lcur, const uint32_t *sh_wsum,
                                              uint32_t mine, uint32_t incl)
{
    const uint32_t BPT = (B + 255u) / 256u;
    uint32_t wbase = 0;
    for (uint32_t w = 0; w < (threadIdx.x >> 6); w++)
        wbase += sh_wsum[w];
    uint32_t run = wbase + incl - mine;
    for (uint32_t q = 0; q < BPT; q++) {
        const uint32_t b = threadIdx.x * BPT + q;
        if (b < B) {
            lofs[b] = run;
            lcur[b] = run;
            run += cntv[b];
        }
    }
}

__device__ __forceinline__ void block_scan_bins(uint32_t B, const uint32_t *cntv, uint32_t *lofs, uint32_t *lcur, uint32_t *sh_wsum)
{
    uint32_t mine, incl;
    scan_bins_begin(B, cntv, sh_wsum, mine, incl);
    __syncthreads();
    scan_bins_end(B, cntv, lofs, lcur, sh_wsum, mine, incl);
}

// Level-1 write-out in whole 32-byte sectors.  A tile leaves T / B = 8 keys per digit on average: written where they
// belong, that is a 32-byte run at a 4-byte-aligned place, 1.87 sectors touched per run (WRITE_SIZE counted exactly that,
// profiles/r2j_*), every one of them a partial write.  But the runs of one digit from CONSECUTIVE tiles lie end to end
// (pos[t + 1][d] = pos[t][d] + count[t][d]), so a block that takes a contiguous range of tiles can hold back the keys
// behind each digit's last sector boundary (a carry of < 8 keys per digit, in LDS) and write them with the next tile's:
// only the two ends of a block's range are partial.  The first sector of a range starts with the `ph` places that belong
// to the range before (phantoms: kept as holes in the carry, never stored).
constexpr uint32_t L1_SECTOR = 8;                              // keys per 32-byte sector

// A tile: its counts, bases and read offsets are consumed from the registers l1_fetch filled a tile ago, the loads of the
// next tile are issued, and the k-mer loop and the write-out run while those are under way.  Six barriers per tile.
// Consuming tile i + 1 between the k-mer loop and the write-out of tile i, so that the wait for the loads would not also
// count the stores just issued (vmcnt is in issue order), takes two barriers fewer and was measured SLOWER
// (profiles/r7_partition_waits.txt): the order here is the one that measured best.
#ifndef BRX_L1SCAT_WAVES
#define BRX_L1SCAT_WAVES 5
#endif
__global__ __launch_bounds__(256, BRX_L1SCAT_WAVES) void l1_scatter_kernel(L1Args a)
{
    // LDS: stage_key[T] | gsm[B] (u64: sector index | keys carried << 32 | phantoms << 36) | cnt[B] | lofs[B] | lcur[B]
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    __shared__ uint32_t pk[PACK_WORDS];
    __shared__ uint32_t bnd[BND_WORDS];
    __shared__ uint32_t sh_r0[3];
    __shared__ uint32_t sh_wsum[4];
    const uint32_t T = L1_TILE;
    const uint32_t B = 1u << a.bits;
    uint32_t *stage_key = (uint32_t *)lds_raw;
    unsigned long long *gsm = (unsigned long long *)(stage_key + T);
    uint32_t *cntv = (uint32_t *)(gsm + B);
    uint32_t *lofs = cntv + B;
    uint32_t *lcur = lofs + B;
    const int shift = a.nbits - a.bits;
    const uint64_t child_mask = (1ull << shift) - 1ull;
    uint32_t lo, hi;
    l1_range(a.n_items, lo, hi);
    if (lo >= hi)
        return;
    for (uint32_t b = threadIdx.x; b < B; b += 256) {
        // where digit b of this range starts: behind all smaller digits and behind digit b of the ranges before
        const unsigned long long p0 = a.coff[b] + a.rsum[(uint64_t)blockIdx.x * B + b];
        const unsigned long long ph = p0 & (L1_SECTOR - 1);
        gsm[b] = (p0 / L1_SECTOR) | (ph << 32) | (ph << 36);
    }
    uint32_t creg[L1_OWN][L1_SECTOR]; // the carries of this lane's digits
#pragma unroll
    for (uint32_t q = 0; q < L1_OWN; q++)
#pragma unroll
        for (uint32_t jj = 0; jj < L1_SECTOR; jj++)
            creg[q][jj] = 0;
    const uint64_t off0 = a.offsets[0];
    l1_search(a, off0, lo, sh_r0);
    uint32_t r_first = sh_r0[0];
    L1Next nx;
    l1_fetch<true>(a, off0, lo, r_first, nx);
    for (uint32_t item = lo; item < hi; item++) {
        l1_landed<true>(nx);
#pragma unroll
        for (uint32_t q = 0; q < L1_OWN; q++)
            if (threadIdx.x + 256u * q < B)
                cntv[threadIdx.x + 256u * q] = nx.m[q]; // the histogram pass already counted this tile
        uint32_t n_here;
        l1_consume(a, off0, item, nx, r_first, pk, bnd, sh_r0, n_here);
        uint32_t mine, incl;
        scan_bins_begin(B, cntv, sh_wsum, mine, incl); // (shares the barrier that ends l1_consume)
        __syncthreads();
        r_first += sh_r0[1];
        scan_bins_end(B, cntv, lofs, lcur, sh_wsum, mine, incl);
        // (past the end of the range: the last tile once more, into registers nobody reads)
        l1_fetch<true>(a, off0, item + 1 < hi ? item + 1 : item, r_first, nx);
        __syncthreads();
        l1_for_each_hash<BRX_L1_UNROLL>(pk, bnd, n_here, a.k, [&](uint64_t h) {
            const uint32_t d = (uint32_t)(h >> shift);
            const uint32_t slot = atomicAdd(&lcur[d], 1u);
            stage_key[slot] = (uint32_t)(h & child_mask);
        });
        __syncthreads();
        // one digit per lane: carry + the tile's keys leave as whole sectors (two 16-byte stores), the rest is the new carry
#pragma unroll
        for (uint32_t q = 0; q < L1_OWN; q++) {
            const uint32_t d = threadIdx.x + 256u * q;
            if (d < B) {
                const unsigned long long m = gsm[d];
                const uint32_t n = cntv[d], base = lofs[d];
                const uint32_t gsx = (uint32_t)m, cc = (uint32_t)(m >> 32) & 15u, ph = (uint32_t)(m >> 36) & 15u;
                const uint32_t tot = cc + n, full = tot / L1_SECTOR, r = tot % L1_SECTOR;
                const uint32_t src = base - cc; // element e >= cc of the run is stage_key[src + e]
                uint32_t *out = a.keys_out + (unsigned long long)gsx * L1_SECTOR;
                for (uint32_t sct = 0; sct < full; sct++) {
                    uint32_t v[L1_SECTOR];
#pragma unroll
                    for (uint32_t jj = 0; jj < L1_SECTOR; jj++) {
                        const uint32_t e = L1_SECTOR * sct + jj;
                        v[jj] = e < cc ? creg[q][jj] : stage_key[src + e];
                    }
                    if (store_ok((unsigned long long)(gsx + sct) * L1_SECTOR + 7u, a.out_cap)) {
                        if (sct == 0 && ph) { // the first sector of the range: its first places are the range before's
#pragma unroll
                            for (uint32_t jj = 0; jj < L1_SECTOR; jj++)
                                if (jj >= ph)
                                    out[jj] = v[jj];
                        } else {
                            uint4 *o4 = reinterpret_cast<uint4 *>(out + L1_SECTOR * sct);
                            o4[0] = make_uint4(v[0], v[1], v[2], v[3]);
                            o4[1] = make_uint4(v[4], v[5], v[6], v[7]);
                        }
                    }
                }
                if (full) {
#pragma unroll
                    for (uint32_t jj = 0; jj < L1_SECTOR; jj++)
                        creg[q][jj] = jj < r ? stage_key[src + L1_SECTOR * full + jj] : 0u;
                    gsm[d] = (unsigned long long)(gsx + full) | ((unsigned long long)r << 32);
                } else {
#pragma unroll
                    for (uint32_t jj = 0; jj < L1_SECTOR; jj++)
                        creg[q][jj] = jj < cc ? creg[q][jj] : (jj < r ? stage_key[src + jj] : 0u);
                    gsm[d] = (unsigned long long)gsx | ((unsigned long long)r << 32) | ((unsigned long long)ph << 36);
                }
            }
        }
        __syncthreads();
    }
    // the end of the range: what is still held back
#pragma unroll
    for (uint32_t q = 0; q < L1_OWN; q++) {
        const uint32_t d = threadIdx.x + 256u * q;
        if (d < B) {
            const unsigned long long m = gsm[d];
            const uint32_t cc = (uint32_t)(m >> 32) & 15u, ph = (uint32_t)(m >> 36) & 15u;
            const unsigned long long g = (unsigned long long)(uint32_t)m * L1_SECTOR;
#pragma unroll
            for (uint32_t jj = 0; jj < L1_SECTOR; jj++)
                if (jj >= ph && jj < cc && store_ok(g + jj, a.out_cap))
                    a.keys_out[g + jj] = creg[q][jj];
        }
    }
}

// ---- levels >= 2: tiles inside parent buckets -----------------------------------------------------------------
__global__ void tiles_from_offsets_kernel(const uint64_t *__restrict__ poff, uint64_t n_parents, uint32_t tile,
                                          uint32_t *__restrict__ ntiles)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_parents)
        return;
    const uint64_t n = poff[p + 1] - poff[p];
    ntiles[p] = (uint32_t)((n + tile - 1) / tile);
}

// One record per work item (tile): where its keys start and how many they are.  A tile used to open with three dependent
// loads (item -> parent -> first item of the parent -> the parent's key range); now it is one load, and the kernels issue it
// a tile ahead.  The row of the item in matrix / pos is the item's own index: items are numbered parent by parent.
struct LnItem {
    uint64_t lo; // first key
    uint32_t n;  // keys of the tile (1 .. tile)
    uint32_t pad;
};

__global__ void fill_items_kernel(const uint64_t *__restrict__ poff, const uint64_t *__restrict__ item_off, uint64_t n_parents,
                                  uint32_t tile, LnItem *__restrict__ items)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_parents)
        return;
    const uint64_t i0 = item_off[p], i1 = item_off[p + 1];
    const uint64_t k1 = poff[p + 1];
    uint64_t k = poff[p];
    for (uint64_t i = i0; i < i1; i++, k += tile) {
        LnItem it;
        it.lo = k;
        it.n = (uint32_t)(k1 - k < tile ? k1 - k : tile);
        it.pad = 0;
        items[i] = it;
    }
}

struct LnArgs {
    const uint32_t *keys_in;
    const LnItem *items;         // per work item
    const unsigned long long *n_items; // device scalar
    uint32_t tile;
    int rem_in, bits;            // digit = key >> (rem_in - bits)
    uint32_t *matrix;            // [item][B] digit counts: tile-major inside a parent, one coalesced row per tile
    const uint64_t *pos;         // where the tile's keys of each digit go (ln_colscan_kernel)
    void *keys_out;
    uint64_t in_cap, out_cap;    // entries of keys_in / keys_out (checked under BRX_DEBUG_BOUNDS)
};

// the item's record: one 16-byte load (ln_item_load only issues it), then into scalar registers -- the same for every
// lane, and the key addresses are then a scalar base + the lane's offset instead of a 64-bit vector address per load
__device__ __forceinline__ uint4 ln_item_load(const LnArgs &a, unsigned long long item)
{
    return *reinterpret_cast<const uint4 *>(a.items + item);
}

__device__ __forceinline__ LnItem ln_item_get(const uint4 &v)
{
    LnItem it;
    it.lo = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)v.y) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)v.x);
    it.n = (uint32_t)__builtin_amdgcn_readfirstlane((int)v.z);
    it.pad = 0;
    return it;
}

// issues the loads of a tile's keys (thread t: keys t, t + 256, ...) and nothing else; how many of them are this thread's
// follows from the record alone (ln_count).  No branch per load: behind the end of a partial tile a lane reads the tile's
// first key again (a tile holds at least one) and nobody looks at it.
template <int KPT>
__device__ __forceinline__ void ln_load(const LnArgs &a, const LnItem &it, uint32_t (&key)[KPT])
{
#pragma unroll
    for (int q = 0; q < KPT; q++) {
        const uint32_t j = (uint32_t)q * 256u + threadIdx.x;
        const uint64_t i = it.lo + (j < it.n ? j : 0u);
        if (store_ok(i, a.in_cap))
            key[q] = a.keys_in[i];
    }
}

__device__ __forceinline__ uint32_t ln_count(const LnItem &it)
{
    return it.n > threadIdx.x ? (it.n - threadIdx.x + 255u) / 256u : 0u;
}

template <int KPT>
#ifndef BRX_LNHIST_WAVES
#define BRX_LNHIST_WAVES 1 // (72 registers, seven waves)
#endif
__global__ __launch_bounds__(256, BRX_LNHIST_WAVES) void ln_hist_kernel(LnArgs a)
{
    extern __shared__ uint32_t lds[]; // hist[B]
    const uint32_t B = 1u << a.bits;
    const int shift = a.rem_in - a.bits;
    const unsigned long long n_items = *a.n_items;
    const ItemRange ir = xcd_items(n_items);
    if (ir.first >= ir.end)
        return;
    uint4 it_raw = ln_item_load(a, ir.first);
    for (unsigned long long item = ir.first; item < ir.end; item += ir.step) {
        const LnItem it = ln_item_get(it_raw);
        uint32_t key[KPT];
        ln_load<KPT>(a, it, key);
        const uint32_t cnt = ln_count(it);
        const unsigned long long next = item + ir.step;
        it_raw = ln_item_load(a, next < ir.end ? next : item); // the record of the next tile, while this one is counted
        for (uint32_t b = threadIdx.x; b < B; b += 256)
            lds[b] = 0;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < KPT; q++)
            if ((uint32_t)q < cnt)
                atomicAdd(&lds[(key[q] >> shift) & (B - 1u)], 1u);
        __syncthreads();
        for (uint32_t b = threadIdx.x; b < B; b += 256)
            a.matrix[B * item + b] = lds[b]; // one coalesced row per tile
        __syncthreads();
    }
}

// positions of a level >= 2 from its tile-major counts: block p scans the columns of parent p's [ntiles][B] rows.
// A parent's keys stay inside the parent's range, so pos = poff[p] + (keys of the parent's digits < b) + (keys of digit
// b in the parent's tiles before t); coff[p*B + b] = where child (p, b) starts, coff[n_parents*B] = total.
__global__ __launch_bounds__(256) void ln_colscan_kernel(const uint32_t *__restrict__ m, const uint64_t *__restrict__ poff,
                                                         const uint64_t *__restrict__ item_off, uint64_t n_parents, uint32_t B,
                                                         uint64_t *__restrict__ pos, uint64_t *__restrict__ coff)
{
    __shared__ uint64_t wsum[4];
    for (uint64_t p = blockIdx.x; p < n_parents; p += gridDim.x) {
        const uint64_t io = item_off[p], nt = item_off[p + 1] - io;
        const uint32_t BPT = (B + 255u) / 256u; // digits per thread (1 or 2)
        uint64_t tot[2] = {0, 0};
        for (uint64_t t = 0; t < nt; t++)
            for (uint32_t q = 0; q < BPT; q++) {
                const uint32_t b = threadIdx.x * BPT + q;
                if (b < B)
                    tot[q] += m[B * (io + t) + b];
            }
        const uint64_t mine = tot[0] + tot[1];
        uint64_t incl = mine;
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t u = __shfl_up(incl, d);
            if ((threadIdx.x & 63) >= (unsigned)d)
                incl += u;
        }
        __syncthreads(); // (wsum of the previous parent has been read)
        if ((threadIdx.x & 63) == 63)
            wsum[threadIdx.x >> 6] = incl;
        __syncthreads();
        uint64_t base = poff[p];
        for (uint32_t w = 0; w < (threadIdx.x >> 6); w++)
            base += wsum[w];
        uint64_t run[2];
        run[0] = base + incl - mine;
        run[1] = run[0] + tot[0];
        for (uint32_t q = 0; q < BPT; q++) {
            const uint32_t b = threadIdx.x * BPT + q;
            if (b < B)
                coff[p * B + b] = run[q];
        }
        for (uint64_t t = 0; t < nt; t++)
            for (uint32_t q = 0; q < BPT; q++) {
                const uint32_t b = threadIdx.x * BPT + q;
                if (b < B) {
                    pos[B * (io + t) + b] = run[q];
                    run[q] += m[B * (io + t) + b];
                }
            }
        if (p == n_parents - 1 && threadIdx.x == 0)
            coff[n_parents * B] = poff[n_parents];
    }
}

// The loads of a tile -- its record, then its count row, its position row and its keys -- are issued at the end of the
// tile before, behind that tile's stores.  Loading keys and rows a whole tile ahead into a second set of registers, with
// the wait for them in front of the write-out, was measured slower (profiles/r7_partition_waits.txt).
template <int KPT, typename OUT>
__global__ __launch_bounds__(256) void ln_scatter_kernel(LnArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    __shared__ uint32_t sh_wsum[4];
    const uint32_t T = a.tile;
    const uint32_t B = 1u << a.bits;
    uint32_t *stage_key = (uint32_t *)lds_raw;
    uint16_t *stage_dig = (uint16_t *)(lds_raw + (size_t)T * 4);
    unsigned long long *gbase = (unsigned long long *)(lds_raw + (size_t)T * 6);
    uint32_t *cntv = (uint32_t *)(lds_raw + (size_t)T * 6 + (size_t)B * 8);
    uint32_t *lofs = cntv + B;
    uint32_t *lcur = lofs + B;
    const int shift = a.rem_in - a.bits;
    const uint32_t child_mask = (1u << shift) - 1u;
    OUT *out = (OUT *)a.keys_out;
    const unsigned long long n_items = *a.n_items;
    const ItemRange ir = xcd_items(n_items);
    if (ir.first >= ir.end)
        return;
    constexpr uint32_t OWN = ((1u << MAX_DIGIT_BITS) + 255u) / 256u; // digits per lane: t, t + 256
    auto load_rows = [&](unsigned long long item, uint32_t(&rc)[OWN], uint64_t(&rp)[OWN]) {
#pragma unroll
        for (uint32_t q = 0; q < OWN; q++) {
            const uint32_t b = threadIdx.x + 256u * q;
            const uint64_t mi = B * item + (b < B ? b : 0u); // (no branch: digits past B read digit 0 and drop it)
            rc[q] = a.matrix[mi];
            rp[q] = a.pos[mi];
        }
    };
    LnItem it = ln_item_get(ln_item_load(a, ir.first));
    uint32_t key[KPT], rc[OWN];
    uint64_t rp[OWN];
    load_rows(ir.first, rc, rp);
    ln_load<KPT>(a, it, key);
    for (unsigned long long item = ir.first; item < ir.end; item += ir.step) {
#pragma unroll
        for (uint32_t q = 0; q < OWN; q++) {
            const uint32_t b = threadIdx.x + 256u * q;
            if (b < B) {
                cntv[b] = rc[q];
                gbase[b] = rp[q];
            }
        }
        const uint32_t cnt = ln_count(it);
        __syncthreads();
        block_scan_bins(B, cntv, lofs, lcur, sh_wsum);
        __syncthreads();
#pragma unroll
        for (int q = 0; q < KPT; q++)
            if ((uint32_t)q < cnt) {
                const uint32_t d = (key[q] >> shift) & (B - 1u);
                const uint32_t slot = atomicAdd(&lcur[d], 1u);
                stage_key[slot] = key[q] & child_mask;
                stage_dig[slot] = (uint16_t)d;
            }
        __syncthreads();
        const uint32_t n_tile = lofs[B - 1] + cntv[B - 1];
        for (uint32_t idx = threadIdx.x; idx < n_tile; idx += 256) {
            const uint32_t d = stage_dig[idx];
            const uint64_t at = gbase[d] + (idx - lofs[d]);
            if (store_ok(at, a.out_cap))
                out[at] = (OUT)stage_key[idx];
        }
        const unsigned long long next = item + ir.step;
        if (next < ir.end) {
            it = ln_item_get(ln_item_load(a, next));
            load_rows(next, rc, rp);
            ln_load<KPT>(a, it, key);
        }
        __syncthreads();
    }
}

// ---- final stage: one wavefront per fine bucket (4096 hashes) -----------------------------------------
constexpr int P3_WAVES = 4;
constexpr uint32_t F_SIZE = 1u << F_BITS;   // 4096 hashes
constexpr uint32_t CNT_WORDS = F_SIZE / 2;  // u16 counters, 2 per word: hash h -> half (h>>11) of word (h & 2047)
constexpr uint32_t BIT_WORDS = F_SIZE / 32; // 128
constexpr uint32_t CHUNK_MAX = 65000;       // keys counted between two clamps (the u16 halves must not carry)

constexpr uint32_t STAGE_KEYS = 704;        // keys of a group of buckets staged in LDS per wave (4 blocks per CU)

constexpr uint32_t EMIT_CAP = 256;          // solid hashes collected per wave between two appends to the key list

// EMIT: also append every solid hash to a list (emit_keys, capacity emit_cap, counter emit_n keeps counting
// past the capacity so the host can tell a truncated list).  The list feeds the probe index
// (brx_index.hpp) without a second pass over the 2^(2k-1)-bit vector.
// BITS: write the bucket's 512-byte slice of the bit vector (not for sparse sets: 2^(2k-1) bits do not fit at k = 21).
template <bool EMIT, bool BITS>
__global__ __launch_bounds__(64 * P3_WAVES) void final_count_kernel(const uint16_t *__restrict__ keys,
                                                                     const uint64_t *__restrict__ off, uint64_t n_buckets,
                                                                     uint32_t abundance, uint32_t *__restrict__ bits,
                                                                     uint64_t *__restrict__ emit_keys, uint64_t emit_cap,
                                                                     unsigned long long *__restrict__ emit_n)
{
    __shared__ uint32_t cnt_all[P3_WAVES][CNT_WORDS];
    __shared__ uint32_t bit_all[P3_WAVES][BIT_WORDS];
    __shared__ __attribute__((aligned(8))) uint16_t stage_all[P3_WAVES][STAGE_KEYS + 8];
    __shared__ uint64_t emit_all[EMIT ? P3_WAVES : 1][EMIT ? EMIT_CAP : 1];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t *cnt = cnt_all[wave];
    uint32_t *bmp = bit_all[wave];
    uint16_t *stage = stage_all[wave];
    uint64_t *ebuf = emit_all[EMIT ? wave : 0];
    uint32_t ecount = 0; // wave-uniform
    auto emit_flush = [&]() {
        if (ecount) {
            unsigned long long base = 0;
            if (lane == 0)
                base = atomicAdd(emit_n, (unsigned long long)ecount);
            base = __shfl(base, 0);
            asm volatile("" ::: "memory");
            for (uint32_t q = lane; q < ecount; q += 64)
                if (base + q < emit_cap)
                    emit_keys[base + q] = ebuf[q];
            asm volatile("" ::: "memory");
            ecount = 0;
        }
    };
    for (uint32_t w = lane; w < CNT_WORDS; w += 64)
        cnt[w] = 0;
    for (uint32_t w = lane; w < BIT_WORDS; w += 64)
        bmp[w] = 0;
    // appends `hkey` of every lane whose flag is set (called by the whole wave)
    auto emit_if = [&](bool flag, uint64_t hkey) {
        const uint64_t bal = __ballot(flag);
        if (bal) {
            if (ecount + 64u > EMIT_CAP)
                emit_flush();
            if (flag)
                ebuf[ecount + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u))] = hkey;
            ecount += (uint32_t)__builtin_popcountll(bal);
        }
    };
    asm volatile("" ::: "memory");

    // consecutive buckets go to one wave, so its key stream is contiguous
    const uint64_t n_waves = (uint64_t)gridDim.x * P3_WAVES;
    const uint64_t wid = (uint64_t)blockIdx.x * P3_WAVES + wave;
    const uint64_t per = (n_buckets + n_waves - 1) / n_waves;
    const uint64_t b_lo = wid * per;
    const uint64_t b_hi = (b_lo + per < n_buckets) ? b_lo + per : n_buckets;

    // groups of up to 63 buckets: one coalesced load brings the 64 offsets that delimit them, one
    // batch of coalesced loads stages all their keys in LDS; the per-bucket loop then runs on LDS only
    uint64_t g0 = b_lo;
    while (g0 < b_hi) {
        int gmax = (int)((b_hi - g0 < 63) ? b_hi - g0 : 63);
        const uint64_t oi = g0 + (uint64_t)lane;
        const uint64_t offv = off[oi <= n_buckets ? oi : n_buckets];
        const uint64_t gs = __shfl(offv, 0);
        // largest prefix of buckets whose keys fit the staging buffer (lane l: does bucket l-1 end inside?)
        const bool fits = lane >= 1 && lane <= gmax && (offv - gs) <= (uint64_t)STAGE_KEYS;
        const uint64_t fm = __ballot(fits) >> 1; // bit j: buckets 0..j fit
        int gcount = (fm == ~0ull >> 1) ? 63 : __builtin_ctzll(~fm);
        if (gcount > gmax)
            gcount = gmax;
        const bool staged = gcount > 0;
        if (!staged)
            gcount = 1; // a single bucket larger than the staging buffer: streamed from global memory
        const uint64_t ge = __shfl(offv, gcount);
        const uint64_t base4 = gs & ~3ull; // 8-byte aligned start of the staged window
        if (staged) {
            const uint32_t nquads = (uint32_t)((ge - base4 + 3) / 4);
            const uint2 *src = reinterpret_cast<const uint2 *>(keys + base4);
            uint2 *dstq = reinterpret_cast<uint2 *>(stage);
            for (uint32_t q = lane; q < nquads; q += 64)
                dstq[q] = src[q];
            asm volatile("" ::: "memory");
        }
        const uint32_t off_lo = (uint32_t)offv, off_hi = (uint32_t)(offv >> 32);
        for (int j = 0; j < gcount; j++) {
            // j is wave-uniform: v_readlane instead of a bpermute through the LDS pipe
            // (the builtin returns a signed int: without the casts an offset with bit 31 set sign-extends over the
            // high word -- every job beyond 2^31 keys)
            const uint64_t s = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(off_hi, j) << 32) |
                               (uint64_t)(uint32_t)__builtin_amdgcn_readlane(off_lo, j);
            const uint64_t e = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(off_hi, j + 1) << 32) |
                               (uint64_t)(uint32_t)__builtin_amdgcn_readlane(off_lo, j + 1);
            const uint64_t n = e - s;
            bool any_bit = false;
            if (n == 0) {
                // empty bucket: a slice of zeros
            } else if (staged && n <= 64) {
                const bool act = (uint64_t)lane < n;
                const uint32_t key = act ? stage[(uint32_t)(s - base4) + lane] : 0u;
                const uint32_t word = key & (CNT_WORDS - 1u), half = key >> (F_BITS - 1);
                bool hot = false, cross = false;
                if (act) {
                    // the lane that increments a counter last sees its final value minus one, so
                    // "old + 1 > abundance" on every lane sets exactly the bits of the final counts
                    const uint32_t old = (atomicAdd(&cnt[word], 1u << (16u * half)) >> (16u * half)) & 0xffffu;
                    const uint32_t c = old + 1u;
                    hot = (c > 255u ? 255u : c) > abundance; // pcon's u8 counters saturate at 255
                    cross = old == abundance && abundance < 255u; // exactly one lane per solid hash sees the crossing
                    if (BITS && hot)
                        atomicOr(&bmp[key >> 5], 1u << (key & 31u));
                }
                if (BITS)
                    any_bit = __ballot(hot) != 0ull;
                else if (EMIT)
                    emit_if(cross, (g0 + (uint64_t)j) * F_SIZE + (uint64_t)key); // no slice: list the hash right away
                asm volatile("" ::: "memory");
                if (act)
                    cnt[word] = 0;
            } else {
                any_bit = true;
                // large bucket: stream it, clamping between chunks so that the packed halves never carry
                uint64_t done = 0;
                while (done < n) {
                    const uint64_t m = (n - done < CHUNK_MAX) ? n - done : CHUNK_MAX;
                    for (uint64_t i = lane; i < m; i += 64) {
                        const uint32_t kk = staged ? (uint32_t)stage[(uint32_t)(s - base4 + done + i)] : (uint32_t)keys[s + done + i];
                        atomicAdd(&cnt[kk & (CNT_WORDS - 1u)], 1u << (16u * (kk >> (F_BITS - 1))));
                    }
                    asm volatile("" ::: "memory");
                    done += m;
                    if (done < n) {
                        for (uint32_t w = lane; w < CNT_WORDS; w += 64) {
                            const uint32_t v = cnt[w];
                            const uint32_t a0 = v & 0xffffu, a1 = v >> 16;
                            cnt[w] = (a0 > 255u ? 255u : a0) | ((a1 > 255u ? 255u : a1) << 16);
                        }
                        asm volatile("" ::: "memory");
                    }
                }
                for (uint32_t w = lane; w < CNT_WORDS; w += 64) { // (wave-uniform trip count)
                    const uint32_t v = cnt[w];
                    // word w holds hashes w (low half) and w + 2048 (high half)
                    const uint32_t c0 = v & 0xffffu, c1 = v >> 16;
                    const bool s0 = (c0 > 255u ? 255u : c0) > abundance, s1 = (c1 > 255u ? 255u : c1) > abundance;
                    if (BITS) {
                        if (s0)
                            atomicOr(&bmp[w >> 5], 1u << (w & 31u));
                        if (s1)
                            atomicOr(&bmp[(w + CNT_WORDS) >> 5], 1u << (w & 31u));
                    } else if (EMIT) {
                        emit_if(s0, (g0 + (uint64_t)j) * F_SIZE + (uint64_t)w);
                        emit_if(s1, (g0 + (uint64_t)j) * F_SIZE + (uint64_t)(w + CNT_WORDS));
                    }
                    if (v)
                        cnt[w] = 0;
                }
            }
            asm volatile("" ::: "memory");
            if (!BITS)
                continue; // hashes were listed above, there is no slice to write
            // flush the slice: 128 words = 2 per lane (LDS is only touched when a bit was set)
            uint32_t *dst = bits + (g0 + (uint64_t)j) * BIT_WORDS;
            uint32_t w0 = 0, w1 = 0;
            if (any_bit) {
                w0 = bmp[2 * lane];
                w1 = bmp[2 * lane + 1];
                bmp[2 * lane] = 0;
                bmp[2 * lane + 1] = 0;
            }
            *reinterpret_cast<uint2 *>(dst + 2 * lane) = make_uint2(w0, w1);
            asm volatile("" ::: "memory");
            if (EMIT && any_bit) {
                // one hash per lane and turn (slices hold a handful of bits: usually a single turn)
                uint64_t rem = (uint64_t)w0 | ((uint64_t)w1 << 32);
                const uint64_t hbase = (g0 + (uint64_t)j) * F_SIZE + 64ull * (uint64_t)lane;
                for (;;) {
                    const uint64_t bal = __ballot(rem != 0ull);
                    if (!bal)
                        break;
                    if (ecount + 64u > EMIT_CAP)
                        emit_flush();
                    if (rem) {
                        const uint32_t pos = ecount + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32),
                                                                                __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
                        ebuf[pos] = hbase + (uint64_t)__builtin_ctzll(rem);
                        rem &= rem - 1ull;
                    }
                    ecount += (uint32_t)__builtin_popcountll(bal);
                }
            }
        }
        g0 += (uint64_t)gcount;
    }
    if (EMIT)
        emit_flush();
}

// ---- final stage without a bit vector: hash-count the buckets one level earlier -------------------------------
// When the set is only listed (lazy bit vector / sparse set) nothing forces the last radix level: a bucket of
// 2^R hashes (R <= 20 bits left in the keys) with a few thousand keys is counted directly in an LDS hash table
// (open addressing, entry = valid | key << 11 | count), and the entries with count > abundance are listed.  That
// replaces the last level's histogram + scatter and the per-4096-hash counting pass.  A TEAM of 1024 lanes (one
// workgroup; buckets of 640 keys and more on average) or 64 lanes (one wave) takes a bucket; a bucket with more keys than the table can take is done in
// 2^lp passes over disjoint key ranges.  lp is chosen for the DISTINCT keys expected -- n x the ratio hf_sample_kernel
// measured on a few buckets: at 20x coverage a bucket of 48 000 keys has ~10 000 different ones -- and a pass whose
// keys still do not fit is repeated with the whole table, then 4x finer.  Each bucket's table has 2.5 slots per distinct key
// expected, not the launch's maximum.  What binds the kernel and what was tried: DESIGN.md section 4,
// profiles/r2_one_kernel_ab.txt.
#ifndef BRX_HF_FLAT
#define BRX_HF_FLAT 1
#endif
constexpr bool HF_FLAT = BRX_HF_FLAT != 0;
constexpr uint32_t HF_VALID = 0x80000000u;
constexpr int HF_CHUNK = 8;
constexpr uint32_t HF_MAX_TRIES = 192; // probes before a key calls the table full (a cluster that long means it nearly is)
__host__ __device__ constexpr uint32_t hf_ebuf(int team) { return team > 64 ? 1024u : 512u; }

template <int TEAM, int BLOCK>
__global__ __launch_bounds__(BLOCK) void hash_final_kernel(const uint32_t *__restrict__ keys, const uint64_t *__restrict__ off,
                                                         uint64_t n_buckets, int R, uint32_t abundance, uint32_t log_t,
                                                         uint64_t *__restrict__ emit_keys, uint64_t emit_cap,
                                                         unsigned long long *__restrict__ emit_n,
                                                         const unsigned long long *__restrict__ dup, uint32_t min_lt, float ratio_forced)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t hf_lds[];
    constexpr int TEAMS = BLOCK / TEAM;
    constexpr uint32_t EB = hf_ebuf(TEAM);
    const uint32_t MIN_LT = min_lt; // smallest table a bucket gets (hf_min_lt: 4 slots per lane and clearing step)
    const uint32_t Tmax = 1u << log_t;
    const int team = threadIdx.x / TEAM, tl = threadIdx.x % TEAM;
    uint32_t *tab = (uint32_t *)hf_lds + (size_t)team * Tmax;
    unsigned long long *ebuf = (unsigned long long *)(hf_lds + (size_t)TEAMS * Tmax * 4) + (size_t)team * EB;
    uint32_t *ctl = (uint32_t *)(hf_lds + (size_t)TEAMS * Tmax * 4 + (size_t)TEAMS * EB * 8) + team * 4; // [0] ecount, [1] overflow
    auto team_sync = [&]() {
        if (TEAM > 64)
            __syncthreads();
        else
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    };
    auto flush = [&]() { // whole team
        team_sync();
        const uint32_t ne = ctl[0] < EB ? ctl[0] : EB;
        __shared__ unsigned long long sh_base[TEAMS];
        if (tl == 0)
            sh_base[team] = ne ? atomicAdd(emit_n, (unsigned long long)ne) : 0ull;
        team_sync();
        const unsigned long long base = sh_base[team];
        for (uint32_t q = tl; q < ne; q += TEAM)
            if (base + q < emit_cap)
                emit_keys[base + q] = ebuf[q];
        team_sync();
        if (tl == 0)
            ctl[0] = 0;
        team_sync();
    };
    if (tl == 0) {
        ctl[0] = 0;
        ctl[1] = 0;
    }
    team_sync();
    // distinct keys expected per key of a bucket (1 when nothing was sampled), with a quarter of room on top
    float ratio = 1.0f;
    if (dup) {
        const float d = (float)dup[0], t = (float)dup[1];
        if (t > 0.0f)
            ratio = fminf(1.0f, 1.25f * d / t + 0.01f);
    }
    if (ratio_forced > 0.0f) // test hook (BRX_HF_RATIO): a wrong guess must only cost time
        ratio = ratio_forced;
    const uint64_t n_teams = (uint64_t)gridDim.x * TEAMS;
    for (uint64_t b = (uint64_t)blockIdx.x * TEAMS + team; b < n_buckets; b += n_teams) { // (team-uniform trip count)
        const uint64_t s0 = off[b], n = off[b + 1] - s0;
        if (n == 0)
            continue;
        // passes: 2^lp disjoint ranges of the R-bit key, each expected to bring <= 5/8 T DISTINCT keys (measured: 3/8 costs
        // configs[3]'s share 39.9 -> 45.7 ms in extra passes, 7/8 costs configs[2] 83 -> 117 ms in overflowing tables; 4
        // slots per key instead of 2.5 below: no difference, 1.5: +23 % -- profiles/r2_one_kernel_ab.txt)
        const uint64_t n_eff = (uint64_t)((float)n * ratio) + 1ull;
        uint32_t lp = 0;
        while (lp < (uint32_t)R && (n_eff >> lp) > (uint64_t)(Tmax / 8u * 5u))
            lp++;
        // the table of THIS bucket: 2.5 slots per distinct key expected, not the launch's maximum -- clearing and scanning
        // cost T / TEAM LDS accesses per lane whatever the bucket holds (k = 21: 745 keys, ~200 distinct, in 2048 slots)
        uint32_t lt = log_t;
        if (lp == 0) {
            const uint32_t want = (uint32_t)n_eff * 5u / 2u;
            lt = MIN_LT < log_t ? MIN_LT : log_t;
            while (lt < log_t && (1u << lt) < want)
                lt++;
        }
        uint32_t T = 1u << lt;
        for (uint32_t pass = 0; pass < (1u << lp);) {
            for (uint32_t q = tl * 4u; q < T; q += TEAM * 4u) // 16 bytes per lane and store (T >= 4 * TEAM)
                *(uint4 *)(tab + q) = make_uint4(0u, 0u, 0u, 0u);
            team_sync();
            for (uint64_t i0 = 0; i0 < n; i0 += (uint64_t)TEAM * HF_CHUNK) {
              // HF_CHUNK independent loads in flight per thread, then the inserts
              uint32_t kbuf[HF_CHUNK];
#pragma unroll
              for (int c = 0; c < HF_CHUNK; c++) {
                  const uint64_t i = i0 + (uint64_t)c * TEAM + tl;
                  kbuf[c] = i < n ? keys[s0 + i] : 0xffffffffu; // (a clamped index instead of the branch: 3.39 -> 5.24 ms)
              }
              if constexpr (HF_FLAT && TEAM > 64) {
#pragma unroll
              for (int c = 0; c < HF_CHUNK; c++) {
                // One key per lane, flat: the loop runs while any lane of the wave is still probing, every turn is the same
                // straight code -- read the slot, claim it if empty, count if it holds the key -- with the two atomics as its
                // only predicated regions (the nested ifs and breaks of the obvious form cost ~30 scalar instructions per
                // turn in exec-mask bookkeeping: the scalar unit, 68 % busy, was the kernel's busiest; profiles/r2j_sq_summary.json)
                const uint32_t key = kbuf[c];
                uint32_t pend = (key != 0xffffffffu && !(lp && (key >> ((uint32_t)R - lp)) != pass)) ? 1u : 0u;
                uint32_t h = (key * 0x9E3779B1u) >> (32u - lt);
                const uint32_t mine = HF_VALID | (key << 11);
                for (uint32_t tries = 0; __any(pend); tries++) {
                    const uint32_t e = tab[h]; // (lanes that are done read a slot they do not use)
                    uint32_t r = e;
                    if (pend & (uint32_t)(e == 0u))
                        r = atomicCAS(&tab[h], 0u, mine | 1u);
                    const uint32_t won = (uint32_t)(e == 0u) & (uint32_t)(r == 0u);
                    const uint32_t same = (uint32_t)((r & 0xfffff800u) == mine);
                    if (pend & same & (uint32_t)((r & 0x400u) == 0u)) // saturates far above 255 and far below the key bits
                        atomicAdd(&tab[h], 1u);
                    pend &= ~(won | same) & 1u;
                    if (tries >= HF_MAX_TRIES) { // (uniform) the table is as good as full: this pass needs a finer split
                        if (pend)
                            ctl[1] = 1;
                        pend = 0;
                    }
                    h = (h + 1u) & (T - 1u);
                }
              }
              } else {
              // (one wave per bucket: the form with breaks measured 7 % faster there -- 66.7 against 71.8 ms at configs[4]'s share)
#pragma unroll
              for (int c = 0; c < HF_CHUNK; c++) {
                const uint32_t key = kbuf[c];
                if (key == 0xffffffffu || (lp && (key >> ((uint32_t)R - lp)) != pass))
                    continue;
                uint32_t h = (key * 0x9E3779B1u) >> (32u - lt);
                const uint32_t mine = HF_VALID | (key << 11);
                for (uint32_t tries = 0;; tries++) {
                    uint32_t e = tab[h];
                    if (e == 0u) {
                        e = atomicCAS(&tab[h], 0u, mine | 1u);
                        if (e == 0u)
                            break;
                    }
                    if ((e & 0xfffff800u) == mine) {
                        if ((e & 0x7ffu) < 1024u) // saturates far above 255 and far below the key bits
                            atomicAdd(&tab[h], 1u);
                        break;
                    }
                    if (tries >= HF_MAX_TRIES) { // the table is (as good as) full of other keys: this pass needs a finer split
                        ctl[1] = 1;
                        break;
                    }
                    h = (h + 1u) & (T - 1u);
                }
              }
              }
            }
            team_sync();
            const uint32_t ovf = ctl[1];
            team_sync();
            if (ovf) { // redo this key range: with the whole table if it had less, else in 4 finer passes
                if (tl == 0)
                    ctl[1] = 0;
                team_sync();
                if (lt < log_t) {
                    lt = log_t;
                    T = Tmax;
                    continue;
                }
                if (lp + 2u <= (uint32_t)R) {
                    lp += 2u;
                    pass <<= 2;
                    continue;
                }
                // cannot split further: cannot happen (2^R <= T * 2^lp by then)
            }
            // list the solid entries: into the team's buffer (a pass holds at most 5/8 T / (abundance + 1) of them; what
            // does not fit goes straight to the global list), one flush per pass
            for (uint32_t q0 = tl * 4u; q0 < T; q0 += TEAM * 4u) { // four entries per lane and LDS read
                const uint4 e4 = *(const uint4 *)(tab + q0);
                const uint32_t ev[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const uint32_t e = ev[j];
                    const uint32_t cnt = e & 0x7ffu;
                    if ((e & HF_VALID) && (cnt > 255u ? 255u : cnt) > abundance) {
                        const unsigned long long hk = (b << R) | (uint64_t)((e >> 11) & 0xfffffu);
                        const uint32_t pos = atomicAdd(&ctl[0], 1u);
                        if (pos < EB) {
                            ebuf[pos] = hk;
                        } else {
                            const unsigned long long gp = atomicAdd(emit_n, 1ull);
                            if (gp < emit_cap)
                                emit_keys[gp] = hk;
                        }
                    }
                }
            }
            team_sync();
            const uint32_t ec = ctl[0]; // read between two barriers: the same value in every thread
            team_sync();
            if (ec > EB / 2u) // one append to the global list per ~EB/2 hashes, not per bucket
                flush();
            pass++;
        }
    }
    flush();
}

// distinct keys per key on a sample of the buckets hash_final_kernel is about to count: block i counts bucket
// i * n_buckets / gridDim.x exactly (as many passes as its n asks for) -> dup[0] += distinct, dup[1] += n
__global__ __launch_bounds__(1024) void hf_sample_kernel(const uint32_t *__restrict__ keys, const uint64_t *__restrict__ off,
                                                         uint64_t n_buckets, int R, uint32_t log_t, unsigned long long *__restrict__ dup)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t hf_lds[];
    __shared__ uint32_t sh_new;
    uint32_t *tab = (uint32_t *)hf_lds;
    const uint32_t T = 1u << log_t;
    const uint64_t b = (uint64_t)blockIdx.x * n_buckets / gridDim.x;
    const uint64_t s0 = off[b], n = off[b + 1] - s0;
    if (threadIdx.x == 0)
        sh_new = 0;
    uint32_t lp = 0;
    while (lp < (uint32_t)R && (n >> lp) > (uint64_t)(T / 8u * 5u))
        lp++;
    uint32_t fresh = 0;
    for (uint32_t pass = 0; pass < (1u << lp); pass++) {
        __syncthreads();
        for (uint32_t q = threadIdx.x; q < T; q += 1024u)
            tab[q] = 0;
        __syncthreads();
        for (uint64_t i = threadIdx.x; i < n; i += 1024u) {
            const uint32_t key = keys[s0 + i];
            if (lp && (key >> ((uint32_t)R - lp)) != pass)
                continue;
            uint32_t h = (key * 0x9E3779B1u) >> (32u - log_t);
            const uint32_t mine = HF_VALID | (key << 11);
            for (uint32_t tries = 0; tries < T; tries++) {
                uint32_t e = tab[h];
                if (e == 0u) {
                    e = atomicCAS(&tab[h], 0u, mine);
                    if (e == 0u) {
                        fresh++;
                        break;
                    }
                }
                if (e == mine)
                    break;
                h = (h + 1u) & (T - 1u);
            }
        }
    }
    atomicAdd(&sh_new, fresh);
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(dup, (unsigned long long)sh_new);
        atomicAdd(dup + 1, (unsigned long long)n);
    }
}

// ---- count spectrum without the u8 table (pcon::spectrum::Spectrum::from_count, src/main.rs:93) ----------------
// One wave per last-level bucket (2^F_BITS hashes, u16 keys): count the keys in LDS, then every key swaps its
// counter for 0 -- exactly one lane per distinct hash gets the count and bins min(count, 255), pcon's saturated
// u8.  Bin 0 (hashes never seen) is 2^(2k-1) minus the rest; the host fills it in.
constexpr int SP_WAVES = 4;
__global__ __launch_bounds__(64 * SP_WAVES) void final_spectrum_kernel(const uint16_t *__restrict__ keys, const uint64_t *__restrict__ off,
                                                                       uint64_t n_buckets, unsigned long long *__restrict__ hist)
{
    __shared__ uint32_t sp_cnt[SP_WAVES][F_SIZE];
    __shared__ unsigned long long sp_hist[256];
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    uint32_t *cnt = sp_cnt[wave];
    for (uint32_t q = lane; q < F_SIZE; q += 64)
        cnt[q] = 0;
    for (uint32_t q = threadIdx.x; q < 256; q += 64 * SP_WAVES)
        sp_hist[q] = 0;
    __syncthreads();
    const uint64_t n_waves = (uint64_t)gridDim.x * SP_WAVES;
    for (uint64_t g = (uint64_t)blockIdx.x * SP_WAVES + wave; g < n_buckets; g += n_waves) {
        const uint64_t s0 = off[g], n = off[g + 1] - s0;
        for (uint64_t i = lane; i < n; i += 64)
            atomicAdd(&cnt[keys[s0 + i]], 1u);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // LDS operations of one wave complete in order
        for (uint64_t i = lane; i < n; i += 64) {
            const uint32_t c = atomicExch(&cnt[keys[s0 + i]], 0u);
            if (c)
                atomicAdd(&sp_hist[c > 255u ? 255u : c], 1ull);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    __syncthreads();
    for (uint32_t q = threadIdx.x; q < 256; q += 64 * SP_WAVES)
        if (sp_hist[q])
            atomicAdd(&hist[q], sp_hist[q]);
}

// ---- count view of the last-level buckets: what an abundance lookup reads (brx_abundance.hip, SRC_PART) -----------------
// Turns every last-level bucket IN PLACE into a lookup structure: the bucket's distinct keys (the low F_BITS bits of the
// hashes counted) in rising order at the front of its own range of `keys`, the rest of the range filled with VIEW_PAD (a
// real key never exceeds F_SIZE - 1), and min(255, count) in `cnt` at the same index (0 beside the padding).  A bucket
// then holds at most F_SIZE sorted entries whatever the coverage, and the count of hash h is found by a binary search
// for h & (F_SIZE - 1) between off[h >> F_BITS] and off[(h >> F_BITS) + 1].
// A wave takes a contiguous run of buckets the way final_count_kernel does -- 64 offsets in one load, the keys of as many
// buckets as fit STAGE_KEYS staged in LDS with coalesced loads, rewritten there and written back whole -- because at
// k = 21 there are 2^29 buckets of a few keys each and a memory round trip per bucket would be all the kernel does.
//   up to 64 keys   a key per lane: rank among the distinct keys and multiplicity from one readlane + ballot per
//                   distinct key
//   more            counted in the wave's F_SIZE u32 bins (no 16-bit halves that could carry) with a bit per bin that is
//                   not zero; a lane owns 64 neighbouring bins, a prefix sum of its bits gives their place in hash order
// Either way the wave has read ALL of a bucket's keys before it writes any, and buckets are disjoint: in place is safe.
constexpr int VW_WAVES = 4;
constexpr uint32_t VIEW_PAD = 0xFFFFu;
constexpr uint64_t VW_PER_WAVE = 63ull * 16ull; // consecutive buckets a wave takes per trip of its block: 16 offset loads
__global__ __launch_bounds__(64 * VW_WAVES) void final_view_kernel(uint16_t *keys, const uint64_t *__restrict__ off, uint64_t n_buckets,
                                                                   uint8_t *__restrict__ cnt_out)
{
    __shared__ uint32_t bins_all[VW_WAVES][F_SIZE];
    __shared__ __attribute__((aligned(8))) uint16_t stage_all[VW_WAVES][STAGE_KEYS + 8];
    __shared__ __attribute__((aligned(4))) uint8_t scnt_all[VW_WAVES][STAGE_KEYS + 8];
    __shared__ uint32_t bmp_all[VW_WAVES][BIT_WORDS]; // which bins of the wave are not zero
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t *bins = bins_all[wave];
    uint16_t *stage = stage_all[wave];
    uint8_t *scnt = scnt_all[wave];
    uint32_t *bmp = bmp_all[wave];
    for (uint32_t q = lane; q < F_SIZE; q += 64)
        bins[q] = 0;
    bmp[2 * lane] = 0;
    bmp[2 * lane + 1] = 0;
    asm volatile("" ::: "memory");

    // blocks loop over chunks of buckets; inside a chunk consecutive buckets go to one wave, so its key stream is contiguous
    const uint64_t n_chunks = (n_buckets + VW_PER_WAVE * VW_WAVES - 1) / (VW_PER_WAVE * VW_WAVES);
    for (uint64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const uint64_t b_lo = (chunk * VW_WAVES + (uint64_t)wave) * VW_PER_WAVE;
        const uint64_t b_hi = b_lo + VW_PER_WAVE < n_buckets ? b_lo + VW_PER_WAVE : n_buckets;
        uint64_t g0 = b_lo;
        while (g0 < b_hi) {
            const int gmax = (int)((b_hi - g0 < 63) ? b_hi - g0 : 63);
            const uint64_t oi = g0 + (uint64_t)lane;
            const uint64_t offv = off[oi <= n_buckets ? oi : n_buckets];
            const uint64_t gs = __shfl(offv, 0);
            // largest prefix of buckets whose keys fit the staging buffer (lane l: does bucket l-1 end inside?)
            const bool fits = lane >= 1 && lane <= gmax && (offv - gs) <= (uint64_t)STAGE_KEYS;
            const uint64_t fm = __ballot(fits) >> 1; // bit j: buckets 0..j fit
            int gcount = (fm == ~0ull >> 1) ? 63 : __builtin_ctzll(~fm);
            if (gcount > gmax)
                gcount = gmax;
            const bool staged = gcount > 0;
            if (!staged)
                gcount = 1; // a single bucket larger than the staging buffer: counted from, and written to, global memory
            const uint64_t ge = __shfl(offv, gcount);
            if (ge == gs) { // nothing but empty buckets (most groups of a small input at large k)
                g0 += (uint64_t)gcount;
                continue;
            }
            const uint64_t base4 = gs & ~3ull; // 8-byte aligned start of the staged window
            const uint32_t nquads = (uint32_t)((ge - base4 + 3) / 4);
            if (staged) {
                // (the window may begin with up to 3 keys of the bucket before and end with 3 of the one behind, which
                // another wave may be rewriting: nobody looks at them, and they are not written back)
                const uint2 *src = reinterpret_cast<const uint2 *>(keys + base4);
                uint2 *dstq = reinterpret_cast<uint2 *>(stage);
                for (uint32_t q = lane; q < nquads; q += 64)
                    dstq[q] = src[q];
                asm volatile("" ::: "memory");
            }
            const uint32_t off_lo = (uint32_t)offv, off_hi = (uint32_t)(offv >> 32);
            for (int j = 0; j < gcount; j++) {
                // (readlane returns a signed int: without the casts an offset with bit 31 set sign-extends)
                const uint64_t s = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(off_hi, j) << 32) |
                                   (uint64_t)(uint32_t)__builtin_amdgcn_readlane(off_lo, j);
                const uint64_t e = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(off_hi, j + 1) << 32) |
                                   (uint64_t)(uint32_t)__builtin_amdgcn_readlane(off_lo, j + 1);
                const uint64_t n = e - s;
                if (n == 0)
                    continue;
                const uint32_t sidx = (uint32_t)(s - base4); // of the bucket's first key in the staged window
                if (staged && n <= 64) {
                    const bool act = (uint64_t)lane < n;
                    const uint32_t key = act ? (uint32_t)stage[sidx + lane] : VIEW_PAD;
                    uint32_t less = 0, mult = 0, distinct = 0;
                    bool lead = false;
                    // one trip per DISTINCT key (at 50x a solid k-mer is there ~35 times): the lowest lane not yet
                    // accounted for names the key, a ballot finds its copies and takes them out
                    for (uint64_t rem = __ballot(act); rem; distinct++) {
                        const int i = __builtin_ctzll(rem); // wave-uniform
                        const uint32_t ki = (uint32_t)__builtin_amdgcn_readlane((int)key, i);
                        const uint64_t eq = __ballot(act && key == ki);
                        rem &= ~eq;
                        if (ki < key)
                            less++;
                        if (key == ki) {
                            mult = (uint32_t)__builtin_popcountll(eq);
                            lead = lane == i;
                        }
                    }
                    asm volatile("" ::: "memory");
                    if (act && lead) {
                        stage[sidx + less] = (uint16_t)key;
                        scnt[sidx + less] = (uint8_t)(mult > 255u ? 255u : mult);
                    }
                    if (act && (uint32_t)lane >= distinct) {
                        stage[sidx + lane] = (uint16_t)VIEW_PAD;
                        scnt[sidx + lane] = 0;
                    }
                    asm volatile("" ::: "memory");
                    continue;
                }
                for (uint64_t i = lane; i < n; i += 64) {
                    const uint32_t kk = (staged ? (uint32_t)stage[sidx + (uint32_t)i] : (uint32_t)keys[s + i]) & (F_SIZE - 1u);
                    atomicAdd(&bins[kk], 1u);
                    atomicOr(&bmp[kk >> 5], 1u << (kk & 31u));
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // LDS operations of one wave complete in order
                // lane l owns hashes 64l .. 64l+63: the bits of its two bitmap words are its distinct keys, a prefix sum
                // over the lanes says where they go, and only bins that were counted are visited
                uint64_t mine = ((uint64_t)bmp[2 * lane + 1] << 32) | (uint64_t)bmp[2 * lane];
                bmp[2 * lane] = 0;
                bmp[2 * lane + 1] = 0;
                const uint32_t nmine = (uint32_t)__builtin_popcountll(mine);
                uint32_t incl = nmine;
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
                    if (lane >= d)
                        incl += up;
                }
                const uint32_t pos = (uint32_t)__shfl((int)incl, 63); // distinct keys (<= n)
                for (uint32_t p = incl - nmine; mine; mine &= mine - 1ull, p++) {
                    const uint32_t h = 64u * (uint32_t)lane + (uint32_t)__builtin_ctzll(mine);
                    const uint32_t v = bins[h];
                    bins[h] = 0;
                    const uint8_t c8 = (uint8_t)(v > 255u ? 255u : v);
                    if (staged) {
                        stage[sidx + p] = (uint16_t)h;
                        scnt[sidx + p] = c8;
                    } else {
                        keys[s + p] = (uint16_t)h;
                        cnt_out[s + p] = c8;
                    }
                }
                for (uint64_t i = (uint64_t)pos + lane; i < n; i += 64) {
                    if (staged) {
                        stage[sidx + (uint32_t)i] = (uint16_t)VIEW_PAD;
                        scnt[sidx + (uint32_t)i] = 0;
                    } else {
                        keys[s + i] = (uint16_t)VIEW_PAD;
                        cnt_out[s + i] = 0;
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            }
            if (staged) {
                // the window back to memory: whole quads where all four keys are this group's, key by key at its two ends
                asm volatile("" ::: "memory");
                for (uint32_t q = lane; q < nquads; q += 64) {
                    const uint64_t at = base4 + 4ull * q;
                    if (at >= gs && at + 4 <= ge) {
                        *reinterpret_cast<uint2 *>(keys + at) = *reinterpret_cast<const uint2 *>(stage + 4u * q);
                        *reinterpret_cast<uint32_t *>(cnt_out + at) = *reinterpret_cast<const uint32_t *>(scnt + 4u * q);
                    } else {
                        for (uint32_t t = 0; t < 4; t++)
                            if (at + t >= gs && at + t < ge) {
                                keys[at + t] = stage[4u * q + t];
                                cnt_out[at + t] = scnt[4u * q + t];
                            }
                    }
                }
                asm volatile("" ::: "memory");
            }
            g0 += (uint64_t)gcount;
        }
    }
}

// concatenates, per level-1 bucket, the segments of every batch (only needed for > 1 batch)
__global__ __launch_bounds__(256) void merge_segments_kernel(const uint32_t *__restrict__ src,
                                                             const uint64_t *__restrict__ src_off,
                                                             const uint64_t *__restrict__ dst_off,
                                                             const uint64_t *__restrict__ dst_shift, uint32_t B1,
                                                             uint32_t *__restrict__ dst)
{
    for (uint32_t b = blockIdx.x; b < B1; b += gridDim.x) {
        const uint64_t lo = src_off[b], hi = src_off[b + 1];
        const uint64_t base = dst_off[b] + dst_shift[b];
        for (uint64_t i = lo + threadIdx.x; i < hi; i += blockDim.x)
            dst[base + (i - lo)] = src[i];
    }
}

__global__ void add_counts_kernel(const uint64_t *__restrict__ off, uint32_t B1, uint32_t *__restrict__ counts,
                                  uint64_t *__restrict__ shift_out)
{
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B1) {
        if (shift_out)
            shift_out[b] = counts[b];
        counts[b] += (uint32_t)(off[b + 1] - off[b]);
    }
}

// A batch either owns its two arrays (own_keys / own_l1off hold them, d_keys / d_l1off point into them) or borrows them
// from the caller (segments received from other ranks: the owners stay empty).
struct PartBatch {
    uint32_t *d_keys = nullptr;  // keys after level 1, grouped by digit 1
    uint64_t n = 0;
    uint64_t *d_l1off = nullptr; // B1 + 1
    DevBuf<uint32_t> own_keys;
    DevBuf<uint64_t> own_l1off;
    bool borrowed() const { return !own_keys; }
    uint64_t cap() const { return own_keys.cap(); }
};

} // namespace

namespace brx {

struct PartState {
    Plan pl;
    Plan pl_wide;     // the same first level, then the widest second digit (big inputs that end in hash_final_kernel)
    bool use_wide = false; // which of the two the levels >= 2 of the finish in progress follow
    std::vector<PartBatch> batches, spare;
    // generic workspace
    DevBuf<uint32_t> d_ntiles;    // per parent
    DevBuf<uint64_t> d_item_off;  // per parent + 1
    DevBuf<LnItem> d_items;       // per work item
    DevBuf<uint32_t> d_matrix;    // per-tile digit counts
    DevBuf<uint64_t> d_pos;       // levels >= 2: exclusive scan of the matrix; level 1: [n_ranges + 1][B] range starts
    DevBuf<uint64_t> d_scan_tmp;
    DevBuf<unsigned long long> d_scalars; // [0] n_items, [1] total keys of the last scan, [2..3] hf_sample_kernel
    DevBuf<uint64_t> d_coff[MAX_LEVELS];  // child offsets (nchild + 1)
    DevBuf<uint32_t> d_keys_mid, d_keys_mid2; // outputs of the middle levels (ping-pong when there are 4 levels)
    DevBuf<uint16_t> d_keys_fin;  // last level output
    DevBuf<uint32_t> d_merged;    // all batches merged per level-1 bucket (only when > 1 batch)
    DevBuf<uint64_t> d_l1off_all;
    DevBuf<uint32_t> d_cnts;      // B1 running counts (merge)
    DevBuf<uint64_t> d_shift;     // B1 (merge)
    // count view for lookups (part_lookup_prepare): d_keys_fin rewritten bucket by bucket, d_coff[nlev - 1] delimits them
    std::atomic<bool> view_valid{false}; // (read without the counter's lock by the entries' first check) cleared by everything that touches the batches or the workspace above
    bool view_empty = false;           // ... of a counter without keys: answers 0 everywhere, nothing to read
    DevBuf<uint8_t> d_view_cnt;        // min(255, count) beside every key of d_keys_fin
};

// the partition workspace is sized in bytes, with a sixteenth and 256 B to spare
template <typename T> static int ws_reserve(DevBuf<T> &b, uint64_t need_bytes)
{
    return b.reserve_bytes(need_bytes, need_bytes / 16 + 256, "partition workspace");
}

// presence-only insertion of a batch (see flat_insert_kernel); table == nullptr: into `bits`
int flat_presence_insert(const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads, uint64_t total_bases, int k,
                         uint32_t *bits, uint64_t *table, uint32_t line_shift, uint32_t m, unsigned long long *d_new, hipStream_t s)
{
    if (!total_bases || !n_reads)
        return BRX_OK;
    const uint64_t n_items64 = (total_bases + L1_TILE - 1) / L1_TILE;
    if (n_items64 >= (1ull << 32)) {
        set_error("batch of %llu bases is too large for one insertion pass; split it", (unsigned long long)total_bases);
        return BRX_ERR_UNSUPPORTED;
    }
    L1Args a;
    memset(&a, 0, sizeof(a));
    a.bases = d_bases;
    a.offsets = d_offsets;
    a.n_reads = n_reads;
    a.total = total_bases;
    a.n_items = (uint32_t)n_items64;
    a.k = k;
    const int grid = a.n_items < 4096u ? (int)a.n_items : 4096;
    if (table)
        flat_insert_kernel<true><<<grid, 256, 0, s>>>(a, nullptr, table, line_shift, m, (uint32_t)k - m + 1u, d_new);
    else
        flat_insert_kernel<false><<<grid, 256, 0, s>>>(a, bits, nullptr, 0, 0, 0, nullptr);
    BRX_HIP(hipGetLastError());
    return BRX_OK;
}

// counts a batch into a counting table (see flat_count_kernel); *d_new grows by the keys that were not there yet
int flat_table_count(const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads, uint64_t total_bases, int k, uint64_t *table,
                     uint32_t *counts, uint32_t line_shift, uint32_t m, unsigned long long *d_new, hipStream_t s)
{
    if (!total_bases || !n_reads)
        return BRX_OK;
    const uint64_t n_items64 = (total_bases + L1_TILE - 1) / L1_TILE;
    if (n_items64 >= (1ull << 32)) {
        set_error("batch of %llu bases is too large for one counting pass; split it", (unsigned long long)total_bases);
        return BRX_ERR_UNSUPPORTED;
    }
    L1Args a;
    memset(&a, 0, sizeof(a));
    a.bases = d_bases;
    a.offsets = d_offsets;
    a.n_reads = n_reads;
    a.total = total_bases;
    a.n_items = (uint32_t)n_items64;
    a.k = k;
    flat_count_kernel<<<read_grid(a.n_items, 4096u), 256, 0, s>>>(a, table, counts, line_shift, m, (uint32_t)k - m + 1u, d_new);
    BRX_HIP(hipGetLastError());
    return BRX_OK;
}

// the tiles of a batch for the two sliced passes below
static int slice_args(const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads, uint64_t total_bases, int k, L1Args &a)
{
    const uint64_t n_items64 = (total_bases + L1_TILE - 1) / L1_TILE;
    if (n_items64 >= (1ull << 32)) {
        set_error("batch of %llu bases is too large for one counting pass; split it", (unsigned long long)total_bases);
        return BRX_ERR_UNSUPPORTED;
    }
    memset(&a, 0, sizeof(a));
    a.bases = d_bases;
    a.offsets = d_offsets;
    a.n_reads = n_reads;
    a.total = total_bases;
    a.n_items = (uint32_t)n_items64;
    a.k = k;
    return BRX_OK;
}

// flat_table_count for a sliced counter (see flat_count_slice_kernel): only the k-mers `part` of `parts` owns; d_stats4
// grows as brx_counter_slice_stats describes
int flat_table_count_slice(const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads, uint64_t total_bases, int k, uint64_t *table,
                           uint32_t *counts, uint32_t line_shift, uint32_t m, uint32_t part, uint32_t parts, unsigned long long *d_new,
                           unsigned long long *d_stats4, hipStream_t s)
{
    if (!total_bases || !n_reads)
        return BRX_OK;
    L1Args a;
    BRX_TRY(slice_args(d_bases, d_offsets, n_reads, total_bases, k, a));
    flat_count_slice_kernel<<<read_grid(a.n_items, 4096u), 256, 0, s>>>(a, table, counts, line_shift, m, (uint32_t)k - m + 1u, part, parts,
                                                                        d_new, d_stats4);
    BRX_HIP(hipGetLastError());
    return BRX_OK;
}

// the sizing pass (see flat_slice_census_kernel): d_out2[0] += the batch's k-mers of the part, d_out2[1] += its valid k-mers
int flat_slice_census(const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads, uint64_t total_bases, int k, uint32_t part,
                      uint32_t parts, unsigned long long *d_out2, hipStream_t s)
{
    if (!total_bases || !n_reads)
        return BRX_OK;
    L1Args a;
    BRX_TRY(slice_args(d_bases, d_offsets, n_reads, total_bases, k, a));
    flat_slice_census_kernel<<<read_grid(a.n_items, 4096u), 256, 0, s>>>(a, part, parts, d_out2);
    BRX_HIP(hipGetLastError());
    return BRX_OK;
}

// level-1 keys are u32 with a digit of at most MAX_DIGIT_BITS stripped: hashes of up to 41 bits, k <= 21
bool part_supported(int k)
{
    return 2 * k - 1 > F_BITS && 2 * k - 1 - F_BITS <= MAX_LEVELS * MAX_DIGIT_BITS && 2 * k - 1 - MAX_DIGIT_BITS <= 32;
}

int part_begin(brx_counter *c)
{
    PartState *st = new PartState();
    c->part = st;
    st->pl = make_plan(c->k);
    const Plan &pl = st->pl;
    st->pl_wide = pl;
    if (pl.nlev == 3 && pl.bits[1] < MAX_DIGIT_BITS) { // three levels: move bits from the last digit into the second
        Plan &w = st->pl_wide;
        const int moved = MAX_DIGIT_BITS - pl.bits[1] < pl.bits[2] ? MAX_DIGIT_BITS - pl.bits[1] : pl.bits[2];
        w.bits[1] += moved;
        w.bits[2] -= moved;
        w.rem_in[2] -= moved;
        w.nchild[1] <<= moved;
    } else if (pl.nlev == 4) {
        // four levels (k = 21: 9/7/7/6, hash count on 2^23 buckets of 18 bits): a 9-bit second digit and just enough third
        // digit to leave the 20 bits an LDS table entry can hold -- 9/9/3/8 -- ends in 2^21 buckets, four times as big:
        // from ~640 keys per bucket on they are taken by 1024-lane workgroups (3.4-5 ms per G keys) instead of one wave
        // each (6-11 ms per G keys, most of it per-bucket overhead on the scalar unit, profiles/r2j_sq_k21_summary.json)
        Plan &w = st->pl_wide;
        const int P = pl.bits[0] + pl.bits[1] + pl.bits[2] + pl.bits[3];
        const int b1 = MAX_DIGIT_BITS;
        int b2 = (pl.nbits - pl.bits[0] - b1) - 20;
        if (b2 < 0)
            b2 = 0;
        const int b3 = P - pl.bits[0] - b1 - b2;
        if (b3 >= 0 && b3 <= MAX_DIGIT_BITS && b2 <= MAX_DIGIT_BITS) {
            w.bits[1] = b1;
            w.bits[2] = b2;
            w.bits[3] = b3;
            w.rem_in[2] = w.rem_in[1] - b1;
            w.rem_in[3] = w.rem_in[2] - b2;
            w.nchild[1] = w.nchild[0] << b1;
            w.nchild[2] = w.nchild[1] << b2;
            w.nchild[3] = w.nchild[2] << b3;
        }
    }
    const char *what = "partition state";
    BRX_TRY(st->d_scalars.reserve(4, 0, what));
    for (int l = 0; l < pl.nlev; l++) {
        const uint64_t nc = pl.nchild[l] > st->pl_wide.nchild[l] ? pl.nchild[l] : st->pl_wide.nchild[l];
        BRX_TRY(st->d_coff[l].reserve(nc + 1, 0, what));
    }
    BRX_TRY(st->d_l1off_all.reserve(pl.nchild[0] + 1, 0, what));
    BRX_TRY(st->d_cnts.reserve(pl.nchild[0] + 1, 0, what));
    return st->d_shift.reserve(pl.nchild[0] + 1, 0, what);
}

void part_free(brx_counter *c)
{
    delete c->part;
    c->part = nullptr;
}

int part_reset(brx_counter *c)
{
    PartState *st = c->part;
    st->view_valid = false;
    for (auto &b : st->batches)
        if (!b.borrowed())
            st->spare.push_back(std::move(b));
    st->batches.clear();
    return BRX_OK;
}

// level-1 output of the (single) local batch: keys grouped by their first digit + bucket offsets
int part_l1_view(brx_counter *c, void **d_keys, void **d_l1off, uint32_t *n_buckets, uint64_t *n_keys)
{
    PartState *st = c->part;
    st->view_valid = false; // (the caller is about to move keys in or out of this counter)
    *n_buckets = (uint32_t)st->pl.nchild[0];
    if (st->batches.empty()) { // nothing counted (an empty shard): no keys, and the caller takes every offset as 0
        *d_keys = nullptr;
        *d_l1off = nullptr;
        *n_keys = 0;
        return BRX_OK;
    }
    if (st->batches.size() != 1 || st->batches[0].borrowed()) {
        set_error("l1_view needs exactly one locally counted batch (have %zu)", st->batches.size());
        return BRX_ERR_ARG;
    }
    *d_keys = st->batches[0].d_keys;
    *d_l1off = st->batches[0].d_l1off;
    *n_keys = st->batches[0].n;
    return BRX_OK;
}

// registers a level-1 segment produced elsewhere (another rank); the memory stays the caller's and
// must outlive finish
int part_add_partitioned(brx_counter *c, const uint32_t *d_keys, const uint64_t *d_l1off, uint64_t n_keys)
{
    PartState *st = c->part;
    st->view_valid = false;
    if (n_keys == 0)
        return BRX_OK;
    PartBatch b;
    b.d_keys = const_cast<uint32_t *>(d_keys);
    b.d_l1off = const_cast<uint64_t *>(d_l1off);
    b.n = n_keys;
    st->batches.push_back(std::move(b));
    return BRX_OK;
}

// matrix / scan scratch for `n_entries` per-tile counters, pos for `n_pos` positions (levels >= 2: one per counter;
// level 1: one per range and digit)
static int ensure_matrix(PartState *st, uint64_t n_entries, uint64_t n_pos)
{
    BRX_TRY(ws_reserve(st->d_matrix, (n_entries + 1) * 4));
    BRX_TRY(ws_reserve(st->d_pos, (n_pos + 2) * 8));
    return ws_reserve(st->d_scan_tmp, scan_tmp_bytes((uint32_t)n_entries) + 64);
}

static size_t scatter_lds_bytes(uint32_t tile, int bits)
{
    const size_t B = (size_t)1 << bits;
    return (size_t)tile * 6 + B * 8 + B * 12 + 64;
}

static size_t l1_scatter_lds_bytes(int bits)
{
    const size_t B = (size_t)1 << bits;
    return (size_t)L1_TILE * 4 + B * 8 + B * 12 + 64; // keys, sector index + carry state, three counters
}

int part_add_batch(brx_counter *c, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads,
                   uint64_t total_bases, hipStream_t s)
{
    PartState *st = c->part;
    const Plan &pl = st->pl;
    st->view_valid = false;
    if (total_bases == 0 || n_reads == 0)
        return BRX_OK;
    const uint64_t max_keys = total_bases; // upper bound of the number of k-mers of this batch
    PartBatch b;
    for (size_t i = 0; i < st->spare.size(); i++)
        if (st->spare[i].cap() >= max_keys) {
            b = std::move(st->spare[i]);
            st->spare.erase(st->spare.begin() + (long)i);
            break;
        }
    if (!b.d_keys) {
        BRX_TRY(ws_reserve(b.own_keys, (max_keys + 1) * 4));
        BRX_TRY(b.own_l1off.reserve(pl.nchild[0] + 1, 0, "partition offsets"));
        b.d_keys = b.own_keys;
        b.d_l1off = b.own_l1off;
    }
    const uint32_t B = 1u << pl.bits[0];
    const uint64_t n_items64 = (total_bases + L1_TILE - 1) / L1_TILE;
    if (n_items64 * B >= (1ull << 32)) {
        set_error("batch of %llu bases is too large for one partition pass; split it", (unsigned long long)total_bases);
        return BRX_ERR_UNSUPPORTED;
    }
    const uint32_t n_items = (uint32_t)n_items64;
    const uint64_t n_entries = (uint64_t)B * n_items;
    // One partition of the tiles into contiguous ranges, a block per range in both kernels: the histogram leaves the
    // range sums the scan turns into range starts, the scatter carries sector remainders from tile to tile of its range.
    // Twice the blocks the chip holds of the scatter at once (5 per CU at 27 KB of LDS): the ranges stay long (~100 tiles
    // at 1 Gbp) and the last round of blocks short.  (BRX_L1_GRID: tests shrink the number of ranges so that small inputs
    // give every block several tiles)
    const char *genv = getenv("BRX_L1_GRID");
    const long gev = genv ? atol(genv) : 0;
    const uint32_t want_ranges = gev > 0 ? (uint32_t)gev : 2560u;
    const uint32_t n_ranges = n_items < want_ranges ? n_items : want_ranges;
    BRX_TRY(ensure_matrix(st, n_entries, ((uint64_t)n_ranges + 1) * B));
    uint64_t *coltot = st->d_pos + (uint64_t)n_ranges * B;
    L1Args a;
    memset(&a, 0, sizeof(a));
    a.bases = d_bases;
    a.offsets = d_offsets;
    a.n_reads = n_reads;
    a.total = total_bases;
    a.n_items = n_items;
    a.k = pl.k;
    a.nbits = pl.nbits;
    a.bits = pl.bits[0];
    a.matrix = st->d_matrix;
    a.n_ranges = n_ranges;
    a.rsum = st->d_pos;
    a.coff = b.d_l1off;
    a.keys_out = b.d_keys;
    a.out_cap = b.cap();
    {
        KernelTimer t("part_l1_hist", s);
        l1_hist_kernel<<<n_ranges, 256, (size_t)B * 4, s>>>(a);
    }
    trace_stage(s, "partition level 1: histograms");
    {
        // where every range starts in every digit, and the digit offsets, from the range sums (col_scan_* above)
        KernelTimer t("offsets_scan", s);
        col_scan_columns_kernel<<<B, 256, 0, s>>>(st->d_pos, n_ranges, B, coltot);
        col_scan_digits_kernel<<<1, 64, 0, s>>>(coltot, B, b.d_l1off, st->d_scalars + 1);
    }
    {
        KernelTimer t("part_l1_scatter", s);
        const size_t lds1 = l1_scatter_lds_bytes(a.bits);
        if (lds1 > 64 * 1024)
            BRX_HIP(hipFuncSetAttribute((const void *)l1_scatter_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds1));
        l1_scatter_kernel<<<n_ranges, 256, lds1, s>>>(a);
    }
    trace_stage(s, "partition level 1: scatter");
    BRX_HIP(hipGetLastError());
    unsigned long long tot = 0;
    BRX_HIP(hipMemcpyAsync(&tot, st->d_scalars + 1, 8, hipMemcpyDeviceToHost, s));
    BRX_HIP(hipStreamSynchronize(s));
    b.n = tot;
    st->batches.push_back(std::move(b));
    return BRX_OK;
}

// one level >= 2: work items -> per-tile histograms -> scan -> scatter -> child offsets
template <typename OUT>
static int run_level(PartState *st, int l, const uint32_t *keys_in, const uint64_t *poff, uint64_t n_parents, uint64_t total,
                     void *keys_out, hipStream_t s, const char *tag_hist, const char *tag_scatter)
{
    const Plan &pl = st->use_wide ? st->pl_wide : st->pl;
    const uint32_t B = 1u << pl.bits[l];
    // 8192 keys per tile whatever the digit width: the (tile, digit) runs a scatter writes are then 32 keys = 128 bytes
    // on average instead of 64, and runs that straddle fewer lines cost fewer read-for-ownership fetches (level 2 of
    // the bench: 4.5 -> 2.7 ms; BRX_SMALL_TILES=1 restores 4096 for 8-bit digits)
    static const bool small_tiles = [] { const char *e = getenv("BRX_SMALL_TILES"); return e && *e == '1'; }();
    const uint32_t tile = (pl.bits[l] > 8 || !small_tiles) ? 8192u : 4096u;
    const uint64_t ub_items = total / tile + n_parents + 1;
    const uint64_t n_entries = (uint64_t)B * ub_items;
    if (n_entries >= (1ull << 32)) {
        set_error("partition level %d needs %llu tile counters; split the input into smaller counters", l + 1,
                  (unsigned long long)n_entries);
        return BRX_ERR_UNSUPPORTED;
    }
    {
        BRX_TRY(ws_reserve(st->d_ntiles, (n_parents + 1) * 4));
        BRX_TRY(ws_reserve(st->d_item_off, (n_parents + 2) * 8));
        BRX_TRY(ws_reserve(st->d_items, (ub_items + 1) * sizeof(LnItem)));
    }
    BRX_TRY(ensure_matrix(st, n_entries > n_parents ? n_entries : n_parents, n_entries > n_parents ? n_entries : n_parents));
    tiles_from_offsets_kernel<<<(unsigned)((n_parents + 255) / 256), 256, 0, s>>>(poff, n_parents, tile, st->d_ntiles);
    BRX_TRY(exclusive_scan_lens(st->d_ntiles, (uint32_t)n_parents, st->d_scan_tmp, st->d_item_off, st->d_scalars, s));
    fill_items_kernel<<<(unsigned)((n_parents + 255) / 256), 256, 0, s>>>(poff, st->d_item_off, n_parents, tile, st->d_items);
    trace_stage(s, tag_hist);
    BRX_HIP(hipMemsetAsync(st->d_matrix, 0, n_entries * 4, s));
    LnArgs a;
    memset(&a, 0, sizeof(a));
    a.keys_in = keys_in;
    a.in_cap = total;
    a.items = st->d_items;
    a.n_items = st->d_scalars;
    a.tile = tile;
    a.rem_in = pl.rem_in[l];
    a.bits = pl.bits[l];
    a.matrix = st->d_matrix;
    a.pos = st->d_pos;
    a.keys_out = keys_out;
    a.out_cap = total + 64;
    const int grid = 256 * 8;
    {
        KernelTimer t(tag_hist, s);
        if (tile == 8192u)
            ln_hist_kernel<32><<<grid, 256, (size_t)B * 4, s>>>(a);
        else
            ln_hist_kernel<16><<<grid, 256, (size_t)B * 4, s>>>(a);
    }
    trace_stage(s, "  histograms done");
    {
        KernelTimer t("offsets_scan", s);
        const unsigned g = n_parents < 4096 ? (unsigned)n_parents : 4096u;
        ln_colscan_kernel<<<g, 256, 0, s>>>(st->d_matrix, poff, st->d_item_off, n_parents, B, st->d_pos, st->d_coff[l]);
    }
    {
        KernelTimer t(tag_scatter, s);
        const size_t lds = scatter_lds_bytes(tile, a.bits);
        if (tile == 8192u)
            ln_scatter_kernel<32, OUT><<<grid, 256, lds, s>>>(a);
        else
            ln_scatter_kernel<16, OUT><<<grid, 256, lds, s>>>(a);
    }
    trace_stage(s, tag_scatter);
    BRX_HIP(hipGetLastError());
    return BRX_OK;
}

// d_hist != nullptr: no set is produced (dst is not touched); the keys go through every level and the final buckets
// are binned into the 256-entry count spectrum (bins 1..255)
// view: no set either; the same levels, then the final buckets become the count view (final_view_kernel)
static int part_finish_impl(brx_counter *c, uint32_t abundance, hipStream_t s, brx_set *dst, unsigned long long *d_hist,
                            bool view = false)
{
    PartState *st = c->part;
    st->view_valid = false; // the levels below overwrite what a view is made of
    const bool no_set = d_hist || view;
    uint64_t total = 0;
    for (auto &b : st->batches)
        total += b.n;
    // Buckets that end in the LDS hash table (no bit vector to write) and would average more keys than one table pass
    // takes even at high coverage: cut them finer at level 2 instead (k = 19: digits 9, 9 in place of 9, 8 -- 2^18
    // buckets with 19 bits left; configs[3]'s share per GPU then has 24 000 keys per bucket, ~5 000 of them distinct)
    // (BRX_WIDE_L2 = the average bucket size from which on the wider digit is used, 0 = never, 1 = always; read per call:
    // the fuzzers force it on small inputs)
    const char *e_wide = getenv("BRX_WIDE_L2");
    const uint64_t wide_from = e_wide && *e_wide ? strtoull(e_wide, nullptr, 10) : 16384ull;
    const bool lazy_on = [] { const char *e = getenv("BRX_LAZY_BITS"); return !(e && *e == '0'); }(); // (per call too)
    st->use_wide = wide_from != 0 && !no_set && dst && (dst->sparse || (index_wanted(c->k) && lazy_on)) &&
                   st->pl_wide.bits[1] != st->pl.bits[1] &&
                   (wide_from == 1 || (st->pl.nlev == 3 ? total / st->pl.nchild[1] > wide_from
                                                        // four levels: as soon as the wider buckets fill a workgroup
                                                        : total / st->pl_wide.nchild[2] > 640));
    const Plan &pl = st->use_wide ? st->pl_wide : st->pl;
    const uint32_t B1 = (uint32_t)pl.nchild[0];

    const uint32_t *keys1 = nullptr;
    const uint64_t *l1off = nullptr;
    if (st->batches.empty() || total == 0) {
        if (view) {
            st->view_empty = true; // nothing counted: every lookup answers 0
            st->view_valid = true;
        }
        if (no_set)
            return BRX_OK; // nothing counted: bins 1..255 stay 0
        if (dst->sparse) {
            BRX_TRY(dst->d_keylist_n.reserve(1, 0, "key list counter"));
            BRX_HIP(hipMemsetAsync(dst->d_keylist_n, 0, 8, s));
            keylist_mark(dst, true); // the empty list
        } else {
            BRX_HIP(hipMemsetAsync(dst->d_bits, 0, dst->nwords * 4, s));
            bits_mark(dst, true);
        }
        return BRX_OK;
    } else if (st->batches.size() == 1) {
        keys1 = st->batches[0].d_keys;
        l1off = st->batches[0].d_l1off;
    } else {
        BRX_TRY(ws_reserve(st->d_merged, (total + 1) * 4));
        BRX_TRY(ensure_matrix(st, B1 + 1, B1 + 1));
        BRX_HIP(hipMemsetAsync(st->d_cnts, 0, (uint64_t)B1 * 4, s));
        for (auto &b : st->batches)
            add_counts_kernel<<<(B1 + 255) / 256, 256, 0, s>>>(b.d_l1off, B1, st->d_cnts, nullptr);
        BRX_TRY(exclusive_scan_lens(st->d_cnts, B1, st->d_scan_tmp, st->d_l1off_all, st->d_scalars + 1, s));
        BRX_HIP(hipMemsetAsync(st->d_cnts, 0, (uint64_t)B1 * 4, s));
        for (auto &b : st->batches) {
            add_counts_kernel<<<(B1 + 255) / 256, 256, 0, s>>>(b.d_l1off, B1, st->d_cnts, st->d_shift);
            merge_segments_kernel<<<B1 < 4096u ? B1 : 4096u, 256, 0, s>>>(b.d_keys, b.d_l1off, st->d_l1off_all, st->d_shift, B1,
                                                                         st->d_merged);
        }
        keys1 = st->d_merged;
        l1off = st->d_l1off_all;
    }

    BRX_TRY(ws_reserve(st->d_keys_fin, (total + 64) * 2));
    // solid-key list for the probe index: a solid hash was seen more than `abundance` times, so there are at
    // most total / (abundance + 1) of them; real data is far below that, and a list that turns out too short
    // is simply not used (the index is then built from the bit vector)
    const bool emit = !no_set && (dst->sparse || index_wanted(c->k));
    // lazy bit vector: when the solid hashes are listed anyway, the 2^(2k-4)-byte vector (16 GiB of slices at k = 19)
    // is written only if somebody asks for it later (ensure_bits); BRX_LAZY_BITS=0 writes it here as before
    const bool lazy = emit && !dst->sparse && lazy_on;
    if (emit) {
        // (a set without bits has nothing but this list: it gets the exact bound)
        const uint64_t div = (dst->sparse || lazy) ? abundance + 1u : (abundance + 1u > 8u ? abundance + 1u : 8u);
        const uint64_t want = total / div + (1ull << 20);
        BRX_TRY(dst->d_keylist.reserve(want, 0, "solid key list"));
        BRX_TRY(dst->d_keylist_n.reserve(1, 0, "key list counter"));
        BRX_HIP(hipMemsetAsync(dst->d_keylist_n, 0, 8, s));
    }
    // levels 2 .. nlev: u32 keys through one or two middle buffers, u16 out of the last level
    static const char *hist_tag[MAX_LEVELS] = {"part_l1_hist", "part_l2_hist", "part_l3_hist", "part_l4_hist"};
    static const char *scat_tag[MAX_LEVELS] = {"part_l1_scatter", "part_l2_scatter", "part_l3_scatter", "part_l4_scatter"};
    if (pl.nlev >= 3)
        BRX_TRY(ws_reserve(st->d_keys_mid, (total + 64) * 4));
    if (pl.nlev >= 4)
        BRX_TRY(ws_reserve(st->d_keys_mid2, (total + 64) * 4));
    const uint32_t *kin = keys1;
    const uint64_t *poff = l1off;
    // no slices to write (lazy / sparse): stop one level early and hash-count the coarser buckets, if they are small
    // enough for an LDS table (k = 19 at 1 Gbp: 131 072 buckets of ~7 600 keys with 20 bits left)
    const bool hf_on = [] { const char *e = getenv("BRX_HASH_FINAL"); return !(e && *e == '0'); }(); // (per call: fuzzers)
    const int R_hf = pl.rem_in[pl.nlev - 1];
    const uint64_t nb_hf = pl.nlev >= 2 ? pl.nchild[pl.nlev - 2] : 0;
    // (up to 2^17 keys per bucket: the table then takes a bucket in a few passes over its key range, see hash_final_kernel)
    static const uint64_t hf_max_avg = [] { const char *e = getenv("BRX_HASH_FINAL_MAX"); return e && *e ? strtoull(e, nullptr, 10) : 131072ull; }();
    const bool hash_final = !no_set && hf_on && (dst->sparse || lazy) && pl.nlev >= 3 && R_hf <= 20 && total / nb_hf <= hf_max_avg;
    for (int l = 1; l < pl.nlev; l++) {
        if (hash_final && l == pl.nlev - 1)
            break;
        if (l == pl.nlev - 1) {
            BRX_TRY(run_level<uint16_t>(st, l, kin, poff, pl.nchild[l - 1], total, st->d_keys_fin, s, hist_tag[l], scat_tag[l]));
        } else {
            uint32_t *kout = (l & 1) ? st->d_keys_mid : st->d_keys_mid2;
            BRX_TRY(run_level<uint32_t>(st, l, kin, poff, pl.nchild[l - 1], total, kout, s, hist_tag[l], scat_tag[l]));
            kin = kout;
        }
        poff = st->d_coff[l];
    }
    if (hash_final) {
        KernelTimer t("part_hash_final", s);
        const uint64_t avg = total / nb_hf;
        // test hooks, read per call: BRX_HF_LOG_T = the launch's table maximum (log2), BRX_HF_MIN_LT = the smallest table a
        // bucket gets, BRX_HF_RATIO = the share of distinct keys to assume instead of the sampled one.  Small or wrongly
        // guessed tables walk the whole ladder (bigger table -> 4x finer passes) on inputs a test can afford.
        const char *e_logt = getenv("BRX_HF_LOG_T"), *e_minlt = getenv("BRX_HF_MIN_LT"), *e_ratio = getenv("BRX_HF_RATIO");
        const float ratio_forced = e_ratio && *e_ratio ? (float)atof(e_ratio) : 0.0f;
        // how many of a bucket's keys are distinct, measured on 64 buckets: sizes each bucket's table and passes
        unsigned long long *dup = st->d_scalars + 2;
        {
            BRX_HIP(hipMemsetAsync(dup, 0, 16, s));
            BRX_HIP(hipFuncSetAttribute((const void *)hf_sample_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 65536));
            const int ns = (int)(nb_hf < 64ull ? nb_hf : 64ull);
            hf_sample_kernel<<<ns, 1024, 65536, s>>>(kin, poff, nb_hf, R_hf, 14, dup);
        }
        if (avg > 640) { // one 1024-thread workgroup per bucket, 16384-entry table
            uint32_t log_t = 14;
            if (e_logt && *e_logt && atoi(e_logt) >= 6 && atoi(e_logt) <= 14)
                log_t = (uint32_t)atoi(e_logt);
            const uint32_t min_lt = e_minlt && *e_minlt && atoi(e_minlt) >= 4 ? (uint32_t)atoi(e_minlt) : 12u;
            const size_t lds = ((size_t)4 << log_t) + hf_ebuf(1024) * 8 + 16;
            BRX_HIP(hipFuncSetAttribute((const void *)hash_final_kernel<1024, 1024>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            const int grid = (int)(nb_hf < 256ull * 4ull ? nb_hf : 256ull * 4ull);
            hash_final_kernel<1024, 1024><<<grid, 1024, lds, s>>>(kin, poff, nb_hf, R_hf, abundance, log_t, dst->d_keylist, dst->d_keylist.cap(),
                                                          dst->d_keylist_n, dup, min_lt, ratio_forced);
        } else { // one wave per bucket; at most 256..2048 table entries, about 4x the average bucket (each bucket then uses
                 // 2.5 slots per distinct key expected: clearing and scanning cost T / 256 LDS accesses per lane).  Sizing
                 // the launch's maximum from the sampled ratio as well (1024 slots = 6 workgroups per CU instead of 3)
                 // measured the same 66.9 ms at configs[4]'s share: the kernel is not short of waves.
            uint32_t log_t = 8;
            while (log_t < 11 && (1ull << log_t) < 4 * avg)
                log_t++;
            if (e_logt && *e_logt && atoi(e_logt) >= 6 && atoi(e_logt) <= 11)
                log_t = (uint32_t)atoi(e_logt);
            const uint32_t min_lt = e_minlt && *e_minlt && atoi(e_minlt) >= 4 ? (uint32_t)atoi(e_minlt) : 8u;
            const size_t lds = 4 * (((size_t)4 << log_t) + hf_ebuf(64) * 8 + 16);
            const uint64_t want = (nb_hf + 3) / 4;
            const int grid = (int)(want < 256ull * 16ull ? want : 256ull * 16ull);
            hash_final_kernel<64, 256><<<grid, 256, lds, s>>>(kin, poff, nb_hf, R_hf, abundance, log_t, dst->d_keylist, dst->d_keylist.cap(),
                                                         dst->d_keylist_n, dup, min_lt, ratio_forced);
        }
        BRX_HIP(hipGetLastError());
        trace_stage(s, "hash final");
        keylist_mark(dst, true);
        bits_mark(dst, !lazy);
        return BRX_OK;
    }
    const uint64_t *fin_off = st->d_coff[pl.nlev - 1];
    if (view) {
        BRX_TRY(ws_reserve(st->d_view_cnt, total + 64));
        {
            KernelTimer t("part_view", s);
            const uint64_t nb = pl.nchild[pl.nlev - 1];
            const uint64_t chunks = (nb + VW_PER_WAVE * VW_WAVES - 1) / (VW_PER_WAVE * VW_WAVES);
            final_view_kernel<<<read_grid(chunks, 2048u), 64 * VW_WAVES, 0, s>>>(st->d_keys_fin, fin_off, nb, st->d_view_cnt);
        }
        BRX_HIP(hipGetLastError());
        trace_stage(s, "count view");
        BRX_HIP(hipStreamSynchronize(s));
        st->view_empty = false;
        st->view_valid = true;
        return BRX_OK;
    }
    if (d_hist) {
        KernelTimer t("part_spectrum", s);
        const uint64_t nb = pl.nchild[pl.nlev - 1];
        const uint64_t want = (nb + SP_WAVES - 1) / SP_WAVES;
        final_spectrum_kernel<<<(int)(want < 256ull * 8ull ? want : 256ull * 8ull), 64 * SP_WAVES, 0, s>>>(st->d_keys_fin, fin_off, nb, d_hist);
        BRX_HIP(hipGetLastError());
        trace_stage(s, "spectrum");
        return BRX_OK;
    }
    {
        KernelTimer t("part_final_count", s);
        const uint64_t nb = pl.nchild[pl.nlev - 1];
        const uint64_t want_waves = nb < (256ull * 16ull * 8ull) ? nb : (256ull * 16ull * 8ull);
        const int grid = (int)((want_waves + P3_WAVES - 1) / P3_WAVES);
        if (dst->sparse || lazy)
            final_count_kernel<true, false><<<grid, 64 * P3_WAVES, 0, s>>>(st->d_keys_fin, fin_off, nb, abundance, nullptr,
                                                                          dst->d_keylist, dst->d_keylist.cap(), dst->d_keylist_n);
        else if (emit)
            final_count_kernel<true, true><<<grid, 64 * P3_WAVES, 0, s>>>(st->d_keys_fin, fin_off, nb, abundance, dst->d_bits,
                                                                         dst->d_keylist, dst->d_keylist.cap(), dst->d_keylist_n);
        else
            final_count_kernel<false, true><<<grid, 64 * P3_WAVES, 0, s>>>(st->d_keys_fin, fin_off, nb, abundance, dst->d_bits,
                                                                          nullptr, 0, nullptr);
    }
    BRX_HIP(hipGetLastError());
    trace_stage(s, "final count");
    keylist_mark(dst, emit);
    bits_mark(dst, !lazy);
    return BRX_OK;
}

int part_finish_into(brx_counter *c, uint32_t abundance, hipStream_t s, brx_set *dst)
{
    const int rc = part_finish_impl(c, abundance, s, dst, nullptr);
#if BRX_DEBUG_BOUNDS
    unsigned long long bad = 0;
    BRX_HIP(hipStreamSynchronize(s));
    BRX_HIP(hipMemcpyFromSymbol(&bad, HIP_SYMBOL(bounds_violations), 8));
    if (bad) {
        set_error("BRX_DEBUG_BOUNDS: %llu scatter stores / key loads of the partition passes were out of range and dropped", bad);
        return BRX_ERR_HIP;
    }
#endif
    return rc;
}

// bins 1..255 of the count spectrum into d_hist (256 x u64, zeroed by the caller); the counter is left as it was
int part_spectrum(brx_counter *c, hipStream_t s, unsigned long long *d_hist)
{
    return part_finish_impl(c, 255u, s, nullptr, d_hist);
}

// The count view of everything counted so far, for abundance lookups: levels 2..n as for the spectrum, then every final
// bucket sorted and counted in place.  Valid -- after this has returned, the stream synchronised -- until the counter is
// next asked for anything that touches its batches or the partition workspace; each of those clears view_valid first.
int part_lookup_prepare(brx_counter *c, hipStream_t s)
{
    if (c->part->view_valid)
        return BRX_OK; // nothing has touched the counter since the view was built
    return part_finish_impl(c, 255u, s, nullptr, nullptr, true);
}

void part_lookup_drop(brx_counter *c)
{
    PartState *st = c->part;
    st->view_valid = false;
    st->d_view_cnt.reset();
}

bool part_lookup_ready(const brx_counter *c) { return c->part && c->part->view_valid; }

// what a lookup reads; false: no valid view.  *keys == nullptr with true: nothing was counted, every count is 0
bool part_lookup_view(const brx_counter *c, const uint16_t **keys, const uint8_t **counts, const uint64_t **off)
{
    const PartState *st = c->part;
    if (!st || !st->view_valid)
        return false;
    *keys = st->view_empty ? nullptr : st->d_keys_fin.get();
    *counts = st->view_empty ? nullptr : st->d_view_cnt.get();
    *off = st->view_empty ? nullptr : st->d_coff[st->pl.nlev - 1].get();
    return true;
}

// how far the view reaches: *n_buckets last-level buckets (off holds one entry more), *n_positions = off[*n_buckets]
bool part_lookup_shape(const brx_counter *c, uint64_t *n_buckets, uint64_t *n_positions)
{
    const PartState *st = c->part;
    if (!st || !st->view_valid)
        return false;
    uint64_t total = 0;
    for (auto &b : st->batches)
        total += b.n;
    *n_buckets = st->pl.nchild[st->pl.nlev - 1];
    *n_positions = st->view_empty ? 0 : total;
    return true;
}

} // namespace brx
