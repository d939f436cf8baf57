// Set algebra (include/brx.h "set algebra", br_amd/setops.py states it in numpy): union, intersection, difference and
// symmetric difference of two strictly ascending lists of u64 keys, by merge path.
//
//   tiles    position d of the merged sequence (ties: the key of A before the equal key of B) is reached after a(d) keys of
//            A and d - a(d) keys of B; a(d) is found by a binary search on the diagonal d.  A tile is MERGE_TILE consecutive
//            positions; merge_split_kernel finds a() at every tile border, once, for both passes.  The search keeps
//            max(0, d - nb) <= a <= min(d, na) whatever the keys hold, and every index it reads lies inside that bracket.
//   a tile   its piece of A and its piece of B go to LDS with one key before and one key behind each (the halo): tile_load,
//            and tile_load_counts for the count bytes of a count list, indexed alike.
//   walk     tile_walk: thread t finds a() of its own diagonal, MERGE_PER_THREAD * t positions into the tile, by the same
//            search in LDS, and decides MERGE_PER_THREAD positions serially.  With ties A-first, A[i] is in B iff the first
//            unconsumed B[j] equals it (j may be the halo behind the piece), and B[j] is in A iff i > 0 and A[i - 1] equals
//            it (i - 1 may be the halo before the piece): no thread asks another one.  An equal pair is (key of A, key of
//            B) and is decided where A's key is taken.  What is done with a decided position is the caller's: the count
//            merge and the joint spectrum.  Set algebra (tile_merge) keeps the same loop written out: through the walk its
//            "set_merge" timer measured up to 1.6 % slower than before on three of ten operations, beyond the noise allowed.
//   check    tile_check: every neighbouring pair of either list, the halo pairs included, must ascend strictly, the borders
//            must not run backwards (they cannot over ascending lists), and no count of a count list is 0.
//   report   tile_report: |A n B| summed with one atomic per tile, the error bits or-ed; a set bit means nothing is written.
//   place    tile_place: a thread's offset among the kept entries of its tile, by a block scan of the threads' counts.
//   pass 1   split, then one kernel that loads, checks, walks and reports every tile; the existing exclusive scan turns the
//            kernel's tile counts into offsets, its total is the size of the result (merge_pass1 on the host).
//   pass 2   the same walk, the kept entries compacted in LDS at their place, then stored as one contiguous run per tile,
//            256 neighbouring entries per step.
// Blocks loop over tiles; the grid cap is read_grid()'s.  Three consumers:
//   set algebra   an operation is a keep rule over "the other list holds it too" (KEEP_A / KEEP_B below).  merge_count_kernel,
//            merge_write_kernel; the size of the result follows from |A|, |B|, |A n B|.  Timer "set_merge".
//   count lists   (include/brx.h "count lists", br_amd/countops.py) add / max / min / sub of two sorted (key, count byte) lists;
//            keep is result >= min_count: a function of the counts, so pass 1 (count_merge_count_kernel) loads them too and
//            no size follows from |A|, |B|, |A n B|.  Pass 2 (count_merge_write_kernel) sums what it wrote: that must be the
//            scanned total.  Its LDS: 2 x 2050 keys, 2048 staged keys, 2 x 2050 + 2048 count bytes, 55 KB static.  Timer
//            "count_merge"; count_hist_kernel (a list's spectrum) under "count_hist".
//   joint    count_joint_kernel: pass 1 without a keep rule -- the pair (ca, cb) of every key of A u B binned into u64[256][256],
//            the bins below 64 x 64 in 16 KB of LDS per block (53 KB static with the pieces), the rest by global adds.  The
//            table is built in scratch and copied out only when both lists passed the checks.  Timer "count_joint".
#include "brx_internal.hpp"

#include <chrono>
#include <string.h>

using namespace brx;

namespace {

typedef unsigned long long u64;

constexpr uint32_t MERGE_PER_THREAD = 8;                   // (br_amd/setops.py PER_THREAD)
constexpr uint32_t MERGE_TILE = 256u * MERGE_PER_THREAD;   // (br_amd/setops.py TILE)
constexpr uint32_t ERR_ORDER = 1u; // the keys of an input do not ascend strictly
constexpr uint32_t ERR_ZERO = 2u;  // a 0 count in an input

// bit 0: keep a key that the other list lacks, bit 1: keep a key that the other list holds too
constexpr uint32_t KEEP_A[4] = {3u, 2u, 1u, 1u}; // union, intersection, difference, symmetric difference
constexpr uint32_t KEEP_B[4] = {1u, 0u, 0u, 1u};

typedef std::chrono::steady_clock Clock;
uint64_t ns_since(Clock::time_point t0) { return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(Clock::now() - t0).count(); }

// keys of `a` among the first d of the merge of a[0 .. na) and b[0 .. nb), d <= na + nb.  lo <= mid < hi <= min(d, na) and
// 0 <= d - 1 - mid < nb hold from the bracket alone: nothing read decides where the next read goes beyond it.
template <typename T> __device__ __forceinline__ T merge_split(const u64 *a, T na, const u64 *b, T nb, T d)
{
    T lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const T mid = lo + (hi - lo) / 2;
        if (a[mid] <= b[d - 1 - mid])
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// split[t] = keys of A before tile t, t = 0 .. n_tiles (the last one: na)
__global__ __launch_bounds__(256) void merge_split_kernel(const u64 *__restrict__ a, uint64_t na, const u64 *__restrict__ b, uint64_t nb,
                                                          uint64_t n_tiles, u64 *__restrict__ split)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, n = na + nb;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t <= n_tiles; t += stride) {
        const uint64_t d = t * MERGE_TILE < n ? t * MERGE_TILE : n;
        split[t] = merge_split<uint64_t>(a, na, b, nb, d);
    }
}

// The pieces of tile t in LDS and each thread's share of the merge.
struct Tile {
    uint64_t a0, b0;  // where the pieces start in A and B
    uint32_t la, lb;  // their lengths, la + lb <= MERGE_TILE
    bool ok;          // the borders run forward
};

// sa / sb: MERGE_TILE + 2 entries each; entry 1 + x = key x of the piece, entry 0 and entry 1 + length the halo (left
// unwritten where the list ends there: the merge asks the global index before it reads them)
__device__ __forceinline__ Tile tile_load(const u64 *__restrict__ a, uint64_t na, const u64 *__restrict__ b, uint64_t nb,
                                          const u64 *__restrict__ split, uint64_t t, u64 *sa, u64 *sb)
{
    const uint64_t n = na + nb;
    const uint64_t d0 = t * MERGE_TILE, d1 = d0 + MERGE_TILE < n ? d0 + MERGE_TILE : n; // (d0 < n: t < n_tiles)
    const uint64_t a0 = split[t], a1 = split[t + 1];
    Tile tl;
    // (a0 <= d0 and a1 <= d1 by the search's bracket; over lists that do not ascend a border may still run backwards)
    tl.ok = a0 <= d0 && a1 <= d1 && a0 <= na && a1 <= na && a1 >= a0 && d1 - a1 >= d0 - a0 && d1 - a1 <= nb;
    tl.a0 = tl.ok ? a0 : 0;
    tl.b0 = tl.ok ? d0 - a0 : 0;
    tl.la = tl.ok ? (uint32_t)(a1 - a0) : 0u; // la + lb = d1 - d0 <= MERGE_TILE, both >= 0
    tl.lb = tl.ok ? (uint32_t)((d1 - a1) - (d0 - a0)) : 0u;
    if (tl.ok) {
        for (uint32_t x = threadIdx.x; x < tl.la + 2u; x += 256u) {
            const uint64_t i = tl.a0 + x; // global index + 1
            if (i >= 1 && i <= na)
                sa[x] = a[i - 1];
        }
        for (uint32_t x = threadIdx.x; x < tl.lb + 2u; x += 256u) {
            const uint64_t j = tl.b0 + x;
            if (j >= 1 && j <= nb)
                sb[x] = b[j - 1];
        }
    }
    __syncthreads();
    return tl;
}

// The thread's MERGE_PER_THREAD positions of the tile, in order: at(q, from_a, i, j, paired) for every position q before the
// tile's end -- the key is sa[1 + i] when from_a, else sb[1 + j]; paired: the other list holds it too.  Positions behind the
// tile's end get no call: the caller pre-sets its outputs.  Returns the keys of A found in B among the positions.
//   bracket  the search of the thread's diagonal reads only inside 0 <= i < la, 0 <= j < lb (merge_split's bracket).
//   a key    i + j = d + q < la + lb at every position: at least one piece has a key left, and take_a reads sa[1 + i] only
//            for i < la, sb[1 + j] only for j < lb.
//   halo     in_b reads sb[1 + j] at j == lb (the entry behind B's piece, its count beside it) and in_a reads sa[i] at
//            i == 0 (the entry before A's piece) only after the global index said that the list has such an entry.
//   pair     ties A-first: an equal pair is decided at A's key (from_a, paired, B's entry at 1 + j); B's key of the pair
//            comes next (not from_a, paired) and yields nothing of its own.
template <typename At>
__device__ __forceinline__ uint32_t tile_walk(const Tile &tl, uint64_t na, uint64_t nb, const u64 *sa, const u64 *sb, At at)
{
    const uint32_t len = tl.la + tl.lb;
    const uint32_t d = threadIdx.x * MERGE_PER_THREAD < len ? threadIdx.x * MERGE_PER_THREAD : len;
    uint32_t i = merge_split<uint32_t>(sa + 1, tl.la, sb + 1, tl.lb, d), j = d - i;
    uint32_t nboth = 0;
#pragma unroll
    for (uint32_t q = 0; q < MERGE_PER_THREAD; q++) {
        if (d + q >= len)
            continue;
        const bool take_a = i < tl.la && (j >= tl.lb || sa[1 + i] <= sb[1 + j]);
        if (take_a) {
            const bool in_b = tl.b0 + j < nb && sb[1 + j] == sa[1 + i];
            at(q, true, i, j, in_b);
            nboth += in_b ? 1u : 0u;
            i++;
        } else {
            const bool in_a = tl.a0 + i > 0 && sa[i] == sb[1 + j];
            at(q, false, i, j, in_a);
            j++;
        }
    }
    return nboth;
}

// Set algebra's positions: key[q], keep bit q of the result; *both = keys of A found in B.  tile_walk's loop with the keep
// rule written into it (see the head of the file); its invariants are tile_walk's, and a fix to one is a fix to both.
__device__ __forceinline__ uint32_t tile_merge(const Tile &tl, uint64_t na, uint64_t nb, const u64 *sa, const u64 *sb, uint32_t keep_a,
                                               uint32_t keep_b, u64 key[MERGE_PER_THREAD], uint32_t *both)
{
    const uint32_t len = tl.la + tl.lb;
    const uint32_t d = threadIdx.x * MERGE_PER_THREAD < len ? threadIdx.x * MERGE_PER_THREAD : len;
    uint32_t i = merge_split<uint32_t>(sa + 1, tl.la, sb + 1, tl.lb, d), j = d - i;
    uint32_t keep = 0, nboth = 0;
#pragma unroll
    for (uint32_t q = 0; q < MERGE_PER_THREAD; q++) {
        key[q] = 0;
        if (d + q >= len)
            continue;
        const bool take_a = i < tl.la && (j >= tl.lb || sa[1 + i] <= sb[1 + j]);
        if (take_a) {
            const u64 x = sa[1 + i];
            const bool in_b = tl.b0 + j < nb && sb[1 + j] == x;
            key[q] = x;
            keep |= ((keep_a >> (in_b ? 1u : 0u)) & 1u) << q;
            nboth += in_b ? 1u : 0u;
            i++;
        } else {
            const u64 x = sb[1 + j];
            const bool in_a = tl.a0 + i > 0 && sa[i] == x;
            key[q] = x;
            keep |= ((keep_b >> (in_a ? 1u : 0u)) & 1u) << q;
            j++;
        }
    }
    *both = nboth;
    return keep;
}

// The thread's ERR_ORDER | ERR_ZERO bits for the tile: every pair (x - 1, x) of a list belongs to the tile that holds x, and
// so does the count of x.  COUNTS false (set algebra): the count pieces are neither loaded nor tested.
template <bool COUNTS>
__device__ __forceinline__ uint32_t tile_check(const Tile &tl, const u64 *sa, const u64 *sb, const uint8_t *sca, const uint8_t *scb)
{
    uint32_t bad = tl.ok ? 0u : ERR_ORDER;
#pragma unroll
    for (uint32_t p = 0; p < 2u; p++) { // A's piece, then B's
        const u64 *sk = p ? sb : sa;
        const uint8_t *sc = p ? scb : sca;
        const uint64_t p0 = p ? tl.b0 : tl.a0;
        const uint32_t lp = p ? tl.lb : tl.la;
        for (uint32_t x = threadIdx.x; x < lp; x += 256u) {
            if (p0 + x > 0 && sk[x] >= sk[1 + x]) // (x == 0: against the halo)
                bad |= ERR_ORDER;
            if (COUNTS && !sc[1 + x])
                bad |= ERR_ZERO;
        }
    }
    return bad;
}

// sum of x over the block into every thread; sh holds 4 entries
__device__ __forceinline__ uint32_t block_sum(uint32_t x, uint32_t *sh)
{
    for (int o = 32; o > 0; o >>= 1)
        x += __shfl_xor(x, o);
    __syncthreads(); // (sh may still be read from the trip before)
    if ((threadIdx.x & 63u) == 0u)
        sh[threadIdx.x >> 6] = x;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}

// ctl[0] += |A n B| of the tile (both: the thread's share), ctl[1] |= the error bits any thread holds in bad.  A thread's
// two bits are summed over the block in one word, a count of up to 256 in each half.
__device__ __forceinline__ void tile_report(uint32_t both, uint32_t bad, uint32_t *sh, u64 *__restrict__ ctl)
{
    const uint32_t n_both = block_sum(both, sh);
    const uint32_t n_bad = block_sum((bad & ERR_ORDER) | ((bad & ERR_ZERO) << 15), sh);
    if (threadIdx.x == 0) {
        if (n_both)
            atomicAdd(&ctl[0], (u64)n_both);
        if (n_bad)
            atomicOr(&ctl[1], (u64)(((n_bad & 0xFFFFu) ? ERR_ORDER : 0u) | ((n_bad >> 16) ? ERR_ZERO : 0u)));
    }
}

// The thread's place among the kept entries of the tile, `mine` of them its own: a wave scan, then the waves before.
// *total = the kept entries of the tile, <= MERGE_TILE: a bit per position.  sh holds 4 entries; the caller's barrier at the
// end of its trip keeps the next trip's sh apart from this one's reads.
__device__ __forceinline__ uint32_t tile_place(uint32_t mine, uint32_t *sh, uint32_t *total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = mine;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(inc, o);
        if (lane >= (uint32_t)o)
            inc += y;
    }
    if (lane == 63u)
        sh[wave] = inc;
    __syncthreads();
    uint32_t at = inc - mine;
    for (uint32_t w = 0; w < wave; w++)
        at += sh[w];
    *total = sh[0] + sh[1] + sh[2] + sh[3];
    return at;
}

// pass 1 of set algebra: counts[t] = kept keys of tile t
__global__ __launch_bounds__(256) void merge_count_kernel(const u64 *__restrict__ a, uint64_t na, const u64 *__restrict__ b, uint64_t nb,
                                                          const u64 *__restrict__ split, uint64_t n_tiles, uint32_t keep_a, uint32_t keep_b,
                                                          u64 *__restrict__ counts, u64 *__restrict__ ctl)
{
    __shared__ u64 sa[MERGE_TILE + 2], sb[MERGE_TILE + 2];
    __shared__ uint32_t sh[4];
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) { // block-uniform
        const Tile tl = tile_load(a, na, b, nb, split, t, sa, sb);
        const uint32_t bad = tile_check<false>(tl, sa, sb, nullptr, nullptr);
        u64 key[MERGE_PER_THREAD];
        uint32_t both = 0;
        const uint32_t keep = tile_merge(tl, na, nb, sa, sb, keep_a, keep_b, key, &both);
        const uint32_t kept = block_sum((uint32_t)__popc(keep), sh);
        if (threadIdx.x == 0)
            counts[t] = kept;
        tile_report(both, bad, sh, ctl);
        __syncthreads(); // (the pieces are written again in the next trip)
    }
}

// offs: the scanned counts.  Runs only after pass 1 has found both lists in order.
__global__ __launch_bounds__(256) void merge_write_kernel(const u64 *__restrict__ a, uint64_t na, const u64 *__restrict__ b, uint64_t nb,
                                                          const u64 *__restrict__ split, uint64_t n_tiles, uint32_t keep_a, uint32_t keep_b,
                                                          const u64 *__restrict__ offs, u64 *__restrict__ out, uint64_t n_out)
{
    __shared__ u64 sa[MERGE_TILE + 2], sb[MERGE_TILE + 2], so[MERGE_TILE];
    __shared__ uint32_t sh[4];
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) { // block-uniform
        const Tile tl = tile_load(a, na, b, nb, split, t, sa, sb);
        u64 key[MERGE_PER_THREAD];
        uint32_t both = 0, total = 0;
        const uint32_t keep = tile_merge(tl, na, nb, sa, sb, keep_a, keep_b, key, &both);
        uint32_t at = tile_place((uint32_t)__popc(keep), sh, &total);
#pragma unroll
        for (uint32_t q = 0; q < MERGE_PER_THREAD; q++)
            if ((keep >> q) & 1u)
                so[at++] = key[q];
        __syncthreads();
        const uint64_t base = offs[t];
        for (uint32_t x = threadIdx.x; x < total; x += 256u)
            if (base + x < n_out) // (always: the counts were taken over the same keys)
                out[base + x] = so[x];
        __syncthreads(); // (the pieces, so and sh are written again in the next trip)
    }
}

// ---- count lists: the same merge with a count byte per key -------------------------------------------------------------------
// min(255, ca + cb), max, min, ca - cb (0 where cb >= ca); a count of 0 stands for "absent"
__device__ __forceinline__ uint32_t count_op(uint32_t op, uint32_t ca, uint32_t cb)
{
    if (op == (uint32_t)BRX_COUNTOP_ADD)
        return ca + cb < 255u ? ca + cb : 255u;
    if (op == (uint32_t)BRX_COUNTOP_MAX)
        return ca > cb ? ca : cb;
    if (op == (uint32_t)BRX_COUNTOP_MIN)
        return ca < cb ? ca : cb;
    return ca > cb ? ca - cb : 0u;
}

// The count pieces beside tile_load's key pieces, indexed alike: entry 1 + x = count x of the piece.  Of the halo only the
// count BEHIND B's piece is ever read (an equal pair is decided where A's key is taken); it is loaded with the rest.
__device__ __forceinline__ void tile_load_counts(const Tile &tl, const uint8_t *__restrict__ ca, uint64_t na, const uint8_t *__restrict__ cb,
                                                 uint64_t nb, uint8_t *sca, uint8_t *scb)
{
    if (tl.ok) {
        for (uint32_t x = threadIdx.x; x < tl.la + 2u; x += 256u) {
            const uint64_t i = tl.a0 + x; // global index + 1
            if (i >= 1 && i <= na)
                sca[x] = ca[i - 1];
        }
        for (uint32_t x = threadIdx.x; x < tl.lb + 2u; x += 256u) {
            const uint64_t j = tl.b0 + x;
            if (j >= 1 && j <= nb)
                scb[x] = cb[j - 1];
        }
    }
    __syncthreads();
}

// A count list's positions: key[q], byte q of *cnt the result count, keep bit q of the result (result >= min_count,
// min_count >= 1); *both = keys of A found in B.  The B key of an equal pair yields nothing.
__device__ __forceinline__ uint32_t tile_merge_counts(const Tile &tl, uint64_t na, uint64_t nb, const u64 *sa, const u64 *sb, const uint8_t *sca,
                                                      const uint8_t *scb, uint32_t op, uint32_t min_count, u64 key[MERGE_PER_THREAD], u64 *cnt,
                                                      uint32_t *both)
{
    uint32_t keep = 0;
    u64 cnts = 0;
#pragma unroll
    for (uint32_t q = 0; q < MERGE_PER_THREAD; q++)
        key[q] = 0;
    *both = tile_walk(tl, na, nb, sa, sb, [&](uint32_t q, bool from_a, uint32_t i, uint32_t j, bool paired) {
        key[q] = from_a ? sa[1 + i] : sb[1 + j];
        const uint32_t r = from_a ? count_op(op, sca[1 + i], paired ? (uint32_t)scb[1 + j] : 0u) : paired ? 0u : count_op(op, 0u, scb[1 + j]);
        keep |= (r >= min_count ? 1u : 0u) << q;
        cnts |= (u64)r << (8u * q);
    });
    *cnt = cnts;
    return keep;
}

// pass 1 of a count merge: counts[t] = kept entries of tile t
__global__ __launch_bounds__(256) void count_merge_count_kernel(const u64 *__restrict__ a, const uint8_t *__restrict__ ca, uint64_t na,
                                                                const u64 *__restrict__ b, const uint8_t *__restrict__ cb, uint64_t nb,
                                                                const u64 *__restrict__ split, uint64_t n_tiles, uint32_t op, uint32_t min_count,
                                                                u64 *__restrict__ counts, u64 *__restrict__ ctl)
{
    __shared__ u64 sa[MERGE_TILE + 2], sb[MERGE_TILE + 2];
    __shared__ uint8_t sca[MERGE_TILE + 2], scb[MERGE_TILE + 2];
    __shared__ uint32_t sh[4];
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) { // block-uniform
        const Tile tl = tile_load(a, na, b, nb, split, t, sa, sb);
        tile_load_counts(tl, ca, na, cb, nb, sca, scb);
        const uint32_t bad = tile_check<true>(tl, sa, sb, sca, scb);
        u64 key[MERGE_PER_THREAD], cnt = 0;
        uint32_t both = 0;
        const uint32_t keep = tile_merge_counts(tl, na, nb, sa, sb, sca, scb, op, min_count, key, &cnt, &both);
        const uint32_t kept = block_sum((uint32_t)__popc(keep), sh);
        if (threadIdx.x == 0)
            counts[t] = kept;
        tile_report(both, bad, sh, ctl);
        __syncthreads(); // (the pieces are written again in the next trip)
    }
}

// pass 2.  offs: the scanned counts; cout may be null (keys only); *written += what the tile stored.  Runs only after pass 1
// has found both lists in order and free of 0 counts.
__global__ __launch_bounds__(256) void count_merge_write_kernel(const u64 *__restrict__ a, const uint8_t *__restrict__ ca, uint64_t na,
                                                                const u64 *__restrict__ b, const uint8_t *__restrict__ cb, uint64_t nb,
                                                                const u64 *__restrict__ split, uint64_t n_tiles, uint32_t op, uint32_t min_count,
                                                                const u64 *__restrict__ offs, u64 *__restrict__ kout, uint8_t *__restrict__ cout,
                                                                uint64_t n_out, u64 *__restrict__ written)
{
    __shared__ u64 sa[MERGE_TILE + 2], sb[MERGE_TILE + 2], so[MERGE_TILE];
    __shared__ uint8_t sca[MERGE_TILE + 2], scb[MERGE_TILE + 2], sco[MERGE_TILE];
    __shared__ uint32_t sh[4];
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) { // block-uniform
        const Tile tl = tile_load(a, na, b, nb, split, t, sa, sb);
        tile_load_counts(tl, ca, na, cb, nb, sca, scb);
        u64 key[MERGE_PER_THREAD], cnt = 0;
        uint32_t both = 0, total = 0;
        const uint32_t keep = tile_merge_counts(tl, na, nb, sa, sb, sca, scb, op, min_count, key, &cnt, &both);
        uint32_t at = tile_place((uint32_t)__popc(keep), sh, &total);
#pragma unroll
        for (uint32_t q = 0; q < MERGE_PER_THREAD; q++)
            if ((keep >> q) & 1u) {
                so[at] = key[q];
                sco[at] = (uint8_t)(cnt >> (8u * q));
                at++;
            }
        __syncthreads();
        const uint64_t base = offs[t];
        const uint32_t fits = base >= n_out ? 0u : n_out - base < total ? (uint32_t)(n_out - base) : total; // (total: the counts were taken over the same entries)
        for (uint32_t x = threadIdx.x; x < fits; x += 256u)
            kout[base + x] = so[x];
        if (cout)
            for (uint32_t x = threadIdx.x; x < fits; x += 256u)
                cout[base + x] = sco[x];
        if (threadIdx.x == 0 && fits)
            atomicAdd(written, (u64)fits);
        __syncthreads(); // (the pieces, so, sco and sh are written again in the next trip)
    }
}

// ---- the joint spectrum of two lists: J[ca][cb] = keys of A u B with those two count bytes ------------------------------------
constexpr uint32_t JOINT_CORNER = 64;               // (br_amd/countops.py JOINT_CORNER) bins ca, cb < this live in LDS
constexpr uint32_t JOINT_NONE = 0xFFFFFFFFu;          // a position that yields no pair
// a u32 bin takes at most MERGE_TILE per tile: 2^21 tiles could add up to exactly 2^32, one tile fewer cannot
constexpr uint32_t JOINT_FLUSH_TILES = (1u << 21) - 1u;

// The joint's positions: pair[q] = ca << 8 | cb of the key at position q, JOINT_NONE for B's key of an equal pair (decided
// at A's key) and behind the tile's end; *both = keys of A found in B.
__device__ __forceinline__ void tile_merge_pairs(const Tile &tl, uint64_t na, uint64_t nb, const u64 *sa, const u64 *sb, const uint8_t *sca,
                                                 const uint8_t *scb, uint32_t pair[MERGE_PER_THREAD], uint32_t *both)
{
#pragma unroll
    for (uint32_t q = 0; q < MERGE_PER_THREAD; q++)
        pair[q] = JOINT_NONE;
    *both = tile_walk(tl, na, nb, sa, sb, [&](uint32_t q, bool from_a, uint32_t i, uint32_t j, bool paired) {
        if (from_a)
            pair[q] = ((uint32_t)sca[1 + i] << 8) | (paired ? (uint32_t)scb[1 + j] : 0u);
        else if (!paired)
            pair[q] = (uint32_t)scb[1 + j];
    });
}

// corner[ca * JOINT_CORNER + cb] -> joint[ca * 256 + cb], one global add per non-zero bin; the corner is left cleared
__device__ __forceinline__ void joint_flush(uint32_t *corner, u64 *__restrict__ joint)
{
    __syncthreads();
    for (uint32_t x = threadIdx.x; x < JOINT_CORNER * JOINT_CORNER; x += 256u) {
        const uint32_t v = corner[x];
        if (v) {
            atomicAdd(&joint[((x / JOINT_CORNER) << 8) | (x % JOINT_CORNER)], (u64)v);
            corner[x] = 0u;
        }
    }
    __syncthreads();
}

// One pass over the tiles: pass 1's checks and |A n B| (ctl as there), and every pair binned -- the corner in LDS, flushed
// after the block's last tile and before a u32 bin could wrap, the pairs outside it straight to the global table.
// A thread folds the equal pairs among its own positions into (pair, n) and adds each once.  Summing equal pairs across the
// wave first (two leader rounds per position: ballots, one lane adds) was measured and lost, 9.6 against 8.2 ms per Gbp on the
// bench's lists and on lists of nothing but 1s alike: same-address LDS adds are not what this pass waits for.
__global__ __launch_bounds__(256) void count_joint_kernel(const u64 *__restrict__ a, const uint8_t *__restrict__ ca, uint64_t na,
                                                          const u64 *__restrict__ b, const uint8_t *__restrict__ cb, uint64_t nb,
                                                          const u64 *__restrict__ split, uint64_t n_tiles, u64 *__restrict__ joint,
                                                          u64 *__restrict__ ctl)
{
    __shared__ u64 sa[MERGE_TILE + 2], sb[MERGE_TILE + 2];
    __shared__ uint8_t sca[MERGE_TILE + 2], scb[MERGE_TILE + 2];
    __shared__ uint32_t corner[JOINT_CORNER * JOINT_CORNER];
    __shared__ uint32_t sh[4];
    for (uint32_t x = threadIdx.x; x < JOINT_CORNER * JOINT_CORNER; x += 256u)
        corner[x] = 0u;
    uint32_t unflushed = 0; // tiles binned since the last flush (block-uniform)
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) { // block-uniform
        const Tile tl = tile_load(a, na, b, nb, split, t, sa, sb); // (its barrier also orders the clearing of the corner)
        tile_load_counts(tl, ca, na, cb, nb, sca, scb);
        const uint32_t bad = tile_check<true>(tl, sa, sb, sca, scb);
        uint32_t pair[MERGE_PER_THREAD], n[MERGE_PER_THREAD], both = 0;
        tile_merge_pairs(tl, na, nb, sa, sb, sca, scb, pair, &both);
#pragma unroll
        for (uint32_t q = 0; q < MERGE_PER_THREAD; q++)
            n[q] = 1u;
#pragma unroll
        for (uint32_t q = 0; q < MERGE_PER_THREAD; q++)
#pragma unroll
            for (uint32_t r = q + 1; r < MERGE_PER_THREAD; r++)
                if (pair[q] != JOINT_NONE && pair[r] == pair[q]) {
                    n[q] += n[r]; // (n[r] is still 1: a pair folded into an earlier one is JOINT_NONE by now)
                    pair[r] = JOINT_NONE;
                }
#pragma unroll
        for (uint32_t q = 0; q < MERGE_PER_THREAD; q++)
            if (pair[q] != JOINT_NONE) {
                const uint32_t pa = pair[q] >> 8, pb = pair[q] & 255u;
                if (pa < JOINT_CORNER && pb < JOINT_CORNER)
                    atomicAdd(&corner[pa * JOINT_CORNER + pb], n[q]); // (the result is not used: an LDS add that returns nothing)
                else
                    atomicAdd(&joint[pair[q]], (u64)n[q]);
            }
        tile_report(both, bad, sh, ctl);
        __syncthreads(); // (the pieces are written again in the next trip)
        if (++unflushed == JOINT_FLUSH_TILES) {
            joint_flush(corner, joint);
            unflushed = 0;
        }
    }
    if (unflushed)
        joint_flush(corner, joint);
}

// The spectrum of a list: hist[v] += count bytes equal to v.  Bins per wave in LDS, flushed once per block.
__global__ __launch_bounds__(256) void count_hist_kernel(const uint8_t *__restrict__ cnts, uint64_t n, u64 *__restrict__ hist)
{
    __shared__ u64 bins[4][256];
    const uint32_t wave = threadIdx.x >> 6;
    for (uint32_t w = 0; w < 4u; w++)
        bins[w][threadIdx.x] = 0ull;
    __syncthreads();
    // the bytes before the first 16-byte border one by one, then 16 per load, then the rest
    const uint64_t head = ((16u - (uint32_t)((uintptr_t)cnts & 15u)) & 15u) < n ? ((16u - (uint32_t)((uintptr_t)cnts & 15u)) & 15u) : n;
    const uint64_t n_vec = (n - head) / 16u, tail = head + n_vec * 16u;
    const uint64_t gtid = (uint64_t)blockIdx.x * 256u + threadIdx.x, stride = (uint64_t)gridDim.x * 256u;
    if (gtid < head)
        atomicAdd(&bins[wave][cnts[gtid]], 1ull);
    if (gtid < n - tail)
        atomicAdd(&bins[wave][cnts[tail + gtid]], 1ull);
    const uint4 *vec = reinterpret_cast<const uint4 *>(cnts + head);
    for (uint64_t i = gtid; i < n_vec; i += stride) {
        const uint4 v = vec[i];
        const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t q = 0; q < 16u; q++)
            atomicAdd(&bins[wave][(w4[q >> 2] >> (8u * (q & 3u))) & 255u], 1ull);
    }
    __syncthreads();
    const u64 sum = bins[0][threadIdx.x] + bins[1][threadIdx.x] + bins[2][threadIdx.x] + bins[3][threadIdx.x];
    if (sum)
        atomicAdd(&hist[threadIdx.x], sum);
}

// ---- host side ------------------------------------------------------------------------------------------------------------
// The two lists of one merge and what pass 1 found; the scratch lives until the plan goes.
struct MergePlan {
    MergePlan(const uint64_t *ka, const uint8_t *ca, uint64_t na_, const uint64_t *kb, const uint8_t *cb, uint64_t nb_)
        : d_a((const u64 *)ka), d_b((const u64 *)kb), d_ca(ca), d_cb(cb), na(na_), nb(nb_)
    {
    }
    DevScratch ws;
    const u64 *d_a, *d_b;
    const uint8_t *d_ca, *d_cb; // the count bytes of count lists; null for set algebra
    uint64_t na, nb, n_tiles = 0, total = 0, both = 0;
    uint32_t op = 0, min_count = 1;
    u64 *d_split = nullptr, *d_counts = nullptr, *d_ctl = nullptr; // ctl: [0] |A n B|, [1] error bits, [2] entries pass 2 wrote
    uint32_t grid() const { return read_grid(n_tiles, 256u * 16u); }
};

// the refusal of lists that are not there or too long; `counted`: count lists, the count bytes must be there too
int lists_given(const char *me, const MergePlan &plan, bool counted)
{
    const uint64_t na = plan.na, nb = plan.nb;
    if ((!plan.d_a && na) || (!plan.d_b && nb) || (counted && ((!plan.d_ca && na) || (!plan.d_cb && nb))) || na > (1ull << 62) ||
        nb > (1ull << 62)) {
        set_error("%s: %s", me, counted ? "null keys or counts, or more than 2^62 entries" : "null keys, or more than 2^62 of them");
        return BRX_ERR_ARG;
    }
    return BRX_OK;
}

// Pass 1 over the plan's lists, `counted` telling whether they are count lists: the split and launch(), the caller's
// kernel that checks every tile and reports into plan->d_ctl (and, with `scan`, leaves its tile counts in plan->d_counts,
// which the scan turns into offsets), under the timer `timer`.  *plan: n_tiles, |A n B| and, with `scan`, the size of the
// result.  BRX_ERR_ARG when a list does not ascend strictly or holds a 0 count; `what` names the pass in a HIP failure.
// Returns after `s` has been synchronised, or at once where both lists are empty.
template <typename Launch>
int merge_pass1(const char *me, const char *what, const char *timer, bool counted, bool scan, hipStream_t s, MergePlan *plan, Launch launch)
{
    BRX_TRY(lists_given(me, *plan, counted));
    const uint64_t na = plan->na, nb = plan->nb;
    const uint64_t n_tiles = (na + nb + MERGE_TILE - 1) / MERGE_TILE;
    plan->n_tiles = n_tiles;
    if (!n_tiles)
        return BRX_OK;
    const uint64_t n_sums = scan ? keys_scan_sums(n_tiles) : 0;
    u64 *d_sums = nullptr;
    BRX_TRY(plan->ws.get(&plan->d_split, n_tiles + 1));
    if (scan) {
        BRX_TRY(plan->ws.get(&plan->d_counts, n_tiles));
        BRX_TRY(plan->ws.get(&d_sums, n_sums + 1));
    }
    BRX_TRY(plan->ws.get(&plan->d_ctl, 3));
    BRX_HIP(hipMemsetAsync(plan->d_ctl, 0, 24, s));
    u64 ctl[2] = {0, 0}, total = 0;
    int st = BRX_OK;
    hipError_t e = hipSuccess;
    {
        KernelTimer kt(timer, s);
        merge_split_kernel<<<read_grid((n_tiles + 256) / 256, 256u * 16u), 256, 0, s>>>(plan->d_a, na, plan->d_b, nb, n_tiles, plan->d_split);
        launch();
        if ((e = hipGetLastError()) == hipSuccess && scan)
            st = keys_scan_exclusive(plan->d_counts, n_tiles, d_sums, s);
    }
    if (st == BRX_OK && e == hipSuccess && (e = hipMemcpyAsync(ctl, plan->d_ctl, 16, hipMemcpyDeviceToHost, s)) == hipSuccess && scan)
        e = hipMemcpyAsync(&total, d_sums + n_sums, 8, hipMemcpyDeviceToHost, s);
    const hipError_t e2 = hipStreamSynchronize(s); // the scratch may go back to the pool when the caller drops the plan
    if (st != BRX_OK)
        return st;
    if (e != hipSuccess || e2 != hipSuccess) {
        set_error("%s: %s: %s", me, what, hipGetErrorString(e != hipSuccess ? e : e2));
        return BRX_ERR_HIP;
    }
    if (ctl[1] & ERR_ORDER) {
        set_error("%s: the keys of an input do not ascend strictly (unordered or repeated keys)", me);
        return BRX_ERR_ARG;
    }
    if (ctl[1] & ERR_ZERO) {
        set_error("%s: a count of 0 in an input (a listed k-mer was seen at least once)", me);
        return BRX_ERR_ARG;
    }
    plan->total = total;
    plan->both = ctl[0];
    return BRX_OK;
}

// Pass 1 of set algebra.  *plan: the size of the result and |A n B|.
int merge_count(const char *me, int op, hipStream_t s, MergePlan *plan)
{
    if (op < 0 || op > 3) {
        set_error("%s: op=%d (BRX_SETOP_UNION 0, INTERSECT 1, DIFFERENCE 2, SYMDIFF 3)", me, op);
        return BRX_ERR_ARG;
    }
    plan->op = (uint32_t)op;
    BRX_TRY(merge_pass1(me, "merge, pass 1", "set_merge", false, true, s, plan, [&] {
        merge_count_kernel<<<plan->grid(), 256, 0, s>>>(plan->d_a, plan->na, plan->d_b, plan->nb, plan->d_split, plan->n_tiles, KEEP_A[op],
                                                       KEEP_B[op], plan->d_counts, plan->d_ctl);
    }));
    // the four sizes follow from |A|, |B| and |A n B|: what the scan found must agree
    const uint64_t na = plan->na, nb = plan->nb, both = plan->both;
    uint64_t want = both; // intersection
    if (op == BRX_SETOP_UNION)
        want = na + nb - both;
    else if (op == BRX_SETOP_DIFFERENCE)
        want = na - both;
    else if (op == BRX_SETOP_SYMDIFF)
        want = na + nb - 2 * both;
    if (both > na || both > nb || plan->total != want) {
        set_error("%s: merge, pass 1: %llu keys kept, |A|=%llu |B|=%llu |A n B|=%llu", me, (u64)plan->total, (u64)na, (u64)nb, (u64)both);
        return BRX_ERR_HIP;
    }
    return BRX_OK;
}

// pass 2 into d_out (plan->total entries); returns after `s` has been synchronised
int merge_write(const char *me, const MergePlan &plan, uint64_t *d_out, hipStream_t s)
{
    if (!plan.total)
        return BRX_OK;
    {
        KernelTimer kt("set_merge", s);
        merge_write_kernel<<<plan.grid(), 256, 0, s>>>(plan.d_a, plan.na, plan.d_b, plan.nb, plan.d_split, plan.n_tiles, KEEP_A[plan.op],
                                                      KEEP_B[plan.op], plan.d_counts, (u64 *)d_out, plan.total);
    }
    const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(s);
    if (e1 != hipSuccess || e2 != hipSuccess) {
        set_error("%s: merge, pass 2: %s", me, hipGetErrorString(e1 != hipSuccess ? e1 : e2));
        return BRX_ERR_HIP;
    }
    return BRX_OK;
}

bool overlap_bytes(const void *p, uint64_t pbytes, const void *q, uint64_t qbytes)
{
    const uintptr_t p0 = (uintptr_t)p, q0 = (uintptr_t)q;
    return p && q && pbytes && qbytes && p0 < q0 + qbytes && q0 < p0 + pbytes;
}

// ---- count lists ------------------------------------------------------------------------------------------------------------
const char *const COUNTOP_NAMES = "BRX_COUNTOP_ADD 0, MAX 1, MIN 2, SUB 3";

// Pass 1 of a count merge, min_count 1 .. 256.  *plan: the size of the result and |A n B|.
int count_merge_count(const char *me, int op, uint32_t min_count, hipStream_t s, MergePlan *plan)
{
    if (op < 0 || op > 3) {
        set_error("%s: op=%d (%s)", me, op, COUNTOP_NAMES);
        return BRX_ERR_ARG;
    }
    BRX_TRY(lists_given(me, *plan, true)); // (pass 1 would say it too: here so that it is said before min_count's range)
    if (min_count < 1u || min_count > 256u) {
        set_error("%s: min_count=%u (1 to 256)", me, min_count);
        return BRX_ERR_ARG;
    }
    plan->op = (uint32_t)op;
    plan->min_count = min_count;
    BRX_TRY(merge_pass1(me, "count merge, pass 1", "count_merge", true, true, s, plan, [&] {
        count_merge_count_kernel<<<plan->grid(), 256, 0, s>>>(plan->d_a, plan->d_ca, plan->na, plan->d_b, plan->d_cb, plan->nb, plan->d_split,
                                                             plan->n_tiles, plan->op, min_count, plan->d_counts, plan->d_ctl);
    }));
    // (what is kept depends on the counts: no size follows from |A|, |B| and |A n B| but the bounds)
    if (plan->both > plan->na || plan->both > plan->nb || plan->total > plan->na + plan->nb - plan->both) {
        set_error("%s: count merge, pass 1: %llu entries kept, |A|=%llu |B|=%llu |A n B|=%llu", me, (u64)plan->total, (u64)plan->na,
                  (u64)plan->nb, (u64)plan->both);
        return BRX_ERR_HIP;
    }
    return BRX_OK;
}

// pass 2 into d_kout and d_cout (may be null), plan->total entries each; returns after `s` has been synchronised
int count_merge_write(const char *me, const MergePlan &plan, uint64_t *d_kout, uint8_t *d_cout, hipStream_t s)
{
    if (!plan.total)
        return BRX_OK;
    u64 written = 0;
    hipError_t e1 = hipSuccess;
    {
        KernelTimer kt("count_merge", s);
        count_merge_write_kernel<<<plan.grid(), 256, 0, s>>>(plan.d_a, plan.d_ca, plan.na, plan.d_b, plan.d_cb, plan.nb, plan.d_split,
                                                            plan.n_tiles, plan.op, plan.min_count, plan.d_counts, (u64 *)d_kout, d_cout,
                                                            plan.total, plan.d_ctl + 2);
        e1 = hipGetLastError();
    }
    if (e1 == hipSuccess)
        e1 = hipMemcpyAsync(&written, plan.d_ctl + 2, 8, hipMemcpyDeviceToHost, s);
    const hipError_t e2 = hipStreamSynchronize(s);
    if (e1 != hipSuccess || e2 != hipSuccess) {
        set_error("%s: count merge, pass 2: %s", me, hipGetErrorString(e1 != hipSuccess ? e1 : e2));
        return BRX_ERR_HIP;
    }
    if (written != plan.total) {
        set_error("%s: count merge, pass 2 wrote %llu entries, the scan found %llu", me, written, (u64)plan.total);
        return BRX_ERR_HIP;
    }
    return BRX_OK;
}

// The joint spectrum of two lists, J[0][0] = 0, accumulated in scratch and copied whole -- to d_out (device) or h_out (host),
// whichever is given -- only when both lists passed pass 1's checks: a refusal leaves them untouched.  *both = |A n B|.
// Returns after `s` has been synchronised.
int count_joint(const char *me, const uint64_t *d_ka, const uint8_t *d_ca, uint64_t na, const uint64_t *d_kb, const uint8_t *d_cb,
                uint64_t nb, hipStream_t s, uint64_t *d_out, uint64_t *h_out, uint64_t *both)
{
    constexpr uint64_t BINS = 65536, BYTES = BINS * sizeof(u64);
    MergePlan plan(d_ka, d_ca, na, d_kb, d_cb, nb);
    BRX_TRY(lists_given(me, plan, true)); // (before the table is got and cleared: a refusal queues nothing)
    *both = 0;
    u64 *d_joint = nullptr;
    BRX_TRY(plan.ws.get(&d_joint, BINS));
    BRX_HIP(hipMemsetAsync(d_joint, 0, BYTES, s));
    BRX_TRY(merge_pass1(me, "joint spectrum", "count_joint", true, false, s, &plan, [&] {
        count_joint_kernel<<<plan.grid(), 256, 0, s>>>(plan.d_a, d_ca, na, plan.d_b, d_cb, nb, plan.d_split, plan.n_tiles, d_joint, plan.d_ctl);
    }));
    if (plan.both > na || plan.both > nb) {
        set_error("%s: joint spectrum: |A|=%llu |B|=%llu |A n B|=%llu", me, (u64)na, (u64)nb, (u64)plan.both);
        return BRX_ERR_HIP;
    }
    hipError_t e = hipSuccess;
    {
        KernelTimer kt("count_joint", s);
        e = d_out ? hipMemcpyAsync(d_out, d_joint, BYTES, hipMemcpyDeviceToDevice, s) : hipMemcpyAsync(h_out, d_joint, BYTES, hipMemcpyDeviceToHost, s);
    }
    const hipError_t e2 = hipStreamSynchronize(s); // the scratch goes back to the pool on return
    if (e != hipSuccess || e2 != hipSuccess) {
        set_error("%s: joint spectrum, copying out: %s", me, hipGetErrorString(e != hipSuccess ? e : e2));
        return BRX_ERR_HIP;
    }
    *both = plan.both;
    return BRX_OK;
}

// The floor of `a op b` before min_count (include/brx.h "count lists", countops.result_floor): 0 = refused, message set
uint32_t result_floor(const char *me, int op, uint32_t fa, uint32_t fb)
{
    if (op == BRX_COUNTOP_MAX || op == BRX_COUNTOP_MIN)
        return fa > fb ? fa : fb;
    if (op == BRX_COUNTOP_SUB) {
        if (fb != 1u) {
            set_error("%s: subtracting a list that kept only counts from %u up: the k-mers it no longer knows would be subtracted as 0", me,
                      fb);
            return 0u;
        }
        return fa;
    }
    if (fa != 1u || fb != 1u) {
        set_error("%s: adding lists that kept only counts from %u and from %u up: two unknown parts could add up to a count that must be "
                  "present (both floors must be 1)", me, fa, fb);
        return 0u;
    }
    return 1u;
}

int operands_ok(const char *me, const brx_set *a, const brx_set *b)
{
    if (!a || !b) {
        set_error("%s: null set", me);
        return BRX_ERR_ARG;
    }
    if (a->k != b->k || a->device != b->device) {
        set_error("%s: the operands differ: a has k = %d on device %d, b has k = %d on device %d", me, a->k, a->device, b->k, b->device);
        return BRX_ERR_ARG;
    }
    if (!(a->k & 1) || a->k < 5 || a->k > 31) {
        set_error("%s: set algebra works on the keys of odd k from 5 to 31 (k=%d)", me, a->k);
        return BRX_ERR_UNSUPPORTED;
    }
    return BRX_OK;
}

// the sorted keys of both operands (one list when they are one set)
struct Operands {
    DevBuf<uint64_t> keys_a, keys_b;
    const uint64_t *d_a = nullptr, *d_b = nullptr;
    uint64_t na = 0, nb = 0;
};

int operands_list(const brx_set *a, const brx_set *b, hipStream_t s, Operands *o)
{
    // (a key list that came from a key file or from set algebra says that it is in order: no sort.  Pass 1 checks the
    // order of whatever it is given, so a wrong flag would be refused, not merged.)
    const uint32_t key_bits = (uint32_t)(2 * a->k - 1);
    bool sorted = false;
    BRX_TRY(set_list_keys(a, s, o->keys_a, &o->na, &sorted));
    if (!sorted)
        BRX_TRY(keys_sort(o->keys_a, nullptr, o->na, key_bits, s));
    o->d_a = o->keys_a;
    if (a == b) {
        o->d_b = o->d_a;
        o->nb = o->na;
        return BRX_OK;
    }
    BRX_TRY(set_list_keys(b, s, o->keys_b, &o->nb, &sorted));
    if (!sorted)
        BRX_TRY(keys_sort(o->keys_b, nullptr, o->nb, key_bits, s));
    o->d_b = o->keys_b;
    return BRX_OK;
}

// two count lists of one k on one device
int lists_ok(const char *me, const brx_counts *a, const brx_counts *b)
{
    BRX_TRY(list_ok(me, a));
    BRX_TRY(list_ok(me, b));
    if (a->k != b->k || a->device != b->device) {
        set_error("%s: the operands differ: a has k = %d on device %d, b has k = %d on device %d", me, a->k, a->device, b->k, b->device);
        return BRX_ERR_ARG;
    }
    return BRX_OK;
}

// *out: a new set of this k on this device, the closed set of the n sorted keys of d_keys (set_build_from_keys takes them
// over); on failure nothing is left behind.  Returns after `s` has been synchronised.
int set_from_keys(const char *me, int k, int device, DevBuf<uint64_t> &d_keys, uint64_t n, hipStream_t s, brx_set **out)
{
    brx_set *set = nullptr;
    int st = set_alloc_unwritten(k, device, &set);
    if (st == BRX_OK)
        st = set_build_from_keys(set, d_keys, n, s, me);
    const hipError_t e = hipStreamSynchronize(s);
    if (st == BRX_OK && e != hipSuccess) {
        set_error("%s: building the set: %s", me, hipGetErrorString(e));
        st = BRX_ERR_HIP;
    }
    if (st != BRX_OK) {
        if (set)
            brx_set_free(set);
        return st;
    }
    *out = set;
    return BRX_OK;
}

} // namespace

namespace brx {

int counts_merge(const char *me, const uint64_t *d_ka, const uint8_t *d_ca, uint64_t na, const uint64_t *d_kb, const uint8_t *d_cb,
                 uint64_t nb, int op, uint32_t min_count, bool want_counts, hipStream_t s, DevBuf<uint64_t> &d_kout,
                 DevBuf<uint8_t> &d_cout, uint64_t *n_out, uint64_t *both)
{
    d_kout.reset();
    d_cout.reset();
    *n_out = 0;
    MergePlan plan(d_ka, d_ca, na, d_kb, d_cb, nb);
    BRX_TRY(count_merge_count(me, op, min_count, s, &plan));
    if (both)
        *both = plan.both;
    if (!plan.total)
        return BRX_OK;
    BRX_TRY(d_kout.reserve(plan.total, 0, "keys of a count list"));
    if (want_counts)
        BRX_TRY(d_cout.reserve(plan.total, 0, "counts of a count list"));
    const int st = count_merge_write(me, plan, d_kout, want_counts ? d_cout.get() : nullptr, s);
    if (st != BRX_OK) {
        d_kout.reset();
        d_cout.reset();
        return st;
    }
    *n_out = plan.total;
    return BRX_OK;
}

} // namespace brx

extern "C" {

int brx_counts_combine_device(const uint64_t *d_ka, const uint8_t *d_ca, uint64_t na, const uint64_t *d_kb, const uint8_t *d_cb,
                              uint64_t nb, int op, uint8_t min_count, uint64_t *d_kout, uint8_t *d_cout, uint64_t cap, uint64_t *n_out,
                              uint64_t *sizes3, void *stream)
{
    const char *me = "brx_counts_combine_device";
    if (!n_out || (!d_kout && (cap || d_cout))) {
        set_error("%s: null n_out, or a capacity or a count array without a key array", me);
        return BRX_ERR_ARG;
    }
    *n_out = 0;
    if (overlap_bytes(d_kout, cap * 8, d_ka, na * 8) || overlap_bytes(d_kout, cap * 8, d_kb, nb * 8) || overlap_bytes(d_cout, cap, d_ca, na) ||
        overlap_bytes(d_cout, cap, d_cb, nb)) {
        set_error("%s: an output array overlaps an input", me);
        return BRX_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    MergePlan plan(d_ka, d_ca, na, d_kb, d_cb, nb);
    BRX_TRY(count_merge_count(me, op, min_count ? min_count : 1u, s, &plan));
    *n_out = plan.total;
    if (sizes3) {
        sizes3[0] = na;
        sizes3[1] = nb;
        sizes3[2] = plan.both;
    }
    if (!d_kout && !cap)
        return BRX_OK; // the sizes only
    if (cap < plan.total) {
        set_error("%s: the result holds %llu entries, the output arrays %llu", me, (u64)plan.total, (u64)cap);
        return BRX_ERR_ARG;
    }
    return count_merge_write(me, plan, d_kout, d_cout, s);
}

int brx_counts_joint_device(const uint64_t *d_ka, const uint8_t *d_ca, uint64_t na, const uint64_t *d_kb, const uint8_t *d_cb,
                            uint64_t nb, uint64_t *d_joint, uint64_t *sizes3, void *stream)
{
    const char *me = "brx_counts_joint_device";
    if (!d_joint) {
        set_error("%s: null d_joint", me);
        return BRX_ERR_ARG;
    }
    const uint64_t bytes = 65536 * sizeof(uint64_t);
    if (overlap_bytes(d_joint, bytes, d_ka, na * 8) || overlap_bytes(d_joint, bytes, d_kb, nb * 8) || overlap_bytes(d_joint, bytes, d_ca, na) ||
        overlap_bytes(d_joint, bytes, d_cb, nb)) {
        set_error("%s: d_joint overlaps an input", me);
        return BRX_ERR_ARG;
    }
    uint64_t both = 0;
    BRX_TRY(count_joint(me, d_ka, d_ca, na, d_kb, d_cb, nb, (hipStream_t)stream, d_joint, nullptr, &both));
    if (sizes3) {
        sizes3[0] = na;
        sizes3[1] = nb;
        sizes3[2] = both;
    }
    return BRX_OK;
}

int brx_counts_compare(const brx_counts_t *a, const brx_counts_t *b, uint64_t *joint65536, uint64_t *stats8)
{
    const char *me = "brx_counts_compare";
    BRX_TRY(lists_ok(me, a, b));
    if (!joint65536) {
        set_error("%s: null joint65536", me);
        return BRX_ERR_ARG;
    }
    auto t0 = Clock::now();
    BRX_TRY(use_device(a->device));
    OwnStream own;
    BRX_HIP(hipStreamCreateWithFlags(&own.s, hipStreamNonBlocking));
    std::vector<uint64_t> joint(65536);
    uint64_t both = 0;
    BRX_TRY(count_joint(me, a->d_keys, a->d_cnts, a->n, b->d_keys, b->d_cnts, b->n, own.s, nullptr, joint.data(), &both));
    // every key of A u B fell in exactly one bin, none in [0][0]
    const uint64_t either = a->n + b->n - both;
    uint64_t binned = 0;
    for (uint64_t v : joint)
        binned += v;
    if (joint[0] || binned != either || either > set_nbits(a->k)) {
        set_error("%s: the joint spectrum holds %llu keys and %llu in bin [0][0], |A|=%llu |B|=%llu |A n B|=%llu at k=%d", me, (u64)binned,
                  (u64)joint[0], (u64)a->n, (u64)b->n, (u64)both, a->k);
        return BRX_ERR_HIP;
    }
    joint[0] = set_nbits(a->k) - either;
    memcpy(joint65536, joint.data(), 65536 * sizeof(uint64_t));
    if (stats8) {
        const uint64_t ns = ns_since(t0);
        const uint64_t st8[8] = {a->n, b->n, both, either, 0, ns, 0, ns};
        memcpy(stats8, st8, sizeof st8);
    }
    return BRX_OK;
}

int brx_counts_info(const brx_counts_t *l, uint64_t *info4)
{
    const char *me = "brx_counts_info";
    BRX_TRY(list_ok(me, l));
    if (!info4) {
        set_error("%s: null info4", me);
        return BRX_ERR_ARG;
    }
    info4[0] = (uint64_t)l->k;
    info4[1] = l->n;
    info4[2] = l->floor;
    info4[3] = (uint64_t)l->device;
    return BRX_OK;
}

int brx_counts_device(const brx_counts_t *l, void **d_keys, void **d_counts, uint64_t *n)
{
    const char *me = "brx_counts_device";
    BRX_TRY(list_ok(me, l));
    if (!d_keys || !d_counts || !n) {
        set_error("%s: null output", me);
        return BRX_ERR_ARG;
    }
    *d_keys = l->n ? (void *)l->d_keys.get() : nullptr;
    *d_counts = l->n ? (void *)l->d_cnts.get() : nullptr;
    *n = l->n;
    return BRX_OK;
}

void brx_counts_free(brx_counts_t *l) { delete l; }

int brx_counts_combine(const brx_counts_t *a, const brx_counts_t *b, int op, uint8_t min_count, brx_counts_t **out, uint64_t *stats8)
{
    const char *me = "brx_counts_combine";
    if (!out) {
        set_error("%s: null out", me);
        return BRX_ERR_ARG;
    }
    *out = nullptr;
    BRX_TRY(lists_ok(me, a, b));
    if (op < 0 || op > 3) {
        set_error("%s: op=%d (%s)", me, op, COUNTOP_NAMES);
        return BRX_ERR_ARG;
    }
    uint32_t floor = result_floor(me, op, a->floor, b->floor);
    if (!floor)
        return BRX_ERR_ARG;
    if (min_count > floor)
        floor = min_count;
    uint64_t st8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto t0 = Clock::now();
    BRX_TRY(use_device(a->device));
    OwnStream own;
    BRX_HIP(hipStreamCreateWithFlags(&own.s, hipStreamNonBlocking));
    brx_counts *res = new brx_counts;
    res->k = a->k;
    res->device = a->device;
    res->floor = (uint8_t)floor;
    const int st = counts_merge(me, a->d_keys, a->d_cnts, a->n, b->d_keys, b->d_cnts, b->n, op, floor, true, own.s, res->d_keys, res->d_cnts,
                                &res->n, &st8[2]);
    if (st == BRX_OK && res->n > set_nbits(a->k)) {
        set_error("%s: %llu entries in the result, only %llu k-mers exist at k=%d", me, (u64)res->n, (u64)set_nbits(a->k), a->k);
        delete res;
        return BRX_ERR_HIP;
    }
    if (st != BRX_OK) {
        delete res;
        return st;
    }
    st8[0] = a->n;
    st8[1] = b->n;
    st8[3] = res->n;
    st8[5] = st8[7] = ns_since(t0);
    *out = res;
    if (stats8)
        memcpy(stats8, st8, sizeof st8);
    return BRX_OK;
}

int brx_counts_spectrum(const brx_counts_t *l, uint64_t *hist256)
{
    const char *me = "brx_counts_spectrum";
    BRX_TRY(list_ok(me, l));
    if (!hist256) {
        set_error("%s: null hist256", me);
        return BRX_ERR_ARG;
    }
    memset(hist256, 0, 256 * sizeof(uint64_t));
    if (l->n) {
        BRX_TRY(use_device(l->device));
        OwnStream own;
        BRX_HIP(hipStreamCreateWithFlags(&own.s, hipStreamNonBlocking));
        DevScratch ws;
        u64 *d_hist = nullptr;
        BRX_TRY(ws.get(&d_hist, 256));
        BRX_HIP(hipMemsetAsync(d_hist, 0, 256 * 8, own.s));
        {
            KernelTimer kt("count_hist", own.s);
            count_hist_kernel<<<read_grid((l->n + 256ull * 64ull - 1) / (256ull * 64ull), 256u * 16u), 256, 0, own.s>>>(l->d_cnts, l->n, d_hist);
            BRX_HIP(hipGetLastError());
        }
        BRX_HIP(hipMemcpyAsync(hist256, d_hist, 256 * 8, hipMemcpyDeviceToHost, own.s));
        BRX_HIP(hipStreamSynchronize(own.s));
    }
    uint64_t seen = 0;
    for (int v = 1; v < 256; v++)
        seen += hist256[v];
    if (hist256[0] || seen != l->n) {
        set_error("%s: the histogram holds %llu entries and %llu counts of 0, the list %llu entries", me, (u64)seen, (u64)hist256[0], (u64)l->n);
        return BRX_ERR_HIP;
    }
    hist256[0] = set_nbits(l->k) - l->n;
    return BRX_OK;
}

int brx_counts_finish(const brx_counts_t *l, uint8_t abundance, brx_set_t **out, uint64_t *stats8)
{
    const char *me = "brx_counts_finish";
    if (!out) {
        set_error("%s: null out", me);
        return BRX_ERR_ARG;
    }
    *out = nullptr;
    BRX_TRY(list_ok(me, l));
    if ((uint32_t)abundance + 1u < l->floor) {
        set_error("%s: the list kept only counts from %d up: a threshold below %d would miss members (abundance=%d)", me, (int)l->floor,
                  (int)l->floor - 1, (int)abundance);
        return BRX_ERR_ARG;
    }
    uint64_t st8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto t0 = Clock::now();
    BRX_TRY(use_device(l->device));
    OwnStream own;
    BRX_HIP(hipStreamCreateWithFlags(&own.s, hipStreamNonBlocking));
    hipStream_t s = own.s;
    DevBuf<uint64_t> d_keys;
    DevBuf<uint8_t> d_none;
    uint64_t kept = 0;
    // count > abundance over a sorted list is a compaction: the merge with an empty B, keys only
    BRX_TRY(counts_merge(me, l->d_keys, l->d_cnts, l->n, nullptr, nullptr, 0, BRX_COUNTOP_ADD, (uint32_t)abundance + 1u, false, s, d_keys, d_none,
                         &kept, nullptr));
    st8[0] = l->n;
    st8[1] = kept;
    st8[4] = ns_since(t0);
    auto t1 = Clock::now();
    BRX_TRY(set_from_keys(me, l->k, l->device, d_keys, kept, s, out));
    st8[6] = ns_since(t1);
    st8[7] = ns_since(t0);
    if (stats8)
        memcpy(stats8, st8, sizeof st8);
    return BRX_OK;
}

int brx_keys_combine_device(const uint64_t *d_a, uint64_t na, const uint64_t *d_b, uint64_t nb, int op, uint64_t *d_out, uint64_t cap,
                            uint64_t *n_out, uint64_t *sizes3, void *stream)
{
    const char *me = "brx_keys_combine_device";
    if (!n_out || (!d_out && cap)) {
        set_error("%s: null n_out, or a capacity without an output array", me);
        return BRX_ERR_ARG;
    }
    *n_out = 0;
    if (overlap_bytes(d_out, cap * 8, d_a, na * 8) || overlap_bytes(d_out, cap * 8, d_b, nb * 8)) {
        set_error("%s: the output array overlaps an input", me);
        return BRX_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    MergePlan plan(d_a, nullptr, na, d_b, nullptr, nb);
    BRX_TRY(merge_count(me, op, s, &plan));
    *n_out = plan.total;
    if (sizes3) {
        sizes3[0] = na;
        sizes3[1] = nb;
        sizes3[2] = plan.both;
    }
    if (!d_out && !cap)
        return BRX_OK; // the sizes only
    if (cap < plan.total) {
        set_error("%s: the result holds %llu keys, the output array %llu", me, (u64)plan.total, (u64)cap);
        return BRX_ERR_ARG;
    }
    return merge_write(me, plan, d_out, s);
}

int brx_set_combine(const brx_set_t *a, const brx_set_t *b, int op, brx_set_t **out, uint64_t *stats8)
{
    const char *me = "brx_set_combine";
    if (!out) {
        set_error("%s: null out", me);
        return BRX_ERR_ARG;
    }
    *out = nullptr;
    BRX_TRY(operands_ok(me, a, b));
    if (op < 0 || op > 3) {
        set_error("%s: op=%d (BRX_SETOP_UNION 0, INTERSECT 1, DIFFERENCE 2, SYMDIFF 3)", me, op);
        return BRX_ERR_ARG;
    }
    uint64_t st8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto t0 = Clock::now();
    BRX_TRY(use_device(a->device));
    OwnStream own;
    BRX_HIP(hipStreamCreateWithFlags(&own.s, hipStreamNonBlocking));
    hipStream_t s = own.s;
    Operands o;
    BRX_TRY(operands_list(a, b, s, &o));
    st8[4] = ns_since(t0);
    auto t1 = Clock::now();
    DevBuf<uint64_t> d_res;
    {
        MergePlan plan(o.d_a, nullptr, o.na, o.d_b, nullptr, o.nb);
        BRX_TRY(merge_count(me, op, s, &plan));
        if (plan.total > set_nbits(a->k)) {
            set_error("%s: %llu keys in the result, only %llu exist at k=%d", me, (u64)plan.total, (u64)set_nbits(a->k), a->k);
            return BRX_ERR_HIP;
        }
        if (plan.total)
            BRX_TRY(d_res.reserve(plan.total, 0, "keys of the combined set"));
        BRX_TRY(merge_write(me, plan, d_res, s));
        st8[0] = o.na;
        st8[1] = o.nb;
        st8[2] = plan.both;
        st8[3] = plan.total;
    }
    o.keys_a.reset(); // (the operands' lists go back before the result's index is built)
    o.keys_b.reset();
    st8[5] = ns_since(t1);
    auto t2 = Clock::now();
    BRX_TRY(set_from_keys(me, a->k, a->device, d_res, st8[3], s, out));
    st8[6] = ns_since(t2);
    st8[7] = ns_since(t0);
    if (stats8)
        memcpy(stats8, st8, sizeof st8);
    return BRX_OK;
}

int brx_set_compare(const brx_set_t *a, const brx_set_t *b, uint64_t *sizes3)
{
    const char *me = "brx_set_compare";
    if (!sizes3) {
        set_error("%s: null sizes3", me);
        return BRX_ERR_ARG;
    }
    BRX_TRY(operands_ok(me, a, b));
    BRX_TRY(use_device(a->device));
    OwnStream own;
    BRX_HIP(hipStreamCreateWithFlags(&own.s, hipStreamNonBlocking));
    Operands o;
    BRX_TRY(operands_list(a, b, own.s, &o));
    MergePlan plan(o.d_a, nullptr, o.na, o.d_b, nullptr, o.nb);
    BRX_TRY(merge_count(me, BRX_SETOP_INTERSECT, own.s, &plan));
    sizes3[0] = o.na;
    sizes3[1] = o.nb;
    sizes3[2] = plan.both;
    return BRX_OK;
}

} // extern "C"
