// Key files (include/brx.h "key files", br_amd/keyfile.py states the format): sorted canonical keys, optionally with their
// counts, written to and read from a file descriptor at any odd k.
//
//   list     a table counter: table_list_kernel, one pass over the slots like table_select_kernel, but with the keepers of
//            4096 slots placed by a block scan and one atomic per block trip; keys with min(255, count) >= min_count and
//            their count bytes; the counter is only read.  A partitioned counter: its count view compacted in place
//            order (view_count_kernel, a scan, view_write_kernel) -- sorted already, the sort below finds nothing to do
//            and is not called.  A set: set_list_keys
//            (brx_index.hip) -- its key list as it is, the lines of its chained table (the same kernel, no counts), or the bits.
//   sort     stable LSD radix sort of (u64 key, optional u8 payload), 8-bit digits, ceil(key_bits / 8) passes between two
//            buffers.  A pass is three steps, each its own launches: digit histograms per tile of 4096 keys, an exclusive
//            scan of the (digit, tile) counts, a scatter that ranks the keys inside their tile.  No workgroup ever waits
//            for another one: what one step leaves is read by the next launch.
//   pack     one wave per 256-key file block: pack_measure_kernel (differences, width by a wave max of bit lengths, bytes
//            per block, key sum), an exclusive scan of the sizes, pack_write_kernel (first key, width, the bit stream
//            gathered byte by byte from the values in LDS, count bytes).
//   unpack   the host walks the block headers of a slice (the size of a block follows from its width byte), uploads the
//            slice and its block offsets; unpack_kernel, one wave per block, extracts the values, prefix-sums them onto
//            the first key (saturating, so that nothing wraps) and checks key < 2^(2k-1) and count >= max(1, floor);
//            order_check_kernel compares every block's first key with the key before it.
//   load     pairs into a counting table through table_merge_kernel (tab_merge_pairs, brx_counttable.hip), keys into a
//            set as the key list a finish leaves; or the pairs as they are into a count list (brx_counts_load_fd; its
//            from_counter is the `list` step above, its save the `pack` step; the merge of two lists is brx_setops.hip's).
// The file passes through two page-locked pieces of BRX_KEYFILE_SLICE_KB KiB (default 8192), one being filled or drained
// by the fd while the other is copied.
#include "brx_internal.hpp"
#include "brx_index.hpp"
#include "brx_keyio.hpp"

#include <errno.h>
#include <string.h>
#include <unistd.h>
#include <chrono>
#include <utility>

using namespace brx;

namespace {

typedef unsigned long long u64;

constexpr uint32_t SORT_TILE = 4096;  // keys per tile of a digit pass
constexpr uint32_t SCAN_CHUNK = 4096; // elements per block trip of the scan
constexpr uint32_t KF_BLOCK = 256;    // keys per file block
constexpr uint32_t KF_MAX_WIDTH = 61;
constexpr u64 KF_SAT = 1ull << 62; // keys and partial sums are clamped here: operands below 2^62 never wrap 64 bits
constexpr uint32_t ERR_KEY = 1, ERR_COUNT = 2, ERR_ORDER = 4;
const char KF_MAGIC[9] = "BRXKMERS";

uint32_t grid_of(uint64_t items, uint32_t per_block) { return read_grid((items + per_block - 1) / per_block + (items ? 0 : 1), 256u * 16u); }

// ---- scan (wave_incl_scan, block_excl_scan: brx_keyio.hpp) ------------------------------------------------------------------
// sums[c] = sum of chunk c of data
__global__ __launch_bounds__(256) void scan_reduce_kernel(const u64 *__restrict__ data, uint64_t n, uint64_t n_chunks, u64 *__restrict__ sums)
{
    __shared__ u64 sh[4];
    for (uint64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) { // block-uniform
        u64 x = 0;
        for (uint32_t j = threadIdx.x; j < SCAN_CHUNK; j += 256u) {
            const uint64_t i = c * SCAN_CHUNK + j;
            if (i < n)
                x += data[i];
        }
        u64 total;
        (void)block_excl_scan(x, sh, &total);
        if (threadIdx.x == 0)
            sums[c] = total;
    }
}

// one block: exclusive scan of sums[0 .. n) in place, the total into sums[n]
__global__ __launch_bounds__(256) void scan_sums_kernel(u64 *__restrict__ sums, uint64_t n)
{
    __shared__ u64 sh[4];
    u64 carry = 0;
    for (uint64_t i0 = 0; i0 < n; i0 += 256u) { // block-uniform
        const uint64_t i = i0 + threadIdx.x;
        const u64 x = i < n ? sums[i] : 0ull;
        u64 total;
        const u64 ex = block_excl_scan(x, sh, &total);
        if (i < n)
            sums[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0)
        sums[n] = carry;
}

// exclusive scan of every chunk in place, starting from the chunk's scanned sum; a thread takes 16 neighbouring elements
__global__ __launch_bounds__(256) void scan_down_kernel(u64 *__restrict__ data, uint64_t n, uint64_t n_chunks, const u64 *__restrict__ sums)
{
    __shared__ u64 sh[4];
    for (uint64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) { // block-uniform
        const uint64_t i0 = c * SCAN_CHUNK + (uint64_t)threadIdx.x * 16u;
        u64 v[16];
        u64 x = 0;
        for (int j = 0; j < 16; j++) {
            v[j] = i0 + j < n ? data[i0 + j] : 0ull;
            x += v[j];
        }
        u64 total;
        u64 at = sums[c] + block_excl_scan(x, sh, &total);
        for (int j = 0; j < 16; j++) {
            if (i0 + j < n)
                data[i0 + j] = at;
            at += v[j];
        }
    }
}

// exclusive scan of d_data[0 .. n) in place; d_sums holds ceil(n / SCAN_CHUNK) + 1 entries, the last one receives the total
int scan_exclusive(u64 *d_data, uint64_t n, u64 *d_sums, hipStream_t s)
{
    const uint64_t n_chunks = (n + SCAN_CHUNK - 1) / SCAN_CHUNK;
    if (n_chunks)
        scan_reduce_kernel<<<read_grid(n_chunks, 256u * 16u), 256, 0, s>>>(d_data, n, n_chunks, d_sums);
    scan_sums_kernel<<<1, 256, 0, s>>>(d_sums, n_chunks);
    if (n_chunks)
        scan_down_kernel<<<read_grid(n_chunks, 256u * 16u), 256, 0, s>>>(d_data, n, n_chunks, d_sums);
    BRX_HIP(hipGetLastError());
    return BRX_OK;
}

// ---- list -----------------------------------------------------------------------------------------------------------------
// A block takes 4096 consecutive slots per trip, 16 per thread and coalesced; the keepers are counted per thread, placed inside the block by a block scan, and the block asks for
// its places with ONE atomic per trip.  (table_select_kernel asks once per wave trip; here nearly every trip holds a keeper,
// and 2^26 adds on one address measured 640 ms per Gbp of reads -- 16 ms of reads behind 620 ms of atomics.)
constexpr uint32_t LIST_PER_THREAD = 16, LIST_CHUNK = 256 * LIST_PER_THREAD;

__global__ __launch_bounds__(256) void table_list_kernel(const uint64_t *__restrict__ lines, const uint32_t *__restrict__ counts, uint64_t n_slots,
                                                         uint32_t min_count, uint64_t *__restrict__ keys, uint8_t *__restrict__ cnts, uint64_t cap,
                                                         u64 *__restrict__ n_out)
{
    __shared__ u64 sh[4];
    __shared__ u64 sh_base;
    const uint64_t n_chunks = (n_slots + LIST_CHUNK - 1) / LIST_CHUNK;
    for (uint64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) { // block-uniform
        uint64_t v[LIST_PER_THREAD];
        uint8_t cn[LIST_PER_THREAD];
        uint32_t mine = 0;
        for (uint32_t j = 0; j < LIST_PER_THREAD; j++) {
            const uint64_t i = c * LIST_CHUNK + (uint64_t)j * 256u + threadIdx.x;
            const uint64_t x = i >= n_slots ? 0ull : table_slot_key(lines, i);
            const uint32_t cnt = (x && counts) ? table_count_read(counts[i]) : 1u;
            const bool keep = x && cnt >= min_count;
            v[j] = keep ? x : 0ull;
            cn[j] = (uint8_t)cnt;
            mine += keep ? 1u : 0u;
        }
        u64 total;
        const u64 before = block_excl_scan((u64)mine, sh, &total);
        if (threadIdx.x == 0)
            sh_base = total ? atomicAdd(n_out, total) : 0ull;
        __syncthreads();
        uint64_t pos = sh_base + before;
        for (uint32_t j = 0; j < LIST_PER_THREAD; j++)
            if (v[j]) {
                if (pos < cap) {
                    keys[pos] = v[j] - 1ull;
                    if (cnts)
                        cnts[pos] = cn[j];
                }
                pos++;
            }
        __syncthreads(); // (sh_base is written again in the next trip)
    }
}

// ---- list of a partitioned counter: its count view, compacted --------------------------------------------------------------
// The count view (brx_partbuild.hip: final_view_kernel) holds, per last-level bucket of 2^VIEW_KEY_BITS hashes, the distinct
// keys in rising order at the front of the bucket's range, VIEW_PAD behind them, and min(255, count) at the same index; the
// buckets follow each other in hash order.  The entries with count >= floor, read position by position, are the file's
// content in the file's order: nothing is sorted, and a keeper's place is the number of keepers before it.
//   view_count_kernel   sums[w] = keepers of wave chunk w (per_wave consecutive buckets): one flat walk over the chunk's
//                       positions, the buckets' borders do not matter to a count
//   scan_exclusive      of the sums; the total sizes the two output arrays
//   view_write_kernel   the chunk again in groups of up to 63 buckets from ONE load of 64 offsets (lane l: where bucket
//                       g0 + l starts); a position finds its bucket by a binary search over the lanes' offsets (6 shuffles)
// Both walk 256 positions a trip, four neighbouring ones per lane from one 8-byte and one 4-byte load, whatever the shape:
// 2^29 buckets of two positions (k = 21), 32 buckets of 9 300 (k = 9), or a range of 70 000 positions behind one key --
// padding is read like a key and kept by nobody, which costs its 3 bytes and no round trip.  Places inside a trip: lane
// order, then the lane's own four -- four ballots and the lanes below.  No LDS, no barrier, no atomics: a wave owns its
// chunk in both passes.  Positions and places are 64-bit; only the distances inside a group are kept in 32 bits for the
// search, and a group that spans 2^32 positions or more is walked bucket by bucket instead, no search needed.
constexpr uint32_t VIEW_KEY_BITS = 12, VIEW_PAD = 0xFFFFu; // (F_BITS and VIEW_PAD of brx_partbuild.hip)
constexpr uint32_t VC_GROUP = 63, VC_MAX_GROUPS = 16, VC_TRIP = 256;

// the four positions at .. at + 3 (at % 4 == 0) of the view, those inside [lo, hi) only: bit q of the result = position
// at + q is kept.  (The quad that holds hi - 1 may reach 3 entries past hi: both arrays are allocated 64 entries longer.)
__device__ __forceinline__ uint32_t view_quad(const uint16_t *__restrict__ vkeys, const uint8_t *__restrict__ vcnts, uint64_t at, uint64_t lo,
                                              uint64_t hi, uint32_t floor, uint32_t key[4], uint32_t cnt[4])
{
    uint32_t keep = 0;
    if (at < hi) {
        const uint2 kv = *reinterpret_cast<const uint2 *>(vkeys + at);
        const uint32_t cv = *reinterpret_cast<const uint32_t *>(vcnts + at);
        key[0] = kv.x & 0xFFFFu;
        key[1] = kv.x >> 16;
        key[2] = kv.y & 0xFFFFu;
        key[3] = kv.y >> 16;
        for (uint32_t q = 0; q < 4u; q++) {
            cnt[q] = (cv >> (8u * q)) & 0xFFu;
            if (at + q >= lo && at + q < hi && key[q] != VIEW_PAD && cnt[q] >= floor)
                keep |= 1u << q;
        }
    }
    return keep;
}

__global__ __launch_bounds__(256) void view_count_kernel(const uint16_t *__restrict__ vkeys, const uint8_t *__restrict__ vcnts,
                                                         const uint64_t *__restrict__ off, uint64_t n_buckets, uint32_t per_wave,
                                                         uint64_t n_wchunks, uint32_t floor, u64 *__restrict__ sums)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t n_bchunks = (n_wchunks + 3ull) / 4ull;
    for (uint64_t bc = blockIdx.x; bc < n_bchunks; bc += gridDim.x) {
        const uint64_t w = bc * 4ull + wave;
        if (w >= n_wchunks)
            continue; // wave-uniform
        const uint64_t b_lo = w * per_wave;
        const uint64_t b_hi = b_lo + per_wave < n_buckets ? b_lo + per_wave : n_buckets;
        const uint64_t lo = off[b_lo], hi = off[b_hi];
        uint32_t key[4], cnt[4];
        u64 mine = 0;
        for (uint64_t q0 = lo & ~3ull; q0 < hi; q0 += VC_TRIP) // wave-uniform
            mine += (u64)__popc(view_quad(vkeys, vcnts, q0 + 4ull * lane, lo, hi, floor, key, cnt));
        for (int o = 32; o > 0; o >>= 1)
            mine += __shfl_xor(mine, o);
        if (lane == 0u)
            sums[w] = mine;
    }
}

// sums: scanned.  walk: positions [lo, hi) of the view from place `run` on; SEARCH: they lie in buckets g0 .. g0 + gcount - 1,
// lane l <= gcount holding in rel where bucket g0 + l starts behind `lo` (lane gcount: hi - lo, below 2^32); otherwise all
// in bucket g0.  Returns the place behind the last keeper.
template <bool SEARCH>
__device__ __forceinline__ u64 view_write_walk(const uint16_t *__restrict__ vkeys, const uint8_t *__restrict__ vcnts, uint64_t lo, uint64_t hi,
                                               uint64_t g0, uint32_t gcount, uint32_t rel, uint32_t floor, u64 run,
                                               uint64_t *__restrict__ keys, uint8_t *__restrict__ cnts, uint64_t cap, uint32_t lane)
{
    for (uint64_t q0 = lo & ~3ull; q0 < hi; q0 += VC_TRIP) { // wave-uniform
        const uint64_t at = q0 + 4ull * lane;
        uint32_t key[4], cnt[4];
        const uint32_t keep = view_quad(vkeys, vcnts, at, lo, hi, floor, key, cnt);
        uint32_t before = 0, total = 0;
        for (uint32_t q = 0; q < 4u; q++) {
            const u64 m = __ballot((keep >> q) & 1u);
            before += __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)); // kept in the lanes below
            total += (uint32_t)__popcll(m);
        }
        if (!total)
            continue; // wave-uniform
        uint32_t bucket[4] = {0u, 0u, 0u, 0u};
        if (SEARCH)
            for (uint32_t q = 0; q < 4u; q++) { // every lane takes part in the shuffles
                const uint32_t p = (uint32_t)(at + q - lo); // (of a kept position: inside [0, hi - lo))
                uint32_t j = 0;
                for (uint32_t step = 32u; step; step >>= 1) {
                    const uint32_t cand = j + step; // <= 63
                    const uint32_t r = __shfl(rel, (int)cand);
                    if (cand < gcount && r <= p)
                        j = cand;
                }
                bucket[q] = j; // the last bucket that starts at or before p: the empty ones before it start there too
            }
        uint64_t pos = run + before;
        for (uint32_t q = 0; q < 4u; q++)
            if ((keep >> q) & 1u) {
                if (pos < cap) { // (always: the sums were taken over the same view)
                    keys[pos] = ((g0 + bucket[q]) << VIEW_KEY_BITS) | (uint64_t)key[q];
                    cnts[pos] = (uint8_t)cnt[q];
                }
                pos++;
            }
        run += total;
    }
    return run;
}

__global__ __launch_bounds__(256) void view_write_kernel(const uint16_t *__restrict__ vkeys, const uint8_t *__restrict__ vcnts,
                                                         const uint64_t *__restrict__ off, uint64_t n_buckets, uint32_t per_wave,
                                                         uint64_t n_wchunks, uint32_t floor, uint64_t wide_span,
                                                         const u64 *__restrict__ sums, uint64_t *__restrict__ keys,
                                                         uint8_t *__restrict__ cnts, uint64_t cap)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t n_bchunks = (n_wchunks + 3ull) / 4ull;
    for (uint64_t bc = blockIdx.x; bc < n_bchunks; bc += gridDim.x) {
        const uint64_t w = bc * 4ull + wave;
        if (w >= n_wchunks)
            continue; // wave-uniform
        const uint64_t b_lo = w * per_wave;
        const uint64_t b_hi = b_lo + per_wave < n_buckets ? b_lo + per_wave : n_buckets;
        if (off[b_lo] == off[b_hi])
            continue; // nothing but empty buckets (most chunks of a small input at large k)
        u64 run = sums[w]; // keepers of the whole view before the next one
        for (uint64_t g0 = b_lo; g0 < b_hi; g0 += VC_GROUP) {
            const uint32_t gcount = b_hi - g0 < VC_GROUP ? (uint32_t)(b_hi - g0) : VC_GROUP;
            const uint64_t oi = g0 + lane;
            const uint64_t offv = off[oi <= n_buckets ? oi : n_buckets];
            const uint32_t off_lo = (uint32_t)offv, off_hi = (uint32_t)(offv >> 32);
            // (readlane returns a signed int: without the casts an offset with bit 31 set sign-extends)
            const uint64_t gs = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)off_hi, 0) << 32) |
                                (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)off_lo, 0);
            const uint64_t ge = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)off_hi, (int)gcount) << 32) |
                                (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)off_lo, (int)gcount);
            if (ge == gs)
                continue;
            if (ge - gs < wide_span) { // (at most 2^32)
                const uint32_t rel = lane <= gcount ? (uint32_t)(offv - gs) : 0xFFFFFFFFu;
                run = view_write_walk<true>(vkeys, vcnts, gs, ge, g0, gcount, rel, floor, run, keys, cnts, cap, lane);
            } else { // 2^32 positions in 63 buckets: bucket by bucket, no distance to keep in 32 bits
                for (uint32_t j = 0; j < gcount; j++) {
                    const uint64_t s = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)off_hi, (int)j) << 32) |
                                       (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)off_lo, (int)j);
                    const uint64_t e = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)off_hi, (int)j + 1) << 32) |
                                       (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)off_lo, (int)j + 1);
                    run = view_write_walk<false>(vkeys, vcnts, s, e, g0 + j, 1u, 0u, floor, run, keys, cnts, cap, lane);
                }
            }
        }
    }
}

// ---- sort -----------------------------------------------------------------------------------------------------------------
// hist[d * n_tiles + t] = keys of tile t whose digit is d
__global__ __launch_bounds__(256) void sort_hist_kernel(const uint64_t *__restrict__ keys, uint64_t n, uint32_t shift, uint64_t n_tiles,
                                                        u64 *__restrict__ hist)
{
    __shared__ uint32_t h[256];
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) { // block-uniform
        h[threadIdx.x] = 0u;
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < SORT_TILE; j += 256u) {
            const uint64_t i = t * SORT_TILE + j;
            if (i < n)
                atomicAdd(&h[(uint32_t)(keys[i] >> shift) & 255u], 1u);
        }
        __syncthreads();
        hist[(uint64_t)threadIdx.x * n_tiles + t] = h[threadIdx.x];
        __syncthreads();
    }
}

// offs: the scanned histogram.  A tile goes out in rounds of 256 keys in index order; inside a round a key's place is the
// digit's running offset + the keys of that digit in the waves before + those in the lanes before (found with 8 ballots)
__global__ __launch_bounds__(256) void sort_scatter_kernel(const uint64_t *__restrict__ keys_in, const uint8_t *__restrict__ pay_in, uint64_t n,
                                                           uint32_t shift, uint64_t n_tiles, const u64 *__restrict__ offs,
                                                           uint64_t *__restrict__ keys_out, uint8_t *__restrict__ pay_out)
{
    __shared__ u64 running[256];
    __shared__ uint32_t wh[4][256];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) { // block-uniform
        running[tid] = offs[(uint64_t)tid * n_tiles + t];
        wh[0][tid] = wh[1][tid] = wh[2][tid] = wh[3][tid] = 0u;
        __syncthreads();
        for (uint32_t r = 0; r < SORT_TILE / 256u; r++) {
            const uint64_t i0 = t * SORT_TILE + (uint64_t)r * 256u;
            if (i0 >= n)
                break; // block-uniform
            const uint64_t i = i0 + tid;
            const bool valid = i < n;
            const uint64_t key = valid ? keys_in[i] : 0ull;
            const uint32_t d = (uint32_t)(key >> shift) & 255u;
            u64 peers = __ballot(valid);
            for (int b = 0; b < 8; b++) {
                const bool bit = (d >> b) & 1u;
                const u64 m = __ballot(bit);
                peers &= bit ? m : ~m;
            }
            const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
            if (valid && rank == 0u)
                wh[wave][d] = (uint32_t)__popcll(peers);
            __syncthreads();
            if (valid) {
                u64 pos = running[d] + rank;
                for (uint32_t w = 0; w < wave; w++)
                    pos += wh[w][d];
                if (pos < n) { // (always: the histogram was taken over the same keys)
                    keys_out[pos] = key;
                    if (pay_in)
                        pay_out[pos] = pay_in[i];
                }
            }
            __syncthreads();
            running[tid] += (u64)(wh[0][tid] + wh[1][tid] + wh[2][tid] + wh[3][tid]);
            wh[0][tid] = wh[1][tid] = wh[2][tid] = wh[3][tid] = 0u;
            __syncthreads();
        }
        __syncthreads();
    }
}

// sorts d_keys[0 .. n) by their low key_bits bits (stable), d_pay along with them; returns after `s` has been synchronised
int sort_pairs(uint64_t *d_keys, uint8_t *d_pay, uint64_t n, uint32_t key_bits, hipStream_t s)
{
    if (n < 2)
        return BRX_OK;
    const uint32_t passes = (key_bits + 7u) / 8u;
    const uint64_t n_tiles = (n + SORT_TILE - 1) / SORT_TILE;
    const uint64_t n_hist = 256ull * n_tiles;
    DevScratch ws;
    uint64_t *d_alt = nullptr;
    uint8_t *d_pay_alt = nullptr;
    u64 *d_hist = nullptr, *d_sums = nullptr;
    BRX_TRY(ws.get(&d_alt, n));
    if (d_pay)
        BRX_TRY(ws.get(&d_pay_alt, n));
    BRX_TRY(ws.get(&d_hist, n_hist));
    BRX_TRY(ws.get(&d_sums, (n_hist + SCAN_CHUNK - 1) / SCAN_CHUNK + 1));
    uint64_t *src = d_keys, *dst = d_alt;
    uint8_t *psrc = d_pay, *pdst = d_pay_alt;
    int st = BRX_OK;
    {
        KernelTimer kt("key_sort", s);
        const uint32_t grid = read_grid(n_tiles, 256u * 16u);
        for (uint32_t p = 0; p < passes && st == BRX_OK; p++) {
            sort_hist_kernel<<<grid, 256, 0, s>>>(src, n, p * 8u, n_tiles, d_hist);
            st = scan_exclusive(d_hist, n_hist, d_sums, s);
            if (st != BRX_OK)
                break;
            sort_scatter_kernel<<<grid, 256, 0, s>>>(src, psrc, n, p * 8u, n_tiles, d_hist, dst, pdst);
            std::swap(src, dst);
            std::swap(psrc, pdst);
        }
        if (st == BRX_OK && src != d_keys) {
            if (hipMemcpyAsync(d_keys, src, n * 8, hipMemcpyDeviceToDevice, s) != hipSuccess ||
                (d_pay && hipMemcpyAsync(d_pay, psrc, n, hipMemcpyDeviceToDevice, s) != hipSuccess))
                st = BRX_ERR_HIP;
        }
    }
    const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(s); // the scratch goes back to the pool below
    if (st == BRX_OK && (e1 != hipSuccess || e2 != hipSuccess)) {
        set_error("key sort: %s", hipGetErrorString(e1 != hipSuccess ? e1 : e2));
        return BRX_ERR_HIP;
    }
    return st;
}

// ---- pack -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t bit_length(u64 v) { return v ? 64u - (uint32_t)__clzll(v) : 0u; }

// per file block: width and bytes; the key sum of everything; ERR_ORDER where a key does not exceed the one before it
__global__ __launch_bounds__(256) void pack_measure_kernel(const uint64_t *__restrict__ keys, uint64_t n, uint64_t n_blocks, uint32_t with_counts,
                                                           uint8_t *__restrict__ width, u64 *__restrict__ size, u64 *__restrict__ key_sum,
                                                           uint32_t *__restrict__ err)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t g = blockIdx.x; g * 4ull < n_blocks; g += gridDim.x) {
        const uint64_t b = g * 4ull + wave;
        if (b >= n_blocks)
            continue; // wave-uniform
        const uint64_t lo = b * KF_BLOCK;
        const uint32_t m = n - lo < KF_BLOCK ? (uint32_t)(n - lo) : KF_BLOCK;
        uint32_t w = 0;
        u64 sum = 0;
        bool bad = false;
        for (uint32_t j = lane; j < m; j += 64u) {
            const u64 key = keys[lo + j];
            sum += key;
            if (lo + j) {
                const u64 prev = keys[lo + j - 1];
                if (key <= prev)
                    bad = true;
                else if (j) {
                    const uint32_t bl = bit_length(key - prev - 1ull);
                    w = bl > w ? bl : w;
                }
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t ow = __shfl_xor(w, o);
            w = ow > w ? ow : w;
            sum += __shfl_xor(sum, o);
        }
        if (__ballot(bad) && lane == 0u)
            atomicOr(err, ERR_ORDER);
        if (lane == 0u) {
            width[b] = (uint8_t)w;
            size[b] = 9ull + ((u64)(m - 1u) * w + 7ull) / 8ull + (with_counts ? m : 0u);
            atomicAdd(key_sum, sum);
        }
    }
}

// off: the scanned sizes.  The values of a block go to LDS; every byte of the bit stream is gathered from the values that
// touch it (two for w >= 8, up to eight for w = 1) and stored once
__global__ __launch_bounds__(256) void pack_write_kernel(const uint64_t *__restrict__ keys, const uint8_t *__restrict__ cnts, uint64_t n,
                                                         uint64_t n_blocks, const uint8_t *__restrict__ width, const u64 *__restrict__ off,
                                                         uint64_t out_bytes, uint8_t *__restrict__ out)
{
    __shared__ u64 vals[4][KF_BLOCK];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t g = blockIdx.x; g * 4ull < n_blocks; g += gridDim.x) { // block-uniform
        const uint64_t b = g * 4ull + wave;
        const bool active = b < n_blocks;
        const uint64_t lo = b * KF_BLOCK;
        const uint32_t m = !active ? 0u : n - lo < KF_BLOCK ? (uint32_t)(n - lo) : KF_BLOCK;
        for (uint32_t j = lane; j + 1u < m; j += 64u)
            vals[wave][j] = keys[lo + j + 1] - keys[lo + j] - 1ull;
        __syncthreads();
        if (active) {
            const uint32_t w = width[b];
            const uint64_t o = off[b];
            const uint32_t nb = (uint32_t)(((u64)(m - 1u) * w + 7ull) / 8ull);
            if (o + 9ull + nb + (cnts ? m : 0u) <= out_bytes) { // (always: the sizes were measured over the same keys)
                const u64 first = keys[lo];
                if (lane < 8u)
                    out[o + lane] = (uint8_t)(first >> (8u * lane));
                else if (lane == 8u)
                    out[o + 8] = (uint8_t)w;
                for (uint32_t i = lane; i < nb; i += 64u) { // (nb > 0 means w >= 1)
                    const int bit0 = (int)(8u * i);
                    u64 byte = 0;
                    for (int j = bit0 / (int)w; j < (int)m - 1 && j * (int)w < bit0 + 8; j++) {
                        const int sh = j * (int)w - bit0;
                        const u64 v = vals[wave][j];
                        byte |= sh >= 0 ? (v << sh) : (v >> (-sh));
                    }
                    out[o + 9ull + i] = (uint8_t)(byte & 0xffull);
                }
                if (cnts)
                    for (uint32_t j = lane; j < m; j += 64u)
                        out[o + 9ull + nb + j] = cnts[lo + j];
            }
        }
        __syncthreads();
    }
}

// ---- unpack ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 sat_add(u64 a, u64 b)
{
    const u64 x = a + b; // (both at most 2^62)
    return x < KF_SAT ? x : KF_SAT;
}

// buf: a slice of the stream that holds n_blk whole blocks, block i of it (block first_block + i of the file) at blk_off[i]
// with a width byte the host has checked (<= 61), so that every byte read here lies inside the block.  A lane extracts four
// neighbouring values; the keys are the first key plus a saturating prefix sum.  Nothing is indexed with a value read.
__global__ __launch_bounds__(256) void unpack_kernel(const uint8_t *__restrict__ buf, const uint32_t *__restrict__ blk_off, uint32_t n_blk,
                                                     uint64_t first_block, uint64_t n, u64 key_limit, uint32_t with_counts, uint32_t min_cnt,
                                                     uint64_t *__restrict__ keys, uint8_t *__restrict__ cnts, u64 *__restrict__ key_sum,
                                                     uint32_t *__restrict__ err)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t g = blockIdx.x; g * 4ull < n_blk; g += gridDim.x) {
        const uint64_t bi = g * 4ull + wave;
        if (bi >= n_blk)
            continue; // wave-uniform
        const uint64_t lo = (first_block + bi) * KF_BLOCK;
        if (lo >= n)
            continue;
        const uint32_t m = n - lo < KF_BLOCK ? (uint32_t)(n - lo) : KF_BLOCK;
        const uint8_t *p = buf + blk_off[bi];
        u64 first = 0;
        for (int t = 0; t < 8; t++)
            first |= (u64)p[t] << (8 * t);
        uint32_t w = p[8];
        w = w > KF_MAX_WIDTH ? KF_MAX_WIDTH : w;
        const uint32_t nb = (uint32_t)(((u64)(m - 1u) * w + 7ull) / 8ull);
        const uint8_t *vb = p + 9;
        const u64 vmask = w ? (~0ull >> (64u - w)) : 0ull;
        uint32_t bad = first >= key_limit ? ERR_KEY : 0u;
        // lane-local inclusive sums of (value + 1) for values 4 lane .. 4 lane + 3
        u64 a[4];
        u64 run = 0;
        for (uint32_t q = 0; q < 4u; q++) {
            const uint32_t j = 4u * lane + q;
            u64 inc = 0;
            if (j + 1u < m) {
                const uint32_t bit = j * w, by = bit >> 3, sh = bit & 7u;
                u64 lo8 = 0, hi = 0;
                for (uint32_t t = 0; t < 8u; t++)
                    if (by + t < nb)
                        lo8 |= (u64)vb[by + t] << (8u * t);
                if (sh && by + 8u < nb)
                    hi = vb[by + 8u];
                const u64 v = ((lo8 >> sh) | (sh ? hi << (64u - sh) : 0ull)) & vmask;
                inc = v + 1ull; // (at most 2^61)
            }
            run = sat_add(run, inc);
            a[q] = run;
        }
        u64 x = run; // inclusive wave scan of the lane totals, saturating
        for (int o = 1; o < 64; o <<= 1) {
            const u64 y = __shfl_up(x, o);
            if (lane >= (uint32_t)o)
                x = sat_add(x, y);
        }
        u64 before = __shfl_up(x, 1);
        if (lane == 0u)
            before = 0;
        const u64 base = sat_add(first < KF_SAT ? first : KF_SAT, before);
        u64 sum = 0;
        if (lane == 0u) {
            keys[lo] = first;
            sum = first;
        }
        for (uint32_t q = 0; q < 4u; q++) {
            const uint32_t j = 4u * lane + q;
            if (j + 1u < m) {
                const u64 key = sat_add(base, a[q]);
                if (key >= key_limit)
                    bad |= ERR_KEY;
                keys[lo + j + 1u] = key;
                sum += key;
            }
        }
        if (with_counts)
            for (uint32_t j = lane; j < m; j += 64u) {
                const uint32_t c = vb[nb + j];
                if (c < min_cnt)
                    bad |= ERR_COUNT;
                if (cnts)
                    cnts[lo + j] = (uint8_t)c;
            }
        for (int o = 32; o > 0; o >>= 1) {
            sum += __shfl_xor(sum, o);
            bad |= __shfl_xor(bad, o);
        }
        if (lane == 0u) {
            atomicAdd(key_sum, sum);
            if (bad)
                atomicOr(err, bad);
        }
    }
}

// every block's first key exceeds the key before it (inside a block the keys increase by construction)
__global__ __launch_bounds__(256) void order_check_kernel(const uint64_t *__restrict__ keys, uint64_t n_blocks, uint32_t *__restrict__ err)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t b = 1 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < n_blocks; b += stride)
        if (keys[b * KF_BLOCK] <= keys[b * KF_BLOCK - 1])
            atomicOr(err, ERR_ORDER);
}

// ---- host side (the pieces: brx_keyio.hpp) -----------------------------------------------------------------------------------
} // namespace

namespace brx {

size_t slice_bytes()
{
    const size_t kb = env_u32("BRX_KEYFILE_SLICE_KB", 8192u);
    return (size_t)(kb < 4u ? 4u : kb > (1u << 20) ? (1u << 20) : kb) * 1024u; // (a block is at most 2210 bytes; offsets are 32 bits)
}

int write_all(int fd, const uint8_t *p, size_t n)
{
    while (n) {
        const ssize_t w = ::write(fd, p, n);
        if (w < 0) {
            if (errno == EINTR)
                continue;
            set_error("key file: write: %s", strerror(errno));
            return BRX_ERR_ARG;
        }
        p += w;
        n -= (size_t)w;
    }
    return BRX_OK;
}

// reads until `want` bytes or the end of the stream; *got = bytes read
int read_upto(int fd, uint8_t *p, size_t want, size_t *got)
{
    size_t have = 0;
    while (have < want) {
        const ssize_t r = ::read(fd, p + have, want - have);
        if (r < 0) {
            if (errno == EINTR)
                continue;
            set_error("key file: read: %s", strerror(errno));
            return BRX_ERR_ARG;
        }
        if (r == 0)
            break;
        have += (size_t)r;
    }
    *got = have;
    return BRX_OK;
}

} // namespace brx

namespace {

void put_header(uint8_t *h, int k, bool with_counts, uint8_t floor, uint64_t n, uint64_t key_sum)
{
    memcpy(h, KF_MAGIC, 8);
    h[8] = 1;
    h[9] = (uint8_t)k;
    h[10] = with_counts ? 1 : 0;
    h[11] = floor;
    const uint32_t blk = KF_BLOCK;
    for (int i = 0; i < 4; i++)
        h[12 + i] = (uint8_t)(blk >> (8 * i));
    for (int i = 0; i < 8; i++) {
        h[16 + i] = (uint8_t)(n >> (8 * i));
        h[24 + i] = (uint8_t)(key_sum >> (8 * i));
    }
}

// sorted keys (and counts) -> the file on out_fd.  stats8[1..3] and [5], [6] are filled here
int pack_and_write(int k, const uint64_t *d_keys, const uint8_t *d_cnts, uint64_t n, uint8_t floor, int out_fd, hipStream_t s, uint64_t *st8)
{
    const uint64_t n_blocks = (n + KF_BLOCK - 1) / KF_BLOCK;
    uint8_t header[32];
    DevScratch ws;
    uint8_t *d_width = nullptr, *d_out = nullptr;
    u64 *d_size = nullptr, *d_sums = nullptr, *d_ctl = nullptr; // ctl: [0] key sum, [1] error bits
    uint64_t total = 0, key_sum = 0, max_w = 0;
    auto t0 = Clock::now();
    if (n) {
        BRX_TRY(ws.get(&d_width, n_blocks));
        BRX_TRY(ws.get(&d_size, n_blocks));
        BRX_TRY(ws.get(&d_sums, (n_blocks + SCAN_CHUNK - 1) / SCAN_CHUNK + 1));
        BRX_TRY(ws.get(&d_ctl, 2));
        BRX_HIP(hipMemsetAsync(d_ctl, 0, 16, s));
        const uint32_t grid = read_grid((n_blocks + 3) / 4, 256u * 16u);
        u64 ctl[2] = {0, 0};
        u64 tot = 0;
        std::vector<uint8_t> widths;
        {
            KernelTimer kt("key_pack", s);
            pack_measure_kernel<<<grid, 256, 0, s>>>(d_keys, n, n_blocks, d_cnts ? 1u : 0u, d_width, d_size, d_ctl, (uint32_t *)(d_ctl + 1));
            BRX_HIP(hipGetLastError());
            BRX_TRY(scan_exclusive(d_size, n_blocks, d_sums, s));
        }
        BRX_HIP(hipMemcpyAsync(ctl, d_ctl, 16, hipMemcpyDeviceToHost, s));
        BRX_HIP(hipMemcpyAsync(&tot, d_sums + (n_blocks + SCAN_CHUNK - 1) / SCAN_CHUNK, 8, hipMemcpyDeviceToHost, s));
        BRX_HIP(hipStreamSynchronize(s));
        if (ctl[1]) {
            set_error("key file: the listed keys are not strictly increasing after the sort (a k-mer listed twice)");
            return BRX_ERR_HIP;
        }
        if (tot > n * 9ull + n_blocks * 9ull + 8ull * n) {
            set_error("key file: %llu packed bytes for %llu keys", tot, (u64)n);
            return BRX_ERR_HIP;
        }
        total = tot;
        key_sum = ctl[0];
        BRX_TRY(ws.get(&d_out, total));
        {
            KernelTimer kt("key_pack", s);
            pack_write_kernel<<<grid, 256, 0, s>>>(d_keys, d_cnts, n, n_blocks, d_width, d_size, total, d_out);
            BRX_HIP(hipGetLastError());
        }
        // (the largest width is a statistic: a small copy of the width bytes, in pieces)
        widths.resize((size_t)(n_blocks < (1u << 20) ? n_blocks : (1u << 20)));
        for (uint64_t at = 0; at < n_blocks; at += widths.size()) {
            const size_t cnt = (size_t)(n_blocks - at < widths.size() ? n_blocks - at : widths.size());
            BRX_HIP(hipMemcpyAsync(widths.data(), d_width + at, cnt, hipMemcpyDeviceToHost, s));
            BRX_HIP(hipStreamSynchronize(s));
            for (size_t i = 0; i < cnt; i++)
                max_w = widths[i] > max_w ? widths[i] : max_w;
        }
        BRX_HIP(hipStreamSynchronize(s));
    }
    st8[5] = ns_since(t0);
    put_header(header, k, d_cnts != nullptr, floor, n, key_sum);
    st8[1] = 32 + total;
    st8[2] = n_blocks;
    st8[3] = max_w;
    // the stream leaves through two page-locked pieces: one is written to the fd while the other is being copied
    auto t1 = Clock::now();
    int st = write_all(out_fd, header, 32);
    if (st == BRX_OK && total) {
        const size_t piece = slice_bytes();
        PinnedPair pin;
        EventPair ev;
        BRX_TRY(pin.get(piece));
        BRX_TRY(ev.make());
        const uint64_t n_pieces = (total + piece - 1) / piece;
        auto start = [&](uint64_t i) -> int {
            const uint64_t at = i * piece, len = total - at < piece ? total - at : piece;
            BRX_HIP(hipMemcpyAsync(pin.p[i & 1], d_out + at, len, hipMemcpyDeviceToHost, s));
            BRX_HIP(hipEventRecord(ev.e[i & 1], s));
            return BRX_OK;
        };
        st = start(0);
        for (uint64_t i = 0; i < n_pieces && st == BRX_OK; i++) {
            if (hipEventSynchronize(ev.e[i & 1]) != hipSuccess) {
                set_error("key file: copy of piece %llu failed", (u64)i);
                st = BRX_ERR_HIP;
                break;
            }
            if (i + 1 < n_pieces)
                st = start(i + 1);
            if (st == BRX_OK) {
                const uint64_t at = i * piece, len = total - at < piece ? total - at : piece;
                st = write_all(out_fd, pin.p[i & 1], (size_t)len);
            }
        }
        (void)hipStreamSynchronize(s); // nothing may still be copying into the pieces when they are released
    }
    st8[6] = ns_since(t1);
    return st;
}

struct KeyHeader {
    int k = 0;
    bool with_counts = false;
    uint8_t floor = 0;
    uint64_t n = 0, key_sum = 0;
};

int read_header(int fd, KeyHeader *h)
{
    uint8_t b[32];
    size_t got = 0;
    BRX_TRY(read_upto(fd, b, 32, &got));
    if (got >= 8 && memcmp(b, KF_MAGIC, 8) != 0) {
        set_error("key file: wrong magic (not a key file)");
        return BRX_ERR_FORMAT;
    }
    if (got < 32) {
        set_error("key file: truncated stream: %llu bytes of the 32-byte header", (u64)got);
        return BRX_ERR_FORMAT;
    }
    if (b[8] != 1) {
        set_error("key file: wrong version %d (this reader knows version 1)", (int)b[8]);
        return BRX_ERR_FORMAT;
    }
    uint32_t blk = 0;
    uint64_t n = 0, sum = 0;
    for (int i = 0; i < 4; i++)
        blk |= (uint32_t)b[12 + i] << (8 * i);
    for (int i = 0; i < 8; i++) {
        n |= (uint64_t)b[16 + i] << (8 * i);
        sum |= (uint64_t)b[24 + i] << (8 * i);
    }
    if (blk != KF_BLOCK) {
        set_error("key file: wrong block size: %u keys per block (must be %u)", blk, KF_BLOCK);
        return BRX_ERR_FORMAT;
    }
    const int k = b[9];
    if (!(k & 1) || k < 5 || k > 31) {
        set_error("key file: k=%d (odd k from 5 to 31)", k);
        return BRX_ERR_FORMAT;
    }
    if (b[10] & ~1u) {
        set_error("key file: unknown flags 0x%02x", (unsigned)b[10]);
        return BRX_ERR_FORMAT;
    }
    if ((b[10] & 1u) ? b[11] < 1 : b[11] != 0) {
        set_error("key file: floor %d in a %s file", (int)b[11], (b[10] & 1u) ? "count" : "set");
        return BRX_ERR_FORMAT;
    }
    if (n > set_nbits(k)) {
        set_error("key file: %llu keys, only %llu exist at k=%d", (u64)n, (u64)set_nbits(k), k);
        return BRX_ERR_FORMAT;
    }
    h->k = k;
    h->with_counts = (b[10] & 1u) != 0;
    h->floor = b[11];
    h->n = n;
    h->key_sum = sum;
    return BRX_OK;
}

// the blocks behind a header, from in_fd to d_keys (and d_cnts when want_counts; both empty when the file holds no key).  st8[1..3], [5], [6] are filled.  Returns after `s` has been synchronised.
int read_blocks(int fd, const KeyHeader &h, bool want_counts, hipStream_t s, DevBuf<uint64_t> &d_keys, DevBuf<uint8_t> &d_cnts, uint64_t *st8)
{
    d_keys.reset();
    d_cnts.reset();
    const uint64_t n = h.n, n_blocks = (n + KF_BLOCK - 1) / KF_BLOCK;
    const size_t piece = slice_bytes();
    uint64_t file_bytes = 32, max_w = 0, ns_fd = 0;
    auto t0 = Clock::now();
    PinnedPair pin, pin_off;
    EventPair ev;
    DevScratch ws;
    uint8_t *d_buf[2] = {nullptr, nullptr};
    uint32_t *d_off[2] = {nullptr, nullptr};
    u64 *d_ctl = nullptr;
    const size_t max_blk = piece / 9 + 1;
    BRX_TRY(pin.get(piece));
    BRX_TRY(pin_off.get(max_blk * 4));
    BRX_TRY(ev.make());
    for (int i = 0; i < 2; i++) {
        BRX_TRY(ws.get(&d_buf[i], piece));
        BRX_TRY(ws.get(&d_off[i], max_blk));
    }
    BRX_TRY(ws.get(&d_ctl, 2));
    if (n) {
        BRX_TRY(d_keys.reserve(n, 0, "keys of the key file"));
        if (h.with_counts && want_counts)
            BRX_TRY(d_cnts.reserve(n, 0, "counts of the key file"));
    }
    auto run = [&]() -> int {
        BRX_HIP(hipMemsetAsync(d_ctl, 0, 16, s));
        uint64_t done = 0;   // blocks handed to the device
        size_t carry = 0;    // bytes of a block cut by the end of the piece before, at the head of the current piece
        bool used[2] = {false, false}, eof = false;
        for (uint64_t it = 0; done < n_blocks; it++) {
            const int cur = (int)(it & 1);
            uint8_t *buf = pin.p[cur];
            uint32_t *offs = (uint32_t *)pin_off.p[cur];
            // (the carried bytes were put at the head of this piece by the trip before, after its event had been waited for)
            size_t got = 0;
            if (!eof) {
                auto tr = Clock::now();
                BRX_TRY(read_upto(fd, buf + carry, piece - carry, &got));
                ns_fd += ns_since(tr);
                eof = got < piece - carry;
            }
            const size_t have = carry + got;
            size_t pos = 0;
            uint32_t nb = 0;
            while (done + nb < n_blocks && pos + 9 <= have) {
                const uint64_t b = done + nb;
                const uint32_t m = n - b * KF_BLOCK < KF_BLOCK ? (uint32_t)(n - b * KF_BLOCK) : KF_BLOCK;
                const uint32_t w = buf[pos + 8];
                if (w > KF_MAX_WIDTH) {
                    set_error("key file: width %u in block %llu (at most %u)", w, (u64)b, KF_MAX_WIDTH);
                    return BRX_ERR_FORMAT;
                }
                const size_t size = 9 + ((size_t)(m - 1) * w + 7) / 8 + (h.with_counts ? m : 0);
                if (pos + size > have)
                    break;
                offs[nb++] = (uint32_t)pos;
                pos += size;
                max_w = w > max_w ? w : max_w;
            }
            if (!nb) { // (a piece holds at least one whole block: the stream has ended)
                set_error("key file: truncated stream: it ends in block %llu of %llu", (u64)done, (u64)n_blocks);
                return BRX_ERR_FORMAT;
            }
            file_bytes += pos;
            BRX_HIP(hipMemcpyAsync(d_buf[cur], buf, pos, hipMemcpyHostToDevice, s));
            BRX_HIP(hipMemcpyAsync(d_off[cur], offs, (size_t)nb * 4, hipMemcpyHostToDevice, s));
            {
                KernelTimer kt("key_unpack", s);
                unpack_kernel<<<read_grid((nb + 3u) / 4u, 256u * 16u), 256, 0, s>>>(d_buf[cur], d_off[cur], nb, done, n, set_nbits(h.k),
                                                                                   h.with_counts ? 1u : 0u, h.floor > 1 ? h.floor : 1u, d_keys,
                                                                                   d_cnts, d_ctl, (uint32_t *)(d_ctl + 1));
                BRX_HIP(hipGetLastError());
            }
            BRX_HIP(hipEventRecord(ev.e[cur], s));
            used[cur] = true;
            done += nb;
            // the rest of this piece opens the next one, once the device is through with that one
            carry = have - pos;
            if (used[cur ^ 1])
                BRX_HIP(hipEventSynchronize(ev.e[cur ^ 1]));
            if (carry)
                memcpy(pin.p[cur ^ 1], buf + pos, carry);
        }
        if (carry) {
            set_error("key file: trailing bytes behind the last block");
            return BRX_ERR_FORMAT;
        }
        if (!eof) {
            uint8_t one;
            size_t got = 0;
            auto tr = Clock::now();
            BRX_TRY(read_upto(fd, &one, 1, &got));
            ns_fd += ns_since(tr);
            if (got) {
                set_error("key file: trailing bytes behind the last block");
                return BRX_ERR_FORMAT;
            }
        }
        if (n_blocks > 1) {
            KernelTimer kt("key_unpack", s);
            order_check_kernel<<<read_grid((n_blocks + 255) / 256, 256u * 16u), 256, 0, s>>>(d_keys, n_blocks, (uint32_t *)(d_ctl + 1));
            BRX_HIP(hipGetLastError());
        }
        u64 ctl[2] = {0, 0};
        BRX_HIP(hipMemcpyAsync(ctl, d_ctl, 16, hipMemcpyDeviceToHost, s));
        BRX_HIP(hipStreamSynchronize(s));
        const uint32_t bad = (uint32_t)ctl[1];
        if (bad & ERR_KEY) {
            set_error("key file: a key is not below 2^%d (k=%d)", 2 * h.k - 1, h.k);
            return BRX_ERR_FORMAT;
        }
        if (bad & ERR_ORDER) {
            set_error("key file: a block does not start above the key before it");
            return BRX_ERR_FORMAT;
        }
        if (bad & ERR_COUNT) {
            set_error("key file: a count of 0, or a count below the file's floor %d", (int)h.floor);
            return BRX_ERR_FORMAT;
        }
        if (ctl[0] != h.key_sum) {
            set_error("key file: the key sum does not match (header %llu, keys %llu)", (u64)h.key_sum, ctl[0]);
            return BRX_ERR_FORMAT;
        }
        return BRX_OK;
    };
    const int st = run();
    const hipError_t e = hipStreamSynchronize(s); // the pieces and the scratch are released below
    st8[1] = file_bytes;
    st8[2] = n_blocks;
    st8[3] = max_w;
    st8[6] = ns_fd;
    st8[5] = ns_since(t0) - ns_fd;
    if (st != BRX_OK || e != hipSuccess) {
        d_keys.reset();
        d_cnts.reset();
        if (st == BRX_OK) {
            set_error("key file: unpack: %s", hipGetErrorString(e));
            return BRX_ERR_HIP;
        }
    }
    return st;
}

// appends " -- the counter has been reset ..." to the message of a failed load
void note_reset()
{
    const std::string m = brx_last_error();
    set_error("%s -- the counter has been reset (empty, floor 1)", m.c_str());
}

const char *strategy_hint(const brx_counter *c)
{
    return c->strategy == BRX_COUNT_DENSE ? "dense" : "partitioned";
}

int table_counter_only(const char *me, brx_counter *c)
{
    if (c->strategy != BRX_COUNT_TABLE) {
        set_error("%s: key files hold the counts of a table counter; this one is %s -- count with the table count strategy (BRX_COUNT_TABLE)", me,
                  strategy_hint(c));
        return BRX_ERR_UNSUPPORTED;
    }
    int world = 0, rank = 0;
    if (tab_merged(c, &world, &rank)) {
        set_error("%s: the counter was merged over %d ranks and holds the share of rank %d; shard files across ranks are not supported", me, world,
                  rank);
        return BRX_ERR_UNSUPPORTED;
    }
    return BRX_OK;
}

// The count view of a partitioned counter (the caller holds its lock and has seen part_lookup_ready) compacted into two
// arrays out of `ws`: the keys counted at least `floor` times, rising, and their count bytes; *n_out of them (none: the
// arrays stay null).  The view is only read.  Returns after `s` has been synchronised.
int list_view(const char *me, const brx_counter *c, uint8_t floor, hipStream_t s, DevScratch &ws, uint64_t **d_keys, uint8_t **d_cnts,
              uint64_t *n_out)
{
    *d_keys = nullptr;
    *d_cnts = nullptr;
    *n_out = 0;
    const uint16_t *vkeys = nullptr;
    const uint8_t *vcnts = nullptr;
    const uint64_t *voff = nullptr;
    uint64_t n_buckets = 0, n_pos = 0;
    if (!part_lookup_view(c, &vkeys, &vcnts, &voff) || !part_lookup_shape(c, &n_buckets, &n_pos)) {
        set_error("%s: the count view is gone", me);
        return BRX_ERR_HIP;
    }
    if (!vkeys || !n_pos || !n_buckets)
        return BRX_OK; // nothing was counted
    if (((uintptr_t)vkeys & 7u) || ((uintptr_t)vcnts & 3u)) { // (the pool hands out aligned blocks: four positions per load)
        set_error("%s: the count view is not aligned", me);
        return BRX_ERR_HIP;
    }
    // buckets per wave: enough wave chunks to fill the device where there are few buckets (k = 9: 32 of them), whole
    // groups and 16 offset loads per chunk where there are many (k = 21: 2^29 buckets, 532 611 sums to scan)
    uint64_t per_wave = (n_buckets + 16383ull) / 16384ull;
    if (per_wave > VC_GROUP)
        per_wave = (per_wave + VC_GROUP - 1) / VC_GROUP * VC_GROUP;
    if (per_wave > VC_GROUP * VC_MAX_GROUPS)
        per_wave = VC_GROUP * VC_MAX_GROUPS;
    const uint64_t n_wchunks = (n_buckets + per_wave - 1) / per_wave;
    const uint64_t n_sums = (n_wchunks + SCAN_CHUNK - 1) / SCAN_CHUNK;
    u64 *d_part = nullptr, *d_sums = nullptr;
    BRX_TRY(ws.get(&d_part, n_wchunks));
    BRX_TRY(ws.get(&d_sums, n_sums + 1));
    const uint32_t grid = read_grid((n_wchunks + 3ull) / 4ull, 256u * 16u);
    {
        KernelTimer kt("key_list", s);
        view_count_kernel<<<grid, 256, 0, s>>>(vkeys, vcnts, voff, n_buckets, (uint32_t)per_wave, n_wchunks, floor, d_part);
        BRX_HIP(hipGetLastError());
        BRX_TRY(scan_exclusive(d_part, n_wchunks, d_sums, s));
    }
    u64 total = 0;
    BRX_HIP(hipMemcpyAsync(&total, d_sums + n_sums, 8, hipMemcpyDeviceToHost, s));
    BRX_HIP(hipStreamSynchronize(s));
    if (total > n_pos) {
        set_error("%s: %llu entries kept from a count view of %llu positions", me, total, (u64)n_pos);
        return BRX_ERR_HIP;
    }
    if (!total)
        return BRX_OK;
    BRX_TRY(ws.get(d_keys, total));
    BRX_TRY(ws.get(d_cnts, total));
    {
        KernelTimer kt("key_list", s);
        // (BRX_VIEW_WIDE_SPAN, read per call: the tests send small groups down the path of a group that spans 2^32 positions)
        const uint32_t e_span = env_u32("BRX_VIEW_WIDE_SPAN", 0u);
        view_write_kernel<<<grid, 256, 0, s>>>(vkeys, vcnts, voff, n_buckets, (uint32_t)per_wave, n_wchunks, floor,
                                               e_span ? (uint64_t)e_span : 1ull << 32, d_part, *d_keys, *d_cnts, total);
        BRX_HIP(hipGetLastError());
    }
    BRX_HIP(hipStreamSynchronize(s));
    *n_out = total;
    return BRX_OK;
}

// The listing half of a save, for brx_counter_save_fd and brx_counts_from_counter (the caller holds the counter's lock and
// has made its device current): the k-mers counted at least *floor = max(min_count, 1, the counter's floor) times, rising,
// with their count bytes, in two arrays out of `ws` (none: the arrays stay null).  A partitioned counter compacts its count
// view and is never floored, a table counter is listed and sorted; the refusals are the save's.  The counter is only read.
// Joins the counter's stream `s`; returns after `s` has been synchronised.
int counter_list(const char *me, brx_counter *c, uint8_t min_count, hipStream_t s, DevScratch &ws, uint64_t **d_keys, uint8_t **d_cnts,
                 uint64_t *n_out, uint8_t *floor)
{
    *d_keys = nullptr;
    *d_cnts = nullptr;
    *n_out = 0;
    if (min_count < 1)
        min_count = 1;
    if (c->strategy == BRX_COUNT_SORTED) {
        // the count view is the file's content in the file's order: compacted, packed, written; never floored
        if (!part_lookup_ready(c)) {
            set_error("%s: a partitioned counter saves its count view: build it first (brx_counter_lookup_prepare; every call that "
                      "counts, finishes or resets drops it), or count with the table count strategy (BRX_COUNT_TABLE)", me);
            return BRX_ERR_UNSUPPORTED;
        }
        BRX_HIP(counter_join(c, s));
        *floor = min_count;
        return list_view(me, c, min_count, s, ws, d_keys, d_cnts, n_out);
    }
    BRX_TRY(table_counter_only(me, c));
    BRX_HIP(counter_join(c, s));
    const uint8_t have = tab_floor(c);
    *floor = have > min_count ? have : min_count;
    uint64_t info[4];
    BRX_TRY(tab_info(c, info, s));
    const uint64_t *lines = nullptr;
    const uint32_t *counts = nullptr;
    uint32_t log_lines = 0, m = 0;
    tab_view(c, &lines, &counts, &log_lines, &m);
    const uint64_t cap = lines ? info[2] : 0;
    if (!cap)
        return BRX_OK;
    u64 *d_n = nullptr;
    BRX_TRY(ws.get(d_keys, cap));
    BRX_TRY(ws.get(d_cnts, cap));
    BRX_TRY(ws.get(&d_n, 1));
    BRX_HIP(hipMemsetAsync(d_n, 0, 8, s));
    const uint64_t n_slots = 8ull << log_lines;
    BRX_TRY(table_list(lines, counts, n_slots, *floor, *d_keys, *d_cnts, cap, d_n, s));
    u64 got = 0;
    BRX_HIP(hipMemcpyAsync(&got, d_n, 8, hipMemcpyDeviceToHost, s));
    BRX_HIP(hipStreamSynchronize(s));
    if (got > cap) {
        set_error("%s: %llu entries listed from a table of %llu k-mers", me, got, (u64)cap);
        return BRX_ERR_HIP;
    }
    *n_out = got;
    return sort_pairs(*d_keys, *d_cnts, got, (uint32_t)(2 * c->k - 1), s);
}

} // namespace

// ---- what set algebra (brx_setops.hip) shares with the key files ------------------------------------------------------------
namespace brx {

uint64_t keys_scan_sums(uint64_t n) { return (n + SCAN_CHUNK - 1) / SCAN_CHUNK; }
int keys_scan_exclusive(unsigned long long *d_data, uint64_t n, unsigned long long *d_sums, hipStream_t s) { return scan_exclusive(d_data, n, d_sums, s); }
int keys_sort(uint64_t *d_keys, uint8_t *d_pay, uint64_t n, uint32_t key_bits, hipStream_t s) { return sort_pairs(d_keys, d_pay, n, key_bits, s); }
int table_list(const uint64_t *lines, const uint32_t *counts, uint64_t n_entries, uint32_t min_count, uint64_t *d_keys, uint8_t *d_cnts,
               uint64_t cap, unsigned long long *d_n, hipStream_t s)
{
    KernelTimer kt("key_list", s);
    table_list_kernel<<<grid_of(n_entries, LIST_CHUNK), 256, 0, s>>>(lines, counts, n_entries, min_count, d_keys, d_cnts, cap, d_n);
    BRX_HIP(hipGetLastError());
    return BRX_OK;
}

int set_build_from_keys(brx_set *set, DevBuf<uint64_t> &d_keys, uint64_t n_keys, hipStream_t s, const char *me)
{
    // the keys become the set's key list: what a finish leaves
    BRX_TRY(set->d_keylist_n.reserve(1, 0, "key list counter"));
    const u64 n = n_keys;
    BRX_HIP(hipMemcpyAsync(set->d_keylist_n, &n, 8, hipMemcpyHostToDevice, s));
    BRX_HIP(hipStreamSynchronize(s));
    set->d_keylist = std::move(d_keys);
    keylist_mark(set, true, true); // (in order: the next listing needs no sort)
    if (set->sparse) {
        BRX_TRY(index_build_from_keys(set, set->d_keylist, n_keys, 0, 0, s));
    } else {
        bits_mark(set, false); // (nothing written yet)
        BRX_TRY(ensure_bits(set, s, me));
        if (!index_wanted(set->k)) { // as after a finish at this k: the bits are the set
            keylist_mark(set, false);
            set->d_keylist.reset();
        }
    }
    return BRX_OK;
}

} // namespace brx

extern "C" {

int brx_sort_keys_device(uint64_t *d_keys, uint8_t *d_payload, uint64_t n, uint32_t key_bits, void *stream)
{
    if ((!d_keys && n) || key_bits < 1 || key_bits > 64) {
        set_error("brx_sort_keys_device: null keys, or key_bits=%u outside 1..64", key_bits);
        return BRX_ERR_ARG;
    }
    return sort_pairs(d_keys, d_payload, n, key_bits, (hipStream_t)stream);
}

int brx_counter_floor(brx_counter_t *c, uint8_t *floor)
{
    if (!c || !floor) {
        set_error("brx_counter_floor: null counter / floor");
        return BRX_ERR_ARG;
    }
    std::lock_guard<std::mutex> g(c->mu);
    *floor = c->strategy == BRX_COUNT_TABLE ? tab_floor(c) : 1;
    return BRX_OK;
}

int brx_counter_save_fd(brx_counter_t *c, uint8_t min_count, int out_fd, uint64_t *stats8)
{
    const char *me = "brx_counter_save_fd";
    if (!c || out_fd < 0) {
        set_error("%s: null counter or bad descriptor", me);
        return BRX_ERR_ARG;
    }
    uint64_t st8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto t0 = Clock::now();
    BRX_TRY(use_device(c->device));
    std::lock_guard<std::mutex> g(c->mu);
    hipStream_t s = c->stream;
    DevScratch ws;
    uint64_t *d_keys = nullptr;
    uint8_t *d_cnts = nullptr;
    uint64_t n = 0;
    uint8_t floor = 1;
    auto t1 = Clock::now();
    BRX_TRY(counter_list(me, c, min_count, s, ws, &d_keys, &d_cnts, &n, &floor));
    st8[4] = ns_since(t1);
    uint8_t one = 0; // (an empty count file still carries the flag: the counts pointer only has to be non-null)
    const int st = pack_and_write(c->k, d_keys, n ? d_cnts : &one, n, floor, out_fd, s, st8);
    st8[0] = n;
    st8[7] = ns_since(t0);
    if (stats8)
        memcpy(stats8, st8, sizeof st8);
    return st;
}

int brx_counter_load_fd(brx_counter_t *c, int in_fd, uint64_t *stats8)
{
    const char *me = "brx_counter_load_fd";
    if (!c || in_fd < 0) {
        set_error("%s: null counter or bad descriptor", me);
        return BRX_ERR_ARG;
    }
    uint64_t st8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto t0 = Clock::now();
    BRX_TRY(use_device(c->device));
    std::lock_guard<std::mutex> g(c->mu);
    BRX_TRY(table_counter_only(me, c));
    uint32_t part = 0, parts = 1;
    if (tab_slice(c, &part, &parts)) {
        set_error("%s: the counter counts slice %u of %u and a file's keys are not filtered; brx_counter_set_slice(c, 0, 1) makes it an "
                  "ordinary counter", me, part, parts);
        return BRX_ERR_ARG;
    }
    hipStream_t s = c->stream;
    BRX_HIP(counter_join(c, c->stream)); // a reset still queued on the caller's stream comes first
    if (tab_floor(c) > 1) {
        set_error("%s: the counter holds a file that kept only counts from %d up; brx_counter_reset it before loading another", me,
                  (int)tab_floor(c));
        return BRX_ERR_ARG;
    }
    // from here on a failure leaves the counter reset, never half loaded
    auto fail = [&](int st) -> int {
        if (tab_reset(c, s) == BRX_OK && hipStreamSynchronize(s) == hipSuccess)
            note_reset();
        return st;
    };
    KeyHeader h;
    int st = read_header(in_fd, &h);
    if (st != BRX_OK)
        return fail(st);
    if (h.k != c->k) { // (an argument fault: the counter is left as it was)
        set_error("%s: the file holds %d-mers, the counter counts %d-mers", me, h.k, c->k);
        return BRX_ERR_ARG;
    }
    if (!h.with_counts) {
        set_error("%s: a set file (keys without counts) cannot be loaded into a counter", me);
        return fail(BRX_ERR_FORMAT);
    }
    uint64_t info[4];
    BRX_TRY(tab_info(c, info, s));
    if (h.floor > 1 && info[2]) {
        set_error("%s: the file kept only counts from %d up and can only be loaded into an empty counter (this one holds %llu k-mers)", me,
                  (int)h.floor, (u64)info[2]);
        return BRX_ERR_ARG;
    }
    DevBuf<uint64_t> d_keys;
    DevBuf<uint8_t> d_cnts;
    st = read_blocks(in_fd, h, true, s, d_keys, d_cnts, st8);
    if (st == BRX_OK && h.n) {
        auto t1 = Clock::now();
        st = tab_merge_pairs(c, d_keys, d_cnts, h.n, s);
        st8[4] = ns_since(t1);
    }
    d_keys.reset(); // (before the counter is reset after a failure)
    d_cnts.reset();
    if (st != BRX_OK)
        return fail(st);
    if (h.floor > 1)
        tab_set_floor(c, h.floor);
    st8[0] = h.n;
    st8[7] = ns_since(t0);
    if (stats8)
        memcpy(stats8, st8, sizeof st8);
    return BRX_OK;
}

int brx_set_save_fd(const brx_set_t *set, int out_fd, uint64_t *stats8)
{
    const char *me = "brx_set_save_fd";
    if (!set || out_fd < 0) {
        set_error("%s: null set or bad descriptor", me);
        return BRX_ERR_ARG;
    }
    if (!(set->k & 1) || set->k < 5 || set->k > 31) {
        set_error("%s: key files hold odd k from 5 to 31 (k=%d)", me, set->k);
        return BRX_ERR_UNSUPPORTED;
    }
    uint64_t st8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto t0 = Clock::now();
    BRX_TRY(use_device(set->device));
    hipStream_t s = nullptr;
    BRX_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    DevBuf<uint64_t> d_keys;
    uint64_t n = 0;
    int st = set_list_keys(set, s, d_keys, &n, nullptr);
    if (st == BRX_OK)
        st = sort_pairs(d_keys, nullptr, n, (uint32_t)(2 * set->k - 1), s);
    st8[4] = ns_since(t0);
    if (st == BRX_OK)
        st = pack_and_write(set->k, d_keys, nullptr, n, 0, out_fd, s, st8);
    (void)hipStreamSynchronize(s);
    (void)hipStreamDestroy(s);
    st8[0] = n;
    st8[7] = ns_since(t0);
    if (stats8)
        memcpy(stats8, st8, sizeof st8);
    return st;
}

int brx_set_load_fd(int in_fd, int device, brx_set_t **out, uint64_t *stats8)
{
    const char *me = "brx_set_load_fd";
    if (!out || in_fd < 0) {
        set_error("%s: null out or bad descriptor", me);
        return BRX_ERR_ARG;
    }
    *out = nullptr;
    uint64_t st8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto t0 = Clock::now();
    BRX_TRY(use_device(device));
    KeyHeader h;
    BRX_TRY(read_header(in_fd, &h));
    hipStream_t s = nullptr;
    BRX_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    DevBuf<uint64_t> d_keys;
    DevBuf<uint8_t> d_cnts;
    brx_set *set = nullptr;
    int st = read_blocks(in_fd, h, false, s, d_keys, d_cnts, st8); // (the counts of a count file are checked and dropped)
    if (st == BRX_OK)
        st = set_alloc_unwritten(h.k, device, &set);
    if (st == BRX_OK) {
        auto t1 = Clock::now();
        st = set_build_from_keys(set, d_keys, h.n, s, me);
        if (st == BRX_OK)
            st8[4] = ns_since(t1);
    }
    (void)hipStreamSynchronize(s);
    (void)hipStreamDestroy(s);
    if (st != BRX_OK) {
        if (set)
            brx_set_free(set);
        return st;
    }
    *out = set;
    st8[0] = h.n;
    st8[7] = ns_since(t0);
    if (stats8)
        memcpy(stats8, st8, sizeof st8);
    return BRX_OK;
}

// ---- count lists (include/brx.h "count lists"): the entries that read and write files; the merge is brx_setops.hip's --------
int brx_counts_load_fd(int in_fd, int device, brx_counts_t **out, uint64_t *stats8)
{
    const char *me = "brx_counts_load_fd";
    if (!out || in_fd < 0) {
        set_error("%s: null out or bad descriptor", me);
        return BRX_ERR_ARG;
    }
    *out = nullptr;
    uint64_t st8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto t0 = Clock::now();
    BRX_TRY(use_device(device));
    KeyHeader h;
    BRX_TRY(read_header(in_fd, &h));
    if (!h.with_counts) {
        set_error("%s: a set file (keys without counts) cannot be loaded as a count list", me);
        return BRX_ERR_FORMAT;
    }
    hipStream_t s = nullptr;
    BRX_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    brx_counts *l = new brx_counts;
    l->k = h.k;
    l->device = device;
    l->floor = h.floor;
    l->n = h.n;
    const int st = read_blocks(in_fd, h, true, s, l->d_keys, l->d_cnts, st8);
    (void)hipStreamSynchronize(s);
    (void)hipStreamDestroy(s);
    if (st != BRX_OK) {
        delete l;
        return st;
    }
    *out = l;
    st8[0] = h.n;
    st8[7] = ns_since(t0);
    if (stats8)
        memcpy(stats8, st8, sizeof st8);
    return BRX_OK;
}

int brx_counts_from_counter(brx_counter_t *c, uint8_t min_count, brx_counts_t **out, uint64_t *stats8)
{
    const char *me = "brx_counts_from_counter";
    if (!c || !out) {
        set_error("%s: null counter or out", me);
        return BRX_ERR_ARG;
    }
    *out = nullptr;
    uint64_t st8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto t0 = Clock::now();
    BRX_TRY(use_device(c->device));
    std::lock_guard<std::mutex> g(c->mu);
    hipStream_t s = c->stream;
    DevScratch ws;
    uint64_t *d_keys = nullptr;
    uint8_t *d_cnts = nullptr;
    uint64_t n = 0;
    uint8_t floor = 1;
    BRX_TRY(counter_list(me, c, min_count, s, ws, &d_keys, &d_cnts, &n, &floor));
    st8[4] = ns_since(t0);
    // the list owns arrays of its own size (a table counter's listing is sized for every k-mer it holds)
    brx_counts *l = new brx_counts;
    l->k = c->k;
    l->device = c->device;
    l->floor = floor;
    l->n = n;
    auto copy = [&]() -> int {
        if (!n)
            return BRX_OK;
        BRX_TRY(l->d_keys.reserve(n, 0, "keys of a count list"));
        BRX_TRY(l->d_cnts.reserve(n, 0, "counts of a count list"));
        BRX_HIP(hipMemcpyAsync(l->d_keys, d_keys, n * 8, hipMemcpyDeviceToDevice, s));
        BRX_HIP(hipMemcpyAsync(l->d_cnts, d_cnts, n, hipMemcpyDeviceToDevice, s));
        BRX_HIP(hipStreamSynchronize(s)); // the listing goes back to the pool below
        return BRX_OK;
    };
    const int st = copy();
    if (st != BRX_OK) {
        (void)hipStreamSynchronize(s);
        delete l;
        return st;
    }
    *out = l;
    st8[0] = n;
    st8[7] = ns_since(t0);
    if (stats8)
        memcpy(stats8, st8, sizeof st8);
    return BRX_OK;
}

int brx_counts_save_fd(const brx_counts_t *l, uint8_t min_count, int out_fd, uint64_t *stats8)
{
    const char *me = "brx_counts_save_fd";
    if (!l || out_fd < 0) {
        set_error("%s: null count list or bad descriptor", me);
        return BRX_ERR_ARG;
    }
    uint64_t st8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto t0 = Clock::now();
    BRX_TRY(use_device(l->device));
    hipStream_t s = nullptr;
    BRX_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    const uint64_t *d_keys = l->d_keys;
    const uint8_t *d_cnts = l->d_cnts;
    uint64_t n = l->n;
    uint8_t floor = l->floor;
    DevBuf<uint64_t> d_kept;
    DevBuf<uint8_t> d_kept_cnts;
    int st = BRX_OK;
    if (min_count > floor) { // one compaction: the merge with an empty B
        floor = min_count;
        st = counts_merge(me, l->d_keys, l->d_cnts, l->n, nullptr, nullptr, 0, BRX_COUNTOP_ADD, floor, true, s, d_kept, d_kept_cnts, &n, nullptr);
        d_keys = d_kept;
        d_cnts = d_kept_cnts;
        st8[4] = ns_since(t0);
    }
    uint8_t one = 0; // (an empty count file still carries the flag: the counts pointer only has to be non-null)
    if (st == BRX_OK)
        st = pack_and_write(l->k, d_keys, n ? d_cnts : &one, n, floor, out_fd, s, st8);
    (void)hipStreamSynchronize(s);
    (void)hipStreamDestroy(s);
    st8[0] = n;
    st8[7] = ns_since(t0);
    if (stats8)
        memcpy(stats8, st8, sizeof st8);
    return st;
}

} // extern "C"
