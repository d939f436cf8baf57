// Solid coverage of reads: which bases of a batch the set supports.  No counterpart in the reference.
//
// For a read s of n bases and a set of k-mer length k (include/brx.h, "coverage"):
//   solid[i]   = KmerSet::get(s[i..i+k)) for 0 <= i <= n-k (src/set/pcon.rs:189-191; every byte coded by nuc2bit, so a byte
//                that is not ACGT is a base like any other),
//   covered[j] = some solid[i] with j-k+1 <= i <= j,
//   a run      = a maximal stretch of covered bases.
//
// One probe per k-mer of the batch, asked the way lane_mask_kernel (brx_onelane.hip) asks: 64 neighbouring positions of
// one read per wave step, so that neighbours share their index lines, through whatever holds the set (bit vector; key
// list + probe index, occupancy bits first; chained table).  Unlike that kernel this one reads the ASCII bytes of a plain
// bases / offsets batch and is cut BY POSITION: a wave takes a tile of READ_TILE positions from the work list of
// brx_tiles.hpp.
//
// Inside a wave the k-mers are indexed by their LAST base e (the DPP scan of brx_correct.hpp builds them that way):
// w[e] = solid[e-k+1].  Then covered[j] = OR of w[j .. j+k-1], which looks FORWARD: the ballot word of a step is held
// back one step, and the step's outputs come from the 128-bit window (held word, next word) -- the solid-start bits by
// one shift, the covered bits by OR-ing the window shifted by 0..k-1 in doubling steps (1, 2, 4, .. : five rounds for
// k = 31), all on wave-uniform values.  A tile starts one position early (the bit that says whether a run is open where
// it begins) and probes k-1 positions past its end (the k-mers that reach back into it): 3 % more probes at k = 31.
// Runs are 0 -> 1 transitions with that carry bit.  Per-read statistics are integer atomic adds of per-tile sums, so
// they do not depend on the launch geometry or on timing.
//
// Split form: the cover kernel also leaves the number of run starts per tile; an exclusive scan numbers the runs of the
// batch in (read, position) order, a second pass over the flags writes every run's start and -- the i-th end of a
// batch belongs to the i-th start -- its end; runs of at least min_len bases are numbered and laid out by two more
// scans, and a copy kernel moves them (brx_pieces.hpp, shared with the trusted stretches of brx_trust.hip).  The order of
// the output is fixed by those scans, never by timing.
#include "brx_correct.hpp"
#include "brx_tiles.hpp"
#include "brx_pieces.hpp"

#include <algorithm>
#include <vector>

using namespace brx;

namespace {

struct CoverArgs {
    const uint32_t *bits; // nullptr: the index is exact (lazy or sparse set)
    IdxView idx;          // lines == nullptr: every probe goes to the bit vector
    int k;
    uint32_t n_reads;
    const uint8_t *bases;
    const uint64_t *offsets;
    TileList tl;                      // work list (brx_tiles.hpp)
    // outputs, each may be null
    uint8_t *flags;
    uint8_t *masked;
    brx_cover_stats_t *stats;
    uint32_t *tile_runs;              // run starts per tile              [tile bound]
    // split form
    const uint64_t *run_base;         // exclusive scan of tile_runs      [tile bound + 1]
    PieceArgs pc;                     // the runs, what is kept of them and where it goes (brx_pieces.hpp); its bases /
                                      // offsets are the batch's
};

// set_get<IDX, LINE_BITS_IN_L2> (brx_index.hpp), kept written out for this one kernel: through the shared function
// cover_kernel<true> measured 8.7 ms per Gbp against 8.0 (profiles/batch_query_refactor.json), with the same registers
// and occupancy, where lane_mask_kernel, which asks the same way, did not change.  Same answers
// (tests/test_gpu_get_routes.py); the chain walk is the one place this copy differs: it is not bounded by the table's size.
template <bool IDX>
__device__ __forceinline__ bool cover_get(const CoverArgs &a, uint64_t km, int k, bool filter)
{
    if (!IDX)
        return probe(a.bits, km, k);
    uint64_t key;
    const uint32_t home = index_locate(a.idx, km, k, key);
    if (filter && !((a.idx.line_bits[home >> 5] >> (home & 31u)) & 1u))
        return false;
    int pr = index_probe_at(a.idx, key, home, 0u);
    for (uint32_t hop = 1; pr == 2 && !a.bits; hop++) // no bit vector: the build chained the key into the next lines
        pr = index_probe_at(a.idx, key, home, hop);
    if (pr == 2) { // the line overflowed at build time and does not hold the key: the bit vector knows
        const uint64_t h = key - 1ull;
        pr = (a.bits[h >> 5] >> (h & 31u)) & 1u;
    }
    return pr == 1;
}

// A wave per tile.
template <bool IDX>
__global__ __launch_bounds__(256) void cover_kernel(CoverArgs a)
{
    TileView t;
    unsigned long long tile;
    if (!tile_view(a.tl, a.offsets, t, tile))
        return;
    const int lane = threadIdx.x & 63;
    const uint32_t k = (uint32_t)a.k;
    const uint64_t mask = kmask(a.k);
    const uint32_t n = t.n, p0 = t.p0, p1 = t.p1;
    const uint8_t *in = a.bases + t.o0;
    const bool filter = IDX && a.idx.line_bits != nullptr && a.idx.line_shift >= 6u; // (LINE_BITS_IN_L2's rule)
    // the k-mers wanted END at e0 .. elim-1: from the base in front of the tile (is a run open there?) to the last
    // k-mer that reaches back into the tile
    const uint32_t e0 = p0 ? p0 - 1u : 0u;
    const uint32_t elim = n - p1 < k - 1u ? n : p1 + k - 1u;
    // the k-mer that ends in front of e0, from one step without probes
    uint64_t carry = 0;
    if (e0) { // (p0 >= READ_TILE: e0 - 64 lies inside the read)
        const uint32_t code = (in[e0 - 64u + (uint32_t)lane] >> 1) & 3u;
        carry = wave_carry(lane_kmer64_dpp(0, code, lane, mask));
    }
    const uint32_t steps = (p1 - e0 + 63u) / 64u; // steps with outputs; step `steps` only supplies the window's upper word
    uint64_t held = 0;     // ballot of the step before: bit l = the k-mer that ENDS at its position l is solid
    uint8_t c_held = 0;    // ... and this lane's byte of it
    uint32_t carry_cov = 0; // covered[] of the position in front of the step being written
    uint32_t n_solid = 0, n_cov = 0, n_runs = 0;
    for (uint32_t st = 0; st <= steps; st++) {
        const uint32_t eb = e0 + 64u * st;
        const uint32_t e = eb + (uint32_t)lane;
        uint64_t w = 0;
        uint8_t c = 0;
        if (eb < elim) {
            c = e < n ? in[e] : (uint8_t)0;
            const uint64_t km = lane_kmer64_dpp(carry, (c >> 1) & 3u, lane, mask);
            bool sol = false;
            if (e < elim && e + 1u >= k)
                sol = cover_get<IDX>(a, km, a.k, filter);
            w = __ballot(sol);
            carry = wave_carry(km);
        }
        if (st) {
            const uint32_t pb = eb - 64u; // positions pb .. pb+63: window = (held, w)
            const uint64_t lo = held, hi = w;
            const uint64_t S = k > 1u ? (lo >> (k - 1u)) | (hi << (65u - k)) : lo; // solid[j] = w[j + k - 1]
            uint64_t clo = lo, chi = hi;
            for (uint32_t have = 1; have < k;) { // OR of the window shifted by 0 .. have-1, doubled
                const uint32_t sh = have < k - have ? have : k - have;
                clo |= (clo >> sh) | (chi << (64u - sh));
                chi |= chi >> sh;
                have += sh;
            }
            const uint64_t Cw = clo;
            // the lanes whose position belongs to the tile: from p0 (lane 1 of the first step when p0 > 0) to p1 - 1
            const uint32_t first = p0 > pb ? p0 - pb : 0u, end = p1 - pb;
            const uint64_t own = (end >= 64u ? ~0ull : (1ull << end) - 1ull) & ~((1ull << first) - 1ull);
            n_solid += (uint32_t)__popcll(S & own);
            n_cov += (uint32_t)__popcll(Cw & own);
            n_runs += (uint32_t)__popcll(Cw & ~((Cw << 1) | carry_cov) & own);
            carry_cov = (uint32_t)(Cw >> 63);
            if ((own >> lane) & 1ull) {
                const uint32_t cov = (uint32_t)(Cw >> lane) & 1u;
                const uint64_t at = t.o0 + pb + (uint32_t)lane;
                if (a.flags)
                    a.flags[at] = (uint8_t)((((uint32_t)(S >> lane) & 1u) ? BRX_COVER_SOLID_START : 0u) | (cov ? BRX_COVER_COVERED : 0u));
                if (a.masked) {
                    const uint8_t l = c_held | 0x20u;
                    const bool letter = l >= (uint8_t)'a' && l <= (uint8_t)'z';
                    a.masked[at] = letter ? (cov ? (uint8_t)(c_held & ~0x20u) : l) : c_held;
                }
            }
        }
        held = w;
        c_held = c;
    }
    if (a.stats && lane < 4) {
        const uint32_t kmers = (p0 == 0u && n >= k) ? n - k + 1u : 0u;
        const uint32_t v = lane == 0 ? kmers : (lane == 1 ? n_solid : (lane == 2 ? n_cov : n_runs));
        if (v)
            atomicAdd(reinterpret_cast<uint32_t *>(a.stats + t.r) + lane, v);
    }
    if (a.tile_runs && lane == 0)
        a.tile_runs[tile] = n_runs;
}

// The runs of the batch, numbered in (read, position) order: a wave per tile reads the covered bits of its positions
// and writes the starts it holds and the ends it SEES -- a 1 -> 0 step at position j ends a run at j-1, the end of a read
// ends an open one.  The first end a tile sees has the number of its first start, less one when a run is open in front
// of it.
__global__ __launch_bounds__(256) void cover_runs_kernel(CoverArgs a)
{
    TileView t;
    unsigned long long tile;
    if (!tile_view(a.tl, a.offsets, t, tile))
        return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint8_t *fl = a.flags + t.o0;
    uint32_t carry = t.p0 ? (uint32_t)(fl[t.p0 - 1u] >> 1) & 1u : 0u; // (BRX_COVER_COVERED = 2)
    uint64_t s_at = a.run_base[tile], e_at = s_at - carry;
    for (uint32_t pb = t.p0; pb < t.p1; pb += 64u) {
        const uint32_t j = pb + lane;
        const bool valid = j < t.p1;
        const uint64_t Cw = __ballot(valid && ((fl[valid ? j : 0u] >> 1) & 1u));
        const uint64_t V = __ballot(valid);
        const uint64_t prev = (Cw << 1) | carry;
        const uint64_t starts = Cw & ~prev, falls = ~Cw & prev & V;
        const uint64_t below = (1ull << lane) - 1ull;
        if ((starts >> lane) & 1ull) {
            const uint64_t i = s_at + (uint32_t)__popcll(starts & below);
            a.pc.run_read[i] = t.r;
            a.pc.run_start[i] = j;
        }
        if ((falls >> lane) & 1ull)
            a.pc.run_end[e_at + (uint32_t)__popcll(falls & below)] = j - 1u;
        s_at += (uint32_t)__popcll(starts);
        e_at += (uint32_t)__popcll(falls);
        carry = (uint32_t)(Cw >> 63);
        if (pb + 64u >= t.p1 && t.p1 - pb < 64u) // the tile ends inside this step: its last position's bit
            carry = (uint32_t)(Cw >> (t.p1 - pb - 1u)) & 1u;
    }
    if (t.p1 == t.n && carry && lane == 0u)
        a.pc.run_end[e_at] = t.n - 1u;
}

// how the kernels reach the set.  Never writes the bit vector: a lazy one stays lazy, the index answers for it
int cover_view(const brx_set *set, hipStream_t s, CoverArgs &a)
{
    BRX_TRY(index_ensure(set, s));
    a.k = set->k;
    // (BRX_LINE_BITS read per call -- A/B and fuzzers: 0 = do not consult the occupancy bits)
    const SetView v = set_view(set, env_u32("BRX_LINE_BITS", 1u) != 0u);
    a.bits = v.bits;
    a.idx = v.idx;
    if (!a.bits && !a.idx.lines) {
        set_error("cover: the set (k=%d) has neither a bit vector nor an index", set->k);
        return BRX_ERR_ARG;
    }
    return BRX_OK;
}

int check_batch(const char *what, const brx_set_t *set, const void *d_bases, const uint64_t *d_offsets, uint32_t n_reads, uint64_t total_bases)
{
    if (!set) {
        set_error("%s: null set", what);
        return BRX_ERR_ARG;
    }
    if (set->k < 1 || set->k > 31) {
        set_error("%s: k=%d (a k-mer must fit 62 bits)", what, set->k);
        return BRX_ERR_ARG;
    }
    return check_batch_args(what, d_bases, d_offsets, n_reads, total_bases);
}

// work list + cover kernel.  `tile_bound` tiles at most (known without asking the device)
int cover_launch(const brx_set *set, CoverArgs &a, uint64_t total_bases, DevScratch &sc, uint64_t &tile_bound, hipStream_t s)
{
    BRX_TRY(cover_view(set, s, a));
    BRX_TRY(tile_list_enqueue(a.tl, a.offsets, a.n_reads, total_bases, "cover", "cover_tiles", sc, tile_bound, s));
    if (a.stats)
        BRX_HIP(hipMemsetAsync(a.stats, 0, (uint64_t)a.n_reads * sizeof(brx_cover_stats_t), s));
    if (a.tile_runs)
        BRX_HIP(hipMemsetAsync(a.tile_runs, 0, tile_bound * 4, s));
    {
        KernelTimer t("cover", s);
        const uint32_t grid = (uint32_t)((tile_bound + 3ull) / 4ull);
        if (a.idx.lines)
            cover_kernel<true><<<grid, 256, 0, s>>>(a);
        else
            cover_kernel<false><<<grid, 256, 0, s>>>(a);
    }
    BRX_HIP(hipGetLastError());
    return BRX_OK;
}

} // namespace

extern "C" {

int brx_set_cover_batch_device(const brx_set_t *set, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads,
                               uint64_t total_bases, uint8_t *d_flags, uint8_t *d_masked, brx_cover_stats_t *d_stats, void *stream)
{
    BRX_TRY(check_batch("brx_set_cover_batch_device", set, d_bases, d_offsets, n_reads, total_bases));
    BRX_TRY(use_device(set->device));
    if (!n_reads || (!d_flags && !d_masked && !d_stats))
        return BRX_OK;
    hipStream_t s = (hipStream_t)stream;
    DevScratch sc;
    CoverArgs a{};
    a.n_reads = n_reads;
    a.bases = d_bases;
    a.offsets = d_offsets;
    a.flags = d_flags;
    a.masked = d_masked;
    a.stats = d_stats;
    uint64_t tile_bound = 0;
    int st = cover_launch(set, a, total_bases, sc, tile_bound, s);
    // the scratch goes back to the pool when this returns: nothing of the call may still be running then
    const hipError_t e = hipStreamSynchronize(s);
    if (st == BRX_OK && e != hipSuccess) {
        set_error("brx_set_cover_batch_device: %s", hipGetErrorString(e));
        st = BRX_ERR_HIP;
    }
    return st;
}

int brx_set_cover_batch(const brx_set_t *set, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads, uint8_t *flags,
                        uint8_t *masked, brx_cover_stats_t *stats)
{
    if (n_reads && !offsets) {
        set_error("brx_set_cover_batch: null offsets");
        return BRX_ERR_ARG;
    }
    const uint64_t total = n_reads ? offsets[n_reads] : 0;
    BRX_TRY(check_batch("brx_set_cover_batch", set, bases, offsets, n_reads, total));
    BRX_TRY(check_offsets("brx_set_cover_batch", offsets, n_reads));
    BRX_TRY(use_device(set->device));
    if (!n_reads || (!flags && !masked && !stats))
        return BRX_OK;
    DevScratch sc;
    uint8_t *d_bases = nullptr, *d_flags = nullptr, *d_masked = nullptr;
    uint64_t *d_off = nullptr;
    brx_cover_stats_t *d_stats = nullptr;
    BRX_TRY(sc.get(&d_bases, total));
    BRX_TRY(sc.get(&d_off, (uint64_t)n_reads + 1));
    if (flags)
        BRX_TRY(sc.get(&d_flags, total));
    if (stats)
        BRX_TRY(sc.get(&d_stats, n_reads));
    if (masked)
        d_masked = d_bases; // case is rewritten in place
    hipStream_t s = nullptr;
    if (total)
        BRX_HIP(hipMemcpyAsync(d_bases, bases, total, hipMemcpyHostToDevice, s));
    BRX_HIP(hipMemcpyAsync(d_off, offsets, ((uint64_t)n_reads + 1) * 8, hipMemcpyHostToDevice, s));
    BRX_TRY(brx_set_cover_batch_device(set, d_bases, d_off, n_reads, total, d_flags, d_masked, d_stats, s));
    if (flags && total)
        BRX_HIP(hipMemcpyAsync(flags, d_flags, total, hipMemcpyDeviceToHost, s));
    if (masked && total)
        BRX_HIP(hipMemcpyAsync(masked, d_masked, total, hipMemcpyDeviceToHost, s));
    if (stats)
        BRX_HIP(hipMemcpyAsync(stats, d_stats, (uint64_t)n_reads * sizeof(brx_cover_stats_t), hipMemcpyDeviceToHost, s));
    BRX_HIP(hipStreamSynchronize(s));
    return BRX_OK;
}

int brx_set_cover_split_batch_device(const brx_set_t *set, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads,
                                     uint64_t total_bases, uint32_t min_len, uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_offsets,
                                     uint32_t *d_piece_read, uint64_t *d_piece_start, uint32_t piece_cap, uint32_t *n_pieces,
                                     uint64_t *out_total, void *stream)
{
    const char *me = "brx_set_cover_split_batch_device";
    BRX_TRY(check_batch(me, set, d_bases, d_offsets, n_reads, total_bases));
    if (!n_pieces || !out_total) {
        set_error("%s: null n_pieces / out_total", me);
        return BRX_ERR_ARG;
    }
    *n_pieces = 0;
    *out_total = 0;
    BRX_TRY(use_device(set->device));
    hipStream_t s = (hipStream_t)stream;
    if (!n_reads) {
        if (d_out_offsets)
            BRX_HIP(hipMemsetAsync(d_out_offsets, 0, 8, s));
        BRX_HIP(hipStreamSynchronize(s));
        return BRX_OK;
    }
    DevScratch sc;
    CoverArgs a{};
    a.n_reads = n_reads;
    a.bases = d_bases;
    a.offsets = d_offsets;
    a.pc.min_len = min_len;
    a.pc.bases = d_bases;
    a.pc.offsets = d_offsets;
    uint64_t tile_bound = total_bases / READ_TILE + n_reads;
    uint64_t *run_base = nullptr, *tmp = nullptr;
    unsigned long long *d_totals = nullptr; // runs, pieces, bytes
    BRX_TRY(sc.get(&a.flags, total_bases));
    BRX_TRY(sc.get(&a.tile_runs, tile_bound));
    BRX_TRY(sc.get(&run_base, tile_bound + 1));
    BRX_TRY(sc.get(&d_totals, 3));
    if (tile_bound >= 0xffffffffull) {
        set_error("%s: batch too large for one call", me);
        return BRX_ERR_ARG;
    }
    BRX_TRY(sc.get(&tmp, scan_tmp_bytes((uint32_t)tile_bound) / 8 + 1));
    int st = cover_launch(set, a, total_bases, sc, tile_bound, s);
    unsigned long long h_tot[3] = {0, 0, 0};
    if (st == BRX_OK) {
        st = exclusive_scan_lens(a.tile_runs, (uint32_t)tile_bound, tmp, run_base, d_totals, s);
        a.run_base = run_base;
        a.pc.n_runs = d_totals;
    }
    auto sync = [&](int st_in) -> int {
        const hipError_t e = hipStreamSynchronize(s);
        if (st_in == BRX_OK && e != hipSuccess) {
            set_error("%s: %s", me, hipGetErrorString(e));
            return BRX_ERR_HIP;
        }
        return st_in;
    };
    if (st == BRX_OK && hipMemcpyAsync(h_tot, d_totals, 8, hipMemcpyDeviceToHost, s) != hipSuccess)
        st = BRX_ERR_HIP;
    st = sync(st);
    if (st != BRX_OK)
        return st;
    const uint64_t n_runs = h_tot[0];
    if (n_runs >= 0xffffffffull) {
        set_error("%s: %llu runs in one batch", me, (unsigned long long)n_runs);
        return BRX_ERR_ARG;
    }
    if (n_runs) {
        uint64_t *piece_of = nullptr, *byte_of = nullptr, *tmp2 = nullptr;
        auto enqueue = [&]() -> int {
            BRX_TRY(sc.get(&a.pc.run_read, n_runs));
            BRX_TRY(sc.get(&a.pc.run_start, n_runs));
            BRX_TRY(sc.get(&a.pc.run_end, n_runs));
            BRX_TRY(sc.get(&a.pc.keep_flag, n_runs));
            BRX_TRY(sc.get(&a.pc.keep_len, n_runs));
            BRX_TRY(sc.get(&piece_of, n_runs + 1));
            BRX_TRY(sc.get(&byte_of, n_runs + 1));
            BRX_TRY(sc.get(&tmp2, scan_tmp_bytes((uint32_t)n_runs) / 8 + 1));
            {
                KernelTimer t("cover_runs", s);
                cover_runs_kernel<<<(uint32_t)((tile_bound + 3ull) / 4ull), 256, 0, s>>>(a);
                piece_keep_launch(a.pc, n_runs, s);
            }
            BRX_TRY(exclusive_scan_lens(a.pc.keep_flag, (uint32_t)n_runs, tmp2, piece_of, d_totals + 1, s));
            BRX_TRY(exclusive_scan_lens(a.pc.keep_len, (uint32_t)n_runs, tmp2, byte_of, d_totals + 2, s));
            BRX_HIP(hipGetLastError());
            BRX_HIP(hipMemcpyAsync(h_tot + 1, d_totals + 1, 16, hipMemcpyDeviceToHost, s));
            return BRX_OK;
        };
        st = sync(enqueue());
        if (st != BRX_OK)
            return st;
        a.pc.piece_of = piece_of;
        a.pc.byte_of = byte_of;
    }
    const uint64_t pieces = h_tot[1], bytes = h_tot[2];
    *n_pieces = (uint32_t)pieces;
    *out_total = bytes;
    if (pieces > piece_cap || bytes > out_cap) {
        set_error("%s: %llu pieces of %llu bytes do not fit piece_cap=%u, out_cap=%llu", me, (unsigned long long)pieces,
                  (unsigned long long)bytes, piece_cap, (unsigned long long)out_cap);
        return BRX_ERR_OVERFLOW;
    }
    if (!d_out_offsets || (bytes && !d_out)) {
        set_error("%s: null d_out / d_out_offsets", me);
        return BRX_ERR_ARG;
    }
    if (!n_runs) {
        BRX_HIP(hipMemsetAsync(d_out_offsets, 0, 8, s));
        return sync(BRX_OK);
    }
    a.pc.out = d_out;
    a.pc.out_offsets = d_out_offsets;
    a.pc.piece_read = d_piece_read;
    a.pc.piece_start = d_piece_start;
    {
        KernelTimer t("cover_copy", s);
        piece_copy_launch(a.pc, n_runs, s);
    }
    st = hipGetLastError() == hipSuccess ? BRX_OK : BRX_ERR_HIP;
    return sync(st);
}

int brx_set_cover_split_batch(const brx_set_t *set, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads, uint32_t min_len,
                              uint8_t **out_bases, uint64_t **out_offsets, uint32_t **piece_read, uint64_t **piece_start,
                              uint32_t *n_pieces)
{
    const char *me = "brx_set_cover_split_batch";
    if ((n_reads && !offsets) || !out_bases || !out_offsets || !piece_read || !piece_start || !n_pieces) {
        set_error("%s: null argument", me);
        return BRX_ERR_ARG;
    }
    *out_bases = nullptr;
    *out_offsets = nullptr;
    *piece_read = nullptr;
    *piece_start = nullptr;
    *n_pieces = 0;
    const uint64_t total = n_reads ? offsets[n_reads] : 0;
    BRX_TRY(check_batch(me, set, bases, offsets, n_reads, total));
    BRX_TRY(check_offsets(me, offsets, n_reads));
    BRX_TRY(use_device(set->device));
    // the bounds of include/brx.h: no retry
    const uint64_t unit = (uint64_t)std::max<uint32_t>(std::max<uint32_t>((uint32_t)set->k, min_len), 1u) + 1ull;
    const uint64_t piece_cap = (uint64_t)n_reads + total / unit;
    if (piece_cap > 0xffffffffull) {
        set_error("%s: batch too large for one call", me);
        return BRX_ERR_ARG;
    }
    DevScratch sc;
    uint8_t *d_bases = nullptr, *d_out = nullptr;
    uint64_t *d_off = nullptr, *d_oo = nullptr, *d_ps = nullptr;
    uint32_t *d_pr = nullptr;
    BRX_TRY(sc.get(&d_bases, total));
    BRX_TRY(sc.get(&d_off, (uint64_t)n_reads + 1));
    BRX_TRY(sc.get(&d_out, total));
    BRX_TRY(sc.get(&d_oo, piece_cap + 1));
    BRX_TRY(sc.get(&d_pr, piece_cap));
    BRX_TRY(sc.get(&d_ps, piece_cap));
    hipStream_t s = nullptr;
    if (total)
        BRX_HIP(hipMemcpyAsync(d_bases, bases, total, hipMemcpyHostToDevice, s));
    if (n_reads)
        BRX_HIP(hipMemcpyAsync(d_off, offsets, ((uint64_t)n_reads + 1) * 8, hipMemcpyHostToDevice, s));
    uint32_t np = 0;
    uint64_t bytes = 0;
    BRX_TRY(brx_set_cover_split_batch_device(set, d_bases, d_off, n_reads, total, min_len, d_out, total, d_oo, d_pr, d_ps,
                                             (uint32_t)piece_cap, &np, &bytes, s));
    uint8_t *ob = (uint8_t *)host_buf_acquire(bytes ? bytes : 1);
    uint64_t *oo = (uint64_t *)host_buf_acquire(((uint64_t)np + 1) * 8);
    uint32_t *pr = (uint32_t *)host_buf_acquire(((uint64_t)np + 1) * 4);
    uint64_t *ps = (uint64_t *)host_buf_acquire(((uint64_t)np + 1) * 8);
    hipError_t e = (ob && oo && pr && ps) ? hipSuccess : hipErrorOutOfMemory;
    if (e == hipSuccess && bytes)
        e = hipMemcpyAsync(ob, d_out, bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(oo, d_oo, ((uint64_t)np + 1) * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && np)
        e = hipMemcpyAsync(pr, d_pr, (uint64_t)np * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && np)
        e = hipMemcpyAsync(ps, d_ps, (uint64_t)np * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess)
        e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        host_buf_release(ob);
        host_buf_release(oo);
        host_buf_release(pr);
        host_buf_release(ps);
        set_error("%s: %s", me, hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? BRX_ERR_NOMEM : BRX_ERR_HIP;
    }
    *out_bases = ob;
    *out_offsets = oo;
    *piece_read = pr;
    *piece_start = ps;
    *n_pieces = np;
    return BRX_OK;
}

} // extern "C"
