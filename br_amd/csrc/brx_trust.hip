// Trusted stretches of reads: the parts of a batch worth counting.  No counterpart in the reference.
//
// For a read s of n bytes, qualities q (Phred+33, may be absent), a floor and acgt_only (include/brx.h, "trusted stretches"):
//   letter[j]  = s[j] is one of ACGTacgt,
//   good[j]    = no floor, or no qualities, or q[j] >= 33 + floor,
//   trusted[j] = (letter[j] or not acgt_only) and good[j],
//   a stretch  = a maximal run of trusted bases.
//
// trusted[] is a function of position j alone -- no k-window, no probe -- so the batch is cut BY POSITION with the work list
// of brx_tiles.hpp, a wave per tile of READ_TILE positions, and a tile learns whether a stretch is open where it begins by
// looking at position p0 - 1 itself.  The kernel streams 2 bytes per base in: a lane takes 16 ALIGNED bytes of bases and 16
// of qualities per step (64 lanes = 1024 bytes: a tile is one step, two when it does not start on a 16-byte border).  Reads
// start at any byte, and bases and qualities at different ones, so
//   - all bits of a tile live on the 16-byte grid of its bases: bit i of the tile is the byte at (first base & ~15) + i, the
//     tile's own bits are [mb, mb + len) and everything outside is masked off -- the head and the tail cost a mask, no loop;
//   - a lane's 16 quality bits sit e = 0 .. 15 bits further along that grid: they are put together from its own mask and the
//     mask of the lane below it (the last lane's goes to lane 0 of the next step; the piece in front of the first step is
//     read once, by all lanes alike, when it holds a position of the tile).
// Letters and floors are tested four bytes at a time in a 32-bit register (bit 7 of every byte answers), the four answers
// gathered with one multiply.  An aligned 16-byte piece that holds one byte of the batch lies in that byte's page, so the
// masked-off bytes it brings along are never outside mapped memory.
//
// Pass 1 per tile: the masks, the stretch starts of the tile (0 -> 1 steps, the bit in front of the tile carried in) and the
// read's statistics by integer atomic adds of per-tile sums.  A scan of the tile counts numbers the stretches of the batch in
// (read, position) order.  Pass 2 recomputes the masks -- 2 bytes per position again, cheaper than storing and reloading a
// flag byte -- and writes every start and the ends it SEES: the i-th end of the batch belongs to the i-th start, exactly as
// in cover_runs_kernel.  Keep (len >= min_len), the two layout scans and the copy are the coverage split's (brx_pieces.hpp).
#include "brx_tiles.hpp"
#include "brx_pieces.hpp"

#include <algorithm>

using namespace brx;

namespace {

struct TrustArgs {
    const uint8_t *bases;
    const uint8_t *quals;   // nullptr: no qualities, or no floor
    const uint64_t *offsets;
    uint32_t n_reads;
    uint32_t thr;           // 33 + floor (34 .. 126)
    uint32_t any_byte;      // 0xffff when acgt_only is off: every byte passes for a letter
    TileList tl;            // work list (brx_tiles.hpp)
    brx_trust_stats_t *stats;
    uint32_t *tile_runs;    // stretch starts per tile            [tile bound]
    const uint64_t *run_base; // exclusive scan of tile_runs      [tile bound + 1]
    PieceArgs pc;
};

// bit 7 of every byte: the byte is one of ACGTacgt.  z = byte ^ letter is 0 for a match; (z & 0x7f) + 0x7f carries into
// bit 7 for every other value below 0x80, and z itself holds bit 7 for the rest.  No carry crosses a byte (0x7f + 0x7f).
__device__ __forceinline__ uint32_t letter4(uint32_t w)
{
    const uint32_t low = w | 0x20202020u;
    auto differs = [low](uint32_t c) {
        const uint32_t z = low ^ c;
        return ((z & 0x7f7f7f7fu) + 0x7f7f7f7fu) | z;
    };
    return ~(differs(0x61616161u) & differs(0x63636363u) & differs(0x67676767u) & differs(0x74747474u)) & 0x80808080u;
}
// bit 7 of every byte: the byte is >= thr, 34 <= thr <= 126.  A byte of 128 and more is; below that, byte + (128 - thr)
// reaches bit 7 exactly when it is (0x7f + 94 stays inside the byte).
__device__ __forceinline__ uint32_t good4(uint32_t q, uint32_t add)
{
    return (((q & 0x7f7f7f7fu) + add) | q) & 0x80808080u;
}
// the four answers (bit 7 of bytes 0..3) as bits 0..3: the multiply sends them to bits 28..31, no two products meet
__device__ __forceinline__ uint32_t gather4(uint32_t m) { return ((m >> 7) * 0x10204080u) >> 28; }
__device__ __forceinline__ uint32_t letter16(const uint4 &v)
{
    return gather4(letter4(v.x)) | (gather4(letter4(v.y)) << 4) | (gather4(letter4(v.z)) << 8) | (gather4(letter4(v.w)) << 12);
}
__device__ __forceinline__ uint32_t good16(const uint4 &v, uint32_t add)
{
    return gather4(good4(v.x, add)) | (gather4(good4(v.y, add)) << 4) | (gather4(good4(v.z, add)) << 8) | (gather4(good4(v.w, add)) << 12);
}
__device__ __forceinline__ bool trusted_byte(const TrustArgs &a, uint64_t at)
{
    const uint8_t l = a.bases[at] | 0x20u;
    const bool letter = l == (uint8_t)'a' || l == (uint8_t)'c' || l == (uint8_t)'g' || l == (uint8_t)'t';
    return (letter || a.any_byte) && (!a.quals || a.quals[at] >= a.thr);
}

// A tile on the 16-byte grid of its bases, and one step of it: the masks of this lane's 16 positions.
struct TrustTile {
    const uint8_t *bb; // the 16-byte border at or below the tile's first base
    const uint8_t *qb; // the quality piece that lane 0 of step 0 owns: bit i of the base grid is quality bit i - e behind it
    uint32_t mb, span; // the tile's bits are [mb, span) of the grid
    uint32_t e;
    uint32_t add;      // good4's addend
    uint32_t g_carry;  // the quality mask of the piece below lane 0's
    uint32_t steps;
};
__device__ __forceinline__ void trust_tile_open(const TrustArgs &a, const TileView &t, TrustTile &g)
{
    const uint8_t *ab = a.bases + t.o0 + t.p0;
    g.mb = (uint32_t)((uintptr_t)ab & 15u);
    g.bb = ab - g.mb;
    g.span = g.mb + (t.p1 - t.p0);
    g.steps = (g.span + 1023u) / 1024u;
    g.e = 0;
    g.qb = nullptr;
    g.add = (0x80u - a.thr) * 0x01010101u;
    g.g_carry = 0;
    if (a.quals) {
        const uint8_t *aq = a.quals + t.o0 + t.p0;
        const uint32_t mq = (uint32_t)((uintptr_t)aq & 15u);
        if (mq <= g.mb) { // the tile's first quality lies in lane 0's own piece
            g.e = g.mb - mq;
            g.qb = aq - mq;
        } else {          // ... in the piece below it, which every lane reads (one request) and lane 0 uses
            g.e = g.mb + 16u - mq;
            g.qb = aq - mq + 16;
            g.g_carry = good16(*reinterpret_cast<const uint4 *>(g.qb - 16), g.add);
        }
    }
}
// L: letter[], G: good[], own: the positions that belong to the tile; T = trusted[] = (L | any_byte) & G & own
__device__ __forceinline__ void trust_step(const TrustArgs &a, TrustTile &g, uint32_t step, uint32_t lane, uint32_t &L, uint32_t &G,
                                           uint32_t &own)
{
    const int ib0 = (int)(1024u * step + 16u * lane);
    const int lo = min(max((int)g.mb - ib0, 0), 16), hi = min(max((int)g.span - ib0, 0), 16);
    own = hi > lo ? (1u << hi) - (1u << lo) : 0u;
    L = 0;
    if (own)
        L = letter16(*reinterpret_cast<const uint4 *>(g.bb + ib0));
    G = 0xffffu;
    if (a.quals) {
        // this lane's quality piece covers bits [ib0 + e, ib0 + e + 16) of the grid
        uint32_t mine = 0;
        if (ib0 + (int)g.e < (int)g.span && ib0 + (int)g.e + 16 > (int)g.mb)
            mine = good16(*reinterpret_cast<const uint4 *>(g.qb + ib0), g.add);
        uint32_t below = (uint32_t)__shfl_up((int)mine, 1);
        if (lane == 0u)
            below = g.g_carry;
        G = ((below >> (16u - g.e)) | (mine << g.e)) & 0xffffu;
        g.g_carry = (uint32_t)__shfl((int)mine, 63);
    }
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
    for (int d = 32; d; d >>= 1)
        v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}

// A wave per tile.  RUNS = false: pass 1 (starts per tile, statistics); true: pass 2 (the stretches' starts and ends).
template <bool RUNS>
__global__ __launch_bounds__(256) void trust_kernel(TrustArgs a)
{
    TileView t;
    unsigned long long tile;
    if (!tile_view(a.tl, a.offsets, t, tile))
        return;
    const uint32_t lane = threadIdx.x & 63u;
    TrustTile g;
    trust_tile_open(a, t, g);
    const uint32_t open = t.p0 ? (trusted_byte(a, t.o0 + t.p0 - 1u) ? 1u : 0u) : 0u; // a stretch reaches the tile from the left
    uint32_t t_carry = 0; // the last bit of the step before
    uint32_t sums = 0;    // pass 1: non_acgt | low_quality << 11 | starts << 22 of this lane (a tile holds 1024 positions)
    uint64_t s_at = 0, e_at = 0;
    if (RUNS) {
        s_at = a.run_base[tile];
        e_at = s_at - open;
    }
    uint32_t T = 0;
    for (uint32_t st = 0; st < g.steps; st++) {
        uint32_t L, G, own;
        trust_step(a, g, st, lane, L, G, own);
        T = (L | a.any_byte) & G & own;
        uint32_t prev = (uint32_t)__shfl_up((int)T, 1) >> 15;
        if (lane == 0u)
            prev = st ? t_carry : 0u;
        uint32_t before = ((T << 1) | prev) & 0xffffu; // trusted[] of the position in front of every bit
        if (st == 0u && lane == 0u)
            before |= open << g.mb;
        const uint32_t starts = T & ~before, falls = ~T & before & own;
        t_carry = (uint32_t)__shfl((int)T, 63) >> 15;
        if (!RUNS) {
            sums += (uint32_t)__popc(~L & own) + ((uint32_t)__popc(L & ~G & own) << 11) + ((uint32_t)__popc(starts) << 22);
        } else {
            // numbers of this lane's starts and ends: an inclusive scan of both counts over the lanes
            const uint32_t cnt = (uint32_t)__popc(starts) | ((uint32_t)__popc(falls) << 16);
            uint32_t inc = cnt;
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t up = (uint32_t)__shfl_up((int)inc, d);
                if ((int)lane >= d)
                    inc += up;
            }
            const uint32_t exc = inc - cnt, all = (uint32_t)__shfl((int)inc, 63);
            const uint32_t pos0 = t.p0 + 1024u * st + 16u * lane - g.mb; // position of bit 0 (wraps below the tile: never used there)
            uint64_t i = s_at + (exc & 0xffffu);
            for (uint32_t m = starts; m; m &= m - 1u, i++) {
                a.pc.run_read[i] = t.r;
                a.pc.run_start[i] = pos0 + (uint32_t)__ffs((int)m) - 1u;
            }
            i = e_at + (exc >> 16);
            for (uint32_t m = falls; m; m &= m - 1u, i++)
                a.pc.run_end[i] = pos0 + (uint32_t)__ffs((int)m) - 2u; // a 1 -> 0 step at j ends a stretch at j - 1
            s_at += all & 0xffffu;
            e_at += all >> 16;
        }
    }
    if (!RUNS) {
        sums = wave_sum(sums);
        if (lane == 0u) {
            a.tile_runs[tile] = sums >> 22;
            if (a.stats) {
                uint32_t *row = reinterpret_cast<uint32_t *>(a.stats + t.r);
                if (t.p0 == 0u)
                    atomicAdd(row + 0, t.n);
                if (sums & 0x7ffu)
                    atomicAdd(row + 1, sums & 0x7ffu);
                if ((sums >> 11) & 0x7ffu)
                    atomicAdd(row + 2, (sums >> 11) & 0x7ffu);
            }
        }
    } else if (t.p1 == t.n) { // the end of a read ends an open stretch
        const uint32_t last = g.span - 1u - 1024u * (g.steps - 1u);
        const uint32_t bit = ((uint32_t)__shfl((int)T, (int)(last >> 4)) >> (last & 15u)) & 1u;
        if (bit && lane == 0u)
            a.pc.run_end[e_at] = t.n - 1u;
    }
}

// pieces and kept_bases of every read, from the runs that were kept
__global__ __launch_bounds__(256) void trust_piece_stats_kernel(PieceArgs pc, brx_trust_stats_t *stats)
{
    const unsigned long long n = *pc.n_runs;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256ull)
        if (pc.keep_flag[i]) {
            uint32_t *row = reinterpret_cast<uint32_t *>(stats + pc.run_read[i]);
            atomicAdd(row + 3, 1u);
            atomicAdd(row + 4, pc.keep_len[i]);
        }
}

// the five columns of n rows added to five u64
__global__ __launch_bounds__(256) void trust_totals_kernel(const brx_trust_stats_t *stats, uint32_t n, unsigned long long *tot5)
{
    unsigned long long v[5] = {0, 0, 0, 0, 0};
    for (uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x; r < n; r += (uint64_t)gridDim.x * 256u) {
        const uint32_t *row = reinterpret_cast<const uint32_t *>(stats + r);
        for (int c = 0; c < 5; c++)
            v[c] += row[c];
    }
    for (int c = 0; c < 5; c++) {
        unsigned long long x = v[c];
        for (int d = 32; d; d >>= 1)
            x += (unsigned long long)__shfl_xor((long long)x, d);
        if ((threadIdx.x & 63u) == 0u && x)
            atomicAdd(tot5 + c, x);
    }
}

} // namespace

namespace brx {
int trust_totals_add(const brx_trust_stats_t *d_stats, uint32_t n_reads, unsigned long long *d_tot5, hipStream_t s)
{
    if (!n_reads)
        return BRX_OK;
    trust_totals_kernel<<<read_grid((n_reads + 255u) / 256u, 1024u), 256, 0, s>>>(d_stats, n_reads, d_tot5);
    BRX_HIP(hipGetLastError());
    return BRX_OK;
}
}

extern "C" {

int brx_trust_split_batch_device(const uint8_t *d_bases, const uint8_t *d_quals, const uint64_t *d_offsets, uint32_t n_reads,
                                 uint64_t total_bases, const brx_trust_opts_t *opts, uint8_t *d_out, uint64_t out_cap,
                                 uint64_t *d_out_offsets, uint32_t *d_piece_read, uint64_t *d_piece_start, uint32_t piece_cap,
                                 brx_trust_stats_t *d_stats, uint32_t *n_pieces, uint64_t *out_total, int device, void *stream)
{
    const char *me = "brx_trust_split_batch_device";
    if (!opts) {
        set_error("%s: null opts", me);
        return BRX_ERR_ARG;
    }
    if (opts->min_quality > 93) {
        set_error("%s: min_quality=%u (Phred+33 qualities end at 93)", me, (unsigned)opts->min_quality);
        return BRX_ERR_ARG;
    }
    if (!n_pieces || !out_total) {
        set_error("%s: null n_pieces / out_total", me);
        return BRX_ERR_ARG;
    }
    *n_pieces = 0;
    *out_total = 0;
    BRX_TRY(check_batch_args(me, d_bases, d_offsets, n_reads, total_bases));
    BRX_TRY(use_device(device));
    hipStream_t s = (hipStream_t)stream;
    auto sync = [&](int st_in) -> int {
        const hipError_t e = hipStreamSynchronize(s);
        if (st_in == BRX_OK && e != hipSuccess) {
            set_error("%s: %s", me, hipGetErrorString(e));
            return BRX_ERR_HIP;
        }
        return st_in;
    };
    if (!n_reads || !total_bases) { // no base, no stretch
        hipError_t e = hipSuccess;
        if (d_out_offsets)
            e = hipMemsetAsync(d_out_offsets, 0, 8, s);
        if (e == hipSuccess && d_stats && n_reads)
            e = hipMemsetAsync(d_stats, 0, (uint64_t)n_reads * sizeof(brx_trust_stats_t), s);
        return sync(e == hipSuccess ? BRX_OK : BRX_ERR_HIP);
    }
    DevScratch sc;
    TrustArgs a{};
    a.bases = d_bases;
    a.quals = opts->min_quality ? d_quals : nullptr;
    a.offsets = d_offsets;
    a.n_reads = n_reads;
    a.thr = 33u + opts->min_quality;
    a.any_byte = opts->acgt_only ? 0u : 0xffffu;
    a.pc.bases = d_bases;
    a.pc.offsets = d_offsets;
    a.pc.min_len = std::max<uint32_t>(opts->min_len, 1u);
    uint64_t tile_bound = total_bases / READ_TILE + n_reads;
    if (tile_bound >= 0xffffffffull) {
        set_error("%s: batch of %llu bases in %u reads is too large for one call", me, (unsigned long long)total_bases, n_reads);
        return BRX_ERR_ARG;
    }
    uint64_t *run_base = nullptr, *tmp = nullptr;
    unsigned long long *d_totals = nullptr; // runs, pieces, bytes
    brx_trust_stats_t *stats = nullptr;     // a scratch copy: nothing of the caller's is written before the sizes are known to fit
    BRX_TRY(sc.get(&a.tile_runs, tile_bound));
    BRX_TRY(sc.get(&run_base, tile_bound + 1));
    BRX_TRY(sc.get(&d_totals, 3));
    BRX_TRY(sc.get(&tmp, scan_tmp_bytes((uint32_t)tile_bound) / 8 + 1));
    if (d_stats)
        BRX_TRY(sc.get(&stats, n_reads));
    a.stats = stats;
    unsigned long long h_tot[3] = {0, 0, 0};
    auto pass1 = [&]() -> int {
        BRX_TRY(tile_list_enqueue(a.tl, d_offsets, n_reads, total_bases, me, "trust", sc, tile_bound, s));
        if (stats)
            BRX_HIP(hipMemsetAsync(stats, 0, (uint64_t)n_reads * sizeof(brx_trust_stats_t), s));
        BRX_HIP(hipMemsetAsync(a.tile_runs, 0, tile_bound * 4, s));
        {
            KernelTimer t("trust", s);
            trust_kernel<false><<<(uint32_t)((tile_bound + 3ull) / 4ull), 256, 0, s>>>(a);
            BRX_TRY(exclusive_scan_lens(a.tile_runs, (uint32_t)tile_bound, tmp, run_base, d_totals, s));
        }
        BRX_HIP(hipGetLastError());
        BRX_HIP(hipMemcpyAsync(h_tot, d_totals, 8, hipMemcpyDeviceToHost, s));
        return BRX_OK;
    };
    int st = sync(pass1());
    if (st != BRX_OK)
        return st;
    a.run_base = run_base;
    a.pc.n_runs = d_totals;
    const uint64_t n_runs = h_tot[0];
    if (n_runs >= 0xffffffffull) {
        set_error("%s: %llu stretches in one batch: too large for one call", me, (unsigned long long)n_runs);
        return BRX_ERR_ARG;
    }
    if (n_runs) {
        uint64_t *piece_of = nullptr, *byte_of = nullptr, *tmp2 = nullptr;
        auto pass2 = [&]() -> int {
            BRX_TRY(sc.get(&a.pc.run_read, n_runs));
            BRX_TRY(sc.get(&a.pc.run_start, n_runs));
            BRX_TRY(sc.get(&a.pc.run_end, n_runs));
            BRX_TRY(sc.get(&a.pc.keep_flag, n_runs));
            BRX_TRY(sc.get(&a.pc.keep_len, n_runs));
            BRX_TRY(sc.get(&piece_of, n_runs + 1));
            BRX_TRY(sc.get(&byte_of, n_runs + 1));
            BRX_TRY(sc.get(&tmp2, scan_tmp_bytes((uint32_t)n_runs) / 8 + 1));
            {
                KernelTimer t("trust", s);
                trust_kernel<true><<<(uint32_t)((tile_bound + 3ull) / 4ull), 256, 0, s>>>(a);
            }
            {
                KernelTimer t("trust_copy", s);
                piece_keep_launch(a.pc, n_runs, s);
                BRX_TRY(exclusive_scan_lens(a.pc.keep_flag, (uint32_t)n_runs, tmp2, piece_of, d_totals + 1, s));
                BRX_TRY(exclusive_scan_lens(a.pc.keep_len, (uint32_t)n_runs, tmp2, byte_of, d_totals + 2, s));
            }
            BRX_HIP(hipGetLastError());
            BRX_HIP(hipMemcpyAsync(h_tot + 1, d_totals + 1, 16, hipMemcpyDeviceToHost, s));
            return BRX_OK;
        };
        st = sync(pass2());
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
    if (pieces && (!d_out_offsets || !d_out)) {
        set_error("%s: null d_out / d_out_offsets", me);
        return BRX_ERR_ARG;
    }
    auto finish = [&]() -> int {
        KernelTimer t("trust_copy", s);
        if (pieces) {
            a.pc.out = d_out;
            a.pc.out_offsets = d_out_offsets;
            a.pc.piece_read = d_piece_read;
            a.pc.piece_start = d_piece_start;
            piece_copy_launch(a.pc, n_runs, s);
        } else if (d_out_offsets) {
            BRX_HIP(hipMemsetAsync(d_out_offsets, 0, 8, s));
        }
        if (d_stats) {
            if (pieces)
                trust_piece_stats_kernel<<<read_grid((n_runs + 255ull) / 256ull, 4096u), 256, 0, s>>>(a.pc, stats);
            BRX_HIP(hipMemcpyAsync(d_stats, stats, (uint64_t)n_reads * sizeof(brx_trust_stats_t), hipMemcpyDeviceToDevice, s));
        }
        BRX_HIP(hipGetLastError());
        return BRX_OK;
    };
    return sync(finish());
}

int brx_trust_split_batch(const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint32_t n_reads,
                          const brx_trust_opts_t *opts, uint8_t **out_bases, uint64_t **out_offsets, uint32_t **piece_read,
                          uint64_t **piece_start, brx_trust_stats_t *stats, uint32_t *n_pieces, int device)
{
    const char *me = "brx_trust_split_batch";
    if (!opts || !out_bases || !out_offsets || !piece_read || !piece_start || !n_pieces) {
        set_error("%s: null argument", me);
        return BRX_ERR_ARG;
    }
    *out_bases = nullptr;
    *out_offsets = nullptr;
    *piece_read = nullptr;
    *piece_start = nullptr;
    *n_pieces = 0;
    if (n_reads && !offsets) {
        set_error("%s: null offsets", me);
        return BRX_ERR_ARG;
    }
    if (opts->min_quality > 93) {
        set_error("%s: min_quality=%u (Phred+33 qualities end at 93)", me, (unsigned)opts->min_quality);
        return BRX_ERR_ARG;
    }
    const uint64_t total = n_reads ? offsets[n_reads] : 0;
    BRX_TRY(check_batch_args(me, bases, offsets, n_reads, total));
    BRX_TRY(check_offsets(me, offsets, n_reads));
    BRX_TRY(use_device(device));
    // the bounds of include/brx.h: no retry
    const uint64_t piece_cap = (uint64_t)n_reads + total / ((uint64_t)std::max<uint32_t>(opts->min_len, 1u) + 1ull);
    if (piece_cap >= 0xffffffffull) {
        set_error("%s: batch too large for one call", me);
        return BRX_ERR_ARG;
    }
    DevScratch sc;
    uint8_t *d_bases = nullptr, *d_quals = nullptr, *d_out = nullptr;
    uint64_t *d_off = nullptr, *d_oo = nullptr, *d_ps = nullptr;
    uint32_t *d_pr = nullptr;
    brx_trust_stats_t *d_st = nullptr;
    BRX_TRY(sc.get(&d_bases, total + 16));
    if (quals)
        BRX_TRY(sc.get(&d_quals, total + 16));
    BRX_TRY(sc.get(&d_off, (uint64_t)n_reads + 1));
    BRX_TRY(sc.get(&d_out, total));
    BRX_TRY(sc.get(&d_oo, piece_cap + 1));
    BRX_TRY(sc.get(&d_pr, piece_cap));
    BRX_TRY(sc.get(&d_ps, piece_cap));
    if (stats)
        BRX_TRY(sc.get(&d_st, n_reads));
    hipStream_t s = nullptr;
    if (total)
        BRX_HIP(hipMemcpyAsync(d_bases, bases, total, hipMemcpyHostToDevice, s));
    if (total && quals)
        BRX_HIP(hipMemcpyAsync(d_quals, quals, total, hipMemcpyHostToDevice, s));
    if (n_reads)
        BRX_HIP(hipMemcpyAsync(d_off, offsets, ((uint64_t)n_reads + 1) * 8, hipMemcpyHostToDevice, s));
    uint32_t np = 0;
    uint64_t bytes = 0;
    BRX_TRY(brx_trust_split_batch_device(d_bases, d_quals, d_off, n_reads, total, opts, d_out, total, d_oo, d_pr, d_ps,
                                         (uint32_t)piece_cap, d_st, &np, &bytes, device, s));
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
    if (e == hipSuccess && stats && n_reads)
        e = hipMemcpyAsync(stats, d_st, (uint64_t)n_reads * sizeof(brx_trust_stats_t), hipMemcpyDeviceToHost, s);
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
