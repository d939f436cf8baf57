// Read-tile work list (brx_cover.hip, brx_abundance.hip): a batch cut BY POSITION.  From the offsets: tiles per read, their
// exclusive scan, the read of every tile.  A wave then takes a tile of READ_TILE positions of one read, so that a
// 62 163-base read keeps 61 waves busy while a 157-base read costs one.  The number of tiles is bounded without asking the
// device (total_bases / READ_TILE + n_reads); the kernels are launched for the bound and a wave past *n_tiles leaves.
#pragma once
#include "brx_internal.hpp"

namespace brx {

constexpr uint32_t READ_TILE = 1024; // positions of a read per wave: 16 steps of 64, a 17th for the k-1 positions behind them

struct TileList {
    uint32_t *tiles_of;          // tiles per read              [n_reads]
    uint64_t *tile_base;         // exclusive scan of tiles_of  [n_reads + 1]
    uint32_t *tile_read;         // read of a tile              [tiles]
    unsigned long long *n_tiles; // = tile_base[n_reads]
};

#if defined(__HIPCC__)
static __global__ __launch_bounds__(256) void tiles_of_kernel(TileList tl, const uint64_t *__restrict__ offsets, uint32_t n_reads)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n_reads)
        return;
    const uint64_t n = offsets[r + 1] - offsets[r];
    tl.tiles_of[r] = (uint32_t)((n + READ_TILE - 1u) / READ_TILE);
}

static __global__ __launch_bounds__(256) void tile_list_kernel(TileList tl, uint32_t n_reads)
{
    for (uint32_t r = blockIdx.x; r < n_reads; r += gridDim.x) {
        const uint64_t tb = tl.tile_base[r], te = tl.tile_base[r + 1];
        for (uint64_t t = tb + threadIdx.x; t < te; t += 256)
            tl.tile_read[t] = r;
    }
}

// what a tile is: its read, the read's place and length, the tile's positions [p0, p1)
struct TileView {
    uint32_t r, n, p0, p1;
    uint64_t o0;
};
// the tile of this wave (blocks of 256 threads, a wave per tile); false: there is none
__device__ __forceinline__ bool tile_view(const TileList &tl, const uint64_t *offsets, TileView &t, unsigned long long &tile)
{
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    tile = (unsigned long long)blockIdx.x * 4ull + wv;
    if (tile >= *tl.n_tiles)
        return false;
    t.r = tl.tile_read[tile];
    t.o0 = offsets[t.r];
    t.n = (uint32_t)(offsets[t.r + 1] - t.o0);
    t.p0 = (uint32_t)(tile - tl.tile_base[t.r]) * READ_TILE;
    t.p1 = t.n - t.p0 < READ_TILE ? t.n : t.p0 + READ_TILE;
    return true;
}

// Reserves the list in `sc` and enqueues its three launches on `s` under the profile timer `timer`.  tile_bound: what the
// caller cuts its grid from, (tile_bound + 3) / 4 blocks.  `what` names the feature in the refusal of a batch too large.
static inline int tile_list_enqueue(TileList &tl, const uint64_t *d_offsets, uint32_t n_reads, uint64_t total_bases, const char *what,
                                    const char *timer, DevScratch &sc, uint64_t &tile_bound, hipStream_t s)
{
    tile_bound = total_bases / READ_TILE + n_reads;
    if (tile_bound / 4ull + 1ull > 0x7fffffffull) {
        set_error("%s: batch of %llu bases in %u reads is too large for one call", what, (unsigned long long)total_bases, n_reads);
        return BRX_ERR_ARG;
    }
    uint64_t *tmp = nullptr;
    BRX_TRY(sc.get(&tl.tiles_of, n_reads));
    BRX_TRY(sc.get(&tl.tile_base, (uint64_t)n_reads + 1));
    BRX_TRY(sc.get(&tl.tile_read, tile_bound));
    BRX_TRY(sc.get(&tl.n_tiles, 1));
    BRX_TRY(sc.get(&tmp, scan_tmp_bytes(n_reads) / 8 + 1));
    KernelTimer t(timer, s);
    tiles_of_kernel<<<(n_reads + 255u) / 256u, 256, 0, s>>>(tl, d_offsets, n_reads);
    BRX_TRY(exclusive_scan_lens(tl.tiles_of, n_reads, tmp, tl.tile_base, tl.n_tiles, s));
    tile_list_kernel<<<read_grid(n_reads, 2048u), 256, 0, s>>>(tl, n_reads);
    return BRX_OK;
}
#endif

} // namespace brx
