// The tail of a split form (brx_cover.hip: covered runs; brx_trust.hip: trusted stretches): the runs of a batch, numbered in
// (read, position) order with their first and last base, are kept where they hold at least min_len bases, numbered and laid
// out by two scans of keep_flag / keep_len, and copied.  The order of the output is fixed by those scans, never by timing.
#pragma once
#include "brx_internal.hpp"

namespace brx {

struct PieceArgs {
    const uint8_t *bases;
    const uint64_t *offsets;
    uint32_t *run_read, *run_start, *run_end; // [runs]
    const unsigned long long *n_runs;
    uint32_t min_len;
    uint32_t *keep_flag, *keep_len;   // [runs]
    const uint64_t *piece_of;         // exclusive scan of keep_flag      [runs + 1]
    const uint64_t *byte_of;          // exclusive scan of keep_len       [runs + 1]
    uint8_t *out;
    uint64_t *out_offsets;
    uint32_t *piece_read;
    uint64_t *piece_start;
};

#if defined(__HIPCC__)
static __global__ __launch_bounds__(256) void piece_keep_kernel(PieceArgs a)
{
    const unsigned long long n = *a.n_runs;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256ull) {
        const uint32_t len = a.run_end[i] - a.run_start[i] + 1u;
        const bool keep = len >= a.min_len;
        a.keep_flag[i] = keep ? 1u : 0u;
        a.keep_len[i] = keep ? len : 0u;
    }
}

// A wave per run that is kept: its row of the piece table and its bytes.
static __global__ __launch_bounds__(256) void piece_copy_kernel(PieceArgs a)
{
    const unsigned long long n = *a.n_runs;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (blockIdx.x == 0 && threadIdx.x == 0)
        a.out_offsets[a.piece_of[n]] = a.byte_of[n];
    for (unsigned long long i = (unsigned long long)blockIdx.x * 4ull + wv; i < n; i += (unsigned long long)gridDim.x * 4ull) {
        if (!a.keep_flag[i])
            continue;
        const uint64_t p = a.piece_of[i], at = a.byte_of[i];
        const uint32_t r = a.run_read[i], s = a.run_start[i], len = a.keep_len[i];
        if (lane == 0u) {
            a.out_offsets[p] = at;
            if (a.piece_read)
                a.piece_read[p] = r;
            if (a.piece_start)
                a.piece_start[p] = s;
        }
        const uint8_t *src = a.bases + a.offsets[r] + s;
        uint8_t *dst = a.out + at;
        for (uint32_t b = lane; b < len; b += 64u)
            dst[b] = src[b];
    }
}

// the two launches, with the grids the coverage split has always cut (n_runs > 0)
static inline void piece_keep_launch(const PieceArgs &a, uint64_t n_runs, hipStream_t s)
{
    piece_keep_kernel<<<read_grid((n_runs + 255ull) / 256ull, 4096u), 256, 0, s>>>(a);
}
static inline void piece_copy_launch(const PieceArgs &a, uint64_t n_runs, hipStream_t s)
{
    piece_copy_kernel<<<read_grid((n_runs + 3ull) / 4ull, 8192u), 256, 0, s>>>(a);
}
#endif

} // namespace brx
