// Shared by the correction kernels (brx_group.hip, brx_one.hip, brx_revscan.hip: groups of lanes per read; brx_onelane.hip:
// one lane per chunk of a read) and their host side (brx_correct.hip): the pass description, the staging-slot layout, the
// control block, the wave-level k-mer scans and the launches the units call across files.
#pragma once
#include "brx_internal.hpp"
#include "brx_index.hpp"
#include "brx_plan.hpp"

#include <type_traits>

namespace brx {

// control block layout (u64 words)
enum { CTL_WORK = 0, CTL_OVERFLOW = 1, CTL_ROUNDS = 2, CTL_PROBES = 3, CTL_TRIGGERS = 4, CTL_FIXES = 5, CTL_TOTAL = 6, CTL_PATHOVF = 7, CTL_NONTERM = 8,
       // the lane-per-chunk form of One's forward pass (brx_onelane.hip): units of the pass, predictions that missed,
       // its work counter, reads handed back to the group kernel
       CTL_LANE_UNITS = 9, CTL_LANE_MISS = 10, CTL_LANE_WORK = 11, CTL_LANE_FAIL = 12,
       // (not reset per pass: summed over the attempt) unit records the replay kernel found UNWRITTEN -- every unit is
       // taken by exactly one lane and leaves a record, so this stays 0; the records are filled with ones before the
       // automaton runs so that a unit nobody scanned could not pass for a result (its read goes to the group kernel)
       // the lean reverse pass (rev_scan_kernel, brx_revscan.hip): reads handed back to the group kernel, this pass / summed
       CTL_REV_HANDBACK = 13, CTL_REV_HANDBACK_SUM = 14,
       CTL_LANE_UNWRITTEN = 15,
       // ... and the triggers it left to the verify pass (this pass / summed)
       CTL_REV_TRIGS = 16, CTL_REV_TRIGS_SUM = 17,
       // builds with -DBRX_AP_COUNT only: 16-byte chunks with fixes that the replay kernels put together from vector
       // loads, whole chunks that went the byte way, chunks shorter than 16 bytes (the ends of a batch of fixes)
       CTL_AP_VEC = 18, CTL_AP_BYTEWAY = 19, CTL_AP_PARTIAL = 20,
       CTL_N = 21 };

// A trigger of a reverse pass that the lean scan could not settle itself (alt_nucs named exactly one alternative): the scan
// goes on as if the method returned None, and the group kernel checks that it does (SRC == 2 of correct_kernel).
struct TrigRec {
    uint32_t r;    // read
    uint32_t i;    // position of the trigger (the base that made the k-mer non-solid)
    uint32_t elen; // error_len's result (Graph / GapSize; the rest of the read when it ran off the end)
    uint32_t pad;
    uint64_t fc;   // first_correct_kmer
};

struct PassParams {
    const uint32_t *bits;
    IdxView idx;      // lines == nullptr: every probe goes to the bitset
    int k;
    int c;            // confirm
    uint32_t n_reads;
    const uint64_t *offsets; // original batch offsets (n_reads+1), relative to batch start
    // input view
    const uint8_t *in;       // original bases or staging buffer
    const uint32_t *in_lens; // nullptr => lengths from offsets (original batch)
    int in_staged;           // 0: read r starts at offsets[r]; 1: at slot(r)
    int flip;                // read the input back to front
    // output view (always staged)
    uint8_t *out;
    uint32_t *out_lens;
    uint32_t slack;          // slot(r) = o + (o>>2)*slack + 64*r
    unsigned long long *ctrl;
    // graph walks (Graph, GapSize): per-group list of visited k-mers, maxpath entries each
    uint64_t *path_k;
    uint32_t maxpath;
    // greedy (greedy.rs): max_search and the per-group LDS carve-up for the alignment
    uint32_t flags;       // tuning switches for A/B runs (BRX_TUNE): 1 no look-ahead reuse, 2 four ALTS probes, 4 unstaged SCEN
    int max_search;
    uint32_t g_dim;       // max (m+1), (n+1) of the DP = k + max_search + 2
    uint32_t g_lds_bytes; // bytes of dynamic LDS per group
    // list mode (one_kernel<G, K, true>): the kernel takes reads only[0 .. *only_n) instead of 0 .. n_reads
    const uint32_t *only = nullptr;
    const unsigned long long *only_n = nullptr;
    // verify mode (correct_kernel<G, M, 2>): the work items are the triggers trig[0 .. min(*only_n, trig_cap)); a read
    // whose trigger does NOT end in None is entered once into redo_list (count at ctrl[CTL_REV_HANDBACK], redo_flag dedupes)
    const TrigRec *trig = nullptr;
    uint32_t trig_cap = 0;
    uint32_t *redo_list = nullptr;
    uint32_t *redo_flag = nullptr;
    // reverse scans: trigger-free rounds REV_BLOCK at a time through the occupancy bits (rev_block_rounds); set by the host
    // only where the index answers in that form (plan_pass, brx_plan.hpp)
    int rev_batch = 0;
};

// states of a group's machine; one_kernel (brx_one.hip) runs the first six of correct_kernel's (brx_group.hip)
enum { ST_INIT = 0, ST_SCAN, ST_ERRLEN, ST_ALTS, ST_SCEN, ST_MORE, ST_WALK, ST_T1, ST_TSCORE, ST_TMORE, ST_GFOLLOW, ST_GVALID };

__host__ __device__ __forceinline__ uint64_t slot_of(uint64_t o, uint64_t r, uint32_t slack)
{
    return o + (o >> 2) * (uint64_t)slack + 64ull * r;
}

#if defined(__HIPCC__)
// look-ahead k-mers per scenario probed in the SCEN round that starts at look-ahead index `sub`
// (the lanes are dealt to the scenarios still alive, so once the wrong ones have died the survivor's
// remaining look-aheads fit one round even in an 8-lane group)
__device__ __forceinline__ uint32_t scen_width(uint32_t sub, uint32_t c, int G, uint32_t flags, uint32_t failmask)
{
    const uint32_t left = c - sub;
    const uint32_t alive = 3u - (uint32_t)__popc(failmask & 7u);
    // G / alive without a division (a variable u32 division is ~25 VALU instructions, paid by the whole wave)
    const uint32_t share = alive <= 1u ? (uint32_t)G : (alive == 2u ? (uint32_t)G / 2u : (uint32_t)G / 3u);
    const uint32_t cap = (sub == 0u && !(flags & 4u)) ? (share < 2u ? share : 2u) : share;
    return left < cap ? left : cap;
}

template <int D>
__device__ __forceinline__ uint32_t dpp_row_shr(uint32_t v)
{
    // lane l of a 16-lane row reads lane l - D of the same row; lanes without such a source read 0
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x110 + D, 0xf, 0xf, true);
}

// codes of the row's lanes first..this one, this lane's code in bits 0-1, the lane before in bits 2-3, ...
__device__ __forceinline__ uint32_t row_scan16(uint32_t code)
{
    uint32_t v = code;
    v |= dpp_row_shr<1>(v) << 2;
    v |= dpp_row_shr<2>(v) << 4;
    v |= dpp_row_shr<4>(v) << 8;
    v |= dpp_row_shr<8>(v) << 16;
    return v;
}
// this lane's k-mer in a 64-lane group: `carry` extended by the codes of lanes 0..lane (own row by the DPP scan, the two
// rows before by row_bcast:15; rows 0 / 1 take those words from `carry`)
__device__ __forceinline__ uint64_t lane_kmer64_dpp(uint64_t carry, uint32_t code, int lane, uint64_t mask)
{
    const uint32_t v = row_scan16(code);
    const uint32_t clo = (uint32_t)carry, chi = (uint32_t)(carry >> 32);
    const uint32_t b1 = (uint32_t)__builtin_amdgcn_update_dpp((int)clo, (int)v, 0x142 /* row_bcast:15 */, 0xe, 0xf, false);
    const uint32_t old2 = (lane < 16) ? chi : clo;
    const uint32_t b2 = (uint32_t)__builtin_amdgcn_update_dpp((int)old2, (int)b1, 0x142, 0xc, 0xf, false);
    const uint32_t jb = 2u * ((uint32_t)(lane & 15) + 1u);
    return (((((uint64_t)b2 << 32) | b1) << jb) | v) & mask; // jb <= 32
}
// the k-mer of lane 63, as a wave-uniform value: the next step's `carry`
__device__ __forceinline__ uint64_t wave_carry(uint64_t km)
{
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(km >> 32), 63) << 32) |
           (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)km, 63);
}
#endif

// ----------------------------------------------------------------------------------------------------------------------
// Trigger-free scan rounds of a reverse pass, REV_BLOCK at a time (one wave per read: one_kernel<64>, correct_kernel<64>,
// rev_scan_kernel).  Nearly every k-mer of a reversed read is absent and four index lines in five are empty, so a round
// of 64 positions, one set_get each, makes the whole wave pay for the key, the line fetch and the slot compares of
// the dozen lanes whose home line holds anything.  Here a round only FILTERS: the lane hashes the newest m-mer of its
// k-mer, takes the minimum over itself and its w - 1 left neighbours (wave_shr DPP moves; the hashes in front of the
// wave's span come from the carried k-mer, in scalar arithmetic), and loads the occupancy bit of that line.  Lanes whose bit is set queue
// (k-mer, line, round << 6 | lane) in LDS; when the block's rounds are through -- or the queue has fewer than 64 places
// left -- the queue is drained a wave at a time: reverse complement, key, index_probe_at, "cannot say" settled on the
// spot as set_get does.  A solid k-mer ORs its bit into the block's answer words; the trigger test then runs over
// those words as it does over a round's ballot.  Probes are pure, so only their order and grouping differ.
// LDS per wave: 128 entries of 16 bytes + REV_BLOCK answer words + REV_BLOCK carried k-mers = 2 112 bytes at REV_BLOCK = 4,
// 8 448 per block of 256: 28 waves of a CU (7 per SIMD) take 59 KB of its 160.
// ----------------------------------------------------------------------------------------------------------------------
#ifndef BRX_REV_BLOCK
#define BRX_REV_BLOCK 4 // rounds per block (tools/ab_build.sh sweeps 2 / 4 / 8)
#endif
constexpr int REV_BLOCK = BRX_REV_BLOCK;
// (REV_MAX_W, the windows the sliding minimum is unrolled for, sits with the rule that admits an index: brx_plan.hpp)
constexpr uint32_t REV_QUEUE = 128; // entries of a wave's queue
static_assert(REV_BLOCK >= 1 && REV_BLOCK <= 16, "BRX_REV_BLOCK: 1 .. 16 rounds");

#if defined(__HIPCC__)
// hash of the canonical form of an m-mer (f: its 2m bits, nothing above): window j = 0 of minimizer_hash_w
__device__ __forceinline__ uint32_t mmer_hash(uint32_t f, uint32_t m)
{
    uint32_t x = __brev(f ^ 0xAAAAAAAAu);
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    const uint32_t r = x >> (32u - 2u * m);
    return (f < r ? f : r) * 0x9E3779B1u;
}

// a wave-uniform value the compiler cannot see to be one (it came through a shuffle): into scalar registers
__device__ __forceinline__ uint32_t uni32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t uni64(uint64_t v) { return ((uint64_t)uni32((uint32_t)(v >> 32)) << 32) | uni32((uint32_t)v); }

// Up to REV_BLOCK rounds of 64 positions from logical position i on, all of them full (the caller checks n - i and the
// room in out).  ld(j): logical base j of the read; outp: where position i's byte goes.  Returns the number of rounds
// committed: kmer and prev then stand behind the last of them, and a return value below REV_BLOCK means that the next
// round holds a trigger (mod.rs:73) -- nothing of it is settled here but bytes the caller's general code writes again.
template <bool HAS_SKIP, typename LD>
__device__ __forceinline__ uint32_t rev_block_rounds(const IdxView &idx, const uint32_t *__restrict__ bits, int k, uint64_t mask, int lane0, LD ld,
                                                     uint32_t i, uint8_t *__restrict__ outp, uint32_t skip_until, uint64_t &kmer, bool &prev)
{
    __shared__ uint4 rev_q[4][REV_QUEUE];
    __shared__ unsigned long long rev_ans[4][2 * REV_BLOCK]; // per wave: the rounds' answer words, then their carried k-mers
    const uint32_t wv = uni32(threadIdx.x >> 6); // (scalar: the queue's address then costs no vector register)
    uint4 *const q = rev_q[wv];
    unsigned long long *const ans = rev_ans[wv];
    unsigned long long *const carry = ans + REV_BLOCK;
    const uint32_t m = idx.m, w = idx.w;
    const uint32_t mm = m >= 16u ? 0xffffffffu : (1u << (2u * m)) - 1u;

    if (lane0 < REV_BLOCK)
        ans[lane0] = 0ull;

    // One loop, one copy of each stage: a trip filters a round (k-mer, sliding minimum, occupancy bit) and queues its
    // survivors; the drain runs when the queue has fewer than 64 places left, and until it is empty after the last round.
    // (Nothing of a round is live across the drain but the next round's byte: the kernels that call this sit at their
    // register limits, and the line of index_probe_at is sixteen registers.)
    uint32_t count = 0; // entries in the queue (wave-uniform); the drain takes them from the top
    bool any_solid = false;
    uint64_t cur_carry = uni64(kmer);
    uint8_t c_next = ld(i + (uint32_t)lane0);
#pragma unroll 1
    for (uint32_t r = 0; r < (uint32_t)REV_BLOCK; r++) {
        {
            // (an opaque copy of the lane id per stage: the lane constants -- addresses, shift counts, masks -- are then
            // made where they are used instead of being kept in registers across the other stage and the caller's code)
            int ln = lane0;
            asm volatile("" : "+v"(ln));
            const uint8_t c8 = c_next;
            if (r + 1u < (uint32_t)REV_BLOCK)
                c_next = ld(i + 64u * (r + 1u) + (uint32_t)ln);
            const uint64_t carry_in = cur_carry;
            const uint64_t km = lane_kmer64_dpp(cur_carry, (uint32_t)nuc2bit(c8), ln, mask);
            outp[64u * r + (uint32_t)ln] = c8; // mod.rs:100, ahead of the answer: a round that is not committed is written again
            if (ln == 63)
                carry[r] = km;
            // (wave_carry(km), written out: through the call every kernel that comes here is scheduled differently)
            cur_carry = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(km >> 32), 63) << 32) |
                        (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)km, 63);
            const uint32_t h = mmer_hash((uint32_t)km & mm, m);
            uint32_t best = h, cur = h;
#pragma unroll
            for (uint32_t s = 1; s < REV_MAX_W; s++)
                if (s < w) { // wave-uniform
                    // lane l takes lane l - 1's value across the rows; lane 0 takes the hash s positions in front of the
                    // span: window s - 1 of the carried k-mer (scalar arithmetic, no vector instruction)
                    const uint32_t front = mmer_hash((uint32_t)(carry_in >> (2u * (s - 1u))) & mm, m);
                    cur = (uint32_t)__builtin_amdgcn_update_dpp((int)front, (int)cur, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
                    best = cur < best ? cur : best;
                }
            const uint32_t home = index_line_of(best, idx.line_shift);
            bool occ = (idx.line_bits[home >> 5] >> (home & 31u)) & 1u;
            if (HAS_SKIP && i + 64u * r + (uint32_t)ln < skip_until)
                occ = false; // (known not solid: error_len asked about it behind a trigger that failed)
            const uint64_t em = __ballot(occ);
            if (occ) {
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(em >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)em, 0u));
                q[count + rank] = make_uint4((uint32_t)km, (uint32_t)(km >> 32), home, (r << 6) | (uint32_t)ln);
            }
            count += (uint32_t)__builtin_popcountll(em);
            __builtin_amdgcn_wave_barrier();
        }
        while (count > REV_QUEUE - 64u || (r + 1u == (uint32_t)REV_BLOCK && count)) {
            const uint32_t cnt = count < 64u ? count : 64u;
            bool sol = false;
            int ln = lane0;
            asm volatile("" : "+v"(ln));
            if ((uint32_t)ln < cnt) {
                const uint4 e = q[count - cnt + (uint32_t)ln];
                const uint64_t fwd = ((uint64_t)e.y << 32) | e.x;
                const uint64_t rc = revcomp(fwd, k);
                const uint64_t key = (((popc64(fwd) & 1) ? rc : fwd) >> 1) + 1ull;
                int a = index_probe_at(idx, key, e.z, 0u);
                if (a == 2) { // "cannot say": settled here, as set_get does
                    if (bits) {
                        const uint64_t hh = key - 1ull; // khash(fwd, k)
                        a = (bits[hh >> 5] >> (hh & 31u)) & 1u;
                    } else {
                        const uint32_t last = 0xffffffffu >> idx.line_shift;
                        for (uint32_t hop = 1; a == 2 && hop <= last; hop++)
                            a = index_probe_at(idx, key, e.z, hop);
                    }
                }
                sol = a == 1;
            }
            if (__ballot(sol)) { // rare in a reverse pass
                any_solid = true;
                if (sol) {
                    const uint32_t tag = q[count - cnt + (uint32_t)ln].w; // (read again: not kept across the probe)
                    atomicOr(ans + (tag >> 6), 1ull << (tag & 63u));
                }
            }
            count -= cnt;
            __builtin_amdgcn_wave_barrier();
        }
    }

    // ---- the trigger test over the block's answer words (mod.rs:73, 99) -------------------------------------------
    uint32_t t = 0;
    if (!any_solid) {
        // no solid k-mer in the block (nearly always): only `previous` can trigger, at the block's first position
        t = prev ? 0u : (uint32_t)REV_BLOCK;
    } else {
        bool pv = prev;
        for (; t < (uint32_t)REV_BLOCK; t++) {
            const uint64_t bs = uni64(ans[t]);
            if (~bs & ((bs << 1) | (pv ? 1ull : 0ull)))
                break;
            pv = (bs >> 63) & 1ull;
        }
        if (t)
            prev = pv;
    }
    if (t)
        kmer = uni64(carry[t - 1u]);
    __builtin_amdgcn_wave_barrier();
    return t;
}
#endif

// the kernels specialised for k = 19 and k = 21 beside the general form: f(std::integral_constant<int, 19 / 21 / 0>)
template <class F>
void dispatch_k(int k, F f)
{
    if (k == 19)
        f(std::integral_constant<int, 19>{});
    else if (k == 21)
        f(std::integral_constant<int, 21>{});
    else
        f(std::integral_constant<int, 0>{});
}

struct LanePassInfo {
    uint64_t in_total_bound; // upper bound of the pass's input bases (sizes the unit tables and the unit staging)
    int method;              // BRX_ONE, BRX_GRAPH or BRX_GAP_SIZE
    uint64_t path_lists;     // visited lists the chain has sized for this attempt (the walk redo cuts its grid from them)
};
// A pass of One, Graph or GapSize with one lane per chunk of a read (brx_onelane.hip), as planned: plan.form is PASS_LANE.
int lane_pass(brx_chain *ch, const PassParams &p, const PassPlan &plan, const LanePassInfo &info, hipStream_t s);
void lane_ws_free(brx_chain *ch);
// the group kernel over a list of reads (p.only / p.only_n): brx_one.hip, brx_group.hip
int launch_one_list(const PassParams &p, hipStream_t s);
int launch_walk_list(const PassParams &p, int method, uint64_t path_lists, hipStream_t s);
// one_kernel over the whole batch at the planned width (brx_one.hip)
void launch_one(const PassParams &p, int width, uint32_t blocks, hipStream_t s);
// a pass of the group kernels as planned (brx_group.hip); a reverse pass in lean form, plan.form PASS_REV_LEAN (brx_revscan.hip)
int launch_group(PassParams p, const PassPlan &pl, const brx_method_t &md, uint32_t blocks, const char *timer, hipStream_t s);
int launch_rev_lean(brx_chain *ch, PassParams p, const PassPlan &pl, const brx_method_t &md, uint64_t path_lists, hipStream_t s);
} // namespace brx
