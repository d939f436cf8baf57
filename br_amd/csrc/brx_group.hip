// Per-read correction scan on gfx950.
//
// Reference: Corrector::correct (src/correct/mod.rs:53-107), Exist<S>::correct_error
// (src/correct/exist/mod.rs:112-150), ScenarioOne (src/correct/exist/one.rs:33-74),
// run_correction's per-record body (src/lib.rs:42-55).
//
// Execution model.  The reference scan is sequential inside a read (i, kmer, previous and the
// output length are loop carried) but every decision is a KmerSet::get, i.e. a random 1-bit
// probe into a 2^(2k-4)-byte table in HBM.  A read is walked by a GROUP of G lanes of one
// wavefront (G = 16/32/64, several reads per wave) that runs a small state machine; in every
// ROUND each lane of every group issues at most one probe, all probes of the wave go out in one
// global_load, and the group then reduces its G answers with a wave ballot:
//
//   SCAN   lanes probe the next G positions speculatively (lane l rolls kmer+bases[i..i+l]);
//          the ballot gives a G-bit solidity mask; the first `!solid && previous` bit is the
//          reference's error trigger; positions before it are accepted (copied to the output).
//   ALTS   4 lanes probe the alternatives of the last base       (alt_nucs, mod.rs:114-128)
//   SCEN   3*c lanes probe the c look-ahead k-mers of I/S/D      (get_score, exist/mod.rs:21-47)
//   MORE   <=3 lanes probe the tie-break k-mer                   (one_more, exist/mod.rs:49-70)
//
// The machine reproduces the reference's results exactly; only the order in which probes are
// issued differs (probes are pure).  Output goes to a per-read slot of a staging buffer
// (capacity = input length * (1 + slack/4) + 64); the reverse pass reads its input back to
// front instead of materialising a reversed copy (src/lib.rs:111 reverses, does not complement).
#include "brx_correct.hpp"

using namespace brx;

namespace {

enum { MODE_ONE = 0, MODE_GRAPH = 1, MODE_INSSUB = 2, MODE_TWO = 3 };

// ---- ScenarioTwo (src/correct/exist/two.rs:34-328), ids in declaration order ---------------------
enum { T_II, T_IS, T_SS, T_SD, T_DD, T_ICI, T_ICS, T_ICD, T_SCI, T_SCS, T_SCD, T_DCI, T_DCD, T_N };

// Everything ScenarioTwo::apply needs once the 16 stage-1 probes are back:
//   K      the corrected k-mer (exist/mod.rs:129)
//   s[j]   2-bit code of seq[j], j < 4 (seq = read from the trigger position on)
//   m1     16 solidity bits: family f = bit>>2 in {B: add(K,a), C: add(add(K,s2),a),
//          D: add(add(K,s1),a), E: add(add(K,s0),a)}, a = bit&3
struct TwoCtx {
    uint64_t K;
    uint32_t s; // s0 | s1<<2 | s2<<4 | s3<<6
    uint32_t m1;
};

__device__ __forceinline__ uint32_t two_s(const TwoCtx &t, int j) { return (t.s >> (2 * j)) & 3u; }
__device__ __forceinline__ uint32_t two_fam(const TwoCtx &t, int f) { return (t.m1 >> (4 * f)) & 0xfu; }

// ScenarioTwo::apply -> (kmer, offset); only meaningful for scenarios whose validity bit is set
__device__ __forceinline__ uint64_t two_apply(const TwoCtx &t, int sc, uint64_t mask, uint32_t &off)
{
    const uint64_t K = t.K;
    const uint64_t altB = (uint64_t)(__ffs(two_fam(t, 0)) - 1) & 3u, altC = (uint64_t)(__ffs(two_fam(t, 1)) - 1) & 3u;
    const uint64_t altD = (uint64_t)(__ffs(two_fam(t, 2)) - 1) & 3u, altE = (uint64_t)(__ffs(two_fam(t, 3)) - 1) & 3u;
    switch (sc) {
    case T_II: off = 3; return K;                                                    // two.rs:96
    case T_IS: off = 2; return K;                                                    // two.rs:97
    case T_SS: off = 2; return add_nuc(K, altB, mask);                               // two.rs:98-114
    case T_SD: off = 1; return add_nuc(K, altB, mask);                               // two.rs:115-126
    case T_DD: off = 0; return add_nuc(K, altB, mask);                               // two.rs:127-134
    case T_ICI: off = 4; return add_nuc(K, two_s(t, 3), mask);                       // two.rs:135-148
    case T_ICS: off = 3; return add_nuc(K, altB, mask);                              // two.rs:149-166
    case T_ICD: off = 3; return add_nuc(add_nuc(K, two_s(t, 2), mask), altC, mask);  // two.rs:167-181
    case T_SCI:
    case T_DCI: off = 4; return add_nuc(add_nuc(K, two_s(t, 1), mask), two_s(t, 3), mask); // two.rs:182-191,231-240
    case T_SCS: off = 3; return add_nuc(add_nuc(K, two_s(t, 1), mask), altD, mask);  // two.rs:192-215
    case T_SCD: off = 2; return add_nuc(add_nuc(K, two_s(t, 1), mask), altD, mask);  // two.rs:216-230
    default: off = 1; return add_nuc(add_nuc(K, two_s(t, 0), mask), altE, mask);     // DCD two.rs:241-254
    }
}

// which scenarios return Some(..) from apply AND pass get_score's `get(kmer)` test (exist/mod.rs:22-25)
__device__ __forceinline__ uint32_t two_valid(const TwoCtx &t, uint32_t rem)
{
    const uint32_t B = two_fam(t, 0), C = two_fam(t, 1), D = two_fam(t, 2), E = two_fam(t, 3);
    const bool nB = __popc(B) == 1, nC = __popc(C) == 1, nD = __popc(D) == 1, nE = __popc(E) == 1;
    const bool b_s1 = (B >> two_s(t, 1)) & 1u, b_s3 = (B >> two_s(t, 3)) & 1u;
    const bool d_s2 = (D >> two_s(t, 2)) & 1u, d_s3 = (D >> two_s(t, 3)) & 1u;
    uint32_t v = (1u << T_II) | (1u << T_IS);
    if (rem >= 2 && !b_s1 && nB) v |= 1u << T_SS;
    if (nB) v |= (1u << T_SD) | (1u << T_DD);
    if (rem >= 4 && b_s3) v |= 1u << T_ICI;
    if (rem >= 4 && !b_s1 && nB) v |= 1u << T_ICS;
    if (rem >= 4 && nC) v |= 1u << T_ICD;
    if (rem >= 4 && d_s3) v |= (1u << T_SCI) | (1u << T_DCI);
    if (rem >= 3 && b_s1 && !d_s2 && nD) v |= 1u << T_SCS;
    if (rem >= 2 && nD) v |= 1u << T_SCD;
    if (rem >= 2 && nE) v |= 1u << T_DCD;
    return v;
}

// ScenarioTwo::correct -> (bases packed 2 bits each, first base in the high bits; count; offset) two.rs:258-325
__device__ __forceinline__ uint32_t two_correct(const TwoCtx &t, int sc, uint64_t mask, uint32_t &nc, uint32_t &offc)
{
    uint32_t off;
    const uint64_t ck = two_apply(t, sc, mask, off);
    switch (sc) {
    case T_II:
    case T_IS: nc = 1; offc = 2; return (uint32_t)(t.K & 3u);
    case T_SS:
    case T_SD:
    case T_DD: nc = 2; offc = off; return (uint32_t)(ck & 0xfu);
    case T_ICI: nc = 1; offc = 3; return (uint32_t)(t.K & 3u);
    case T_ICD: nc = 2; offc = off - 1; return (uint32_t)(ck & 0xfu);
    case T_ICS: nc = 2; offc = off + 1; return (uint32_t)(ck & 0xfu);
    case T_SCI:
    case T_SCS:
    case T_SCD:
    case T_DCD: nc = 3; offc = off; return (uint32_t)(ck & 0x3fu);
    default: nc = 0; offc = 1; return 0; // DCI, two.rs:323
    }
}

// ---- bio 1.6.0 alignment::pairwise::Aligner::global for Greedy (greedy.rs:56-89) ------------------
// Affine gaps (open -1, extend -1), match +1 / mismatch -1, no clipping; `>`-only updates in the
// order match/subst, ins, del; traceback through per-layer back pointers; Ins consumes x, Del y.
// Restated from the crate's published algorithm (source not in the container; tie-breaks unpinned,
// SURVEY H3) -- the same restatement the CPU checker uses, laid out here as a systolic
// anti-diagonal sweep: lane l of the group owns DP row band*G+l+1, row values travel to the next
// lane by shuffle, the back-pointer matrix lives in LDS.
enum { TBV_START = 0, TBV_INS = 1, TBV_DEL = 2, TBV_SUBST = 3, TBV_MATCH = 4, TBV_XCLIP = 5 };
enum { OPV_MATCH = 0, OPV_SUBST = 1, OPV_DEL = 2, OPV_INS = 3 };
constexpr int BIO_MIN = -858993459;

struct GreedyLds {
    uint8_t *x, *y, *ops, *bT; // x: before+read, y: before+path, ops: traceback (reversed), bT: band boundary tb_s
    int *bS, *bI;              // band boundary scores
    uint16_t *tb;              // (m+1) x (n+1) back pointers: s | i<<3 | d<<6
};

__device__ __forceinline__ GreedyLds greedy_carve(uint8_t *base, uint32_t dim)
{
    // dim = max row/column count; all regions 16-byte aligned
    const uint32_t a = (dim + 15u) & ~15u;
    GreedyLds L;
    L.x = base;
    L.y = base + a;
    L.ops = base + 2 * a;          // 2*a bytes
    L.bT = base + 4 * a;
    L.bS = (int *)(base + 5 * a);  // 4*a bytes
    L.bI = (int *)(base + 9 * a);  // 4*a bytes
    L.tb = (uint16_t *)(base + 13 * a);
    return L;
}

template <int G>
__device__ bool greedy_align(const GreedyLds &L, int gl, int m, int n, int nb, int &off_out)
{
    const int go = -1, ge = -1;
    const int W = m + 1;
    for (int band = 0; band * G < m; band++) {
        const int row = band * G + gl + 1;
        const bool arow = row <= m;
        const uint8_t pch = arow ? L.x[row - 1] : (uint8_t)0;
        int S_cur = go + ge * row, I_cur = S_cur, D_cur = BIO_MIN, S_prev1 = S_cur, tbs_cur = TBV_INS; // column 0
        const bool last_lane = (gl == G - 1);
        const bool more = (band + 1) * G < m;
        for (int t = 0; t < n + G - 1; t++) {
            int upS = __shfl_up(S_cur, 1, G), upI = __shfl_up(I_cur, 1, G);
            int upT = __shfl_up(tbs_cur, 1, G), upS1 = __shfl_up(S_prev1, 1, G);
            const int j = t - gl + 1;
            const bool act = arow && j >= 1 && j <= n;
            if (act) {
                if (gl == 0) {
                    if (band == 0) { // DP row 0
                        upS = go + ge * j;
                        upI = BIO_MIN;
                        upT = TBV_DEL;
                        upS1 = (j == 1) ? 0 : go + ge * (j - 1);
                    } else {
                        upS = L.bS[j];
                        upI = L.bI[j];
                        upT = L.bT[j];
                        upS1 = L.bS[j - 1];
                    }
                }
                const uint8_t q = L.y[j - 1];
                const int m_score = upS1 + (pch == q ? 1 : -1);
                int bestI, tbi, bestD, tbd;
                const int i_score = upI + ge, s_score = upS + go + ge;
                if (i_score > s_score) { bestI = i_score; tbi = TBV_INS; } else { bestI = s_score; tbi = upT; }
                const int d_score = D_cur + ge, s2 = S_cur + go + ge;
                if (d_score > s2) { bestD = d_score; tbd = TBV_DEL; } else { bestD = s2; tbd = tbs_cur; }
                int bestS = BIO_MIN, tbs = TBV_XCLIP;
                if (m_score > bestS) { bestS = m_score; tbs = (pch == q) ? TBV_MATCH : TBV_SUBST; }
                if (bestI > bestS) { bestS = bestI; tbs = TBV_INS; }
                if (bestD > bestS) { bestS = bestD; tbs = TBV_DEL; }
                S_prev1 = S_cur;
                S_cur = bestS;
                I_cur = bestI;
                D_cur = bestD;
                tbs_cur = tbs;
                L.tb[j * W + row] = (uint16_t)(tbs | (tbi << 3) | (tbd << 6));
                if (last_lane && more) {
                    L.bS[j] = bestS;
                    L.bI[j] = bestI;
                    L.bT[j] = (uint8_t)tbs;
                }
            }
        }
        if (last_lane && more)
            L.bS[0] = go + ge * row;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

    // traceback from (m, n); every lane walks the same pointers (LDS broadcast reads)
    auto tbS = [&](int i, int j) -> int {
        if (i == 0) return j == 0 ? TBV_START : TBV_DEL;
        if (j == 0) return TBV_INS;
        return L.tb[j * W + i] & 7;
    };
    auto tbI = [&](int i, int j) -> int {
        if (j == 0) return i == 1 ? TBV_START : TBV_INS;
        return (L.tb[j * W + i] >> 3) & 7; // i >= 1 whenever the Ins layer is entered
    };
    auto tbD = [&](int i, int j) -> int {
        if (i == 0) return j == 1 ? TBV_START : TBV_DEL;
        return (L.tb[j * W + i] >> 6) & 7;
    };
    int i = m, j = n, nops = 0;
    int layer = tbS(i, j);
    while (nops < m + n + 2) {
        int next, op;
        if (layer == TBV_INS) { op = OPV_INS; next = tbI(i, j); i--; }
        else if (layer == TBV_DEL) { op = OPV_DEL; next = tbD(i, j); j--; }
        else if (layer == TBV_MATCH || layer == TBV_SUBST) { op = (layer == TBV_MATCH) ? OPV_MATCH : OPV_SUBST; next = tbS(i - 1, j - 1); i--; j--; }
        else break;
        if (gl == 0)
            L.ops[nops] = (uint8_t)op;
        nops++;
        layer = next;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    // operations[before_seq.len()..].windows(2), greedy.rs:67-86 (ops are stored back to front)
    int offset = 0;
    for (int w = nb; w + 1 < nops; w++) {
        const int a = L.ops[nops - 1 - w], b = L.ops[nops - 2 - w];
        if (a == OPV_DEL) offset -= 1;
        else if (a == OPV_INS) offset += 1;
        if (a == OPV_MATCH && b == OPV_MATCH) {
            int oc = 0;
            for (int e = 0; e < nops; e++) {
                const int op = L.ops[e];
                if (op == OPV_DEL) oc -= 1;
                else if (op == OPV_INS) oc += 1;
                else break;
            }
            off_out = offset - oc;
            return true;
        }
    }
    return false;
}

// bit of a k-mer in the 32*G-bit visited filter of a walk
__device__ __forceinline__ uint32_t walk_filter_index(uint64_t kmer, int G)
{
    const uint32_t x = (uint32_t)(kmer ^ (kmer >> 23) ^ (kmer >> 41)) * 0x9E3779B1u;
    return x >> (32 - 5 - (G == 4 ? 2 : G == 8 ? 3 : G == 16 ? 4 : G == 32 ? 5 : 6));
}

// index of the n-th (0-based) set bit of a small mask
__device__ __forceinline__ uint32_t nth_bit(uint32_t mask, uint32_t n)
{
    for (uint32_t q = 0; q < n; q++)
        mask &= mask - 1u;
    return (uint32_t)__ffs(mask) - 1u;
}

// look-aheads per surviving scenario in a TSCORE round (Two): one while every valid scenario is still in, then as
// many as the group's lanes allow
__device__ __forceinline__ uint32_t two_width(uint32_t sub, uint32_t c, int G, uint32_t alive)
{
    const uint32_t left = c - sub;
    const uint32_t na = (uint32_t)__popc(alive);
    uint32_t cap = sub == 0u ? 1u : (uint32_t)G / (na ? na : 1u);
    if (cap < 1u)
        cap = 1u;
    return left < cap ? left : cap;
}

// SRC: where the work comes from -- 0 every read of the batch, 1 the reads of a list made on the device (p.only), 2 the
// triggers a lean reverse pass left open (p.trig; see rev_scan_kernel): the group enters at alt_nucs, writes nothing, and
// flags the read for a redo unless the method returns None
template <int G, int M, int SRC = 0>
// One fits 80 VGPRs without spilling: 6 waves per SIMD instead of 5 (the kernel waits on memory 60 % of the
// time, measured 8 % faster), and its 64-lane form (no group shuffles to keep) fits 72: 7 waves; the other methods
// keep the compiler's own choice
// Greedy: the compiler's own choice is 110 registers = 4 waves per SIMD; its LDS (the alignment table, ~2 KB a group)
// allows 5.  Held to 96 registers (20 bytes of scratch) it runs 5: 79.7 -> 69.1 ms per Gbp fwd+rev on the same box
// (profiles/r4m_greedy_ab.txt) -- a round of a group is a dependent trip to memory, and more groups hide it.
#ifndef BRX_GREEDY_WAVES
#define BRX_GREEDY_WAVES 5
#endif
// Two: the compiler's choice is 101 registers = 5 waves; held to 85 it runs 6: 65.2 -> 54.8 ms per Gbp fwd+rev (7 waves,
// 72 registers: 64.2 -- spills).  Graph's group kernel (92 registers, 5 waves) does not move at 6: 50.95 / 51.56.
#ifndef BRX_TWO_WAVES
#define BRX_TWO_WAVES 6
#endif
#ifndef BRX_GAPSIZE_WAVES
#define BRX_GAPSIZE_WAVES 5
#endif
#ifndef BRX_GRAPH_WAVES
#define BRX_GRAPH_WAVES 1 // (92 registers = 5 waves)
#endif
__global__ __launch_bounds__(256, (M == BRX_ONE ? (G == 64 ? 7 : 6)
                                                : (M == BRX_GAP_SIZE ? BRX_GAPSIZE_WAVES : (M == BRX_GREEDY ? BRX_GREEDY_WAVES : (M == BRX_TWO ? BRX_TWO_WAVES : BRX_GRAPH_WAVES))))) void correct_kernel(PassParams p)
{
    constexpr bool HAS_ERRLEN = (M == BRX_GRAPH || M == BRX_GAP_SIZE);
    constexpr bool HAS_ONE = (M == BRX_ONE || M == BRX_GAP_SIZE);
    constexpr bool HAS_WALK = HAS_ERRLEN;
    constexpr bool HAS_TWO = (M == BRX_TWO);
    constexpr bool HAS_GREEDY = (M == BRX_GREEDY);
    constexpr bool HAS_PATH = HAS_WALK || HAS_GREEDY;
    constexpr bool LIST = SRC == 1, VERIFY = SRC == 2;
    extern __shared__ __attribute__((aligned(16))) uint8_t dyn_lds[];

    const int lane = threadIdx.x & 63;
    const int gl = lane & (G - 1);
    const int gshift = lane & ~(G - 1);
    const uint64_t GM = (G == 64) ? ~0ull : ((1ull << (G & 63)) - 1ull);
    const int k = p.k;
    const uint32_t c = (uint32_t)p.c;
    const uint64_t mask = kmask(k);
    const uint32_t gid = blockIdx.x * (256 / G) + threadIdx.x / G; // global group index (path scratch slot)
    unsigned long long *path = HAS_PATH ? (unsigned long long *)p.path_k + (uint64_t)gid * p.maxpath : nullptr;
    GreedyLds gL = {};
    if (HAS_GREEDY)
        gL = greedy_carve(dyn_lds + (size_t)(threadIdx.x / G) * p.g_lds_bytes, p.g_dim);

    // group-uniform state (replicated in every lane of the group)
    uint32_t r = 0, n = 0, cap = 0, i = 0, olen = 0;
    const uint8_t *in = nullptr;
    uint8_t *out = nullptr;
    uint64_t kmer = 0, corr = 0;
    bool prev = false, have = false;
    int st = ST_INIT, mode = HAS_TWO ? MODE_TWO : (M == BRX_GRAPH ? MODE_GRAPH : MODE_ONE);
    uint32_t sub = 0, failmask = 0, passmask = 0;
    uint8_t ch_t = 0;
    uint32_t hop = 0;  // consecutive re-runs of the current round (sparse sets: which line of the chain is probed)
    bool slow = false; // this round is the bitset re-run of a round the probe index could not answer
    bool was_unres = false, kept_sol = false; // per lane: its probe of that round was unanswered / its answer
    // error_len / walk state
    uint32_t elen = 0, ej = 0, npath = 0, gap = 0;
    // Graph / GapSize: error_len (mod.rs:130-152) has probed the k-mers that end at i + 1 .. i + elen - 1 and found none
    // solid.  When the trigger then FAILS, the scan goes on over exactly those k-mers (the read's base stays in the
    // k-mer, mod.rs:91-96), so positions below skip_until are copied through without asking again.  In a reverse pass
    // -- where a trigger is a chance hit and error_len runs to the end of the read -- that is the rest of the read.
    uint32_t skip_until = 0;
    uint64_t fc = 0, ek = 0, wk = 0;
    // Brent cycle detector of the graph walk (see ST_WALK)
    uint64_t tort = 0;
    uint32_t bpow = 1, blam = 0;
    bool brent = false;
    uint32_t wfilt = 0; // this lane's 32 bits of the walk's visited-filter (exact-scan walks)
    TwoCtx tw = {0, 0, 0};
    uint32_t tvalid = 0;
    // greedy state: iteration, path length in bases, alignment offset
    uint32_t git = 0, gnl = 0, steps = 0;
    int goff = 0;
    // ... and its viewed set (greedy.rs:136): <= max_search + 1 k-mers, kept one per lane of the group when it has that
    // many lanes (a scan of the chain's list in memory was a dependent round trip per iteration)
    uint64_t gvis = 0;
    const bool greg = HAS_GREEDY && (uint32_t)p.max_search + 1u <= (uint32_t)G;
    // statistics
    // per-wave totals (wave-uniform, so they live in scalar registers instead of four VGPRs of a kernel that is at its
    // register limit): the lanes note their events of a round in `ev`, the end of the round ballots them
    uint32_t n_rounds = 0, n_probes = 0, n_trig = 0, n_fix = 0;
    enum { EV_ROUND = 1, EV_PROBE = 2, EV_TRIG = 4, EV_FIX = 8 };

    auto fetch = [&]() {
        for (;;) {
            unsigned long long w = 0;
            if (gl == 0)
                w = atomicAdd(p.ctrl + CTL_WORK, 1ull);
            w = __shfl(w, gshift);
            // LIST: the reads of a list made on the device (what the lane-per-chunk pass handed back)
            unsigned long long n_work = (unsigned long long)p.n_reads;
            if (LIST || VERIFY)
                n_work = *p.only_n;
            if (VERIFY && n_work > (unsigned long long)p.trig_cap)
                n_work = p.trig_cap; // (triggers beyond the buffer were not recorded: their reads were handed back whole)
            if (w >= n_work) {
                have = false;
                return;
            }
            have = true;
            TrigRec tr = {0, 0, 0, 0, 0};
            if (VERIFY)
                tr = p.trig[w];
            r = VERIFY ? tr.r : (LIST ? p.only[w] : (uint32_t)w);
            const uint64_t o0 = p.offsets[r], o1 = p.offsets[r + 1];
            if (p.in_staged) {
                in = p.in + slot_of(o0, r, p.slack);
                n = p.in_lens[r];
                if (n == 0xffffffffu) {
                    // an earlier pass of this attempt gave up on this read (slot or walk-list
                    // overflow): keep it poisoned; the host redoes the batch with more workspace
                    if (gl == 0)
                        p.out_lens[r] = 0xffffffffu;
                    continue;
                }
            } else {
                in = p.in + o0;
                n = (uint32_t)(o1 - o0);
            }
            const uint64_t s0 = slot_of(o0, r, p.slack), s1 = slot_of(o1, (uint64_t)r + 1, p.slack);
            out = p.out + s0;
            cap = (uint32_t)(s1 - s0);
            st = ST_INIT;
            i = 0;
            olen = 0;
            kmer = 0;
            prev = false;
            steps = 0;
            skip_until = 0;
            if (VERIFY) {
                // enter where the scan's trigger branch and error_len would have left the group (mod.rs:73-75 with
                // mod.rs:130-152 / gap_size.rs:97-108): the read is unchanged up to the trigger
                i = tr.i;
                olen = tr.i;
                uint64_t km = 0;
                for (int j = 0; j < k; j++)
                    km = (km << 2) | nuc2bit(in[p.flip ? (n - 1u - (tr.i + 1u - (uint32_t)k + (uint32_t)j)) : (tr.i + 1u - (uint32_t)k + (uint32_t)j)]);
                kmer = km;
                ch_t = in[p.flip ? (n - 1u - tr.i) : tr.i];
                elen = tr.elen;
                fc = tr.fc;
                if (HAS_TWO)
                    mode = MODE_TWO;
                else if (M == BRX_GRAPH)
                    mode = MODE_GRAPH;
                else if (M == BRX_GAP_SIZE) {
                    mode = elen < (uint32_t)k ? MODE_GRAPH : (elen == (uint32_t)k ? MODE_ONE : MODE_INSSUB);
                    gap = elen > (uint32_t)k ? elen - (uint32_t)k : 0u;
                } else
                    mode = MODE_ONE;
                st = ST_ALTS;
            }
            return;
        }
    };
    // logical base j of the current read (the reverse pass reads the buffer back to front)
    auto ld = [&](uint32_t j) -> uint8_t { return in[p.flip ? (n - 1u - j) : j]; };
    // A read is finished (or given up) at ONE place, the end of the round: every call site of an inlined fetch() redefines
    // the whole group state and costs a block of register copies at the join (one_kernel: 7 000 -> 4 900 lines of ISA)
    int done = 0; // 0 no, 1 finished, 16 + the CTL_* counter of the reason the read was given up
    bool flag_read = false; // VERIFY: this trigger does not end in None (or outgrew a workspace): the read is redone
    auto end_read = [&](int how) {
        if (VERIFY && how != 1) {
            flag_read = true;
            done = 1;
        } else {
            done = how;
        }
    };
    auto finish = [&]() { end_read(1); };
    auto overflow = [&]() { end_read(16 + CTL_OVERFLOW); };
    auto nonterminating = [&]() { end_read(16 + CTL_NONTERM); };
    auto path_overflow = [&]() { end_read(16 + CTL_PATHOVF); };
    // k-mer of this lane after appending the 2-bit codes of lanes 0..gl of the group to `carry`
    auto lane_kmer = [&](uint64_t carry, uint64_t code) -> uint64_t {
        uint64_t val = code;
#pragma unroll
        for (int d = 1; d < G && d < 32; d <<= 1) {
            const uint64_t other = __shfl_up(val, d, G);
            if (gl >= d)
                val |= other << (2 * d);
        }
        const int nb = gl + 1;
        return (nb >= k) ? (val & mask) : (((carry << (2 * nb)) | val) & mask);
    };

    // 2-bit codes of the first WB = min(G, 32) lanes of the group, lane 0's base in the top bits
    constexpr int WB = G < 32 ? G : 32;
    auto group_window = [&](uint64_t code) -> uint64_t {
        uint64_t val = code;
#pragma unroll
        for (int d = 1; d < WB; d <<= 1) {
            const uint64_t other = __shfl_up(val, d, G);
            if (gl >= d)
                val |= other << (2 * d);
        }
        return __shfl(val, gshift + WB - 1);
    };
    // km extended by the window bases b0 .. b0+nb-1 (b0 + nb <= WB, nb <= 31)
    auto ext = [&](uint64_t km, uint64_t W, uint32_t b0, uint32_t nb) -> uint64_t {
        const uint64_t bits = (W >> (2u * ((uint32_t)WB - b0 - nb))) & ((1ull << (2u * nb)) - 1ull);
        return ((km << (2u * nb)) | bits) & mask;
    };
    uint64_t win = 0; // bases seq[i .. i+WB) at the current trigger

    fetch();

    while (__any(have)) {
        if (G == 64) {
            // trigger-free rounds of the 64-lane form (every method's reverse pass is almost only these) in a loop of
            // their own, as in one_kernel: 64 positions, one probe each, ballot, accept; a round with a trigger is
            // left to the general code below, which redoes its (pure) probes
            // (REV_BLOCK rounds at a time where the occupancy bits can filter them: rev_block_rounds, brx_correct.hpp.  Not
            // Greedy's kernel: its alignment already takes dynamic LDS per group, and with the queue's 8 KB beside it
            // configs[2] measured 902 ms per step against 891)
            while (!HAS_GREEDY && p.rev_batch && have && st == ST_SCAN && !slow && n - i >= 64u * REV_BLOCK + 1u && olen + 64u * REV_BLOCK + 2u <= cap) {
                const uint8_t *const in_b = (const uint8_t *)uni64((uint64_t)in);
                uint8_t *const out_b = (uint8_t *)uni64((uint64_t)(out + olen));
                const uint32_t n_b = uni32(n), i_b = uni32(i);
                const bool flip_b = p.flip != 0;
                const uint32_t t = rev_block_rounds<HAS_ERRLEN>(p.idx, p.bits, k, mask, lane,
                                                                [in_b, n_b, flip_b](uint32_t j) -> uint8_t { return in_b[flip_b ? (n_b - 1u - j) : j]; }, i_b,
                                                                out_b, uni32(skip_until), kmer, prev);
                olen += 64u * t;
                i += 64u * t;
                n_rounds += t;
                n_probes += 64u * t;
                steps += t;
                if (t < (uint32_t)REV_BLOCK)
                    break;
            }
            while (have && st == ST_SCAN && !slow && n - i >= 65u && olen + 66u <= cap) {
                const uint8_t c8 = ld(i + (uint32_t)lane);
                const uint64_t km = lane_kmer64_dpp(kmer, (uint32_t)nuc2bit(c8), lane, mask);
                bool s1 = false;
                if (HAS_ERRLEN && i + (uint32_t)lane < skip_until) {
                    // (known not solid: error_len asked about it behind the trigger that failed)
                } else if (p.idx.lines) {
                    // (an overflowed index line is settled by the lane that met it, set_get: leaving the round to the
                    // general code and its re-run cost two full rounds of the group, ten times per 10 kb read)
                    s1 = set_get<true, LINE_BITS_KEPT>(p.idx, p.bits, km, k);
                } else {
                    s1 = probe(p.bits, km, k);
                }
                const uint64_t bs = __ballot(s1);
                const uint64_t trig = ~bs & ((bs << 1) | (prev ? 1ull : 0ull)); // mod.rs:73
                if (trig)
                    break;
                out[olen + (uint32_t)lane] = c8; // mod.rs:100
                olen += 64u;
                i += 64u;
                kmer = wave_carry(km);
                prev = (bs >> 63) & 1ull; // mod.rs:99
                n_rounds += 1u;
                n_probes += 64u;
                steps++;
            }
            // error_len (mod.rs:130-152) in a loop of its own, too: a trigger of a REVERSE pass is a chance hit, and error_len
            // then runs to the end of the read -- 64 k-mers a round, none of them solid -- through the general round's whole
            // state dispatch (Graph's reverse pass spent 5.6 G vector instructions where One's spends 2.6 G).  Full blocks
            // without a solid k-mer stay here; the block that ends the search (a hit, the end of the read) is left to the
            // general code, which redoes its (pure) probes.
            while (HAS_ERRLEN && have && st == ST_ERRLEN && !slow && n - i > ej + 1u + 64u) {
                const uint8_t c8 = ld(i + ej + 1u + (uint32_t)lane);
                const uint64_t km = lane_kmer64_dpp(ek, (uint32_t)nuc2bit(c8), lane, mask);
                const bool s1 = p.idx.lines ? set_get<true, LINE_BITS_KEPT>(p.idx, p.bits, km, k) : probe(p.bits, km, k);
                if (__ballot(s1))
                    break;
                ek = wave_carry(km);
                ej += 64u;
                n_rounds += 1u;
                n_probes += 64u;
                steps++;
            }
        }
        if (HAS_WALK) {
            // Walk steps (graph.rs:61-82, gap_size.rs:57-85) in a loop of their own, too: four probes, one successor, the
            // cycle detector's bookkeeping, the list -- a fifth of a general round's instructions.  A reverse pass's walks
            // follow the genome for hundreds to thousands of steps (the k-mer in front of a chance trigger is a genome
            // k-mer), each a dependent trip to memory, and the launch that verifies or redoes them lasts as long as the
            // walkers' steps take.  A step that ends the walk (no unique successor, a revisit, the target, the last step
            // of a fixed-length walk, a full list) changes nothing here and is left to the general round, which asks the
            // same (pure) probes again.  Narrow groups: the loop runs while at least as many groups of the wave walk as do
            // anything else, and for eight steps at most while any other group waits.
            constexpr uint64_t LEADERS = G == 64 ? 1ull : (G == 32 ? 0x0000000100000001ull : (G == 16 ? 0x0001000100010001ull : (G == 8 ? 0x0101010101010101ull : 0x1111111111111111ull)));
            for (uint32_t it = 0;; it++) {
                const bool wfast = have && st == ST_WALK && !slow && (brent || mode == MODE_INSSUB);
                const uint32_t nw = (uint32_t)__builtin_popcountll(__ballot(wfast) & LEADERS);
                const uint32_t no = (uint32_t)__builtin_popcountll(__ballot(have && !wfast) & LEADERS);
                if (nw == 0u || nw < no || (no != 0u && it >= 8u))
                    break;
                bool s1 = false, u1 = false;
                if (wfast && gl < 4) {
                    const uint64_t q = add_nuc(wk, (uint64_t)gl, mask); // next_nucs(kmer), mod.rs:118-128
                    if (p.idx.lines) {
                        const int pr = index_probe(p.idx, q, k);
                        s1 = pr == 1;
                        u1 = pr == 2;
                    } else {
                        s1 = probe(p.bits, q, k);
                    }
                }
                if (__ballot(u1))
                    break; // an overflowed index line: the general round and its re-run settle it
                const uint32_t am = (uint32_t)((__ballot(s1) >> gshift) & 0xfull);
                bool simple = wfast && __popc(am) == 1;
                uint64_t nk = 0;
                if (simple) {
                    nk = add_nuc(wk, (uint64_t)(__ffs(am) - 1), mask);
                    simple = !(brent && nk == tort) && !(!brent && npath >= p.maxpath) &&
                             !(mode == MODE_GRAPH ? nk == fc : gap <= 1u) && steps < (1u << 24) + 64u * n;
                }
                if (simple) {
                    if (brent && ++blam == bpow) {
                        tort = nk;
                        bpow *= 2u;
                        blam = 0;
                    }
                    if (gl == 0 && npath < p.maxpath)
                        __hip_atomic_store(path + npath, (unsigned long long)nk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (npath < 0xfffffff0u)
                        npath++;
                    wk = nk;
                    if (mode != MODE_GRAPH)
                        gap--;
                    steps++;
                }
                n_rounds += nw;
                n_probes += 4u * nw;
                if (__ballot(wfast && !simple))
                    break;
            }
        }
        uint32_t ev = 0;
        bool do_probe = false;
        uint64_t pk = 0;
        uint8_t ch = 0;
        uint32_t sc_s = 0; // scenario index of this lane in SCEN / TSCORE
        bool sc_active = false;

        // ---------------- phase 1: choose this round's probe --------------------------------
        if (have) {
            ev |= (gl == 0) ? EV_ROUND : 0u;
            if (st == ST_INIT) {
                if (n < (uint32_t)k) {
                    // mod.rs:56-58: shorter than k, returned verbatim (cap >= n + 64 always)
                    for (uint32_t j = gl; j < n; j += G)
                        out[j] = ld(j);
                    olen = n;
                } else {
                    uint64_t km = 0;
                    for (int j = 0; j < k; j++)
                        km = (km << 2) | nuc2bit(ld((uint32_t)j));
                    kmer = km;
                    for (uint32_t j = gl; j < (uint32_t)k; j += G)
                        out[j] = ld(j);
                    olen = (uint32_t)k;
                    i = (uint32_t)k;
                    do_probe = (gl == 0);
                    pk = kmer;
                }
            } else if (st == ST_SCAN) {
                const uint32_t pos = i + (uint32_t)gl;
                const bool valid = pos < n;
                ch = valid ? ld(pos) : (uint8_t)0;
                pk = lane_kmer(kmer, nuc2bit(ch));
                do_probe = valid && !(HAS_ERRLEN && pos < skip_until);
            } else if (HAS_ERRLEN && st == ST_ERRLEN) {
                // error_len, mod.rs:130-152: probe seq[i+1..] until the first solid k-mer
                const uint32_t rem = n - i;
                const uint32_t j = ej + 1u + (uint32_t)gl;
                const bool valid = j < rem;
                const uint8_t c2 = valid ? ld(i + j) : (uint8_t)0;
                pk = lane_kmer(ek, nuc2bit(c2));
                do_probe = valid;
            } else if (st == ST_ALTS) {
                // alt_nucs: the alternative equal to the read's own base IS the trigger k-mer, already
                // known to be non-solid -> three probes instead of four
                do_probe = gl < 4 && ((p.flags & 2u) || (uint64_t)gl != (kmer & 3ull));
                pk = add_nuc(kmer >> 2, (uint64_t)gl, mask);
                if ((HAS_ONE || HAS_TWO || HAS_GREEDY) && !(p.flags & 8u)) {
                    // the bases the scenarios will look at, fetched once (one coalesced load per group)
                    const uint32_t wp = i + (uint32_t)gl;
                    win = group_window((gl < WB && wp < n) ? nuc2bit(ld(wp)) : 0ull);
                }
            } else if (HAS_ONE && st == ST_SCEN) {
                // get_score look-ahead, staged: look-ahead k-mers [sub, sub+width) of the three
                // scenarios per round (first the two nearest ones: a wrong scenario almost always dies
                // there, so its remaining probes are never issued).  Same verdict as probing all c.
                const uint32_t width = scen_width(sub, c, G, p.flags, failmask);
                const uint32_t e = (uint32_t)gl;
                const uint32_t alive = ~failmask & 7u; // never 0 here
                // which surviving scenario this lane works for: e / width by two compares (at most three scenarios)
                const uint32_t ord = (e >= width ? 1u : 0u) + (e >= 2u * width ? 1u : 0u);
                sc_active = e < 3u * width && ord < (uint32_t)__popc(alive);
                const uint32_t a1 = alive & (alive - 1u);
                sc_s = !sc_active ? 0u : (ord == 0u ? (uint32_t)__ffs(alive) - 1u : (ord == 1u ? (uint32_t)__ffs(a1) - 1u : 2u));
                const uint32_t j = sub + (sc_active ? e - ord * width : 0u);
                const uint32_t off = 2u - sc_s; // I:2 S:1 D:0 (one.rs:57-63)
                if (sc_active) {
                    if (c + 3u <= (uint32_t)WB && !(p.flags & 8u)) {
                        pk = ext(corr, win, off, j + 1u);
                    } else {
                        pk = corr;
                        for (uint32_t q = 0; q <= j; q++)
                            pk = add_nuc(pk, nuc2bit(ld(i + off + q)), mask);
                    }
                    do_probe = true;
                }
            } else if (HAS_ONE && st == ST_MORE) {
                if (gl < 3 && ((passmask >> gl) & 1u)) {
                    const uint32_t off = 2u - (uint32_t)gl;
                    const uint32_t rem = n - i;
                    if (rem > c + off + 1u) { // exist/mod.rs:54
                        if (c + 3u <= (uint32_t)WB && !(p.flags & 8u)) {
                            pk = ext(corr, win, off, c + 1u);
                        } else {
                            pk = corr;
                            for (uint32_t q = 0; q <= c; q++)
                                pk = add_nuc(pk, nuc2bit(ld(i + off + q)), mask);
                        }
                        do_probe = true;
                    }
                }
            } else if (HAS_WALK && st == ST_WALK) {
                do_probe = gl < 4; // next_nucs(kmer), mod.rs:118-128
                pk = add_nuc(wk, (uint64_t)gl, mask);
            } else if (HAS_TWO && st == ST_T1) {
                // the 16 distinct probes behind every ScenarioTwo::apply (see TwoCtx)
                const uint32_t rem = n - i;
                const int fam = gl >> 2;
                if (gl < 16) {
                    uint64_t basek = corr;
                    bool ok = true;
                    if (fam == 1) { ok = rem >= 3; basek = add_nuc(corr, two_s(tw, 2), mask); }
                    else if (fam == 2) { ok = rem >= 2; basek = add_nuc(corr, two_s(tw, 1), mask); }
                    else if (fam == 3) { basek = add_nuc(corr, two_s(tw, 0), mask); }
                    pk = add_nuc(basek, (uint64_t)(gl & 3), mask);
                    do_probe = ok;
                }
            } else if (HAS_TWO && st == ST_TSCORE) {
                // get_score of the scenarios still alive, `sub` look-aheads done so far: first the nearest k-mer of
                // every valid scenario (13 lanes; most scenarios die there), then the lanes are dealt to the survivors
                const uint32_t alive = tvalid & ~failmask;
                const uint32_t width = two_width(sub, c, G, alive);
                const uint32_t ord = (uint32_t)gl / width;
                sc_active = ord < (uint32_t)__popc(alive);
                sc_s = sc_active ? nth_bit(alive, ord) : 0u;
                const uint32_t j = sub + (uint32_t)gl % width;
                if (sc_active) {
                    uint32_t off;
                    pk = two_apply(tw, (int)sc_s, mask, off);
                    // get_score look-ahead, exist/mod.rs:33-41: seq[i+off .. i+off+j], out of the window fetched at ALTS
                    if (off + j + 1u <= (uint32_t)WB && !(p.flags & 8u)) {
                        pk = ext(pk, win, off, j + 1u);
                    } else {
                        for (uint32_t q = 0; q <= j; q++)
                            pk = add_nuc(pk, nuc2bit(ld(i + off + q)), mask);
                    }
                    do_probe = true;
                }
            } else if (HAS_TWO && st == ST_TMORE) {
                if (gl < T_N && ((passmask >> gl) & 1u)) {
                    uint32_t nc, offc;
                    const uint32_t cb = two_correct(tw, gl, mask, nc, offc);
                    const uint32_t rem = n - i;
                    if (rem > c + offc + 1u) { // exist/mod.rs:54
                        pk = corr >> 2;
                        for (uint32_t q = 0; q < nc; q++)
                            pk = add_nuc(pk, (uint64_t)((cb >> (2 * (nc - 1 - q))) & 3u), mask);
                        if (offc + c + 1u <= (uint32_t)WB && !(p.flags & 8u)) {
                            pk = ext(pk, win, offc, c + 1u);
                        } else {
                            for (uint32_t q = 0; q <= c; q++)
                                pk = add_nuc(pk, nuc2bit(ld(i + offc + q)), mask);
                        }
                        do_probe = true;
                    }
                }
            } else if (HAS_GREEDY && st == ST_GFOLLOW) {
                do_probe = gl < 4; // follow_graph -> next_nucs, greedy.rs:91-102
                pk = add_nuc(wk, (uint64_t)gl, mask);
            } else if (HAS_GREEDY && st == ST_GVALID) {
                // check_next_kmers, greedy.rs:104-117 -- and, in the lanes behind its c probes, follow_graph of the NEXT
                // iteration (next_nucs of the same k-mer, greedy.rs:91-102): an iteration of greedy's loop nearly always
                // ends in "the look-ahead does not hold, go on", and then the four answers are already there -- one round
                // per iteration instead of two (7 of the ~15 rounds of a trigger)
                const uint32_t rem2 = n - i - git;
                const uint32_t e = sub * G + (uint32_t)gl;
                if (rem2 >= c && e < c) {
                    if (git + e + 1u <= (uint32_t)WB && !(p.flags & 8u)) {
                        pk = ext(wk, win, git, e + 1u);
                    } else {
                        pk = wk;
                        for (uint32_t q = 0; q <= e; q++)
                            pk = add_nuc(pk, nuc2bit(ld(i + git + q)), mask);
                    }
                    do_probe = true;
                } else if (c + 4u <= (uint32_t)G && (uint32_t)gl >= c && (uint32_t)gl < c + 4u) {
                    pk = add_nuc(wk, (uint64_t)((uint32_t)gl - c), mask);
                    do_probe = true;
                }
            }
            // runaway guard: no read needs anywhere near this many rounds (greedy can move the read cursor
            // backwards for ever on some inputs -- the reference spins; a logic error must not hang the GPU)
            if (++steps > (1u << 24) + 64u * n)
                do_probe = false;
        }

        // ---------------- phase 2: one probe per lane, whole wave at once ---------------------
        bool sol = false;
        bool retry = false;
        if (p.idx.lines) {
            // probe index (brx_index.hpp): the line of the k-mer's minimizer, shared by the neighbouring
            // lanes.  A line that overflowed at build time cannot say "absent": the GROUP then repeats
            // this round against the bitset (phase 1 is a pure function of the group state, so the next
            // iteration recomputes the same probes); the other groups of the wave carry on.
            bool unres = false;
            if (do_probe) {
                if (!slow) {
                    const int pr = index_probe(p.idx, pk, k);
                    sol = pr == 1;
                    unres = pr == 2;
                    ev |= EV_PROBE;
                } else if (was_unres) {
                    if (p.bits) {
                        sol = probe(p.bits, pk, k);
                    } else { // sparse set: the build chained the key into the hop-th line after its own
                        const int pr = index_probe(p.idx, pk, k, hop);
                        sol = pr == 1;
                        unres = pr == 2;
                    }
                    ev |= EV_PROBE;
                } else {
                    sol = kept_sol; // answered by the index in the round being repeated
                }
            }
            retry = ((__ballot(unres) >> gshift) & GM) != 0ull;
            hop = retry ? hop + 1u : 0u;
            slow = retry;
            was_unres = unres;
            kept_sol = sol;
        } else if (do_probe) {
            sol = probe(p.bits, pk, k);
            ev |= EV_PROBE;
        }
        const uint64_t ball = __ballot(sol);
        const uint64_t gmask = (ball >> gshift) & GM;

        // ---------------- phase 3: group-uniform transitions ----------------------------------
        if (have && !retry) {
            bool fail = false;   // correct_error returned None
            int apply_s = -1;    // One scenario to apply
            int apply_t = -1;    // Two scenario to apply
            bool apply_path = false;
            uint32_t path_offset = 0;
            // Greedy: what follows the four answers `am` of next_nucs(wk) (greedy.rs:147-168, up to match_alignement)
            auto greedy_after_follow = [&](uint32_t am) {
                if (__popc(am) == 1) { // follow_graph succeeded: extend the path
                    const uint64_t a = (uint64_t)(__ffs(am) - 1);
                    if (gl == 0)
                        gL.y[k - 1 + (int)gnl] = bit2nuc(a);
                    gnl++;
                    wk = add_nuc(wk, a, mask);
                }
                // greedy.rs:153-157 (a failed follow leaves kmer in the set -> None).  The viewed set holds at most
                // max_search + 1 k-mers: one per lane of the group when it has that many (`greg`), else the chain's list
                bool hit = false;
                if (greg) {
                    hit = (uint32_t)gl < npath && gvis == wk;
                } else {
                    for (uint32_t j = gl; j < npath; j += G)
                        hit |= __hip_atomic_load(path + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == wk;
                }
                const uint64_t anyhit = (__ballot(hit) >> gshift) & GM;
                const uint32_t rem = n - i;
                if (anyhit || rem < git) { // greedy.rs:159-161
                    fail = true;
                } else if (!greg && npath >= p.maxpath) {
                    path_overflow();
                } else {
                    if (greg) {
                        if ((uint32_t)gl == npath)
                            gvis = wk;
                    } else if (gl == 0) {
                        __hip_atomic_store(path + npath, (unsigned long long)wk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    if (gl == 0 && git >= 1u)
                        gL.x[k - 1 + (int)git - 1] = ld(i + git - 1u);
                    npath++;
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    // greedy.rs:163-168 returns Some iff match_alignement finds an offset AND check_next_kmers
                    // holds.  Both are pure, so the cheap one goes first: the c look-ahead probes (GVALID), and the
                    // (k+i)^2 alignment only for the few candidates that pass them.
                    sub = 0;
                    st = ST_GVALID;
                }
            };
            if (st == ST_INIT) {
                if (n < (uint32_t)k) {
                    finish();
                } else {
                    prev = gmask & 1ull; // mod.rs:67
                    if (i >= n)
                        finish();
                    else
                        st = ST_SCAN;
                }
            } else if (st == ST_SCAN) {
                const uint32_t left = n - i;
                const uint32_t nvalid = left < (uint32_t)G ? left : (uint32_t)G;
                const uint64_t vmask = (nvalid >= 64) ? ~0ull : ((1ull << nvalid) - 1ull);
                const uint64_t prevmask = (gmask << 1) | (prev ? 1ull : 0ull);
                const uint64_t trig = ~gmask & prevmask & vmask; // mod.rs:73
                const uint32_t nacc = trig ? (uint32_t)__builtin_ctzll(trig) : nvalid;
                if (olen + nacc + 1u > cap) {
                    overflow();
                } else {
                    if ((uint32_t)gl < nacc)
                        out[olen + (uint32_t)gl] = ch; // mod.rs:100
                    olen += nacc;
                    i += nacc;
                    if (trig) {
                        kmer = __shfl(pk, gshift + (int)nacc);
                        ch_t = (uint8_t)__shfl((int)ch, gshift + (int)nacc);
                        ev |= (gl == 0) ? EV_TRIG : 0u;
                        if (HAS_ERRLEN) {
                            st = ST_ERRLEN;
                            ej = 0;
                            ek = kmer;
                        } else {
                            st = ST_ALTS;
                        }
                    } else {
                        kmer = __shfl(pk, gshift + (int)nacc - 1);
                        prev = (gmask >> (nacc - 1)) & 1ull; // mod.rs:99
                        if (i >= n)
                            finish();
                    }
                }
            } else if (HAS_ERRLEN && st == ST_ERRLEN) {
                const uint32_t rem = n - i;
                const uint32_t first = ej + 1u;
                const uint32_t left = rem > first ? rem - first : 0u;
                const uint32_t nvalid = left < (uint32_t)G ? left : (uint32_t)G;
                const uint64_t vmask = (nvalid >= 64) ? ~0ull : ((1ull << nvalid) - 1ull);
                const uint64_t smask = gmask & vmask;
                bool done = false, hit_end = false;
                if (smask) {
                    const int t = __builtin_ctzll(smask);
                    elen = first + (uint32_t)t;
                    fc = __shfl(pk, gshift + t);
                    done = true;
                } else if (nvalid < (uint32_t)G) {
                    elen = rem; // ran off the read: the last k-mer built is not solid
                    const uint64_t last = __shfl(pk, gshift + (nvalid ? (int)nvalid - 1 : 0));
                    fc = nvalid ? last : ek;
                    done = true;
                    hit_end = true;
                } else {
                    ek = __shfl(pk, gshift + G - 1);
                    ej += G;
                }
                if (done) {
                    if (M == BRX_GRAPH) {
                        mode = MODE_GRAPH;
                    } else { // gap_size.rs:97-108
                        if (elen < (uint32_t)k)
                            mode = MODE_GRAPH;
                        else if (elen == (uint32_t)k)
                            mode = MODE_ONE;
                        else {
                            mode = MODE_INSSUB;
                            gap = elen - (uint32_t)k;
                        }
                    }
                    // Graph with a non-solid target: every walk k-mer is solid, so `kmer ==
                    // first_correct_kmer` (graph.rs:79) can never hold and the walk can only end in
                    // None (branch, dead end or revisit) -- same outcome, no walk.
                    if (mode == MODE_GRAPH && hit_end)
                        fail = true;
                    else
                        st = ST_ALTS;
                }
            } else if (st == ST_ALTS) {
                const uint32_t am = (uint32_t)(gmask & 0xfull);
                if (__popc(am) != 1) {
                    fail = true; // exist/mod.rs:123-126, graph.rs:51-55, gap_size.rs:47-50
                } else {
                    corr = add_nuc(kmer >> 2, (uint64_t)(__ffs(am) - 1), mask);
                    const uint32_t rem = n - i;
                    if (HAS_ONE && mode == MODE_ONE) {
                        failmask = 0;
                        for (uint32_t s = 0; s < 3; s++)
                            if ((2u - s) + c > rem) // exist/mod.rs:27-29
                                failmask |= 1u << s;
                        if (failmask == 7u) {
                            fail = true;
                        } else if (c == 0u) {
                            passmask = 7u & ~failmask;
                            if (__popc(passmask) == 1)
                                apply_s = __ffs(passmask) - 1;
                            else
                                st = ST_MORE;
                        } else {
                            sub = 0;
                            st = ST_SCEN;
                        }
                    } else if (HAS_WALK && (mode == MODE_GRAPH || mode == MODE_INSSUB)) {
                        // graph.rs:57-59 / gap_size.rs:52-55: path = [alt], viewed = {corr}
                        if (gl == 0)
                            __hip_atomic_store(path, (unsigned long long)corr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        npath = 1;
                        wk = corr;
                        st = ST_WALK;
                        // Graph's viewed_kmer set (graph.rs:47,71-75) only decides WHEN a walk that has
                        // entered a cycle returns None: the walk is deterministic (unique successor), so
                        // once a k-mer repeats it can never reach first_correct_kmer any more (every k-mer
                        // of the cycle was visited before and was not it) -- any cycle detector gives the
                        // same result.  Brent's needs O(1) state instead of a scan of the visited list.
                        // Not used when corr == first_correct_kmer (corr is never compared on entry) nor
                        // for the fixed-length walk of GapSize (a late detection could run past its end).
                        brent = (mode == MODE_GRAPH) && (corr != fc);
                        {
                            const uint32_t f0 = walk_filter_index(corr, G); // viewed = {corr}
                            wfilt = ((uint32_t)gl == (f0 >> 5)) ? (1u << (f0 & 31u)) : 0u;
                        }
                        tort = corr;
                        bpow = 1;
                        blam = 0;
                    } else if (HAS_GREEDY) {
                        // greedy.rs:135-145: before = kmer2seq(kmer >> 2, k-1); path = [alt]; viewed = {corr}
                        const uint64_t pre = kmer >> 2;
                        for (int j = gl; j < k - 1; j += G) {
                            const uint8_t b = bit2nuc((pre >> (2 * (k - 2 - j))) & 3ull);
                            gL.x[j] = b;
                            gL.y[j] = b;
                        }
                        if (gl == 0) {
                            gL.y[k - 1] = bit2nuc(corr & 3ull);
                            if (greg)
                                gvis = corr;
                            else
                                __hip_atomic_store(path, (unsigned long long)corr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                        gnl = 1;
                        npath = 1;
                        wk = corr;
                        git = 0;
                        st = ST_GFOLLOW;
                        // (next_nucs of the three alternatives asked beside alt_nucs -- 3 + 12 probes fill the group's
                        // sixteen lanes -- saves this round too; measured 69.8 against 68.9 ms per Gbp: nothing, not kept)
                    } else if (HAS_TWO) {
                        uint32_t s4 = 0;
                        for (uint32_t j = 0; j < 4 && j < rem; j++)
                            s4 |= (uint32_t)nuc2bit(ld(i + j)) << (2 * j);
                        tw.K = corr;
                        tw.s = s4;
                        tw.m1 = 0;
                        st = ST_T1;
                    }
                }
            } else if (HAS_ONE && st == ST_SCEN) {
                const bool bad = sc_active && !sol;
                const uint32_t w_used = scen_width(sub, c, G, p.flags, failmask); // as dealt in phase 1
#pragma unroll
                for (uint32_t s = 0; s < 3; s++) {
                    const uint64_t b = (__ballot(bad && sc_s == s) >> gshift) & GM;
                    if (b)
                        failmask |= 1u << s;
                }
                sub += w_used;
                if (failmask == 7u) {
                    fail = true; // exist/mod.rs:132-134
                } else if (sub >= c) {
                    passmask = 7u & ~failmask;
                    if (__popc(passmask) == 1)
                        apply_s = __ffs(passmask) - 1; // exist/mod.rs:135-137
                    else
                        st = ST_MORE;
                }
            } else if (HAS_ONE && st == ST_MORE) {
                const uint32_t keep = (uint32_t)(gmask & 7ull) & passmask;
                if (__popc(keep) == 1)
                    apply_s = __ffs(keep) - 1; // exist/mod.rs:143-144
                else
                    fail = true;
            } else if (HAS_WALK && st == ST_WALK) {
                const uint32_t am = (uint32_t)(gmask & 0xfull);
                if (__popc(am) != 1) {
                    fail = true; // graph.rs:64-67, gap_size.rs:60-68
                } else {
                    const uint64_t nk = add_nuc(wk, (uint64_t)(__ffs(am) - 1), mask);
                    bool revisit;
                    // GapSize's fixed-length walk (gap_size.rs:57-85): the walk is deterministic -- every k-mer is the unique
                    // solid successor of the one before -- so two equal k-mers drag everything behind them along, and a repeat
                    // ANYWHERE in the walk shows as "the LAST k-mer was seen before".  The viewed set is therefore asked once,
                    // when the gap is walked, instead of at every step: a reverse pass's rare long walks (thousands of steps
                    // along the genome) had saturated the filter below and scanned their own list at every step -- quadratic,
                    // 3 us a step, a 9 ms tail on the launch.  (A walk the reference would have cut short at its first revisit
                    // goes on here to the end of the gap or to its first branch: None either way.)
                    const bool deferred = !brent && mode == MODE_INSSUB;
                    if (deferred) {
                        revisit = false;
                    } else if (brent) {
                        blam++;
                        revisit = (nk == tort);
                        if (!revisit && blam == bpow) {
                            tort = nk;
                            bpow *= 2u;
                            blam = 0;
                        }
                    } else {
                        // viewed_kmer.contains(&kmer): graph.rs:71, gap_size.rs:75.  The visited list is scanned only
                        // when a 32*G-bit filter spread over the group's lanes says the k-mer MAY have been seen (a
                        // new k-mer nearly never does; always scanning costs GapSize 9 % more time, never scanning --
                        // which would be wrong -- 4 % less)
                        const uint32_t fidx = walk_filter_index(nk, G);
                        const bool mine = (uint32_t)gl == (fidx >> 5);
                        const bool maybe = ((__ballot(mine && ((wfilt >> (fidx & 31u)) & 1u)) >> gshift) & GM) != 0ull;
                        revisit = false;
                        if (maybe) {
                            bool hit = false;
                            const uint32_t stored = npath < p.maxpath ? npath : p.maxpath;
                            for (uint32_t j = gl; j < stored; j += G)
                                hit |= __hip_atomic_load(path + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nk;
                            revisit = ((__ballot(hit) >> gshift) & GM) != 0ull;
                        }
                        if (mine)
                            wfilt |= 1u << (fidx & 31u);
                    }
                    if (revisit) {
                        fail = true;
                    } else if (npath >= p.maxpath && !brent) {
                        path_overflow(); // the exact scan needs every visited k-mer
                    } else {
                        // the visited list doubles as the corrected path; beyond maxpath a (Brent) walk goes
                        // on unrecorded and only a SUCCESS needs the batch redone with a larger list
                        if (gl == 0 && npath < p.maxpath)
                            __hip_atomic_store(path + npath, (unsigned long long)nk, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
                        if (npath < 0xfffffff0u)
                            npath++;
                        wk = nk;
                        if (mode == MODE_GRAPH) {
                            if (nk == fc) { // graph.rs:79-81
                                if (npath > p.maxpath) {
                                    path_overflow();
                                } else {
                                    apply_path = true;
                                    path_offset = elen + 1u; // graph.rs:84
                                }
                            }
                        } else if (--gap == 0u) {
                            // the deferred viewed-set check: nk against every k-mer of the walk before it (the list holds
                            // them all: a walk that outgrew it was stopped above)
                            bool hit = false;
                            for (uint32_t j = gl; j + 1u < npath; j += G)
                                hit |= __hip_atomic_load(path + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nk;
                            if (((__ballot(hit) >> gshift) & GM) != 0ull) {
                                fail = true; // gap_size.rs:75-81
                            } else {
                                apply_path = true;
                                path_offset = npath; // gap_size.rs:87-88
                            }
                        }
                    }
                }
            } else if (HAS_TWO && st == ST_T1) {
                const uint32_t rem = n - i;
                tw.m1 = (uint32_t)(gmask & 0xffffull);
                tvalid = two_valid(tw, rem);
                for (int sc = 0; sc < T_N; sc++) { // exist/mod.rs:27-29
                    uint32_t off;
                    (void)two_apply(tw, sc, mask, off);
                    if (off + c > rem)
                        tvalid &= ~(1u << sc);
                }
                if (tvalid == 0u) {
                    fail = true;
                } else if (c == 0u) {
                    passmask = tvalid;
                    if (__popc(passmask) == 1)
                        apply_t = __ffs(passmask) - 1;
                    else
                        st = ST_TMORE;
                } else {
                    failmask = 0;
                    sub = 0;
                    st = ST_TSCORE;
                }
            } else if (HAS_TWO && st == ST_TSCORE) {
                const bool bad = sc_active && !sol;
                const uint64_t badmask = (__ballot(bad) >> gshift) & GM;
                const uint32_t alive = tvalid & ~failmask; // as dealt in phase 1
                const uint32_t width = two_width(sub, c, G, alive);
                const uint64_t wmask = width >= 64u ? ~0ull : (1ull << width) - 1ull;
                uint32_t rest = alive;
                for (uint32_t ord = 0; rest; ord++, rest &= rest - 1u)
                    if ((badmask >> (ord * width)) & wmask)
                        failmask |= rest & (0u - rest); // lowest set bit = the ord-th surviving scenario
                sub += width;
                passmask = tvalid & ~failmask;
                if (passmask == 0u) {
                    fail = true;
                } else if (sub >= c) {
                    if (__popc(passmask) == 1)
                        apply_t = __ffs(passmask) - 1;
                    else
                        st = ST_TMORE;
                }
            } else if (HAS_TWO && st == ST_TMORE) {
                const uint32_t keep = (uint32_t)(gmask & ((1ull << T_N) - 1ull)) & passmask;
                if (__popc(keep) == 1)
                    apply_t = __ffs(keep) - 1;
                else
                    fail = true;
            } else if (HAS_GREEDY && st == ST_GFOLLOW) {
                greedy_after_follow((uint32_t)(gmask & 0xfull));
            } else if (HAS_GREEDY && st == ST_GVALID) {
                const uint32_t rem2 = n - i - git;
                bool ok = rem2 >= c, done = false;
                if (ok && c > 0u) {
                    const uint32_t leftc = c - sub * G;
                    const uint32_t nv = leftc < (uint32_t)G ? leftc : (uint32_t)G;
                    const uint64_t vm = (nv >= 64u) ? ~0ull : ((1ull << nv) - 1ull);
                    ok = (gmask & vm) == vm;
                    sub++;
                    done = ok && sub * G >= c;
                } else if (ok) {
                    done = true;
                }
                // the next iteration: its follow_graph was asked in this very round when the lanes allow (phase 1)
                auto next_iteration = [&]() {
                    st = ST_GFOLLOW;
                    if (++git >= (uint32_t)p.max_search)
                        fail = true;
                    else if (c + 4u <= (uint32_t)G)
                        greedy_after_follow((uint32_t)(gmask >> c) & 0xfu);
                };
                if (!ok) {
                    next_iteration();
                } else if (done && !greedy_align<G>(gL, gl, k - 1 + (int)git, k - 1 + (int)gnl, k - 1, goff)) {
                    next_iteration(); // the look-ahead held but no alignment offset: next iteration (greedy.rs:163)
                } else if (done) {
                    // greedy.rs:165-167: offset = (local_corr.len() as i64 + off) as usize, wrapping add
                    if (VERIFY) {
                        flag_read = true;
                        finish();
                    } else if (olen + gnl + 1u > cap) {
                        overflow();
                    } else {
                        for (uint32_t j = gl; j < gnl; j += G)
                            out[olen + j] = gL.y[k - 1 + (int)j];
                        olen += gnl;
                        kmer = wk;
                        prev = true;
                        const long long ni = (long long)i + (long long)gnl + (long long)goff;
                        i = (ni < 0 || ni > (long long)n) ? n : (uint32_t)ni;
                        ev |= (gl == 0) ? EV_FIX : 0u;
                        if (i >= n)
                            finish();
                        else
                            st = ST_SCAN;
                    }
                }
            }
            if (have && !done && steps > (1u << 24) + 64u * n) {
                fail = false;
                apply_s = apply_t = -1;
                apply_path = false;
                nonterminating();
            }

            if (VERIFY && (fail || apply_s >= 0 || apply_t >= 0 || apply_path)) {
                flag_read |= !fail; // None is what the lean scan assumed
                finish();
            } else if (fail) {
                // mod.rs:91-96
                if (olen + 2u > cap) {
                    overflow();
                } else {
                    if (gl == 0)
                        out[olen] = ch_t;
                    olen += 1;
                    if (HAS_ERRLEN)
                        skip_until = i + elen; // (see its declaration)
                    i += 1;
                    prev = false;
                    if (i >= n) {
                        finish();
                    } else if (HAS_ERRLEN && skip_until >= n) {
                        // error_len ran off the read: no k-mer behind the trigger is solid, so no later one can trigger
                        // (`previous` stays false) and the scan copies the rest of the read through (mod.rs:99-102) -- here
                        // in one go, every lane's loads independent, instead of 64 bases a dependent round.  This is how
                        // nearly every read of a reverse pass ends.
                        const uint32_t left = n - i;
                        if (olen + left + 1u > cap) {
                            overflow();
                        } else {
                            for (uint32_t j = (uint32_t)gl; j < left; j += (uint32_t)G)
                                out[olen + j] = ld(i + j);
                            olen += left;
                            i = n;
                            finish();
                        }
                    } else {
                        st = ST_SCAN;
                    }
                }
            } else if (apply_s >= 0) {
                // mod.rs:75-89 with one.rs:65-71
                if (olen + 2u > cap) {
                    overflow();
                } else {
                    if (gl == 0)
                        out[olen] = bit2nuc(corr & 3ull);
                    olen += 1;
                    kmer = corr;
                    prev = true;
                    i += 2u - (uint32_t)apply_s;
                    ev |= (gl == 0) ? EV_FIX : 0u;
                    // The c look-ahead k-mers of the winning scenario ARE the next c scan k-mers and were
                    // all found solid: the reference's loop would copy these c bases with previous = true
                    // (mod.rs:99-102).  Accept them without probing again.
                    if (c > 0u && c + 3u <= (uint32_t)WB && olen + c + 1u <= cap && !(p.flags & 9u)) {
                        const uint32_t off = 2u - (uint32_t)apply_s;
                        if ((uint32_t)gl < c)
                            out[olen + (uint32_t)gl] = ld(i + (uint32_t)gl);
                        kmer = ext(kmer, win, off, c); // window positions are relative to the trigger
                        olen += c;
                        i += c;
                    }
                    if (i >= n)
                        finish();
                    else
                        st = ST_SCAN;
                }
            } else if (HAS_TWO && apply_t >= 0) {
                // mod.rs:75-89 with two.rs:258-325
                uint32_t nc, offc;
                const uint32_t cb = two_correct(tw, apply_t, mask, nc, offc);
                if (olen + nc + 1u > cap) {
                    overflow();
                } else {
                    uint64_t km = kmer >> 2;
                    for (uint32_t q = 0; q < nc; q++) {
                        const uint64_t b = (cb >> (2 * (nc - 1 - q))) & 3u;
                        km = add_nuc(km, b, mask);
                        if (gl == 0)
                            out[olen + q] = bit2nuc(b);
                    }
                    olen += nc;
                    kmer = km;
                    prev = true;
                    i += offc;
                    ev |= (gl == 0) ? EV_FIX : 0u;
                    if (i >= n)
                        finish();
                    else
                        st = ST_SCAN;
                }
            } else if (HAS_WALK && apply_path) {
                // mod.rs:75-89: the whole walked path replaces `path_offset` read bases
                if (olen + npath + 1u > cap) {
                    overflow();
                } else {
                    for (uint32_t j = gl; j < npath; j += G)
                        out[olen + j] = bit2nuc(__hip_atomic_load(path + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 3ull);
                    olen += npath;
                    kmer = wk;
                    prev = true;
                    i += path_offset;
                    ev |= (gl == 0) ? EV_FIX : 0u;
                    if (i >= n)
                        finish();
                    else
                        st = ST_SCAN;
                }
            }
        }
        if (done) {
            if (VERIFY) {
                if (flag_read && gl == 0 && atomicExch(p.redo_flag + r, 1u) == 0u) {
                    p.redo_list[atomicAdd(p.ctrl + CTL_REV_HANDBACK, 1ull)] = r;
                    atomicAdd(p.ctrl + CTL_REV_HANDBACK_SUM, 1ull);
                }
                flag_read = false;
            } else if (gl == 0) {
                p.out_lens[r] = done == 1 ? olen : 0xffffffffu;
                if (done != 1)
                    atomicAdd(p.ctrl + (done - 16), 1ull);
            }
            done = 0;
            fetch();
        }
        // end of the round, every lane back together: count the events
        n_rounds += (uint32_t)__builtin_popcountll(__ballot(ev & EV_ROUND));
        n_probes += (uint32_t)__builtin_popcountll(__ballot(ev & EV_PROBE));
        n_trig += (uint32_t)__builtin_popcountll(__ballot(ev & EV_TRIG));
        n_fix += (uint32_t)__builtin_popcountll(__ballot(ev & EV_FIX));
    }

    // statistics: one atomic per wave per counter
    if (lane == 0) {
        if (n_rounds)
            atomicAdd(p.ctrl + CTL_ROUNDS, (unsigned long long)n_rounds);
        if (n_probes)
            atomicAdd(p.ctrl + CTL_PROBES, (unsigned long long)n_probes);
        if (n_trig)
            atomicAdd(p.ctrl + CTL_TRIGGERS, (unsigned long long)n_trig);
        if (n_fix)
            atomicAdd(p.ctrl + CTL_FIXES, (unsigned long long)n_fix);
    }
}

// Method M's group kernel as planned: over the whole batch (PASS_GROUP), or, after a lean reverse scan, over the triggers
// it left open (p.trig) and over the reads it handed back (p.only)
template <int M>
int launch_method(const PassParams &p, const PassPlan &pl, uint32_t blocks, hipStream_t s)
{
    const int G = pl.width;
    const size_t lds = pl.lds;
    if constexpr (M == BRX_ONE) {
        if (p.trig) { // the triggers One's lean reverse pass left open (BRX_REV_LEAN_ONE), one 8-lane group each
            correct_kernel<8, BRX_ONE, 2><<<blocks, 256, lds, s>>>(p);
            return BRX_OK;
        }
        if (p.only)
            return launch_one_list(p, s);
    }
    if (M == BRX_ONE && pl.one_kernel) {
        launch_one(p, G, blocks, s);
        return BRX_OK;
    }
    if constexpr (M == BRX_GRAPH || M == BRX_GAP_SIZE) {
        if (p.trig) {
            // the triggers a lean reverse pass left open, one narrow group each (a walk step is four probes)
            if (pl.verify_width == 4)
                correct_kernel<4, M, 2><<<blocks, 256, lds, s>>>(p);
            else
                correct_kernel<8, M, 2><<<blocks, 256, lds, s>>>(p);
            return BRX_OK;
        }
        if (p.only) {
            // the reads whose trigger did not end in None: a reverse pass over them, 64 lanes a read as usual
            correct_kernel<64, M, 1><<<blocks, 256, lds, s>>>(p);
            return BRX_OK;
        }
    }
    if (lds > 64 * 1024) {
        const void *fn = G == 16 ? (const void *)correct_kernel<16, M>
                       : G == 32 ? (const void *)correct_kernel<32, M> : (const void *)correct_kernel<64, M>;
        BRX_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    if constexpr (M == BRX_GRAPH || M == BRX_GAP_SIZE) { // (the only methods with 4- and 8-lane groups in this kernel)
        if (G == 4) {
            correct_kernel<4, M><<<blocks, 256, lds, s>>>(p);
            return BRX_OK;
        }
        if (G == 8) {
            correct_kernel<8, M><<<blocks, 256, lds, s>>>(p);
            return BRX_OK;
        }
    }
    if (G <= 8 && M == BRX_ONE)
        correct_kernel<8, BRX_ONE><<<blocks, 256, lds, s>>>(p);
    else if (G <= 16)
        correct_kernel<16, M><<<blocks, 256, lds, s>>>(p);
    else if (G == 32)
        correct_kernel<32, M><<<blocks, 256, lds, s>>>(p);
    else
        correct_kernel<64, M><<<blocks, 256, lds, s>>>(p);
    return BRX_OK;
}

} // namespace

namespace brx {

// Graph's / GapSize's group kernel over the reads p.only[0 .. *p.only_n) (8-lane groups; the visited lists of the chain
// are sized for blocks of groups at least as wide (sized_path_lists), so the grid stays inside them)
int launch_walk_list(const PassParams &p, int method, uint64_t path_lists, hipStream_t s)
{
    const uint32_t bl = list_grid(path_lists, 32u, 128u); // 32 eight-lane groups per block (the chain sizes at least 64 lists)
    if (method == BRX_GRAPH)
        correct_kernel<8, BRX_GRAPH, 1><<<bl, 256, 0, s>>>(p);
    else
        correct_kernel<8, BRX_GAP_SIZE, 1><<<bl, 256, 0, s>>>(p);
    BRX_HIP(hipGetLastError());
    return BRX_OK;
}

// one launch of the group kernels, under `timer`; BRX_TUNE and max_search are for these kernels alone
int launch_group(PassParams p, const PassPlan &pl, const brx_method_t &md, uint32_t blocks, const char *timer, hipStream_t s)
{
    p.max_search = md.max_search;
    p.flags = pl.flags;
    p.g_dim = pl.g_dim;
    p.g_lds_bytes = pl.g_lds_bytes;
    KernelTimer t(timer, s);
    switch (md.method) {
    case BRX_ONE: BRX_TRY(launch_method<BRX_ONE>(p, pl, blocks, s)); break;
    case BRX_TWO: BRX_TRY(launch_method<BRX_TWO>(p, pl, blocks, s)); break;
    case BRX_GRAPH: BRX_TRY(launch_method<BRX_GRAPH>(p, pl, blocks, s)); break;
    case BRX_GREEDY: BRX_TRY(launch_method<BRX_GREEDY>(p, pl, blocks, s)); break;
    case BRX_GAP_SIZE: BRX_TRY(launch_method<BRX_GAP_SIZE>(p, pl, blocks, s)); break;
    default: break;
    }
    BRX_HIP(hipGetLastError());
    return BRX_OK;
}

} // namespace brx
