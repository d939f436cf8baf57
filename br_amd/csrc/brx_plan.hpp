// The correction chain's switches and the rule that turns them into a pass: host only, no HIP call, so that the rule can
// be run and checked without a GPU (tests/pass_plan_host.cpp).
//
//   read_correct_tuning()  the ONE place that reads the chain's environment switches: once per batch, on the thread that
//                          calls the library (getenv on a library thread would race with a host that changes its
//                          environment).  A chain reads BRX_MAXPATH through it when it is created.
//   plan_pass()            pure: tuning + facts of the set + the pass -> the form the pass takes (lane per chunk, group
//                          kernel, lean reverse scan), how wide, through the index or the bit vector, in block form or not.
//                          brx_correct.hip's chain loop, the launches of the group kernels (brx_group.hip, brx_revscan.hip) and
//                          brx_onelane.hip only execute what it returns.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include "../../include/brx.h"

#if defined(__HIPCC__)
#define BRX_PLAN_HD __host__ __device__
#else
#define BRX_PLAN_HD
#endif

#ifndef BRX_LANE_WAVES
#define BRX_LANE_WAVES 7 // waves per SIMD the automaton is compiled for (tools/ab_build.sh sweeps it)
#endif

namespace brx {

struct CorrectTuning {
    // lanes per read; BRX_GROUP / BRX_GROUP_REV override (per batch, so tests can sweep them).  The values as given: a
    // variable that is set, to whatever, switches off the small-batch widening (group_width)
    bool group_set = false, group_rev_set = false;
    int group = 0, group_rev = 0;
    // BRX_GROUP_WALK = 4 / 8 / 16: lanes per read of Graph's and GapSize's forward passes.
    // measured at 1 Gbp, k = 19 (fwd+rev ms, tools/method_bench.py): 16 lanes + bit vector 135 / 158 (graph / gap_size),
    // 8 lanes + bit vector 140 / 145, 8 lanes + probe index 120 / 142, 4 lanes + probe index 123 / 151
    int group_walk = 8;
    int rev_verify_g = 8;  // BRX_REV_VERIFY_G = 4 / 8: lanes per open trigger of the verify pass
    bool one_v1 = false;   // BRX_ONE_V1=1: One through the first form of its kernel, correct_kernel (A/B runs; results are identical)
    // BRX_BALANCE=1: fewer groups with the same whole number of reads each (pass_blocks).
    // Measured (profiles/r2_one_kernel_ab.txt): NOT a win -- 4 168 waves instead of 8 192 leave the SIMDs waiting on
    // memory (VALU busy 65 % instead of 79 %, 32.6 ms against 27.2); kept for the record.
    bool balance = false;
    uint32_t tune = 0;     // BRX_TUNE: PassParams::flags of the group kernels (A/B runs)
    // BRX_REV_LEAN=0: reverse passes of Graph / GapSize through the 64-lane group kernel as before the lean scan
    bool rev_lean = true;
    // BRX_REV_BATCH=0: the reverse scans' trigger-free rounds one at a time, as before rev_block_rounds
    bool rev_batch = true;
    // BRX_REV_LEAN_ONE=1: One's reverse pass in lean form, too (measured: profiles/r4o_rev_lean_ab.txt; Two's and Greedy's
    // reverse passes cost 4 ms per Gbp of their 55 / 69 in the group kernel: the form bought nothing for them either)
    bool rev_lean_one = false;
    // BRX_INDEX_FWD: bit mask (1 << method) of the methods whose FORWARD pass probes the index; measured per method
    // (tools/method_bench.py, 1 Gbp): One 1.4x faster through it; Graph / GapSize 10-12 % faster with 8-lane groups
    // (BRX_GROUP_WALK); Two / Greedy (16-lane groups) see profiles/r2_one_kernel_ab.txt.  Default: One, Graph, Greedy,
    // GapSize (Two: 69 ms through the bit vector, 72 through the index)
    unsigned index_fwd = 29u;
    // BRX_LANE_REV (bit 0: Graph, bit 1: GapSize): REVERSE passes in lane form too.
    // Their scan meets hardly a solid k-mer (the read is read back to front, not complemented), so over the
    // solidity mask it is bit runs of sixteen positions a round -- but the rare trigger runs error_len to the
    // END OF THE READ (hundreds of rounds of one lane, whose wave waits for it), and GapSize then walks a gap
    // of thousands of fixed steps along the genome (a deep-coverage set has long unbranched paths), which no
    // unit's edit list holds: the lanes hand the read back.  Measured (profiles/r4c_*, r4e_*):
    //   2^25 lines (configs[1]'s set)     graph 65.6 -> 75.4 ms per Gbp fwd+rev, gap_size 92 -> 211 (1 845 reads redone)
    //   2^28 lines (configs[4]'s share)   graph + gap_size 714 -> 1 598 ms per step with both (770 ms of redo)
    //   2^29 lines, 8x coverage, -a 1     graph + gap_size 932 -> 748 ms per 8 Gbp (walks die young in a set
    //                                     with holes: nothing is handed back)
    //   2^28 lines (configs[4]'s share)   Graph alone in lane form: 836 -> 877 ms per step (r4f)
    // Only the last case gains (its 64-lane group kernels take ~180 ms per 8 Gbp pass at 2^29 lines), and a
    // deep-coverage set of that size would hand reads back like the second.  So the form is OFF unless asked
    // for; the switch stays for measurements and for the fuzzer, which sweeps it.
    unsigned lane_rev = 0u;
    bool line_bits = true;     // BRX_LINE_BITS=0: do not consult the index's occupancy bits (A/B and fuzzers)
    uint32_t redo_max = 4096u; // BRX_REDO_MAX: most poisoned reads a sub chain redoes (tests: 0 = never)
    uint32_t maxpath = 0;      // BRX_MAXPATH: a chain's first visited-list length (tests: short, so that walks outgrow it); 0 = unset
    bool lane = true;          // BRX_LANE=0: the group kernels only
    bool lane_walk = true;     // BRX_LANE_WALK=0: ... for Graph and GapSize
    // BRX_LANE_MAX_LOG_LINES: One against a LARGE index stays with the group kernel: every lane of a wave probes a line of
    // a different read, 64 unrelated pages per load, and past 2^26 lines (4 GiB) that costs more than the lanes save --
    // same box, correction of 2 / 3.5 / 6.25 Gbp against sets of 41 / 73 / 130 M k-mers (2^26 / 2^27 / 2^28 lines): lanes
    // 56.6 / 132.5 / 256 ms, groups 61.0 / 107.9 / 197 ms.  (The walking methods gain at 2^28 lines all the same: their
    // group kernels are latency-bound, BASELINE configs[4]'s share 5.1 -> 6.9 Gbases/s.)
    uint32_t lane_max_log_lines = 26u;
    // BRX_LANE_CHUNK: bases per unit, at least 64; 0 = automatic (lane_chunk)
    uint32_t lane_chunk = 0;
    uint32_t lane_sync = 4u;   // BRX_LANE_SYNC: 1 .. 32
    // BRX_LANE_TAIL=1: the last fifth of the batch's reads is cut at C / 2, the last twentieth at C / 4 (chunk_of).  OFF by
    // default: measured at configs[1] (profiles/r4i_lane_tail_ab.txt) the pass got 0.9 ms SLOWER (2.35 M units instead of
    // 1.8 M: every unit start stalls its wave, and the sync / replay kernels grow with the units), as did guided draws
    // (no change) -- the thinning tail of the launch is not where its time goes.
    // (One only: a walking corrector's fix has to fit its unit's list, and short units hand more reads back)
    bool lane_tail = false;
    // BRX_LANE_MASK: the solidity mask of the original k-mers (lane_mask_kernel) -- 0: never, every SCAN / error_len
    // position is probed; 1: for the walking correctors, whose error_len it shortens to a bit scan (rounds 1.97 G -> 0.96 G
    // per Gbp for Graph; both launches 65.0 -> 52.6 ms with 10.2 ms of mask kernel to pay for it; BASELINE configs[4]'s
    // share, 2^28 index lines: 6.58 -> 7.13 Gbases/s on one box); 2: for One as well (there the mask kernel costs what the
    // shorter scan saves: rounds 1.24 G -> 0.59 G, launch 16 -> 12 ms, mask 8.7 ms).  Either way the index lines fetched
    // are the same ones: the mask kernel fetches them for 64 neighbouring positions at a time instead of lane by lane.
    uint32_t lane_mask = 1u;
    bool lane_succ = true;     // BRX_LANE_SUCC=0: the walking lanes without the index's successor table
    uint32_t ap_grid = 1u << 20; // BRX_AP_GRID: blocks of the replay kernels; each block loops over reads
};

inline CorrectTuning read_correct_tuning()
{
    CorrectTuning t;
    const auto is1 = [](const char *name) { const char *e = getenv(name); return e && *e == '1'; };
    const auto not0 = [](const char *name) { const char *e = getenv(name); return !(e && *e == '0'); };
    const auto num = [](const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; }; // ("" reads as 0)
    const auto u32 = [](const char *name, uint32_t dflt) { const char *e = getenv(name); return e && *e ? (uint32_t)strtoul(e, nullptr, 10) : dflt; };
    t.group_set = getenv("BRX_GROUP") != nullptr;
    t.group = num("BRX_GROUP", 0);
    t.group_rev_set = getenv("BRX_GROUP_REV") != nullptr;
    t.group_rev = num("BRX_GROUP_REV", 0);
    t.group_walk = num("BRX_GROUP_WALK", 8);
    if (t.group_walk != 4 && t.group_walk != 16)
        t.group_walk = 8;
    t.rev_verify_g = num("BRX_REV_VERIFY_G", 8) == 4 ? 4 : 8;
    t.one_v1 = is1("BRX_ONE_V1");
    t.balance = is1("BRX_BALANCE");
    t.tune = (uint32_t)num("BRX_TUNE", 0);
    t.rev_lean = not0("BRX_REV_LEAN");
    t.rev_batch = not0("BRX_REV_BATCH");
    t.rev_lean_one = is1("BRX_REV_LEAN_ONE");
    t.index_fwd = (unsigned)num("BRX_INDEX_FWD", 29);
    t.lane_rev = u32("BRX_LANE_REV", 0u);
    t.line_bits = not0("BRX_LINE_BITS");
    t.redo_max = (uint32_t)num("BRX_REDO_MAX", 4096);
    const int maxpath = num("BRX_MAXPATH", 0);
    t.maxpath = maxpath >= 1 && maxpath <= (1 << 20) ? (uint32_t)maxpath : 0u;
    t.lane = u32("BRX_LANE", 1u) != 0u;
    t.lane_walk = u32("BRX_LANE_WALK", 1u) != 0u;
    t.lane_max_log_lines = u32("BRX_LANE_MAX_LOG_LINES", 26u);
    t.lane_chunk = u32("BRX_LANE_CHUNK", 0u);
    if (t.lane_chunk != 0u && t.lane_chunk < 64u)
        t.lane_chunk = 64u;
    t.lane_sync = u32("BRX_LANE_SYNC", 4u);
    t.lane_sync = t.lane_sync < 1u ? 1u : (t.lane_sync > 32u ? 32u : t.lane_sync);
    t.lane_tail = u32("BRX_LANE_TAIL", 0u) != 0u;
    t.lane_mask = u32("BRX_LANE_MASK", 1u);
    t.lane_succ = u32("BRX_LANE_SUCC", 1u) != 0u;
    t.ap_grid = u32("BRX_AP_GRID", 1u << 20);
    return t;
}

// what plan_pass needs to know of the set the chain corrects against
struct SetFacts {
    int k = 0;
    bool has_bits = false;     // the bit vector is there (not a sparse set, not a lazy vector)
    bool has_idx = false;      // a probe index is there and wanted
    uint32_t idx_log_lines = 0;
    uint32_t idx_m = 0, idx_w = 0;
    bool has_line_bits = false; // ... with current occupancy bits
};

constexpr uint32_t REV_MAX_W = 8; // windows the reverse scans' sliding minimum is unrolled for (m = 15: k <= 22)
// the set's index answers a reverse scan in block form, rev_block_rounds (the rule lane_mask_kernel has for the occupancy
// bits -- at most 2^26 lines -- and a window count the sliding minimum is instantiated for)
inline bool rev_block_applies(const SetFacts &f)
{
    return f.has_idx && f.has_line_bits && f.idx_log_lines <= 26u && f.idx_w >= 1u && f.idx_w <= REV_MAX_W;
}

// ---- sizes and grids ---------------------------------------------------------------------------------------------------

// headroom of the chain's byte-sized workspaces
inline uint64_t ws_headroom(uint64_t need) { return need / 8 + 256; }

constexpr uint64_t RESIDENT_LANES = 256ull * 4ull * 6ull * 64ull; // CUs x SIMDs x waves x lanes at occupancy 6
constexpr uint32_t MAX_BLOCKS = 256u * 8u;
// Visited lists a chain always has, however few reads its batch holds: one block of the narrowest kernel that indexes them
// by its global group number (4-lane groups: 64 a block).  The list and verify launches size their grids from the lists
// the chain has (sized_path_lists), never from a width of their own.
constexpr uint32_t MIN_PATH_LISTS = 64u;

inline int group_width(const CorrectTuning &t, bool reverse_pass, bool indexed, uint32_t n_reads)
{
    // The reverse pass of run_correction (src/lib.rs:48-55) sees almost only non-solid k-mers and hardly
    // ever triggers, so wide groups waste nothing there and save rounds.  BRX_GROUP_REV falls back to BRX_GROUP.
    const bool rev_own = reverse_pass && t.group_rev_set;
    const bool set = rev_own || t.group_set;
    // measured (tools/ab_correct.py): bitset probes 16/64 (+3 % over 16/16); with the probe index the shared
    // probe code is the larger part of a round and 8 groups per wave amortise it better: 8/64 (+5 % over 16/64)
    const int dflt = reverse_pass ? 64 : (indexed ? 8 : 16);
    int g = set ? (rev_own ? t.group_rev : t.group) : dflt;
    if (!set) {
        // small batches (the reference's 8192 records): with fewer reads than resident groups the GPU idles and
        // the time is one read's chain of rounds -- wider groups advance further per round
        while (g < 64 && (uint64_t)n_reads * (uint64_t)g * 2u <= RESIDENT_LANES)
            g *= 2;
    }
    return (g == 4 || g == 8 || g == 16 || g == 32 || g == 64) ? g : dflt;
}

inline uint32_t pass_blocks(const CorrectTuning &t, uint32_t n_reads, int G, bool balanced = false)
{
    const uint32_t groups_per_block = 256u / (uint32_t)G;
    // persistent-ish grid: enough groups to fill the chip, reads pulled from a work counter
    uint64_t want = ((uint64_t)n_reads + groups_per_block - 1) / groups_per_block;
    if (balanced && t.balance) {
        // Reads of a batch take about the same time, and a wave costs the same instructions whether 8 of its groups
        // are busy or 3: 100 000 reads over 49 152 resident 8-lane groups is two reads each and a third for a few,
        // i.e. a last third of the kernel run by mostly idle waves.  Fewer groups with the same whole number of reads
        // each end together.  (Not a win: see CorrectTuning::balance.)
        const uint64_t resident_blocks = 256ull * 7; // CUs x (waves per SIMD x 4 SIMDs / 4 waves per block): one_kernel runs 7 per SIMD
        const uint64_t resident_groups = resident_blocks * groups_per_block;
        if ((uint64_t)n_reads > resident_groups) {
            const uint64_t per_group = ((uint64_t)n_reads + resident_groups - 1) / resident_groups;
            const uint64_t groups = ((uint64_t)n_reads + per_group - 1) / per_group;
            want = (groups + groups_per_block - 1) / groups_per_block;
        }
    }
    if (want > MAX_BLOCKS)
        want = MAX_BLOCKS;
    if (want < 1)
        want = 1;
    return (uint32_t)want;
}

// visited lists of a chain for a batch of n_reads (the walking methods' group kernels index them by global group number).
// Computed ONCE per attempt: the workspace is sized from it and every list / verify grid is cut from the same number.
inline uint64_t sized_path_lists(const CorrectTuning &t, uint32_t n_reads)
{
    const uint64_t g = (uint64_t)pass_blocks(t, n_reads, t.group_walk) * (256u / (uint32_t)t.group_walk);
    return g < MIN_PATH_LISTS ? MIN_PATH_LISTS : g;
}

// grid of a launch over a list (a few reads, or the open triggers, which are many): the grid loops over it; as many groups
// as the visited lists the chain has sized allow, `per_block` groups a block
inline uint32_t list_grid(uint64_t path_lists, uint32_t per_block, uint32_t cap)
{
    const uint64_t b = path_lists / per_block;
    return b < 1u ? 1u : (b > cap ? cap : (uint32_t)b);
}

BRX_PLAN_HD inline uint32_t greedy_lds_bytes(uint32_t dim)
{
    const uint32_t a = (dim + 15u) & ~15u;
    return 13u * a + ((2u * dim * dim + 15u) & ~15u);
}

// Greedy needs LDS for the alignment back pointers: pick the narrowest group width that fits (0: none does)
inline int greedy_group(int G, int k, int max_search, uint32_t *dim, uint32_t *per_group)
{
    *dim = (uint32_t)(k + max_search + 2);
    *per_group = greedy_lds_bytes(*dim);
    for (; G <= 64; G *= 2)
        if ((uint64_t)(256 / G) * *per_group <= 160u * 1024u)
            return G;
    return 0;
}

inline const char *pass_timer_name(int method)
{
    static const char *const names[5] = {"correct_pass", "correct_pass_two", "correct_pass_graph", "correct_pass_greedy",
                                         "correct_pass_gap_size"};
    return names[method];
}

// ---- the plan of one pass ----------------------------------------------------------------------------------------------

enum PassForm {
    PASS_LANE,      // one lane per chunk of a read (brx_onelane.hip)
    PASS_GROUP,     // a group of lanes per read: one_kernel / correct_kernel
    PASS_REV_LEAN,  // reverse pass: rev_scan_kernel, then the verify and redo launches of the group kernel
    PASS_NO_LDS     // error: Greedy's alignment table does not fit LDS at any width
};

struct PassPlan {
    PassForm form = PASS_GROUP;
    bool use_idx = false;   // probes go through the index (else through the bit vector)
    bool rev_batch = false; // reverse scan: trigger-free rounds in blocks through the occupancy bits (rev_block_rounds)
    // GROUP / REV_LEAN
    int width = 0;           // lanes per read after every adjustment (REV_LEAN: of the scan)
    bool one_kernel = false; // One through one_kernel (else correct_kernel: width 32, or BRX_ONE_V1)
    uint32_t blocks = 0;     // grid of the pass over the batch
    uint32_t flags = 0;      // BRX_TUNE, for the group kernels
    uint32_t g_dim = 0, g_lds_bytes = 0, lds = 0; // Greedy: table side, LDS per group and per block
    int verify_width = 0;      // REV_LEAN: lanes per open trigger (One's verify kernel exists at 8 only)
    int verify_grid_width = 0; // ... and the width the verify grid is cut for (BRX_REV_VERIFY_G, whatever the method)
    // LANE
    uint32_t chunk = 0, sync = 0;
    bool use_mask = false, use_succ = false;
    uint32_t r_half = 0xffffffffu, r_quarter = 0xffffffffu; // graded tail: reads from here on are cut at C / 2, C / 4
    uint64_t units_bound = 0;
    uint32_t ap_grid = 0;
};

// chunk length: enough units to keep ~4.6e5 lanes busy a few times over, not so short that the stretch a unit's
// predecessor re-scans in front of its sync point (a few dozen bases) becomes the larger part
inline uint32_t lane_chunk(const CorrectTuning &t, uint64_t in_total_bound)
{
    if (t.lane_chunk)
        return t.lane_chunk;
    // (measured at configs[1], same box: 256 -> 11.7 ms per launch, 512 -> 11.65, 768 -> 12.4, 1090 -> 12.6, 2048 -> 16.7:
    // a lane should get about four units, or the lanes that got one more than the others run the tail alone)
    constexpr uint64_t RESIDENT = 256ull * 4ull * BRX_LANE_WAVES * 64ull;
    const uint64_t want = in_total_bound / (4ull * RESIDENT);
    return want < 256ull ? 256u : (want > 2048ull ? 2048u : (uint32_t)want);
}

// the lane form of a pass of One, Graph or GapSize, where it applies (false: the group kernels run the pass)
inline bool plan_lane(const CorrectTuning &t, const SetFacts &f, int method, int confirm, uint32_t n_reads, uint64_t in_total_bound,
                      PassPlan &pl)
{
    const bool walk = method != BRX_ONE;
    if (!t.lane || f.k > 31 || n_reads == 0)
        return false;
    // the window of a round shows 8 bases: look-aheads up to off + c + 1 <= 8 (Graph has none; One and GapSize's One branch do)
    if (method != BRX_GRAPH && (confirm < 1 || confirm > 5))
        return false;
    if (walk && !t.lane_walk)
        return false;
    if (!walk && pl.use_idx && f.idx_log_lines > t.lane_max_log_lines)
        return false;
    if (!pl.use_idx && !f.has_bits)
        return false;
    const uint32_t C = lane_chunk(t, in_total_bound);
    const bool graded = !walk && t.lane_tail && n_reads >= 64u;
    const uint32_t c_min = graded ? ((C >> 2) < 64u ? 64u : (C >> 2)) : C;
    const uint64_t units_bound = in_total_bound / c_min + (uint64_t)n_reads + 1ull;
    if (units_bound >= 0xfffffff0ull) // (unit numbers are 32 bits)
        return false;
    pl.form = PASS_LANE;
    pl.chunk = C;
    pl.sync = t.lane_sync;
    pl.use_mask = walk ? t.lane_mask >= 1u : t.lane_mask >= 2u;
    pl.use_succ = walk && pl.use_idx && t.lane_succ;
    pl.r_half = graded ? n_reads - n_reads / 5u : 0xffffffffu;
    pl.r_quarter = graded ? n_reads - n_reads / 20u : 0xffffffffu;
    pl.units_bound = units_bound;
    pl.ap_grid = t.ap_grid;
    return true;
}

// dir 1: a scan of the reads back to front (tuned for absent k-mers); revcomp: the second scan runs over the reverse
// complement instead, which is a forward pass in every respect (the caller passes dir 0); flip: the pass reads its input
// back to front; in_total_bound: upper bound of the pass's input bases
inline PassPlan plan_pass(const CorrectTuning &t, const SetFacts &f, int method, int confirm, int max_search, int dir, bool revcomp,
                          bool flip, uint32_t n_reads, uint64_t in_total_bound)
{
    PassPlan pl;
    const bool walker = method == BRX_GRAPH || method == BRX_GAP_SIZE;
    // the index pays where whole groups probe neighbouring k-mers: One's passes and the (nearly trigger-free) reverse
    // scans of every method; walks probe 4 successors of one k-mer per round and gain nothing from shared lines
    pl.use_idx = f.has_idx && (!f.has_bits || ((t.index_fwd >> method) & 1u) || (dir == 1 && method != BRX_GREEDY));
    pl.rev_batch = dir == 1 && !revcomp && t.rev_batch && pl.use_idx && t.line_bits && rev_block_applies(f); // (back to front, not complemented)
    pl.flags = t.tune;

    // forward passes of One, Graph and GapSize (and, when asked for, the reverse ones of the latter two): lane form
    const bool lane_dir = dir == 0 ? !flip : ((method == BRX_GRAPH && (t.lane_rev & 1u)) || (method == BRX_GAP_SIZE && (t.lane_rev & 2u)));
    if ((method == BRX_ONE || walker) && lane_dir && plan_lane(t, f, method, confirm, n_reads, in_total_bound, pl))
        return pl;

    int gw = dir ? group_width(t, true, false, n_reads) : group_width(t, false, f.has_idx, n_reads); // (forward: 8 exists for One only)
    if (gw < 16 && method != BRX_ONE) {
        // the walking methods spend most of their rounds on one walk step = 4 probes: narrow groups keep the lanes busy
        // there (BRX_GROUP_WALK); Two and Greedy need 16 lanes for their stage-1 probes
        gw = walker ? t.group_walk : 16;
    }
    if (dir == 1 && (walker || (method == BRX_ONE && t.rev_lean_one)) && gw == 64 && t.rev_lean) {
        pl.form = PASS_REV_LEAN;
        pl.width = 64;
        pl.blocks = pass_blocks(t, n_reads, 64);
        pl.verify_width = walker ? t.rev_verify_g : 8;
        pl.verify_grid_width = t.rev_verify_g;
        return pl;
    }
    pl.form = PASS_GROUP;
    if (method == BRX_GREEDY) {
        gw = greedy_group(gw, f.k, max_search, &pl.g_dim, &pl.g_lds_bytes);
        if (!gw) {
            pl.form = PASS_NO_LDS;
            return pl;
        }
        pl.lds = (uint32_t)(256 / gw) * pl.g_lds_bytes;
    }
    pl.width = gw;
    pl.one_kernel = method == BRX_ONE && gw != 32 && !t.one_v1; // (4-lane groups exist in this form only)
    pl.blocks = pass_blocks(t, n_reads, gw, method == BRX_ONE);
    return pl;
}

} // namespace brx
