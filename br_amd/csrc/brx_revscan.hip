// ======================================================================================================================
// Reverse passes of Graph / GapSize, lean form.  run_correction's second direction (src/lib.rs:48-55) reads
// the read back to front WITHOUT complementing it: hardly a k-mer is solid, a trigger (mod.rs:73) is a chance hit, and what
// follows it is all but always one of
//   error_len (mod.rs:130-152) runs off the read        -> Graph: None (the target is not solid, no walk can reach it);
//                                                          GapSize with error_len < k: the same
//   alt_nucs does not name exactly one alternative      -> None for every method (exist/mod.rs:123-126, graph.rs:51-55,
//                                                          greedy.rs, gap_size.rs:47-50)
//   one alternative (the k-mer in front of the trigger is a genome k-mer, the alternative its successor in the genome)
//                                                       -> the method goes to work and returns None after all: the walk
//                                                          follows the genome and never meets a target that lies in a
//                                                          reversed read; the scenarios' look-aheads do not hold
// i.e. the read leaves the pass as it came.  This kernel scans on that assumption -- scan, error_len, alt_nucs, one wave
// per read, 64 k-mers a round, nothing of the methods' state -- and NOTES every trigger of the third kind (TrigRec).  A
// second launch, correct_kernel<8, M, 2> (<4, M, 2> on request), takes the notes as its work items: a narrow group enters the method at
// alt_nucs with the state the scan would have had there, runs it, writes nothing, and flags the read unless the result
// is None; flagged reads (none for Graph, 4 956 of 100 000 for GapSize over the bench's data) are then corrected from
// scratch by the 64-lane group kernel over their list (correct_kernel<64, M, 1>).  A read none of whose triggers is flagged is exactly the copy the reference makes:
// by induction over its triggers, each was reached with the reference's state and returned None like the reference's.
// What it saves is the group kernel's register file (5 waves per SIMD against 7 here) and the instructions of its state
// dispatch around rounds that are nearly all "64 positions, nothing".
// ======================================================================================================================
#include "brx_correct.hpp"

using namespace brx;

namespace {

#ifndef BRX_REV_WAVES
#define BRX_REV_WAVES 7 // (8 / 7 / 6 waves measure the same: profiles/r4o_rev_lean_ab.txt; 62 registers for k = 19 / 21)
#endif
template <int KT, int M>
__global__ __launch_bounds__(256, BRX_REV_WAVES) void rev_scan_kernel(const PassParams pp, uint32_t *__restrict__ handback, uint32_t *__restrict__ redo_flag,
                                                                          TrigRec *__restrict__ notes, uint32_t trig_cap)
{
    // (the fields the loop needs, by value: a lambda that captures the parameter block by reference makes the compiler
    // keep a copy of all of it in scratch)
    const IdxView idx = pp.idx;
    const uint32_t *const bits = pp.bits;
    unsigned long long *const ctrl = pp.ctrl;
    const uint32_t n_reads = pp.n_reads, slack = pp.slack;
    const uint64_t *const offsets = pp.offsets;
    const uint8_t *const in_base = pp.in;
    const uint32_t *const in_lens = pp.in_lens;
    const bool in_staged = pp.in_staged != 0, flip = pp.flip != 0, rev_batch = pp.rev_batch != 0;
    uint8_t *const out_base = pp.out;
    uint32_t *const out_lens = pp.out_lens;
    constexpr bool HAS_ERRLEN = (M == BRX_GRAPH || M == BRX_GAP_SIZE);
    const int lane = threadIdx.x & 63;
    const int k = KT ? KT : pp.k;
    const uint64_t mask = kmask(k);
    uint32_t n_rounds = 0, n_probes = 0, n_trig = 0;

    // KmerSet::get.  An index line that overflowed at build time cannot say "absent" (one probe in a thousand, i.e. nearly
    // every 10 kb read meets one): the lane asks the bit vector, or -- sparse sets, whose keys chain into the following
    // lines -- the next lines of the chain, while its wave waits.
    // (always_inline: left to itself the compiler CALLS the probe from the three places that ask -- s_swappc, registers saved
    // through lanes and scratch -- and the scan ran at 9.1 ms per Gbp where one_kernel<64>'s identical loop takes 5.7)
    auto ask = [&](uint64_t km) __attribute__((always_inline)) -> bool { return idx.lines ? set_get<true, LINE_BITS_KEPT>(idx, bits, km, k) : probe(bits, km, k); };
    auto last_of = [&](uint64_t km, uint32_t l) __attribute__((always_inline)) -> uint64_t {
        return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(km >> 32), (int)l) << 32) |
               (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)km, (int)l);
    };

    for (;;) {
        unsigned long long w = 0;
        if (lane == 0)
            w = atomicAdd(ctrl + CTL_WORK, 1ull);
        // (lane 0's value into a scalar register: everything derived from it -- the read's pointers, its length, the
        // loop state -- then lives in scalar registers, too)
        const uint32_t r = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)w);
        if (__builtin_amdgcn_readfirstlane((int)(uint32_t)(w >> 32)) != 0 || r >= n_reads)
            break;
        const uint64_t o0 = offsets[r], o1 = offsets[r + 1];
        const uint8_t *in;
        uint32_t n;
        if (in_staged) {
            in = in_base + slot_of(o0, r, slack);
            n = in_lens[r];
            if (n == 0xffffffffu) { // poisoned by an earlier pass of this attempt: stays poisoned
                if (lane == 0)
                    out_lens[r] = 0xffffffffu;
                continue;
            }
        } else {
            in = in_base + o0;
            n = (uint32_t)(o1 - o0);
        }
        const uint64_t s0 = slot_of(o0, r, slack), s1 = slot_of(o1, (uint64_t)r + 1, slack);
        uint8_t *out = out_base + s0;
        const uint32_t cap = (uint32_t)(s1 - s0);
        auto ld = [&](uint32_t j) __attribute__((always_inline)) -> uint8_t { return in[flip ? (n - 1u - j) : j]; };

        if (n < (uint32_t)k) { // mod.rs:56-58
            for (uint32_t j = (uint32_t)lane; j < n; j += 64u)
                out[j] = ld(j);
            if (lane == 0)
                out_lens[r] = n;
            continue;
        }
        bool hb = n + 1u > cap; // (the group kernel's slot check; it poisons the read)
        uint64_t kmer = 0;
        uint32_t i = (uint32_t)k, skip_until = 0, trig_read = 0;
        bool prev = false;
        if (!hb) {
            for (int j = 0; j < k; j++)
                kmer = (kmer << 2) | nuc2bit(ld((uint32_t)j));
            if (lane < k)
                out[lane] = ld((uint32_t)lane);
            prev = ask(kmer); // mod.rs:67
            n_rounds++;
            n_probes++;
        }
        while (!hb && i < n) {
            // ---- scan, REV_BLOCK full rounds at a time where the occupancy bits can filter them (rev_block_rounds) ----
            if (rev_batch && n - i >= 64u * REV_BLOCK + 1u) {
                const uint32_t t = rev_block_rounds<HAS_ERRLEN>(idx, bits, k, mask, lane,
                                                                [in, n, flip](uint32_t j) -> uint8_t { return in[flip ? (n - 1u - j) : j]; }, i,
                                                                out + i, skip_until, kmer, prev);
                for (uint32_t q = 0; q < t; q++) { // (what the one-round form below counts: the positions it asks about)
                    const uint32_t p0 = i + 64u * q;
                    const uint32_t skipped = (HAS_ERRLEN && skip_until > p0) ? (skip_until - p0 < 64u ? skip_until - p0 : 64u) : 0u;
                    n_probes += 64u - skipped;
                }
                n_rounds += t;
                i += 64u * t;
                if (t == (uint32_t)REV_BLOCK)
                    continue;
            }
            // ---- scan: 64 positions (mod.rs:68-104 while nothing triggers) -------------------------------------------
            const uint32_t pos = i + (uint32_t)lane;
            const bool valid = pos < n;
            const uint8_t c8 = valid ? ld(pos) : (uint8_t)0;
            const uint64_t km = lane_kmer64_dpp(kmer, (uint32_t)nuc2bit(c8), lane, mask);
            // (positions below skip_until: error_len asked about them behind a trigger that failed -- not solid)
            const bool asks = valid && !(HAS_ERRLEN && pos < skip_until);
            const bool a1 = asks && ask(km);
            n_rounds++;
            n_probes += (uint32_t)__builtin_popcountll(__ballot(asks));
            const uint32_t left = n - i;
            const uint32_t cnt = left < 64u ? left : 64u;
            const uint64_t vmask = cnt >= 64u ? ~0ull : ((1ull << cnt) - 1ull);
            const uint64_t bs = __ballot(a1);
            const uint64_t trig = ~bs & ((bs << 1) | (prev ? 1ull : 0ull)) & vmask; // mod.rs:73
            if (!trig) {
                if (valid)
                    out[pos] = c8; // mod.rs:100 (nothing changes the read here: output position == input position)
                kmer = last_of(km, cnt - 1u);
                prev = (bs >> (cnt - 1u)) & 1ull; // mod.rs:99
                i += cnt;
                continue;
            }
            const uint32_t t = (uint32_t)__builtin_ctzll(trig);
            if ((uint32_t)lane < t)
                out[pos] = c8;
            i += t;
            kmer = last_of(km, t); // the k-mer that triggered; the read's base stays in it when the method fails (mod.rs:91-96)
            trig_read++;
            uint32_t elen = 0;
            uint64_t fc = 0;
            bool hit_end = false;
            if (HAS_ERRLEN) {
                // ---- error_len, mod.rs:130-152: the k-mers behind the trigger until the first solid one ---------------
                uint64_t ek = kmer;
                uint32_t ej = 0;
                const uint32_t rem = n - i;
                for (;;) {
                    const uint32_t j = ej + 1u + (uint32_t)lane;
                    const bool v2 = j < rem;
                    const uint8_t c2 = v2 ? ld(i + j) : (uint8_t)0;
                    const uint64_t km2 = lane_kmer64_dpp(ek, (uint32_t)nuc2bit(c2), lane, mask);
                    const bool a2 = v2 && ask(km2);
                    n_rounds++;
                    n_probes += (uint32_t)__builtin_popcountll(__ballot(v2));
                    const uint64_t sm = __ballot(a2);
                    if (sm) {
                        const uint32_t t2 = (uint32_t)__builtin_ctzll(sm);
                        elen = ej + 1u + t2;
                        fc = last_of(km2, t2);
                        break;
                    }
                    if (rem <= ej + 1u + 64u) { // ran off the read: the last k-mer built is not solid
                        const uint32_t nv = rem - (ej + 1u);
                        elen = rem;
                        fc = nv ? last_of(km2, nv - 1u) : ek;
                        hit_end = true;
                        break;
                    }
                    ek = last_of(km2, 63u);
                    ej += 64u;
                }
            }
            // Graph: a target that is not solid cannot be reached (every walk k-mer is solid, graph.rs:79); GapSize sends
            // error_len < k the same way (gap_size.rs:97-108)
            const bool none_already = HAS_ERRLEN && hit_end && (M == BRX_GRAPH || elen < (uint32_t)k);
            if (!none_already) {
                // ---- alt_nucs: the read's own base is the trigger k-mer, known not solid ----------------------------
                const bool asks3 = lane < 4 && (uint64_t)lane != (kmer & 3ull);
                const bool a3 = asks3 && ask(add_nuc(kmer >> 2, (uint64_t)(lane & 3), mask));
                n_rounds++;
                n_probes += 3u;
                if (__builtin_popcountll(__ballot(a3)) == 1) {
                    // A unique alternative: the method goes to work -- in a reverse pass all but always to return None
                    // after all (a walk along the genome that never meets the target, scenarios that do not hold).  The
                    // scan goes on as if it had; the group kernel's verify pass checks this trigger (SRC == 2).
                    unsigned long long at = 0;
                    if (lane == 0)
                        at = atomicAdd(ctrl + CTL_REV_TRIGS, 1ull);
                    const uint32_t at_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)at);
                    if (__builtin_amdgcn_readfirstlane((int)(uint32_t)(at >> 32)) != 0 || at_lo >= trig_cap) {
                        hb = true; // (no room to note it: the whole read goes to the group kernel)
                        break;
                    }
                    if (lane == 0) {
                        notes[at_lo] = TrigRec{r, i, elen, 0u, fc};
                        atomicAdd(ctrl + CTL_REV_TRIGS_SUM, 1ull);
                    }
                }
            }
            // ---- None: mod.rs:91-96 ------------------------------------------------------------------------------------
            if (lane == 0)
                out[i] = ld(i);
            if (HAS_ERRLEN)
                skip_until = i + elen;
            i += 1u;
            prev = false;
            if (HAS_ERRLEN && skip_until >= n) {
                // no k-mer behind the trigger is solid: nothing triggers any more (`previous` stays false)
                for (uint32_t j = i + (uint32_t)lane; j < n; j += 64u)
                    out[j] = ld(j);
                i = n;
            }
        }
        if (lane == 0) {
            if (hb) {
                if (atomicExch(redo_flag + r, 1u) == 0u) {
                    handback[atomicAdd(ctrl + CTL_REV_HANDBACK, 1ull)] = r;
                    atomicAdd(ctrl + CTL_REV_HANDBACK_SUM, 1ull);
                }
            } else {
                out_lens[r] = n;
            }
        }
        if (!hb)
            n_trig += trig_read; // (a read handed back counts its events in the group kernel)
    }
    if (lane == 0) {
        if (n_rounds)
            atomicAdd(ctrl + CTL_ROUNDS, (unsigned long long)n_rounds);
        if (n_probes)
            atomicAdd(ctrl + CTL_PROBES, (unsigned long long)n_probes);
        if (n_trig)
            atomicAdd(ctrl + CTL_TRIGGERS, (unsigned long long)n_trig);
    }
}

template <int M>
void launch_rev_scan(const PassParams &p, uint32_t *list, uint32_t *flag, TrigRec *trig, uint32_t trig_cap, uint32_t blocks, hipStream_t s)
{
    dispatch_k(p.k, [&](auto K) { rev_scan_kernel<decltype(K)::value, M><<<blocks, 256, 0, s>>>(p, list, flag, trig, trig_cap); });
}

} // namespace

namespace brx {

// a reverse pass in lean form (rev_scan_kernel), then the group kernel over the triggers it left open and over the reads
// it handed back; both grids stay inside the visited lists the chain has sized (see launch_walk_list)
int launch_rev_lean(brx_chain *ch, PassParams p, const PassPlan &pl, const brx_method_t &md, uint64_t path_lists, hipStream_t s)
{
    // room for four open triggers per read on average (the bench's data: 1.2); a scan that finds no room hands its read back
    const uint64_t trig_cap64 = 4ull * p.n_reads + 4096ull;
    const uint32_t trig_cap = trig_cap64 > 0x7fffffffull ? 0x7fffffffu : (uint32_t)trig_cap64;
    const uint64_t list_bytes = (uint64_t)p.n_reads * 4ull, trig_bytes = (uint64_t)trig_cap * sizeof(TrigRec);
    BRX_TRY(ch->d_rev_list.reserve_bytes(list_bytes, ws_headroom(list_bytes), "workspace"));
    BRX_TRY(ch->d_rev_flag.reserve_bytes(list_bytes, ws_headroom(list_bytes), "workspace"));
    BRX_TRY(ch->d_rev_trig.reserve_bytes(trig_bytes, ws_headroom(trig_bytes), "workspace"));
    BRX_HIP(hipMemsetAsync(p.ctrl + CTL_REV_HANDBACK, 0, 8, s));
    BRX_HIP(hipMemsetAsync(p.ctrl + CTL_REV_TRIGS, 0, 8, s));
    BRX_HIP(hipMemsetAsync(ch->d_rev_flag, 0, (uint64_t)p.n_reads * 4ull, s));
    TrigRec *trig = (TrigRec *)ch->d_rev_trig.get();
    {
        KernelTimer t(pass_timer_name(md.method), s);
        switch (md.method) {
        case BRX_ONE: launch_rev_scan<BRX_ONE>(p, ch->d_rev_list, ch->d_rev_flag, trig, trig_cap, pl.blocks, s); break;
        case BRX_GRAPH: launch_rev_scan<BRX_GRAPH>(p, ch->d_rev_list, ch->d_rev_flag, trig, trig_cap, pl.blocks, s); break;
        case BRX_GAP_SIZE: launch_rev_scan<BRX_GAP_SIZE>(p, ch->d_rev_list, ch->d_rev_flag, trig, trig_cap, pl.blocks, s); break;
        default: set_error("launch_rev_lean: method %u", md.method); return BRX_ERR_ARG;
        }
        BRX_HIP(hipGetLastError());
    }
    // (a list is a few reads and the grid loops over it; the open triggers are many: as many groups as the lists allow)
    const auto rest = [&](const PassParams &q, uint32_t groups_per_block, const char *timer) -> int {
        BRX_HIP(hipMemsetAsync(q.ctrl + CTL_WORK, 0, 8, s));
        return launch_group(q, pl, md, list_grid(path_lists, groups_per_block, MAX_BLOCKS), timer, s);
    };
    // the open triggers, one narrow group each
    PassParams v = p;
    v.trig = trig;
    v.trig_cap = trig_cap;
    v.only_n = p.ctrl + CTL_REV_TRIGS;
    v.redo_list = ch->d_rev_list;
    v.redo_flag = ch->d_rev_flag;
    BRX_TRY(rest(v, 256u / (uint32_t)pl.verify_grid_width, "rev_verify"));
    // ... and the reads whose trigger did not end in None (or that found no room for a note), from scratch
    p.only = ch->d_rev_list;
    p.only_n = p.ctrl + CTL_REV_HANDBACK;
    return rest(p, 4u, "rev_redo"); // (64-lane groups)
}

} // namespace brx
