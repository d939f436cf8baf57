// ======================================================================================================================
// correct::One, second form (the metric's kernel).  Same rounds, same probes, same bytes out as correct_kernel<G, BRX_ONE>;
// what changed is how many instructions a round costs.  rocprofv3's SQ counters showed the first form issue-bound, not
// memory-bound (VALU busy ~75 % of every SIMD's cycles, 27 of 64 lanes active: profiles/r1k_sq_summary.json), and
// tools/valu_rate.hip showed every VALU instruction costs the same issue slot while a ds_bpermute costs six:
//   - the lanes' k-mers come from a DPP row_shr scan of 2-bit codes in 32-bit registers (2 instructions per step, no
//     LDS crossbar) instead of a 64-bit __shfl_up scan (8 per step);
//   - the group's next k-mer after a SCAN round is cut from the group's code window (one 32-bit broadcast issued before
//     the probe's memory wait) instead of two 64-bit shuffles after it;
//   - k is a template parameter for the k's that matter (19, 21), which turns the variable 64-bit shifts into constants;
//   - event counters are one packed register, flushed per wave every 256 rounds.
// G = 8 / 16: groups inside one DPP row.  G = 64: one group per wave, group state in scalar registers.
// ======================================================================================================================
#include "brx_correct.hpp"

using namespace brx;

namespace {

__device__ __forceinline__ uint32_t row_scan4(uint32_t code)
{
    uint32_t v = code;
    v |= dpp_row_shr<1>(v) << 2;
    v |= dpp_row_shr<2>(v) << 4;
    return v; // lanes of the row's later groups also carry codes of the group before: the caller keeps 2 * (gl + 1) bits
}
__device__ __forceinline__ uint32_t row_scan8(uint32_t code)
{
    uint32_t v = code;
    v |= dpp_row_shr<1>(v) << 2;
    v |= dpp_row_shr<2>(v) << 4;
    v |= dpp_row_shr<4>(v) << 8;
    return v; // lanes 8..15 of a row also carry codes of lanes 0..7: the caller keeps 2 * (gl + 1) bits
}

template <int G, int KT, bool LIST = false>
#ifndef BRX_ONE64_WAVES
#define BRX_ONE64_WAVES 7 // (the 64-lane form, every One chain's reverse pass; tools/ab_build.sh sweeps it)
#endif
__global__ __launch_bounds__(256, (G == 64 ? BRX_ONE64_WAVES : 7)) void one_kernel(PassParams p)
{
    static_assert(G == 4 || G == 8 || G == 16 || G == 64, "one_kernel: 4, 8, 16 or 64 lanes per read");
    const int lane0 = threadIdx.x & 63;
    int lane = lane0, gl = lane0 & (G - 1), gshift = lane0 & ~(G - 1); // re-derived every round from an opaque copy (see the loop)
    constexpr uint32_t GM32 = G >= 32 ? 0xffffffffu : ((1u << (G & 31)) - 1u);
    const int k = KT ? KT : p.k;
    const uint32_t c = (uint32_t)p.c;
    const uint64_t mask = kmask(k);
    uint32_t bcast_addr = (uint32_t)(gshift + G - 1) * 4u; // ds_bpermute address of the group's last lane
    uint32_t nb2 = 2u * ((uint32_t)gl + 1u);               // bits of this lane's scan value
    constexpr int WB = G == 4 ? 16 : (G < 32 ? G : 32);          // bases in the look-ahead window

    // group-uniform state
    uint32_t r = 0, n = 0, cap = 0, i = 0, olen = 0;
    const uint8_t *in = nullptr;
    uint8_t *out = nullptr;
    uint64_t kmer = 0, corr = 0;
    bool prev = false, have = false;
    int st = ST_INIT;
    uint32_t sub = 0, failmask = 0, passmask = 0;
    uint32_t hop = 0;
    bool slow = false, was_unres = false, kept_sol = false;
    typename std::conditional<(G < 32), uint32_t, uint64_t>::type win = 0; // seq[i .. i+WB) at the trigger, 2 bits per base
    uint32_t steps = 0;
    // events of this lane since the last flush: rounds | probes << 8 | triggers << 16 | fixes << 24 (flushed every
    // 255 rounds at most, so no field overflows)
    uint32_t ev = 0, since_flush = 0;
    // the base this lane probes in the next SCAN round, loaded at the end of the round before (G < 64): a round is a
    // dependent chain base load -> k-mer -> probe -> transition, and this takes the first link out of it
    uint8_t pf_ch = 0;

    auto flush = [&]() {
        // per-field sums over the wave, then one atomic per counter: every 255 rounds, so it is noise (and keeps the
        // totals out of the register file of a kernel that sits at its 80-VGPR limit)
        uint32_t a = ev & 0xffu, b = (ev >> 8) & 0xffu, cc = (ev >> 16) & 0xffu, d = ev >> 24;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            a += __shfl_xor(a, o);
            b += __shfl_xor(b, o);
            cc += __shfl_xor(cc, o);
            d += __shfl_xor(d, o);
        }
        if (lane == 0) {
            if (a)
                atomicAdd(p.ctrl + CTL_ROUNDS, (unsigned long long)a);
            if (b)
                atomicAdd(p.ctrl + CTL_PROBES, (unsigned long long)b);
            if (cc)
                atomicAdd(p.ctrl + CTL_TRIGGERS, (unsigned long long)cc);
            if (d)
                atomicAdd(p.ctrl + CTL_FIXES, (unsigned long long)d);
        }
        ev = 0;
        since_flush = 0;
    };

    auto fetch = [&]() {
        for (;;) {
            unsigned long long w = 0;
            if (gl == 0)
                w = atomicAdd(p.ctrl + CTL_WORK, 1ull);
            w = __shfl(w, gshift);
            // LIST: the reads of a list made on the device (the few reads the lane-per-chunk pass handed back)
            if (w >= (LIST ? *p.only_n : (unsigned long long)p.n_reads)) {
                have = false;
                return;
            }
            have = true;
            r = LIST ? p.only[w] : (uint32_t)w;
            const uint64_t o0 = p.offsets[r], o1 = p.offsets[r + 1];
            if (p.in_staged) {
                in = p.in + slot_of(o0, r, p.slack);
                n = p.in_lens[r];
                if (n == 0xffffffffu) { // poisoned by an earlier pass of this attempt: stays poisoned
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
            return;
        }
    };
    auto ld = [&](uint32_t j) -> uint8_t { return in[p.flip ? (n - 1u - j) : j]; };
    // The read is finished (or given up) at ONE place, the end of the round: every call site of an inlined fetch()
    // redefines the whole group state, and the compiler pays for each with a block of register copies at the join.
    int done = 0; // 0 no, 1 finished, 16 + the CTL_* counter of the reason the read was given up
    auto finish = [&]() { done = 1; };
    auto give_up = [&](int which) { done = 16 + which; };
    // this lane's k-mer: `carry` extended by the codes of lanes 0..gl of the group (scan = those codes, 32 bits)
    auto lane_kmer = [&](uint64_t carry, uint32_t code, uint32_t &scan_out) -> uint64_t {
        if (G == 4) {
            const uint32_t v = row_scan4(code) & ((1u << nb2) - 1u);
            scan_out = v;
            return ((carry << nb2) | v) & mask;
        } else if (G == 8) {
            const uint32_t v = row_scan8(code) & ((1u << nb2) - 1u);
            scan_out = v;
            return ((carry << nb2) | v) & mask;
        } else if (G == 16) {
            const uint32_t v = row_scan16(code);
            scan_out = v;
            return ((carry << nb2) | v) & mask; // nb2 <= 32
        } else {
            // 64 lanes = 4 rows: own row's codes + the 16-base words of the two rows before (row 0 / 1: of `carry`)
            scan_out = 0;
            return lane_kmer64_dpp(carry, code, lane, mask);
        }
    };
    // km extended by window bases b0 .. b0+nb-1 (b0 + nb <= WB; the window holds seq[i .. i+WB) at the trigger)
    auto ext = [&](uint64_t km, uint32_t b0, uint32_t nb) -> uint64_t {
        const uint64_t bits = (uint64_t)((win >> (2u * ((uint32_t)WB - b0 - nb))) & (decltype(win))((1ull << (2u * nb)) - 1ull));
        return ((km << (2u * nb)) | bits) & mask;
    };

    fetch();

    while (__any(have)) {
        // The compiler hoists every lane constant out of this loop (2*(gl+1), gl-3, (gl==0)<<16, ...) and then, at the
        // 80-register limit, spills some of them to scratch and reloads them in the SCAN path.  Deriving them from an
        // opaque copy of the lane id costs four instructions per round and keeps the register file for the state.
        lane = lane0;
        asm volatile("" : "+v"(lane));
        gl = lane & (G - 1);
        gshift = lane & ~(G - 1);
        bcast_addr = (uint32_t)(lane | (G - 1)) * 4u;
        nb2 = 2u * ((uint32_t)gl + 1u);
        if (G == 64) {
            // One group per wave: everything below is wave-uniform.  The reverse pass of run_correction (src/lib.rs:48-55)
            // reads the bases back to front WITHOUT complementing them, so hardly any of its k-mers is solid and nearly
            // every round is "64 positions, no trigger": that round in a loop of its own, without the state dispatch,
            // the trigger machinery and the register copies at their joins.  A round that does find a trigger is left to the general
            // code below, which redoes its probes (they are pure).
            // REV_BLOCK such rounds at a time where the set's occupancy bits can filter them (rev_block_rounds,
            // brx_correct.hpp); the rounds left over, and the round that holds a trigger, go through the loop behind it.
            while (p.rev_batch && have && st == ST_SCAN && !slow && n - i >= 64u * REV_BLOCK + 1u && olen + 64u * REV_BLOCK + 2u <= cap) {
                // (the packed counters take REV_BLOCK rounds at once: make room first, so that no field passes 255 and
                // since_flush stays below the 255 the one-round paths test for)
                if (since_flush + REV_BLOCK >= 255u)
                    flush();
                const uint8_t *const in_b = (const uint8_t *)uni64((uint64_t)in);
                uint8_t *const out_b = (uint8_t *)uni64((uint64_t)(out + olen));
                const uint32_t n_b = uni32(n), i_b = uni32(i);
                const bool flip_b = p.flip != 0;
                const uint32_t t = rev_block_rounds<false>(p.idx, p.bits, k, mask, lane,
                                                           [in_b, n_b, flip_b](uint32_t j) -> uint8_t { return in_b[flip_b ? (n_b - 1u - j) : j]; }, i_b,
                                                           out_b, 0u, kmer, prev);
                olen += 64u * t;
                i += 64u * t;
                ev += ((lane == 0) ? t : 0u) + (t << 8);
                steps += t;
                since_flush += t;
                if (t < (uint32_t)REV_BLOCK)
                    break;
            }
            while (have && st == ST_SCAN && !slow && n - i >= 65u && olen + 66u <= cap) {
                const uint8_t c8 = ld(i + (uint32_t)lane);
                uint32_t sc;
                const uint64_t km = lane_kmer(kmer, (uint32_t)nuc2bit(c8), sc);
                // (an overflowed index line is settled by the lane that met it, set_get)
                const bool s1 = p.idx.lines ? set_get<true, LINE_BITS_KEPT>(p.idx, p.bits, km, k) : probe(p.bits, km, k);
                const uint64_t bs = __ballot(s1);
                const uint64_t trig = ~bs & ((bs << 1) | (prev ? 1ull : 0ull)); // mod.rs:73
                if (trig)
                    break;
                out[olen + (uint32_t)lane] = c8; // mod.rs:100
                olen += 64u;
                i += 64u;
                kmer = wave_carry(km);
                prev = (bs >> 63) & 1ull; // mod.rs:99
                ev += ((lane == 0) ? 1u : 0u) + (1u << 8);
                steps++;
                if (++since_flush == 255u)
                    flush();
            }
        }
        bool do_probe = false;
        uint64_t pk = 0;
        uint8_t ch = 0;
        uint32_t sc_s = 0, scan = 0, gwin = 0;
        bool sc_active = false;

        // ---------------- phase 1 -----------------------------------------------------------------------------------
        if (have) {
            ev += (gl == 0) ? 1u : 0u;
            if (st == ST_SCAN) {
                const uint32_t pos = i + (uint32_t)gl;
                const bool valid = pos < n;
                if (G < 64)
                    ch = pf_ch; // prefetched for exactly this i (every way into SCAN ends with the prefetch below)
                else
                    ch = valid ? ld(pos) : (uint8_t)0;
                pk = lane_kmer(kmer, (uint32_t)nuc2bit(ch), scan);
                do_probe = valid;
                if (G <= 16) // all G codes of the group, for the k-mer the group leaves this round with
                    gwin = (uint32_t)__builtin_amdgcn_ds_bpermute((int)bcast_addr, (int)scan);
            } else if (st == ST_INIT) {
                if (n < (uint32_t)k) {
                    for (uint32_t j = gl; j < n; j += G) // mod.rs:56-58
                        out[j] = ld(j);
                    olen = n;
                } else {
                    if (G == 64) {
                        // (one base per lane and the scan that builds the rounds' k-mers: k loads in flight per lane were
                        // the kernel's register peak)
                        const uint8_t cj = lane < k ? ld((uint32_t)lane) : (uint8_t)0;
                        const uint64_t kv = lane_kmer64_dpp(0ull, (uint32_t)nuc2bit(cj), lane, mask);
                        kmer = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(kv >> 32), k - 1) << 32) |
                               (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)kv, k - 1);
                        if (lane < k)
                            out[lane] = cj;
                    } else {
                        uint64_t km = 0;
                        for (int j = 0; j < k; j++)
                            km = (km << 2) | nuc2bit(ld((uint32_t)j));
                        kmer = km;
                        for (uint32_t j = gl; j < (uint32_t)k; j += G)
                            out[j] = ld(j);
                    }
                    olen = (uint32_t)k;
                    i = (uint32_t)k;
                    do_probe = (gl == 0);
                    pk = kmer;
                }
            } else if (st == ST_ALTS) {
                do_probe = gl < 4 && (uint64_t)gl != (kmer & 3ull); // the read's own base is the trigger k-mer: known non-solid
                pk = (kmer & ~3ull) | (uint64_t)gl;                  // add_nuc(kmer >> 2, gl)
                // the bases the scenarios will look at, fetched once: seq[i .. i+WB)
                if (G == 4) {
                    // four bases per lane: one (unaligned) dword, the four codes gathered into a byte by one multiply
                    const uint32_t w4 = i + 4u * (uint32_t)gl;
                    uint32_t raw = 0;
                    if (w4 + 4u <= n) {
                        const uint8_t *q = p.flip ? in + (n - 4u - w4) : in + w4;
                        __builtin_memcpy(&raw, q, 4);
                        if (p.flip)
                            raw = __builtin_bswap32(raw);
                    } else {
                        for (uint32_t t = 0; t < 4u && w4 + t < n; t++)
                            raw |= (uint32_t)ld(w4 + t) << (8u * t);
                    }
                    // bytes b0..b3 (b0 = first base) -> b0<<6 | b1<<4 | b2<<2 | b3: the four products land in bits 24-31, every
                    // other partial product below bit 24 or beyond bit 31, none overlapping
                    uint32_t v = ((((raw >> 1) & 0x03030303u) * 0x40100401u) >> 24);
                    v |= dpp_row_shr<1>(v) << 8;
                    v |= dpp_row_shr<2>(v) << 16;
                    if (gl != 3)
                        v &= (1u << (8u * ((uint32_t)gl + 1u))) - 1u;
                    win = (uint32_t)__builtin_amdgcn_ds_bpermute((int)bcast_addr, (int)v);
                }
                const uint32_t wp = i + (uint32_t)gl;
                const uint32_t cd = (G != 4 && gl < WB && wp < n) ? (uint32_t)nuc2bit(ld(wp)) : 0u;
                if (G == 4) {
                } else if (G == 8) {
                    const uint32_t v = row_scan8(cd) & ((1u << nb2) - 1u);
                    win = (uint32_t)__builtin_amdgcn_ds_bpermute((int)bcast_addr, (int)v);
                } else if (G == 16) {
                    win = (uint32_t)__builtin_amdgcn_ds_bpermute((int)bcast_addr, (int)row_scan16(cd));
                } else {
                    // rows 0 and 1 of the wave hold the 32 window bases
                    const uint32_t v = row_scan16(cd);
                    const uint32_t w0 = (uint32_t)__builtin_amdgcn_readlane((int)v, 15), w1 = (uint32_t)__builtin_amdgcn_readlane((int)v, 31);
                    win = ((uint64_t)w0 << 32) | w1;
                }
            } else if (st == ST_SCEN && (G == 8 || G == 16)) {
                // get_score's look-aheads (exist/mod.rs:21-47) with a FIXED lane -> probe map (dealing the lanes to the
                // surviving scenarios at run time cost more instructions than the rounds it saved):
                //   stage A (sub == 0): lane 2s + j probes look-ahead j < 2 of scenario s -- a wrong scenario dies here;
                //   stage B: the lowest scenario still in and not yet complete gets lanes 0.. for its look-aheads sub..c-1.
                uint32_t off, j;
                if (sub == 0u) {
                    sc_s = (uint32_t)gl >> 1;
                    j = (uint32_t)gl & 1u;
                    sc_active = gl < 6 && !((failmask >> sc_s) & 1u) && j < c;
                } else {
                    sc_s = (uint32_t)__ffs(7u & ~failmask & ~passmask) - 1u;
                    j = sub + (uint32_t)gl;
                    sc_active = j < c;
                }
                off = 2u - sc_s; // I:2 S:1 D:0 (one.rs:57-63)
                if (sc_active) {
                    if (c + 3u <= (uint32_t)WB) {
                        pk = ext(corr, off, j + 1u);
                    } else {
                        pk = corr;
                        for (uint32_t q = 0; q <= j; q++)
                            pk = add_nuc(pk, nuc2bit(ld(i + off + q)), mask);
                    }
                    do_probe = true;
                }
            } else if (st == ST_SCEN) {
                const uint32_t width = scen_width(sub, c, G, 0u, failmask);
                const uint32_t e = (uint32_t)gl;
                const uint32_t alive = ~failmask & 7u;
                // ord = e / width, e % width -- at most three scenarios, so two compares do the division
                const uint32_t ord = (e >= width ? 1u : 0u) + (e >= 2u * width ? 1u : 0u);
                sc_active = e < 3u * width && ord < (uint32_t)__popc(alive);
                const uint32_t a1 = alive & (alive - 1u);
                sc_s = !sc_active ? 0u : (ord == 0u ? (uint32_t)__ffs(alive) - 1u : (ord == 1u ? (uint32_t)__ffs(a1) - 1u : 2u));
                const uint32_t j = sub + (sc_active ? e - ord * width : 0u);
                const uint32_t off = 2u - sc_s; // I:2 S:1 D:0 (one.rs:57-63)
                if (sc_active) {
                    if (c + 3u <= (uint32_t)WB) {
                        pk = ext(corr, off, j + 1u);
                    } else {
                        pk = corr;
                        for (uint32_t q = 0; q <= j; q++)
                            pk = add_nuc(pk, nuc2bit(ld(i + off + q)), mask);
                    }
                    do_probe = true;
                }
            } else { // ST_MORE
                if (gl < 3 && ((passmask >> gl) & 1u)) {
                    const uint32_t off = 2u - (uint32_t)gl;
                    const uint32_t rem = n - i;
                    if (rem > c + off + 1u) { // exist/mod.rs:54
                        if (c + 3u <= (uint32_t)WB) {
                            pk = ext(corr, off, c + 1u);
                        } else {
                            pk = corr;
                            for (uint32_t q = 0; q <= c; q++)
                                pk = add_nuc(pk, nuc2bit(ld(i + off + q)), mask);
                        }
                        do_probe = true;
                    }
                }
            }
            if (++steps > (1u << 24) + 64u * n) // runaway guard, as in correct_kernel
                do_probe = false;
        }

        // ---------------- phase 2: one probe per lane -----------------------------------------------------------------
        bool sol = false, retry = false;
        if (p.idx.lines) {
            bool unres = false;
            if (do_probe) {
                if (!slow) {
                    // (through the occupancy bits this costs the forward pass 0.5 ms: its k-mers are mostly present, and
                    // the extra dependent load only lengthens the round)
                    const int pr = index_probe(p.idx, pk, k);
                    sol = pr == 1;
                    unres = pr == 2;
                    ev += 1u << 8;
                } else if (was_unres) {
                    if (p.bits) {
                        sol = probe(p.bits, pk, k);
                    } else {
                        const int pr = index_probe(p.idx, pk, k, hop);
                        sol = pr == 1;
                        unres = pr == 2;
                    }
                    ev += 1u << 8;
                } else {
                    sol = kept_sol;
                }
            }
            const uint64_t ub = __ballot(unres);
            retry = G == 64 ? ub != 0ull : (((uint32_t)(ub >> gshift) & GM32) != 0u);
            hop = retry ? hop + 1u : 0u;
            slow = retry;
            was_unres = unres;
            kept_sol = sol;
        } else if (do_probe) {
            sol = probe(p.bits, pk, k);
            ev += 1u << 8;
        }
        const uint64_t ball = __ballot(sol);

        // ---------------- phase 3 -------------------------------------------------------------------------------------
        if (have && !retry) {
            bool fail = false;
            int apply_s = -1;
            if (st == ST_SCAN) {
                const uint32_t left = n - i;
                const uint32_t nvalid = left < (uint32_t)G ? left : (uint32_t)G;
                uint32_t nacc;
                bool trg;
                bool last_sol;
                if (G == 64) {
                    const uint64_t vmask = (nvalid >= 64) ? ~0ull : ((1ull << nvalid) - 1ull);
                    const uint64_t trig = ~ball & ((ball << 1) | (prev ? 1ull : 0ull)) & vmask; // mod.rs:73
                    trg = trig != 0ull;
                    nacc = trg ? (uint32_t)__builtin_ctzll(trig) : nvalid;
                    last_sol = nacc ? ((ball >> (nacc - 1u)) & 1ull) : prev;
                } else {
                    const uint32_t gm = (uint32_t)(ball >> gshift) & GM32;
                    const uint32_t vmask = (1u << nvalid) - 1u; // G <= 16
                    const uint32_t trig = ~gm & ((gm << 1) | (prev ? 1u : 0u)) & vmask;
                    trg = trig != 0u;
                    nacc = trg ? (uint32_t)__builtin_ctz(trig) : nvalid;
                    last_sol = nacc ? ((gm >> (nacc - 1u)) & 1u) : prev;
                }
                if (olen + nacc + 1u > cap) {
                    give_up(CTL_OVERFLOW);
                } else {
                    if ((uint32_t)gl < nacc)
                        out[olen + (uint32_t)gl] = ch; // mod.rs:100
                    olen += nacc;
                    i += nacc;
                    // the k-mer the group goes on with: after the accepted bases, plus the trigger base if there is one
                    const uint32_t ncodes = nacc + (trg ? 1u : 0u);
                    if (G == 64) {
                        const int src = (int)ncodes - 1; // ncodes >= 1: nvalid >= 1 in SCAN
                        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)pk, src);
                        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(pk >> 32), src);
                        kmer = ((uint64_t)hi << 32) | lo;
                    } else {
                        kmer = ((kmer << (2u * ncodes)) | (uint64_t)(gwin >> (2u * ((uint32_t)G - ncodes)))) & mask;
                    }
                    if (trg) {
                        ev += (gl == 0) ? (1u << 16) : 0u;
                        st = ST_ALTS;
                    } else {
                        prev = last_sol; // mod.rs:99
                        if (i >= n)
                            finish();
                    }
                }
            } else if (st == ST_INIT) {
                if (n < (uint32_t)k) {
                    finish();
                } else {
                    prev = (ball >> gshift) & 1ull; // mod.rs:67
                    if (i >= n)
                        finish();
                    else
                        st = ST_SCAN;
                }
            } else if (st == ST_ALTS) {
                const uint32_t am = (uint32_t)(ball >> gshift) & 0xfu;
                if (__popc(am) != 1) {
                    fail = true; // exist/mod.rs:123-126
                } else {
                    corr = (kmer & ~3ull) | (uint64_t)(__ffs(am) - 1);
                    const uint32_t rem = n - i;
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
                }
            } else if (st == ST_SCEN && (G == 8 || G == 16)) {
                const uint32_t badm = (uint32_t)(__ballot(sc_active && !sol) >> gshift) & GM32;
                const uint32_t two = c < 2u ? c : 2u;
                bool finished = false;
                if (sub == 0u) {
                    failmask |= ((badm & 3u) ? 1u : 0u) | ((badm & 12u) ? 2u : 0u) | ((badm & 48u) ? 4u : 0u);
                    passmask = 0; // from here on: the scenarios whose c look-aheads all held
                    sub = two;
                    if (c <= 2u) {
                        passmask = 7u & ~failmask;
                        finished = true;
                    }
                } else {
                    const uint32_t cur = (uint32_t)__ffs(7u & ~failmask & ~passmask) - 1u; // as in phase 1
                    if (badm) {
                        failmask |= 1u << cur;
                        sub = two;
                    } else {
                        const uint32_t left = c - sub;
                        sub += left < (uint32_t)G ? left : (uint32_t)G;
                        if (sub >= c) {
                            passmask |= 1u << cur;
                            sub = two;
                        }
                    }
                }
                if (failmask == 7u) {
                    fail = true; // exist/mod.rs:132-134
                } else if (finished || (7u & ~failmask & ~passmask) == 0u) {
                    if (passmask == 0u)
                        fail = true;
                    else if (__popc(passmask) == 1)
                        apply_s = __ffs(passmask) - 1; // exist/mod.rs:135-137
                    else
                        st = ST_MORE;
                }
            } else if (st == ST_SCEN) {
                const bool bad = sc_active && !sol;
                const uint32_t w_used = scen_width(sub, c, G, 0u, failmask);
                // lanes [ord*w, (ord+1)*w) worked for the ord-th surviving scenario
                const uint64_t bb = __ballot(bad);
                const uint32_t badm = G == 64 ? 0u : ((uint32_t)(bb >> gshift) & GM32);
                uint32_t alive = ~failmask & 7u, ord = 0;
                for (uint32_t s = 0; s < 3; s++)
                    if ((alive >> s) & 1u) {
                        bool any;
                        if (G == 64) {
                            const uint64_t wm = (w_used >= 64u ? ~0ull : ((1ull << w_used) - 1ull)) << (ord * w_used);
                            any = (bb & wm) != 0ull;
                        } else {
                            any = ((badm >> (ord * w_used)) & ((1u << w_used) - 1u)) != 0u;
                        }
                        if (any)
                            failmask |= 1u << s;
                        ord++;
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
            } else { // ST_MORE
                const uint32_t keep = (uint32_t)(ball >> gshift) & 7u & passmask;
                if (__popc(keep) == 1)
                    apply_s = __ffs(keep) - 1; // exist/mod.rs:143-144
                else
                    fail = true;
            }
            if (have && steps > (1u << 24) + 64u * n) {
                fail = false;
                apply_s = -1;
                give_up(CTL_NONTERM);
            }
            if (fail) {
                // mod.rs:91-96: the trigger base is copied through
                if (olen + 2u > cap) {
                    give_up(CTL_OVERFLOW);
                } else {
                    if (gl == 0)
                        out[olen] = ld(i);
                    olen += 1;
                    i += 1;
                    prev = false;
                    if (i >= n)
                        finish();
                    else
                        st = ST_SCAN;
                }
            } else if (apply_s >= 0) {
                // mod.rs:75-89 with one.rs:65-71
                if (olen + 2u > cap) {
                    give_up(CTL_OVERFLOW);
                } else {
                    if (gl == 0)
                        out[olen] = bit2nuc(corr & 3ull);
                    olen += 1;
                    kmer = corr;
                    prev = true;
                    const uint32_t off = 2u - (uint32_t)apply_s;
                    i += off;
                    ev += (gl == 0) ? (1u << 24) : 0u;
                    // the c look-ahead k-mers of the winning scenario ARE the next c scan k-mers, all found solid: the
                    // reference's loop would copy these bases with previous = true (mod.rs:99-102)
                    if (c > 0u && c + 3u <= (uint32_t)WB && olen + c + 1u <= cap) {
                        for (uint32_t q = (uint32_t)gl; q < c; q += (uint32_t)G)
                            out[olen + q] = ld(i + q);
                        kmer = ext(kmer, off, c);
                        olen += c;
                        i += c;
                    }
                    if (i >= n)
                        finish();
                    else
                        st = ST_SCAN;
                }
            }
        }
        if (G < 64 && have && !done && !retry && st == ST_SCAN) {
            const uint32_t pos = i + (uint32_t)gl;
            pf_ch = pos < n ? ld(pos) : (uint8_t)0;
        }
        if (done) {
            if (gl == 0) {
                p.out_lens[r] = done == 1 ? olen : 0xffffffffu;
                if (done != 1)
                    atomicAdd(p.ctrl + (done - 16), 1ull);
            }
            done = 0;
            fetch();
        }
        if (++since_flush == 255u)
            flush();
    }
    flush();
}

template <int G>
void launch_one_width(const PassParams &p, uint32_t blocks, hipStream_t s)
{
    dispatch_k(p.k, [&](auto K) { one_kernel<G, decltype(K)::value><<<blocks, 256, 0, s>>>(p); });
}

} // namespace

namespace brx {

// One's group kernel over the whole batch at the planned width (the caller checks the launch)
void launch_one(const PassParams &p, int width, uint32_t blocks, hipStream_t s)
{
    if (width == 4)
        launch_one_width<4>(p, blocks, s);
    else if (width == 8)
        launch_one_width<8>(p, blocks, s);
    else if (width == 16)
        launch_one_width<16>(p, blocks, s);
    else
        launch_one_width<64>(p, blocks, s);
}

// One's group kernel over the reads p.only[0 .. *p.only_n): what the lane-per-chunk pass could not stitch
int launch_one_list(const PassParams &p, hipStream_t s)
{
    const uint32_t blocks = 128; // 4096 eight-lane groups; the list is a few reads, and the grid loops over it
    dispatch_k(p.k, [&](auto K) { one_kernel<8, decltype(K)::value, true><<<blocks, 256, 0, s>>>(p); });
    BRX_HIP(hipGetLastError());
    return BRX_OK;
}

} // namespace brx
