// The correction chain, host side: the chain object, the attempt loop that runs each method's passes as planned
// (brx_plan.hpp) through the kernel families -- brx_group.hip (correct_kernel), brx_one.hip (one_kernel),
// brx_revscan.hip (rev_scan_kernel), brx_onelane.hip (lane per chunk) --, the redo of poisoned reads, the compaction of
// the staged result, and the host-batch and async entries.
#include "brx_correct.hpp"
#include <chrono>

#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <thread>
#include <vector>

using namespace brx;

namespace {

// one workgroup per read (grid-stride): staged slot -> compact output, reversing if needed
__global__ __launch_bounds__(256) void compact_kernel(const uint8_t *__restrict__ stage, const uint32_t *__restrict__ lens,
                                                      const uint64_t *__restrict__ offsets, uint32_t n_reads,
                                                      uint32_t slack, int reversed, const uint64_t *__restrict__ out_offsets,
                                                      uint8_t *__restrict__ out)
{
    for (uint32_t r = blockIdx.x; r < n_reads; r += gridDim.x) {
        const uint64_t s0 = slot_of(offsets[r], r, slack);
        const uint8_t *src = stage + s0;
        uint32_t n = lens[r];
        {   // a read redone outside the batch that does not fit its slot has its length here but its bytes elsewhere (they
            // are copied over this read's place afterwards): copy no more than the slot holds
            const uint64_t slot = slot_of(offsets[r + 1], (uint64_t)r + 1, slack) - s0;
            if ((uint64_t)n > slot)
                n = (uint32_t)slot;
        }
        uint8_t *dst = out + out_offsets[r];
        // bytes up to the first 16-byte boundary of dst, then 16 bytes per lane (unaligned load, byte order reversed
        // in registers when the staged read is stored back to front, aligned store), then the tail
        uint32_t head = (uint32_t)((16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u);
        if (head > n)
            head = n;
        const uint32_t nv = (n - head) / 16u;
        for (uint32_t j = threadIdx.x; j < head; j += blockDim.x)
            dst[j] = reversed ? src[n - 1u - j] : src[j];
        for (uint32_t v = threadIdx.x; v < nv; v += blockDim.x) {
            const uint32_t j = head + 16u * v;
            uint4 q;
            if (reversed) {
                __builtin_memcpy(&q, src + (n - 16u - j), 16);
                q = make_uint4(__builtin_bswap32(q.w), __builtin_bswap32(q.z), __builtin_bswap32(q.y), __builtin_bswap32(q.x));
            } else {
                __builtin_memcpy(&q, src + j, 16);
            }
            *reinterpret_cast<uint4 *>(dst + j) = q;
        }
        for (uint32_t j = head + 16u * nv + threadIdx.x; j < n; j += blockDim.x)
            dst[j] = reversed ? src[n - 1u - j] : src[j];
    }
}

} // namespace

extern "C" {

int brx_chain_new(const brx_set_t *set, const brx_method_t *methods, uint32_t n_methods, bool two_side,
                  brx_chain_t **out)
{
    return brx_chain_new_pass(set, methods, n_methods, two_side ? BRX_PASS_NONE : BRX_PASS_REVERSE, out);
}

int brx_chain_second_pass(const brx_chain_t *ch)
{
    if (!ch) {
        set_error("null argument");
        return BRX_ERR_ARG;
    }
    return ch->second_pass;
}

int brx_chain_new_pass(const brx_set_t *set, const brx_method_t *methods, uint32_t n_methods, int second_pass,
                       brx_chain_t **out)
{
    return chain_new(set, methods, n_methods, second_pass, read_correct_tuning(), out);
}

} // extern "C"

int brx::chain_new(const brx_set_t *set, const brx_method_t *methods, uint32_t n_methods, int second_pass, const CorrectTuning &tuning,
                   brx_chain_t **out)
{
    if (!set || !out || (!methods && n_methods)) {
        set_error("null argument");
        return BRX_ERR_ARG;
    }
    if (second_pass != BRX_PASS_NONE && second_pass != BRX_PASS_REVERSE && second_pass != BRX_PASS_REVCOMP) {
        set_error("unknown second-pass mode %d (0 none, 1 reverse, 2 revcomp)", second_pass);
        return BRX_ERR_ARG;
    }
    for (uint32_t m = 0; m < n_methods; m++)
        if (methods[m].method > BRX_GAP_SIZE) {
            set_error("unknown correction method %u", methods[m].method);
            return BRX_ERR_ARG;
        }
    BRX_TRY(use_device(set->device));
    brx_chain *ch = new brx_chain();
    ch->set = set;
    ch->device = set->device;
    ch->methods.assign(methods, methods + n_methods);
    ch->two_side = second_pass == BRX_PASS_NONE;
    ch->second_pass = second_pass;
    if (tuning.maxpath) // (BRX_MAXPATH)
        ch->maxpath_seen = tuning.maxpath;
    hipError_t e = hipStreamCreateWithFlags(&ch->stream, hipStreamNonBlocking);
    if (e == hipSuccess)
        e = ch->d_ctrl.reserve(CTL_N, 0, "chain control block") == BRX_OK ? hipSuccess : hipErrorOutOfMemory;
    if (e == hipSuccess)
        e = hipHostMalloc((void **)&ch->h_ctrl, CTL_N * 8, hipHostMallocDefault);
    if (e != hipSuccess) {
        set_error("chain alloc: %s", hipGetErrorString(e));
        brx_chain_free(ch);
        return BRX_ERR_HIP;
    }
    *out = ch;
    return BRX_OK;
}

extern "C" {

// A handful of reads that outgrew their workspace -- a graph walk longer than the visited list (GapSize at BASELINE
// configs[4]'s per-GPU share: 18 of 625 000) or a correction that grows the read beyond its output slot -- should not
// cost the whole batch a second run.  Everything else of the batch is final and sits in its own slot of the last
// staging buffer, so the poisoned reads are taken out as a small batch of their own and corrected by a second chain
// with a longer list / more slack (same set, methods and direction rule; all on the GPU).  A redone read that fits its
// slot is written back into it; one that does not goes to `side` and is copied over its place in the compact output
// after the compaction (its final length is entered in `lens`, so every other read lands where it should).
// BRX_OK: lens / slots patched, the batch is complete.  BRX_ERR_UNSUPPORTED: not applicable (too many reads) -- the
// caller redoes the whole batch with a larger workspace as before.
struct SideRead {
    uint32_t r;
    std::vector<uint8_t> bytes;
};
static int correct_batch_host(brx_chain_t *ch, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads, const CorrectTuning &tuning,
                              uint8_t **out_bases, uint64_t **out_offsets);
static int redo_poisoned_reads(brx_chain *ch, const CorrectTuning &tuning, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads,
                               uint8_t *d_stage, uint32_t *d_lens, int stage_reversed, uint32_t slack, uint32_t sub_slack,
                               uint32_t maxpath, std::vector<SideRead> &side, hipStream_t s)
{
    if (ch->is_sub)
        return BRX_ERR_UNSUPPORTED;
    std::vector<uint32_t> lens(n_reads);
    std::vector<uint64_t> offs((size_t)n_reads + 1);
    BRX_HIP(hipMemcpyAsync(lens.data(), d_lens, (size_t)n_reads * 4, hipMemcpyDeviceToHost, s));
    BRX_HIP(hipMemcpyAsync(offs.data(), d_offsets, ((size_t)n_reads + 1) * 8, hipMemcpyDeviceToHost, s));
    BRX_HIP(hipStreamSynchronize(s));
    std::vector<uint32_t> ids;
    for (uint32_t r = 0; r < n_reads; r++)
        if (lens[r] == 0xffffffffu) {
            if (ids.size() >= tuning.redo_max)
                return BRX_ERR_UNSUPPORTED;
            ids.push_back(r);
        }
    if (ids.empty())
        return BRX_ERR_UNSUPPORTED;
    std::vector<uint64_t> moff(ids.size() + 1, 0);
    for (size_t j = 0; j < ids.size(); j++)
        moff[j + 1] = moff[j] + (offs[ids[j] + 1] - offs[ids[j]]);
    std::vector<uint8_t> mb(moff.back() ? moff.back() : 1);
    for (size_t j = 0; j < ids.size(); j++)
        if (moff[j + 1] > moff[j])
            BRX_HIP(hipMemcpyAsync(mb.data() + moff[j], d_bases + offs[ids[j]], moff[j + 1] - moff[j], hipMemcpyDeviceToHost, s));
    BRX_HIP(hipStreamSynchronize(s));
    if (!ch->sub) {
        brx_chain *sub = nullptr;
        BRX_TRY(chain_new(ch->set, ch->methods.data(), (uint32_t)ch->methods.size(), ch->second_pass, tuning, &sub));
        sub->is_sub = true;
        ch->sub = sub;
    }
    if (ch->sub->maxpath_seen < maxpath)
        ch->sub->maxpath_seen = maxpath;
    if (ch->sub->slack_seen < sub_slack)
        ch->sub->slack_seen = sub_slack;
    uint8_t *ob = nullptr;
    uint64_t *oo = nullptr;
    BRX_TRY(correct_batch_host(ch->sub, mb.data(), moff.data(), (uint32_t)ids.size(), tuning, &ob, &oo)); // (the parent batch's switches)
    int st = BRX_OK;
    std::vector<uint8_t> rev;
    for (size_t j = 0; j < ids.size() && st == BRX_OK; j++) {
        const uint32_t r = ids[j];
        const uint64_t s0 = slot_of(offs[r], r, slack), s1 = slot_of(offs[r + 1], (uint64_t)r + 1, slack);
        const uint64_t len = oo[j + 1] - oo[j];
        if (len >= 0xffffffffull) {
            st = BRX_ERR_UNSUPPORTED;
            break;
        }
        const uint8_t *src = ob + oo[j];
        if (len + 1 > s1 - s0) {
            // does not fit its slot: keep the bytes aside (forward order), enter the length, patch after compaction
            side.push_back(SideRead{r, std::vector<uint8_t>(src, src + len)});
            const uint32_t l32s = (uint32_t)len;
            if (hipMemcpy(d_lens + r, &l32s, 4, hipMemcpyHostToDevice) != hipSuccess) {
                set_error("redo of poisoned reads: length patch failed");
                st = BRX_ERR_HIP;
            }
            continue;
        }
        if (ch->second_pass == BRX_PASS_REVCOMP) { // the stage holds the second scan's reads: the other strand
            rev.assign(src, src + len);
            revcomp_host(rev.data(), rev.size());
            src = rev.data();
        } else if (stage_reversed) { // the last pass stored its reads back to front
            rev.assign(src, src + len);
            std::reverse(rev.begin(), rev.end());
            src = rev.data();
        }
        const uint32_t l32 = (uint32_t)len;
        hipError_t e = len ? hipMemcpy(d_stage + s0, src, len, hipMemcpyHostToDevice) : hipSuccess;
        if (e == hipSuccess)
            e = hipMemcpy(d_lens + r, &l32, 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            set_error("redo of poisoned reads: %s", hipGetErrorString(e));
            st = BRX_ERR_HIP;
        }
    }
    brx_buf_free(ob);
    brx_buf_free(oo);
    return st;
}

// the batch entry proper; the caller holds ch->mu (a chain owns ONE workspace: staging buffers, control block, visited
// lists -- two batches at once on one chain would share them)
static int correct_batch_device_locked(brx_chain_t *ch, const CorrectTuning &tuning, const uint8_t *d_bases, const uint64_t *d_offsets,
                                       uint32_t n_reads, uint64_t total_bases, uint8_t *d_out, uint64_t out_cap,
                                       uint64_t *d_out_offsets, uint64_t *out_total, void *stream)
{
    hipStream_t s = (hipStream_t)stream; // nullptr = the legacy default stream
    *out_total = 0;
    if (n_reads == 0) {
        BRX_HIP(hipMemsetAsync(d_out_offsets, 0, 8, s));
        BRX_HIP(hipStreamSynchronize(s));
        return BRX_OK;
    }
    const int k = ch->set->k;
    if ((k & 1) == 0) {
        set_error("correction needs an odd k (parity-canonical set), got %d", k);
        return BRX_ERR_ARG;
    }

    // (lens, scan scratch) do not depend on slack
    {
        for (int q = 0; q < 2; q++)
            BRX_TRY(ch->d_lens[q].reserve(n_reads, n_reads / 8 + 64, "read lengths"));
        const uint64_t tmp_bytes = scan_tmp_bytes(n_reads);
        BRX_TRY(ch->d_scan_tmp.reserve_bytes(tmp_bytes, ws_headroom(tmp_bytes), "workspace"));
    }

    // walks (Two/Graph/Greedy/GapSize forward passes) are faster on the bit vector: materialise a lazy one now
    if (ch->set->bits_stale && !ch->set->sparse)
        for (const brx_method_t &md : ch->methods)
            if (md.method != BRX_ONE) {
                BRX_TRY(ensure_bits(ch->set, s, "correction"));
                break;
            }
    // probe index of the set (built here when the set has none yet, e.g. after a finish_into)
    BRX_TRY(index_ensure(ch->set, s));
    const IdxView idx = set_view(ch->set, tuning.line_bits).idx;
    SetFacts facts;
    facts.k = k;
    facts.has_bits = !no_bits(ch->set);
    facts.has_idx = idx.lines != nullptr;
    facts.idx_log_lines = idx.lines ? 32u - idx.line_shift : 0u;
    facts.idx_m = idx.m;
    facts.idx_w = idx.w;
    facts.has_line_bits = idx.line_bits != nullptr;

    const int n_dirs = ch->two_side ? 1 : 2;
    // BRX_PASS_REVCOMP: the second scan runs over the reverse complement of the first scan's output, materialised in the
    // other staging buffer.  It meets as many solid k-mers as the first, so it IS a forward pass in every respect
    // (lane automata, group widths, index rule) and only the byte map around it differs.
    const bool revcomp = ch->second_pass == BRX_PASS_REVCOMP;
    const int n_methods = (int)ch->methods.size();
    uint64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<SideRead> side; // redone reads that do not fit their staging slot (redo_poisoned_reads)
    bool needs_path = false;
    for (int m = 0; m < n_methods; m++)
        needs_path |= (ch->methods[m].method == BRX_GRAPH || ch->methods[m].method == BRX_GAP_SIZE ||
                       ch->methods[m].method == BRX_GREEDY);
    uint32_t maxpath = ch->maxpath_seen; // visited-list capacity per group (4096: 1 GiB of scratch at 32768 groups); grows x8 on overflow

    for (uint32_t slack = ch->slack_seen, attempt = 0;; attempt++) {
        if (attempt > 12) {
            set_error("correction output / graph walks do not fit the workspace after 12 enlargements; giving up");
            return BRX_ERR_OVERFLOW;
        }
        // (at least one block of the narrowest list / verify kernel); every list and verify grid of the attempt is cut from it
        const uint64_t path_lists = sized_path_lists(tuning, n_reads);
        if (needs_path) {
            // one visited list per group that can be resident: walking methods run BRX_GROUP_WALK-lane groups or wider, so
            // a grid of pass_blocks blocks of such groups bounds every width (a handful of redone reads needs a handful of
            // lists, not 32768 of them)
            const uint64_t path_bytes = path_lists * maxpath * 8ull;
            BRX_TRY(ch->d_path.reserve_bytes(path_bytes, ws_headroom(path_bytes), "workspace"));
        }
        const uint64_t stage_need = total_bases + (total_bases >> 2) * slack + 64ull * ((uint64_t)n_reads + 1) + 64;
        for (int q = 0; q < 2; q++)
            BRX_TRY(ch->d_stage[q].reserve(stage_need, 0, "staging"));

        // the chain: src/lib.rs:44-55.  buffer "rev" = stored back to front w.r.t. the original read
        const uint8_t *cur = d_bases;
        const uint32_t *cur_lens = nullptr;
        int cur_staged = 0, cur_rev = 0, pp = 0;
        bool any_overflow = false;
        BRX_HIP(hipMemsetAsync(ch->d_ctrl, 0, CTL_N * 8, s));
        for (int scan = 0; scan < n_dirs && !any_overflow; scan++) {
            const int dir = revcomp ? 0 : scan; // 1: a scan of the reads back to front (tuned for absent k-mers)
            if (revcomp && scan == 1 && cur_staged) { // (an empty method list leaves nothing staged: rejected below)
                revcomp_stage(cur, cur_lens, d_offsets, n_reads, slack, ch->d_stage[pp], ch->d_lens[pp], s);
                cur = ch->d_stage[pp];
                cur_lens = ch->d_lens[pp];
                pp ^= 1;
            }
            for (int m = 0; m < n_methods; m++) {
                const brx_method_t &md = ch->methods[m];
                const uint64_t in_total_bound = cur_staged ? ch->d_stage[0].bytes() : total_bases;
                const PassPlan plan = plan_pass(tuning, facts, md.method, md.confirm, md.max_search, dir, revcomp, cur_rev != dir, n_reads,
                                                in_total_bound);
                PassParams p;
                p.bits = facts.has_bits ? ch->set->d_bits.get() : nullptr;
                p.idx = plan.use_idx ? idx : IdxView{nullptr, 0, 0, 0};
                p.k = k;
                p.c = md.confirm;
                p.n_reads = n_reads;
                p.offsets = d_offsets;
                p.in = cur;
                p.in_lens = cur_lens;
                p.in_staged = cur_staged;
                p.flip = (cur_rev != dir);
                p.out = ch->d_stage[pp];
                p.out_lens = ch->d_lens[pp];
                p.slack = slack;
                p.ctrl = (unsigned long long *)ch->d_ctrl.get();
                p.path_k = ch->d_path;
                p.maxpath = maxpath;
                BRX_HIP(hipMemsetAsync(ch->d_ctrl + CTL_WORK, 0, 8, s));
                p.flags = 0; // (BRX_TUNE and max_search: set by the group launches, for their kernels alone)
                p.rev_batch = plan.rev_batch ? 1 : 0;
                p.max_search = 0;
                p.g_dim = 0;
                p.g_lds_bytes = 0;
                switch (plan.form) {
                case PASS_LANE: BRX_TRY(lane_pass(ch, p, plan, LanePassInfo{in_total_bound, md.method, path_lists}, s)); break;
                case PASS_REV_LEAN: BRX_TRY(launch_rev_lean(ch, p, plan, md, path_lists, s)); break;
                case PASS_GROUP: BRX_TRY(launch_group(p, plan, md, plan.blocks, pass_timer_name(md.method), s)); break;
                case PASS_NO_LDS:
                    set_error("greedy: k=%d with max_search=%d needs a %u x %u alignment table that does not fit LDS", k, (int)md.max_search,
                              plan.g_dim, plan.g_dim);
                    return BRX_ERR_UNSUPPORTED;
                }
                cur = ch->d_stage[pp];
                cur_lens = ch->d_lens[pp];
                cur_staged = 1;
                cur_rev = dir;
                pp ^= 1;
            }
        }
        if (n_methods == 0) {
            // no corrector: identity (a reverse of a reverse).  Copy through one staged pass-less path.
            set_error("empty method list");
            return BRX_ERR_ARG;
        }
        static const bool tr_attempts = [] { const char *e = getenv("BRX_TRACE"); return e && *e == '1'; }();
        if (tr_attempts)
            fprintf(stderr, "[brx correct] attempt %u launched: slack %u maxpath %u n_reads %u\n", attempt, slack, maxpath, n_reads);
        BRX_HIP(hipMemcpyAsync(ch->h_ctrl, ch->d_ctrl, CTL_N * 8, hipMemcpyDeviceToHost, s));
        BRX_HIP(hipStreamSynchronize(s));
        if (tr_attempts)
            fprintf(stderr, "[brx correct] attempt %u done: slot overflows %llu, walk list overflows %llu, nonterminating %llu, "
                            "lean reverse passes: %llu open triggers verified, %llu reads redone\n", attempt,
                    (unsigned long long)ch->h_ctrl[CTL_OVERFLOW], (unsigned long long)ch->h_ctrl[CTL_PATHOVF],
                    (unsigned long long)ch->h_ctrl[CTL_NONTERM], (unsigned long long)ch->h_ctrl[CTL_REV_TRIGS_SUM],
                    (unsigned long long)ch->h_ctrl[CTL_REV_HANDBACK_SUM]);
        stats[4] = attempt;
        if (ch->h_ctrl[CTL_NONTERM] != 0) {
            set_error("%llu read(s): the scan does not terminate (e.g. greedy moving the read cursor backwards for ever; "
                      "the reference spins on such input)", (unsigned long long)ch->h_ctrl[CTL_NONTERM]);
            return BRX_ERR_UNSUPPORTED;
        }
        if (ch->h_ctrl[CTL_OVERFLOW] != 0 || ch->h_ctrl[CTL_PATHOVF] != 0) {
            // some read outgrew its output slot / a graph walk outgrew its visited list: redo the
            // batch on the GPU with a larger workspace (never on the CPU)
            stats[5] += ch->h_ctrl[CTL_OVERFLOW]; // reads that outgrew their slot / walks that outgrew the list,
            stats[6] += ch->h_ctrl[CTL_PATHOVF];  // summed over the attempts that were thrown away or patched
            bool patched = false;
            if (ch->h_ctrl[CTL_OVERFLOW] + ch->h_ctrl[CTL_PATHOVF] <= tuning.redo_max) {
                side.clear();
                const int rst = redo_poisoned_reads(ch, tuning, d_bases, d_offsets, n_reads, const_cast<uint8_t *>(cur),
                                                    const_cast<uint32_t *>(cur_lens), cur_rev, slack,
                                                    ch->h_ctrl[CTL_OVERFLOW] ? slack * 4u : slack,
                                                    ch->h_ctrl[CTL_PATHOVF] ? maxpath * 8u : maxpath, side, s);
                if (rst == BRX_OK) {
                    // the few long walks were redone by the sub chain with its own longer list; this chain keeps its
                    // list size (growing it x8 for every group of the grid is 8 GiB per chain after one event)
                    patched = true;
                    if (ch->sub) // events of the redone reads, which the first attempt gave up on
                        for (int q = 0; q < 4; q++)
                            stats[q] += ch->sub->last_stats[q];
                }
                else if (rst != BRX_ERR_UNSUPPORTED)
                    return rst;
            }
            if (!patched) {
                side.clear();
                if (ch->h_ctrl[CTL_OVERFLOW] != 0)
                    slack *= 4;
                if (ch->h_ctrl[CTL_PATHOVF] != 0)
                    maxpath *= 8;
                ch->slack_seen = slack;
                ch->maxpath_seen = maxpath;
                continue;
            }
        }
        {
            const uint64_t unw = ch->h_ctrl[CTL_LANE_UNWRITTEN] + (ch->sub ? ch->sub->last_stats[7] >> 56 : 0);
            stats[7] = (ch->h_ctrl[CTL_LANE_UNITS] & 0xffffffffull) | ((ch->h_ctrl[CTL_LANE_FAIL] & 0xffffffull) << 32) |
                       ((unw > 255 ? 255ull : unw) << 56);
            if (unw) // an invariant of the lane form is broken (the output is still right: those reads went to the group kernel)
                fprintf(stderr, "[brx correct] WARNING: %llu unit record(s) were never written by the lane pass\n", (unsigned long long)unw);
        }
#ifdef BRX_AP_COUNT
        fprintf(stderr, "[brx correct] replay chunks with fixes: %llu vector, %llu byte way, %llu partial\n", (unsigned long long)ch->h_ctrl[CTL_AP_VEC],
                (unsigned long long)ch->h_ctrl[CTL_AP_BYTEWAY], (unsigned long long)ch->h_ctrl[CTL_AP_PARTIAL]);
#endif
        stats[0] += ch->h_ctrl[CTL_ROUNDS];
        stats[1] += ch->h_ctrl[CTL_PROBES];
        stats[2] += ch->h_ctrl[CTL_TRIGGERS];
        stats[3] += ch->h_ctrl[CTL_FIXES];

        // out_offsets = exclusive scan of final lengths
        BRX_TRY(exclusive_scan_lens(cur_lens, n_reads, ch->d_scan_tmp, d_out_offsets,
                                    (unsigned long long *)(ch->d_ctrl + CTL_TOTAL), s));
        BRX_HIP(hipMemcpyAsync(ch->h_ctrl, ch->d_ctrl, CTL_N * 8, hipMemcpyDeviceToHost, s));
        BRX_HIP(hipStreamSynchronize(s));
        const uint64_t total = ch->h_ctrl[CTL_TOTAL];
        *out_total = total;
        memcpy(ch->last_stats, stats, sizeof(stats));
        if (total > out_cap) {
            set_error("corrected batch needs %llu bytes, output buffer has %llu", (unsigned long long)total,
                      (unsigned long long)out_cap);
            return BRX_ERR_OVERFLOW;
        }
        if (revcomp) {
            revcomp_compact(cur, cur_lens, d_offsets, n_reads, slack, d_out_offsets, d_out, s);
        } else {
            KernelTimer t("compact", s);
            const uint32_t grid = read_grid(n_reads, 1u << 20);
            compact_kernel<<<grid, 256, 0, s>>>(cur, cur_lens, d_offsets, n_reads, slack, cur_rev, d_out_offsets, d_out);
        }
        BRX_HIP(hipStreamSynchronize(s));
        for (const SideRead &sr : side) { // the few reads that outgrew their slot: their bytes go straight to their place
            uint64_t at = 0;
            BRX_HIP(hipMemcpy(&at, d_out_offsets + sr.r, 8, hipMemcpyDeviceToHost));
            if (!sr.bytes.empty())
                BRX_HIP(hipMemcpy(d_out + at, sr.bytes.data(), sr.bytes.size(), hipMemcpyHostToDevice));
        }
        return BRX_OK;
    }
}

int brx_chain_correct_batch_device(brx_chain_t *ch, const uint8_t *d_bases, const uint64_t *d_offsets,
                                   uint32_t n_reads, uint64_t total_bases, uint8_t *d_out, uint64_t out_cap,
                                   uint64_t *d_out_offsets, uint64_t *out_total, void *stream)
{
    return chain_correct_batch_device(ch, read_correct_tuning(), d_bases, d_offsets, n_reads, total_bases, d_out, out_cap, d_out_offsets,
                                      out_total, stream);
}

} // extern "C"

int brx::chain_correct_batch_device(brx_chain_t *ch, const CorrectTuning &tuning, const uint8_t *d_bases, const uint64_t *d_offsets,
                                    uint32_t n_reads, uint64_t total_bases, uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_offsets,
                                    uint64_t *out_total, void *stream)
{
    if (!ch || !d_offsets || !d_out_offsets || !out_total || (!d_bases && total_bases) || (!d_out && out_cap)) {
        set_error("null argument");
        return BRX_ERR_ARG;
    }
    BRX_TRY(use_device(ch->device));
    std::lock_guard<std::mutex> g(ch->mu);
    return correct_batch_device_locked(ch, tuning, d_bases, d_offsets, n_reads, total_bases, d_out, out_cap, d_out_offsets, out_total,
                                       stream);
}

extern "C" {

int brx_chain_correct_batch(brx_chain_t *ch, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                            uint8_t **out_bases, uint64_t **out_offsets)
{
    return correct_batch_host(ch, bases, offsets, n_reads, read_correct_tuning(), out_bases, out_offsets);
}

// a batch from host memory under the switches in `tuning` (read by the entry, on the caller's thread)
static int correct_batch_host(brx_chain_t *ch, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads, const CorrectTuning &tuning,
                              uint8_t **out_bases, uint64_t **out_offsets)
{
    if (!ch || !offsets || !out_bases || !out_offsets || (!bases && n_reads)) {
        set_error("null argument");
        return BRX_ERR_ARG;
    }
    *out_bases = nullptr;
    *out_offsets = nullptr;
    BRX_TRY(use_device(ch->device));
    // BRX_TRACE=2: host wall time of the call's stages on stderr (where a batch from host memory spends its time)
    static const bool tr_host = [] { const char *e = getenv("BRX_TRACE"); return e && *e == '2'; }();
    const auto t_in = std::chrono::steady_clock::now();
    auto ms_since = [&](std::chrono::steady_clock::time_point t0) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    };
    // ONE lock from the upload to the download: the chain's own d_in / d_off / d_out staging is part of the workspace
    // a concurrent call on the same chain would overwrite (include/brx.h: "a chain serialises concurrent calls")
    std::lock_guard<std::mutex> g(ch->mu);
    uint64_t total = 0;
    {
        // The batch goes up at PCIe speed only from page-locked memory.  A caller that filled a brx_host_alloc buffer is
        // copied from directly; anything else is first moved into the chain's own page-locked block by four threads
        // (the runtime's built-in staging of pageable memory managed 6-10 GB/s: 8-13 ms of a 82 MB batch).
        const uint64_t base0 = offsets[0], tot = offsets[n_reads] - base0;
        const uint8_t *src = bases + base0;
        if (tot >= (4u << 20) && !host_buf_is_pinned(src)) {
            if (ch->h_in_cap < tot) {
                host_buf_release(ch->h_in);
                ch->h_in = (uint8_t *)host_buf_acquire(tot + tot / 8);
                ch->h_in_cap = ch->h_in ? tot + tot / 8 : 0;
            }
            if (ch->h_in) {
                const int nt = 4;
                std::vector<std::thread> th;
                for (int t = 1; t < nt; t++)
                    th.emplace_back([&, t] { memcpy(ch->h_in + tot * t / nt, src + tot * t / nt, tot * (t + 1) / nt - tot * t / nt); });
                memcpy(ch->h_in, src, tot / nt);
                for (auto &x : th)
                    x.join();
                src = ch->h_in;
            }
        }
        // (upload_batch takes `bases` as the start of the stream offsets[] index into)
        BRX_TRY(upload_batch(src - base0, offsets, n_reads, ch->d_in, ch->d_off, &total, ch->stream));
    }
    const uint64_t off_bytes = ((uint64_t)n_reads + 1) * 8;
    BRX_TRY(ch->d_out_off.reserve_bytes(off_bytes, ws_headroom(off_bytes), "workspace"));
    const double t_up = ms_since(t_in);
    uint64_t out_total = 0;
    uint64_t want = total + total / 16 + 4096;
    for (int attempt = 0; attempt < 3; attempt++) {
        BRX_TRY(ch->d_out.reserve(want, ws_headroom(want), "workspace"));
        int st = correct_batch_device_locked(ch, tuning, ch->d_in, ch->d_off, n_reads, total, ch->d_out, ch->d_out.cap(), ch->d_out_off,
                                             &out_total, ch->stream);
        if (st == BRX_ERR_OVERFLOW && out_total > ch->d_out.cap()) {
            want = out_total + 64;
            continue;
        }
        if (st != BRX_OK)
            return st;
        break;
    }
    const double t_dev = ms_since(t_in);
    // the corrected batch comes back into pooled page-locked blocks (released by brx_buf_free like any other)
    uint8_t *hb = (uint8_t *)host_buf_acquire(out_total ? out_total : 1);
    uint64_t *ho = (uint64_t *)host_buf_acquire(((size_t)n_reads + 1) * 8);
    if (!hb || !ho) {
        host_buf_release(hb);
        host_buf_release(ho);
        set_error("host malloc failed");
        return BRX_ERR_NOMEM;
    }
    hipError_t e = hipSuccess;
    if (out_total)
        e = hipMemcpyAsync(hb, ch->d_out, out_total, hipMemcpyDeviceToHost, ch->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(ho, ch->d_out_off, ((size_t)n_reads + 1) * 8, hipMemcpyDeviceToHost, ch->stream);
    if (e == hipSuccess)
        e = hipStreamSynchronize(ch->stream);
    if (e != hipSuccess) {
        host_buf_release(hb);
        host_buf_release(ho);
        set_error("D2H: %s", hipGetErrorString(e));
        return BRX_ERR_HIP;
    }
    *out_bases = hb;
    *out_offsets = ho;
    if (tr_host)
        fprintf(stderr, "[brx batch %p] %u reads %llu bases: upload %.2f ms, passes %.2f, download %.2f (at %.2f ms of the clock)\n", (void *)ch,
                n_reads, (unsigned long long)total, t_up, t_dev - t_up, ms_since(t_in) - t_dev,
                std::chrono::duration<double, std::milli>(t_in.time_since_epoch()).count());
    return BRX_OK;
}

// ---- one batch in flight per chain -----------------------------------------------------------------------------------
// brx_chain_correct_batch is upload -> passes -> download, back to back on one stream: 82 MB up, ~3 ms of kernels,
// 82 MB down per 8192-record batch, nothing overlapping (9 Gbases/s from page-locked memory against 36 for the passes
// alone).  The overlap a host needs is BETWEEN batches -- the next one's upload under this one's kernels under the last
// one's download -- and chains are the unit that owns a stream and a workspace.  So the asynchronous form is per chain:
// _async starts the batch on a thread of the library and returns, _wait hands out its result; a host keeps two or three
// chains of the same set busy in turn from ONE thread (INTEGRATION.md has the loop run_correction would use).
namespace {
struct AsyncJob {
    std::thread th;
    int status = BRX_OK;
    uint8_t *ob = nullptr;
    uint64_t *oo = nullptr;
    std::string err;
};
} // namespace

int brx_chain_correct_batch_async(brx_chain_t *ch, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads)
{
    if (!ch || !offsets || (!bases && n_reads)) {
        set_error("null argument");
        return BRX_ERR_ARG;
    }
    if (ch->async_job) {
        set_error("chain already has a batch in flight: brx_chain_correct_batch_wait first (one per chain; use several chains)");
        return BRX_ERR_ARG;
    }
    AsyncJob *job = new AsyncJob();
    ch->async_job = job;
    // (the switches are read here, on the caller's thread: the library's thread does not read them from the environment)
    job->th = std::thread([ch, job, bases, offsets, n_reads, tuning = read_correct_tuning()] {
        job->status = correct_batch_host(ch, bases, offsets, n_reads, tuning, &job->ob, &job->oo);
        if (job->status != BRX_OK)
            job->err = brx_last_error(); // (the message lives in this thread: carried over to the waiter)
    });
    return BRX_OK;
}

int brx_chain_correct_batch_wait(brx_chain_t *ch, uint8_t **out_bases, uint64_t **out_offsets)
{
    if (!ch || !out_bases || !out_offsets) {
        set_error("null argument");
        return BRX_ERR_ARG;
    }
    *out_bases = nullptr;
    *out_offsets = nullptr;
    AsyncJob *job = (AsyncJob *)ch->async_job;
    if (!job) {
        set_error("no batch in flight on this chain");
        return BRX_ERR_ARG;
    }
    job->th.join();
    ch->async_job = nullptr;
    const int st = job->status;
    if (st == BRX_OK) {
        *out_bases = job->ob;
        *out_offsets = job->oo;
    } else {
        set_error("%s", job->err.c_str());
    }
    delete job;
    return st;
}

int brx_chain_last_stats(const brx_chain_t *ch, uint64_t *stats8)
{
    if (!ch || !stats8)
        return BRX_ERR_ARG;
    memcpy(stats8, ch->last_stats, sizeof(ch->last_stats));
    return BRX_OK;
}

void brx_chain_free(brx_chain_t *ch)
{
    if (!ch)
        return;
    if (ch->async_job) { // a batch still in flight: let it finish, drop its result
        uint8_t *ob = nullptr;
        uint64_t *oo = nullptr;
        (void)brx_chain_correct_batch_wait(ch, &ob, &oo);
        brx_buf_free(ob);
        brx_buf_free(oo);
    }
    if (ch->sub)
        brx_chain_free(ch->sub);
    ch->sub = nullptr;
    host_buf_release(ch->h_in);
    ch->h_in = nullptr;
    if (use_device(ch->device) == BRX_OK) {
        if (ch->h_ctrl)
            (void)hipHostFree(ch->h_ctrl);
        if (ch->stream)
            (void)hipStreamDestroy(ch->stream);
    }
    lane_ws_free(ch);
    delete ch; // its device buffers go back to the pool here, with the chain's device current
}

} // extern "C"
