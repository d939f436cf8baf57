// Stand-alone host program over br_amd/csrc/brx_plan.hpp: reads the correction switches from its environment as the
// library does (read_correct_tuning) and prints what plan_pass and the grid rules make of the cases on its command
// line, one line per case.  Built and run by test_pass_plan_cpu.py with -fsanitize=address,undefined; the expected lines
// are written out there.
//
//   tuning                      the record itself
//   blocks:N,G                  pass_blocks(N reads, G lanes)
//   lists:N                     sized_path_lists(N reads) and the grids cut from them
//   pass:K,BITS,LOG,W,OCC,METHOD,CONFIRM,MAX_SEARCH,DIR,REVCOMP,FLIP,N_READS,IN_TOTAL
//                               plan_pass for a set of this k (BITS: bit vector present; LOG: log2 of the index's lines,
//                               0 = no index; W: its windows; OCC: occupancy bits present)
#include "../br_amd/csrc/brx_plan.hpp"

#include <stdio.h>
#include <string.h>

using namespace brx;

static const char *const METHODS[5] = {"one", "two", "graph", "greedy", "gap_size"};

static int print_pass(const CorrectTuning &t, const char *spec)
{
    unsigned long long v[13];
    if (sscanf(spec, "%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu,%llu", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8, v + 9,
               v + 10, v + 11, v + 12) != 13 || v[5] > 4)
        return 1;
    SetFacts f;
    f.k = (int)v[0];
    f.has_bits = v[1] != 0;
    f.has_idx = v[2] != 0;
    f.idx_log_lines = (uint32_t)v[2];
    f.idx_w = (uint32_t)v[3];
    f.idx_m = f.has_idx ? (uint32_t)f.k - f.idx_w + 1u : 0u;
    f.has_line_bits = v[4] != 0;
    const int method = (int)v[5], dir = (int)v[8];
    const PassPlan pl = plan_pass(t, f, method, (int)v[6], (int)v[7], dir, v[9] != 0, v[10] != 0, (uint32_t)v[11], v[12]);
    printf("%s dir%d ", METHODS[method], dir);
    switch (pl.form) {
    case PASS_LANE:
        printf("LANE idx=%d mask=%d succ=%d chunk=%u sync=%u tail=%u/%u units<=%llu ap_grid=%u\n", pl.use_idx, pl.use_mask, pl.use_succ, pl.chunk, pl.sync,
               pl.r_half, pl.r_quarter, (unsigned long long)pl.units_bound, pl.ap_grid);
        break;
    case PASS_GROUP:
        printf("GROUP %s width=%d idx=%d rev_batch=%d blocks=%u lds=%u/%u tune=%u\n", pl.one_kernel ? "one_kernel" : "correct_kernel", pl.width, pl.use_idx,
               pl.rev_batch, pl.blocks, pl.g_lds_bytes, pl.lds, pl.flags);
        break;
    case PASS_REV_LEAN:
        printf("REV_LEAN scan=%d verify=%d/%d idx=%d rev_batch=%d blocks=%u\n", pl.width, pl.verify_width, pl.verify_grid_width, pl.use_idx, pl.rev_batch,
               pl.blocks);
        break;
    case PASS_NO_LDS:
        printf("NO_LDS table=%ux%u\n", pl.g_dim, pl.g_dim);
        break;
    }
    return 0;
}

int main(int argc, char **argv)
{
    const CorrectTuning t = read_correct_tuning();
    for (int i = 1; i < argc; i++) {
        const char *a = argv[i];
        unsigned n = 0, g = 0;
        if (!strcmp(a, "tuning")) {
            printf("tuning group=%d/%d group_rev=%d/%d walk=%d verify=%d one_v1=%d balance=%d tune=%u rev_lean=%d rev_batch=%d rev_lean_one=%d "
                   "index_fwd=%u lane_rev=%u line_bits=%d redo_max=%u maxpath=%u lane=%d lane_walk=%d max_log_lines=%u chunk=%u sync=%u tail=%d mask=%u "
                   "succ=%d ap_grid=%u\n",
                   t.group_set, t.group, t.group_rev_set, t.group_rev, t.group_walk, t.rev_verify_g, t.one_v1, t.balance, t.tune, t.rev_lean, t.rev_batch,
                   t.rev_lean_one, t.index_fwd, t.lane_rev, t.line_bits, t.redo_max, t.maxpath, t.lane, t.lane_walk, t.lane_max_log_lines, t.lane_chunk,
                   t.lane_sync, t.lane_tail, t.lane_mask, t.lane_succ, t.ap_grid);
        } else if (sscanf(a, "blocks:%u,%u", &n, &g) == 2 && g >= 1 && g <= 256) {
            printf("blocks reads=%u width=%u plain=%u balanced=%u\n", n, g, pass_blocks(t, n, (int)g), pass_blocks(t, n, (int)g, true));
        } else if (sscanf(a, "lists:%u", &n) == 1) {
            const uint64_t lists = sized_path_lists(t, n); // once; every grid below is cut from it
            printf("lists reads=%u lists=%llu verify_grid=%ux%u redo_grid=%ux4 walk_list_grid=%ux32\n", n, (unsigned long long)lists,
                   list_grid(lists, 256u / (uint32_t)t.rev_verify_g, MAX_BLOCKS), 256u / (uint32_t)t.rev_verify_g, list_grid(lists, 4u, MAX_BLOCKS),
                   list_grid(lists, 32u, 128u));
        } else if (!strncmp(a, "pass:", 5) && print_pass(t, a + 5) == 0) {
        } else {
            fprintf(stderr, "pass_plan_host: cannot read case '%s'\n", a);
            return 2;
        }
    }
    return 0;
}
