#!/usr/bin/env python3
"""The second-pass modes of a chain (include/brx.h BRX_PASS_*, br_amd/strand.py) on bench.py's configs[1] workload: 1e5
synthetic 10 kb reads at 50x, k = 19, abundance 3, the set built from ALL reads, the first --correct reads corrected,
device-resident.  Prints ONE JSON line; for each chain (One; Graph + GapSize) and each mode (none, reverse, revcomp):

  ms_per_gbp         the whole brx_chain_correct_batch_device call by HIP events, best of --repeat after a warm-up
  cover              k-mers / solid k-mers / covered bases / runs of the corrected reads (and of the input, once)
  genome_fraction    the fraction of the reads' k-mers that are k-mers of the synthetic genome: a presence set built
                     from brx_synth_genome_device (cut into overlapping pieces), the cover pass run against it
  kernels            the profile timers of one call

and, once, the rc compaction kernel against compact_kernel(reversed = 1) on the same batch in this process (profile
timers "strand_compact" / "compact" of the One chain in revcomp / reverse mode): both move the same bytes.

    python tools/strand_bench.py [--reads 100000] [--correct 20000] [--repeat 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MODES = ("none", "reverse", "revcomp")
CHAINS = {"one": [("one", 5, 7)], "graph_gap_size": [("graph", 5, 7), ("gap_size", 5, 7)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--correct", type=int, default=20_000)
    ap.add_argument("--read-len", type=int, default=10_000)
    ap.add_argument("--coverage", type=int, default=50)
    ap.add_argument("-k", type=int, default=19)
    ap.add_argument("--abundance", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--chains", default="one,graph_gap_size")
    args = ap.parse_args()

    import numpy as np
    import torch
    import br_amd
    from br_amd import _lib, synth

    dev = 0
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream().cuda_stream
    k, a, n_reads, read_len = args.k, args.abundance, args.reads, args.read_len
    n_corr = min(args.correct, n_reads)
    genome_len = max(n_reads * read_len // args.coverage, read_len)
    cfg = synth.config(genome_len=genome_len, read_len=read_len)
    d_genome = torch.empty(genome_len, dtype=torch.uint8, device="cuda")
    synth.genome_device(cfg, dev, d_genome.data_ptr(), stream)
    cap = int(n_reads * read_len * 1.03) + (1 << 20)
    d_bases = torch.empty(cap, dtype=torch.uint8, device="cuda")
    d_off = torch.empty(n_reads + 1, dtype=torch.int64, device="cuda")
    total_all = synth.reads_device(cfg, dev, d_genome.data_ptr(), 0, n_reads, d_bases.data_ptr(), cap, d_off.data_ptr(), stream)
    counter = br_amd.Counter(k, dev)
    counter.add_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, total_all, stream)
    gs = counter.finish(a, stream)
    del counter

    # the genome's own k-mers (either strand: the set is canonical): pieces that overlap by k - 1 bases, each counted once
    piece = 100_000
    starts = list(range(0, genome_len, piece))
    parts = [d_genome[s:min(s + piece + k - 1, genome_len)] for s in starts]
    g_off = torch.tensor(np.concatenate(([0], np.cumsum([p.numel() for p in parts]))), dtype=torch.int64, device="cuda")
    g_bases = torch.cat(parts)
    counter = br_amd.Counter(k, dev)
    counter.add_batch_device(g_bases.data_ptr(), g_off.data_ptr(), len(parts), g_bases.numel(), stream)
    truth = counter.finish(0, stream)
    torch.cuda.synchronize()
    del counter, parts, g_bases, d_genome

    total = int(d_off[n_corr].item())          # the corrected subset: the first n_corr reads
    gbp = total / 1e9
    d_out = torch.empty(int(total * 1.08) + (1 << 20), dtype=torch.uint8, device="cuda")
    d_out_off = torch.empty(n_corr + 1, dtype=torch.int64, device="cuda")
    d_stats = torch.empty((n_corr, 4), dtype=torch.int32, device="cuda")

    def stats_of(kset, bases, offs, tot):
        kset.cover_batch_device(bases.data_ptr(), offs.data_ptr(), n_corr, tot, None, None, d_stats.data_ptr(), stream)
        torch.cuda.synchronize()
        s = d_stats.cpu().numpy().view(np.uint32).astype(np.int64).sum(axis=0)
        return {"bases": int(tot), "kmers": int(s[0]), "solid": int(s[1]), "covered": int(s[2]), "runs": int(s[3]),
                "solid_fraction": round(float(s[1]) / max(int(s[0]), 1), 5), "covered_fraction": round(float(s[2]) / max(tot, 1), 5)}

    res = {"tool": "strand_bench",
           "workload": "configs[1]: %d synthetic %d bp reads, %dx, k=%d, abundance %d; the first %d reads corrected, device-resident"
                       % (n_reads, read_len, args.coverage, k, a, n_corr),
           "bases_corrected": total, "index": gs.index_info(), "genome_kmers": truth.popcount(),
           "input": {"cover": stats_of(gs, d_bases, d_off, total),
                     "genome_fraction": stats_of(truth, d_bases, d_off, total)["solid_fraction"]},
           "chains": {}}
    timers = {}
    for cname in args.chains.split(","):
        res["chains"][cname] = {}
        for mode in MODES:
            chain = br_amd.Chain(gs, CHAINS[cname], second_pass=mode)

            def run():
                return chain.correct_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n_corr, total, d_out.data_ptr(), d_out.numel(),
                                                  d_out_off.data_ptr(), stream)
            run()   # warm-up: workspaces, index, successor table
            best = None
            for _ in range(args.repeat):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out_total = run()
                e1.record()
                e1.synchronize()
                ms = e0.elapsed_time(e1)
                best = ms if best is None else min(best, ms)
            st = chain.last_stats()
            _lib.profile_enable(True)
            _lib.profile_reset()
            run()
            torch.cuda.synchronize()
            prof = {nm: round(v["total_ms"], 3) for nm, v in _lib.profile_all().items() if v["launches"]}
            _lib.profile_enable(False)
            timers[(cname, mode)] = prof
            res["chains"][cname][mode] = {"ms_per_gbp": round(best / gbp, 3), "fixes": st["fixes"], "lane_units": st["lane_units"],
                                          "overflow_retries": st["overflow_retries"],
                                          "cover": stats_of(gs, d_out, d_out_off, out_total),
                                          "genome_fraction": stats_of(truth, d_out, d_out_off, out_total)["solid_fraction"],
                                          "kernels_ms": prof}
            del chain
    if ("one", "revcomp") in timers and ("one", "reverse") in timers:
        rc, cp = timers[("one", "revcomp")].get("strand_compact"), timers[("one", "reverse")].get("compact")
        if rc and cp:
            res["compaction"] = {"strand_compact_ms": rc, "compact_reversed_ms": cp, "ratio": round(rc / cp, 3),
                                 "strand_stage_ms": timers[("one", "revcomp")].get("strand"),
                                 "gb_per_s_strand_compact": round(2 * total / rc / 1e6, 1), "gb_per_s_compact": round(2 * total / cp / 1e6, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
