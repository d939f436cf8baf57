#!/usr/bin/env python3
"""K-mer abundance of reads (include/brx.h "abundance", br_amd/csrc/brx_abundance.hip) on bench.py's synthetic workload:
10 kb reads at 50x of a uniform random genome, device-resident, one batch, k = 25.  The reads are counted once into a
table counter (BRX_COUNT_TABLE); then, in the same process, ONE JSON line:

  abundance_stats     brx_counter_abundance_batch_device, statistics only: ms per Gbp by HIP events around the call (best
                      of --repeat), and the same split per kernel from the brx_profile_* timers of one more call
  abundance_profile   the same call with the per-base profile as well
  cover               brx_set_cover_batch_device (flags + statistics) of the same batch against the set finished from the
                      same counter -- the yardstick: the same probes, without the 4-byte counter load per hit and the LDS
                      atomic per position
  ratio_*             abundance over cover

    python tools/abundance_bench.py [--reads 100000] [--repeat 3] [--out profiles/abundance_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--read-len", type=int, default=10_000)
    ap.add_argument("--coverage", type=int, default=50)
    ap.add_argument("-k", type=int, default=25)
    ap.add_argument("--abundance", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default="", help="also write the line to this file")
    args = ap.parse_args()

    import numpy as np
    import torch
    import br_amd
    from br_amd import _lib, synth
    from br_amd import abundance as ab

    dev = 0
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream().cuda_stream
    k, a, n_reads, read_len = args.k, args.abundance, args.reads, args.read_len
    genome_len = max(n_reads * read_len // args.coverage, read_len)
    cfg = synth.config(genome_len=genome_len, read_len=read_len)
    d_genome = torch.empty(genome_len, dtype=torch.uint8, device="cuda")
    synth.genome_device(cfg, dev, d_genome.data_ptr(), stream)
    cap = int(n_reads * read_len * 1.03) + (1 << 20)
    d_bases = torch.empty(cap, dtype=torch.uint8, device="cuda")
    d_off = torch.empty(n_reads + 1, dtype=torch.int64, device="cuda")
    total = synth.reads_device(cfg, dev, d_genome.data_ptr(), 0, n_reads, d_bases.data_ptr(), cap, d_off.data_ptr(), stream)
    torch.cuda.synchronize()
    gbp = total / 1e9

    cnt = br_amd.Counter(k, dev, _lib.COUNT_TABLE)
    cnt.add_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, total, stream)
    gs = cnt.finish(a, stream)
    torch.cuda.synchronize()
    info = cnt.table_info(stream)

    d_profile = torch.empty(total, dtype=torch.uint8, device="cuda")
    d_flags = torch.empty(total, dtype=torch.uint8, device="cuda")
    d_stats = torch.zeros((n_reads, ab.STATS_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    d_cstats = torch.zeros((n_reads, 4), dtype=torch.int32, device="cuda")

    def stats_only():
        cnt.abundance_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, total, a, None, None, d_stats.data_ptr(), stream)

    def with_profile():
        cnt.abundance_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, total, a, d_profile.data_ptr(), None,
                                   d_stats.data_ptr(), stream)

    def cover_call():
        gs.cover_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, total, d_flags.data_ptr(), None, d_cstats.data_ptr(), stream)

    def cover_stats_only():
        gs.cover_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, total, None, None, d_cstats.data_ptr(), stream)

    def timed(fn):
        fn()  # (first call: the probe index of the set, the pool's blocks)
        best = None
        for _ in range(args.repeat):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            best = ms if best is None else min(best, ms)
        return best

    def profiled(fn):
        _lib.profile_enable(True)
        _lib.profile_reset()
        fn()
        torch.cuda.synchronize()
        prof = {nm: round(v["total_ms"] / gbp, 3) for nm, v in _lib.profile_all().items() if v["launches"]}
        _lib.profile_enable(False)
        return prof

    ms_stats, ms_prof = timed(stats_only), timed(with_profile)
    ms_cover, ms_cover_stats = timed(cover_call), timed(cover_stats_only)
    prof_stats, prof_prof, prof_cover = profiled(stats_only), profiled(with_profile), profiled(cover_call)

    # the two must tell the same story: k-mers above the threshold = solid k-mers of the set finished with it
    st = d_stats.cpu().numpy().view(ab.STATS_DTYPE).reshape(-1)
    cs = d_cstats.cpu().numpy().view(np.uint32)
    agree = bool(np.array_equal(st["above"], cs[:, 1]) and np.array_equal(st["kmers"], cs[:, 0]))
    kmers = int(st["kmers"].astype(np.int64).sum())

    res = {"tool": "abundance_bench",
           "workload": "%d synthetic %d bp reads, %dx, k %d, abundance %d, device-resident, one batch" % (n_reads, read_len, args.coverage, k, a),
           "bases": int(total), "kmers": kmers, "table": info,
           "abundance_stats": {"ms_per_gbp": round(ms_stats / gbp, 3), "kernels_ms_per_gbp": prof_stats},
           "abundance_profile": {"ms_per_gbp": round(ms_prof / gbp, 3), "kernels_ms_per_gbp": prof_prof},
           "cover": {"ms_per_gbp": round(ms_cover / gbp, 3), "stats_only_ms_per_gbp": round(ms_cover_stats / gbp, 3),
                     "kernels_ms_per_gbp": prof_cover, "solid": int(gs.popcount())},
           "ratio_profile_over_cover": round(ms_prof / ms_cover, 3),
           "ratio_stats_over_cover_stats": round(ms_stats / ms_cover_stats, 3),
           "lookup_kernel_ns_per_kmer": round(prof_prof.get("abund", 0.0) * gbp * 1e6 / max(kmers, 1), 4),
           "median_of_medians": int(np.median(st["median"])), "absent_share": round(float(st["absent"].astype(np.int64).sum()) / max(kmers, 1), 5),
           "above_equals_cover_solid": agree}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
