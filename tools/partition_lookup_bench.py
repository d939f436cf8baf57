#!/usr/bin/env python3
"""Abundance from the partitioned counter against the hash table, on bench.py's synthetic workload (10 kb reads at 50x of a
uniform random genome, device-resident, one batch), at k = 19 and k = 21, all legs in ONE process.  ONE JSON line, ms per
Gbp, best of --repeat by a host clock around work that ends in a device synchronise:

  (a) partitioned  count (brx_set_count_add_batch_device into a new BRX_COUNT_SORTED counter), part_view (brx_counter_lookup_prepare: the
                   radix levels 2..n + the view kernel; the kernels' shares from the brx_profile_* timers of one more
                   call), abundance statistics only, abundance with the per-base profile
  (b) table        the same on a BRX_COUNT_TABLE counter at the same k (no view to build)
  (c) cover        brx_set_cover_batch_device (flags + statistics) on the set finished from (a)'s counter

total_* = count + view + abundance statistics: what `--abundance-report` pays for its counter.  The legs must agree: the
statistics of (a) and (b) byte for byte, and their `above` with (c)'s solid k-mers.

    python tools/partition_lookup_bench.py [--reads 100000] [--repeat 3] [--out profiles/partition_lookup_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--read-len", type=int, default=10_000)
    ap.add_argument("--coverage", type=int, default=50)
    ap.add_argument("-k", type=int, action="append", default=None, help="repeatable; default 19 and 21")
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
    a, n_reads, read_len = args.abundance, args.reads, args.read_len
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
    d_profile = torch.empty(total, dtype=torch.uint8, device="cuda")
    d_flags = torch.empty(total, dtype=torch.uint8, device="cuda")
    d_stats = torch.zeros((n_reads, ab.STATS_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    d_cstats = torch.zeros((n_reads, 4), dtype=torch.int32, device="cuda")

    def timed(fn, before=None, warm=True):
        """best of --repeat, ms per Gbp; `before` runs untimed ahead of every call"""
        best = None
        for i in range(args.repeat + (1 if warm else 0)):
            if before:
                before()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            if not (warm and i == 0):
                best = ms if best is None else min(best, ms)
        return round(best / gbp, 3)

    def profiled(fn, before=None):
        if before:
            before()
        torch.cuda.synchronize()
        _lib.profile_enable(True)
        _lib.profile_reset()
        fn()
        torch.cuda.synchronize()
        prof = {nm: round(v["total_ms"] / gbp, 3) for nm, v in _lib.profile_all().items() if v["launches"]}
        _lib.profile_enable(False)
        return prof

    def leg(k, strategy):
        # count: into a NEW counter every time, as a run of the command line does (the table grows as the reads come in)
        best = None
        for i in range(args.repeat + 1):
            cnt = None
            cnt = br_amd.Counter(k, dev, strategy)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cnt.add_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, total, stream)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            if i:
                best = ms if best is None else min(best, ms)

        def stats_only():
            cnt.abundance_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, total, a, None, None, d_stats.data_ptr(), stream)

        def with_profile():
            cnt.abundance_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, total, a, d_profile.data_ptr(), None,
                                       d_stats.data_ptr(), stream)

        res = {"count": round(best / gbp, 3)}
        res["part_view"] = timed(lambda: cnt.prepare_lookup(stream), before=cnt.drop_lookup)
        res["part_view_kernels"] = profiled(lambda: cnt.prepare_lookup(stream), before=cnt.drop_lookup)
        res["abundance_stats"] = timed(stats_only)
        res["abundance_profile"] = timed(with_profile)
        res["abundance_kernels"] = profiled(with_profile)
        res["total_count_view_stats"] = round(res["count"] + res["part_view"] + res["abundance_stats"], 3)
        return cnt, res, d_stats.cpu().numpy().view(ab.STATS_DTYPE).reshape(-1).copy()

    out = {"tool": "partition_lookup_bench",
           "workload": "%d synthetic %d bp reads, %dx, abundance %d, device-resident, one batch" % (n_reads, read_len, args.coverage, a),
           "bases": int(total), "unit": "ms per Gbp, best of %d" % args.repeat}
    for k in args.k or [19, 21]:
        part, res_a, st_a = leg(k, _lib.COUNT_SORTED)
        kmers = int(st_a["kmers"].astype(np.int64).sum())
        gs = part.finish(a, stream)  # (drops the view: every lookup above is done)
        torch.cuda.synchronize()

        def cover_call():
            gs.cover_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, total, d_flags.data_ptr(), None, d_cstats.data_ptr(), stream)

        res_c = {"cover": timed(cover_call), "solid": int(gs.popcount())}
        cs = d_cstats.cpu().numpy().view(np.uint32)
        del gs, part
        table, res_b, st_b = leg(k, _lib.COUNT_TABLE)
        res_b["table"] = table.table_info(stream)
        del table
        _lib.lib().brx_devpool_trim()
        out["k%d" % k] = {
            "kmers": kmers, "partitioned": res_a, "table": res_b, "cover": res_c,
            "partitioned_over_table_total": round(res_a["total_count_view_stats"] / res_b["total_count_view_stats"], 4),
            "partitioned_over_table_lookup": round(res_a["abundance_stats"] / res_b["abundance_stats"], 4),
            "lookup_kernel_ns_per_kmer": {"partitioned": round(res_a["abundance_kernels"].get("abund", 0.0) * gbp * 1e6 / max(kmers, 1), 4),
                                          "table": round(res_b["abundance_kernels"].get("abund", 0.0) * gbp * 1e6 / max(kmers, 1), 4)},
            "stats_equal": bool(st_a.tobytes() == st_b.tobytes()),
            "above_equals_cover_solid": bool(np.array_equal(st_a["above"], cs[:, 1]) and np.array_equal(st_a["kmers"], cs[:, 0])),
            "median_of_medians": int(np.median(st_a["median"]))}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
