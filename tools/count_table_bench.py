#!/usr/bin/env python3
"""Counted set build at k = 25 (include/brx.h BRX_COUNT_TABLE, br_amd/csrc/brx_counttable.hip) on bench.py's synthetic
workload: 10 kb reads at 50x of a uniform random genome, device-resident, one batch.  Prints ONE JSON line:

  counted            count + finish at k (default 25), abundance 3: ms per Gbp by HIP events around both calls (best of
                     --repeat, a fresh counter each time so that the table's allocation and zeroing are inside), the same
                     split per kernel from the brx_profile_* timers of one more run, the table's size and the bytes of
                     HBM it held at the peak
  presence           brx_set_insert_batch_device at the same k on the same batch, same box, same call: the same
                     find-or-insert without the counter update -- what the counters cost is counted / presence
  partitioned_k21    the partitioned build (count + finish) at k = 21 on the same batch
  genome_share       share of the reads' k-mers that are k-mers of the genome, before and after correct::one (forward +
                     reverse) with the counted set, and after the same with the presence set (which holds every k-mer of
                     the reads, so nothing triggers)

    python tools/count_table_bench.py [--reads 100000] [--repeat 3] [--out profiles/count_table_bench.json]
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

    def timed(fn, repeat=args.repeat):
        best, keep = None, None
        for _ in range(repeat):
            keep = None
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            keep = fn()
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            best = ms if best is None else min(best, ms)
        return best, keep

    def counted_build(kk, strategy=_lib.COUNT_AUTO):
        cnt = br_amd.Counter(kk, dev, strategy)
        cnt.add_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, total, stream)
        return cnt, cnt.finish(a, stream)

    def presence_build():
        s = br_amd.Pcon.new(k, dev)
        _lib.check(_lib.lib().brx_set_insert_batch_device(s._h, d_bases.data_ptr(), d_off.data_ptr(), n_reads, total, stream))
        return s

    def profiled(fn):
        _lib.profile_enable(True)
        _lib.profile_reset()
        keep = fn()
        torch.cuda.synchronize()
        prof = {nm: round(v["total_ms"] / gbp, 3) for nm, v in _lib.profile_all().items() if v["launches"]}
        _lib.profile_enable(False)
        del keep
        return prof

    free0 = torch.cuda.mem_get_info()[0]
    ms_counted, (cnt, gs) = timed(lambda: counted_build(k))
    info = cnt.table_info(stream)
    held = free0 - torch.cuda.mem_get_info()[0]  # counter + set, after the build (the device pool keeps freed blocks)
    solid = gs.popcount()
    del cnt
    ms_presence, ps = timed(presence_build)
    presence_keys = ps.popcount()
    ms_part, keep = timed(lambda: counted_build(21))
    part_solid = keep[1].popcount()
    del keep
    prof_counted = profiled(lambda: counted_build(k))
    prof_presence = profiled(presence_build)
    prof_part = profiled(lambda: counted_build(21))

    # share of the reads' k-mers that are genome k-mers: cover statistics against the presence set of the genome itself
    g_off = torch.tensor([0, genome_len], dtype=torch.int64, device="cuda")
    genome_set = br_amd.Pcon.new(k, dev)
    _lib.check(_lib.lib().brx_set_insert_batch_device(genome_set._h, d_genome.data_ptr(), g_off.data_ptr(), 1, genome_len, stream))
    d_stats = torch.empty((n_reads, 4), dtype=torch.int32, device="cuda")
    d_out = torch.empty(int(total * 1.05) + (1 << 20), dtype=torch.uint8, device="cuda")
    d_out_off = torch.empty(n_reads + 1, dtype=torch.int64, device="cuda")

    def share(bases, offs, tot):
        genome_set.cover_batch_device(bases.data_ptr(), offs.data_ptr(), n_reads, tot, None, None, d_stats.data_ptr(), stream)
        torch.cuda.synchronize()
        s = d_stats.cpu().numpy().view(np.uint32).astype(np.int64).sum(axis=0)
        return round(float(s[1]) / max(int(s[0]), 1), 5)

    def after_one(the_set):
        chain = br_amd.Chain(the_set, [("one", 5, 7)], two_side=False)
        out_total = chain.correct_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, total, d_out.data_ptr(), d_out.numel(),
                                               d_out_off.data_ptr(), stream)
        torch.cuda.synchronize()
        return share(d_out, d_out_off, out_total), chain.last_stats()["fixes"]

    before = share(d_bases, d_off, total)
    after_counted, fixes_counted = after_one(gs)
    after_presence, fixes_presence = after_one(ps)

    res = {"tool": "count_table_bench",
           "workload": "%d synthetic %d bp reads, %dx, abundance %d, device-resident, one batch" % (n_reads, read_len, args.coverage, a),
           "bases": int(total),
           "counted": {"k": k, "ms_per_gbp": round(ms_counted / gbp, 3), "kernels_ms_per_gbp": prof_counted, "table": info,
                       "solid": int(solid), "bytes_held_after_build": int(held)},
           "presence": {"k": k, "ms_per_gbp": round(ms_presence / gbp, 3), "kernels_ms_per_gbp": prof_presence, "keys": int(presence_keys)},
           "counted_over_presence": round(ms_counted / ms_presence, 3),
           "count_kernel_over_insert_kernel": round(prof_counted.get("tab_count", 0.0) / max(prof_presence.get("index_insert_reads", 0.0), 1e-9), 3),
           "count_kernel_ns_per_kmer": round(prof_counted.get("tab_count", 0.0) * gbp * 1e6 / total, 4),
           "partitioned_k21": {"k": 21, "ms_per_gbp": round(ms_part / gbp, 3), "kernels_ms_per_gbp": prof_part, "solid": int(part_solid)},
           "genome_share": {"k": k, "before": before, "after_one_counted_set": after_counted, "fixes_counted_set": int(fixes_counted),
                            "after_one_presence_set": after_presence, "fixes_presence_set": int(fixes_presence)}}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
