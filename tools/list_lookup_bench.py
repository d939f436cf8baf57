#!/usr/bin/env python3
"""Abundance from a count list against the hash table, on bench.py's synthetic workload (10 kb reads at 50x of a uniform
random genome, device-resident, one batch), at k = 19, 21 and 25, all legs in ONE process.  ONE JSON line, ms per Gbp, the
median of --repeat runs by a host clock around work that ends in a device synchronise:

  table        abundance statistics from a BRX_COUNT_TABLE counter of the batch
  list         the count list of that counter (CountList.from_counter): list_dir = brx_counts_lookup_prepare with the chosen
               directory (and the "list_dir" kernel's share from the brx_profile_* timers of one more call), abundance
               statistics from the list, the directory's bytes and its fullest bucket
  partitioned  at k = 19 and 21: abundance statistics from the count view of a BRX_COUNT_SORTED counter

The legs must agree: the statistics of all of them byte for byte.

    python tools/list_lookup_bench.py [--reads 100000] [--repeat 5] [--out profiles/list_lookup_bench.json]
"""
import argparse
import json
import os
import statistics
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
    ap.add_argument("-k", type=int, action="append", default=None, help="repeatable; default 19, 21 and 25")
    ap.add_argument("--abundance", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default="", help="also write the line to this file")
    args = ap.parse_args()

    import torch
    import br_amd
    from br_amd import _lib, synth
    from br_amd import abundance as ab
    from br_amd.set import CountList

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
    d_stats = torch.zeros((n_reads, ab.STATS_DTYPE.itemsize), dtype=torch.uint8, device="cuda")

    def timed(fn, before=None):
        """median of --repeat after one warm-up, ms per Gbp; `before` runs untimed ahead of every call"""
        ms = []
        for i in range(args.repeat + 1):
            if before:
                before()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i:
                ms.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(ms) / gbp, 3)

    def kernel_ms(fn, name, before=None):
        if before:
            before()
        torch.cuda.synchronize()
        _lib.profile_enable(True)
        _lib.profile_reset()
        fn()
        torch.cuda.synchronize()
        prof = _lib.profile_all()
        _lib.profile_enable(False)
        return round(prof.get(name, {"total_ms": 0.0})["total_ms"] / gbp, 3)

    def stats_of(obj):
        def call():
            obj.abundance_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, total, a, None, None, d_stats.data_ptr(), stream)
        ms = timed(call)
        kern = kernel_ms(call, "abund")
        return ms, kern, d_stats.cpu().numpy().tobytes()

    out = {"tool": "list_lookup_bench",
           "workload": "%d synthetic %d bp reads, %dx, abundance %d, device-resident, one batch" % (n_reads, read_len, args.coverage, a),
           "bases": int(total), "unit": "ms per Gbp, median of %d" % args.repeat}
    for k in args.k or [19, 21, 25]:
        table = br_amd.Counter(k, dev, _lib.COUNT_TABLE)
        table.add_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, total, stream)
        torch.cuda.synchronize()
        t_ms, t_kern, t_stats = stats_of(table)
        lst = CountList.from_counter(table)
        del table
        _lib.lib().brx_devpool_trim()
        res = {"entries": lst.n, "list_bytes": 9 * lst.n,
               "table": {"abundance_stats": t_ms, "abund_kernel": t_kern},
               "list": {"list_dir": timed(lst.prepare_lookup, before=lst.drop_lookup),
                        "list_dir_kernel": kernel_ms(lst.prepare_lookup, "list_dir", before=lst.drop_lookup)}}
        l_ms, l_kern, l_stats = stats_of(lst)
        info = lst.lookup_info()
        res["list"].update({"abundance_stats": l_ms, "abund_kernel": l_kern, "log2_buckets": info["log2_buckets"],
                            "directory_bytes": info["directory_bytes"], "fullest_bucket": info["fullest_bucket"]})
        res["list_over_table_lookup"] = round(l_ms / t_ms, 4)
        res["stats_equal"] = bool(l_stats == t_stats)
        del lst
        if k in (19, 21):
            part = br_amd.Counter(k, dev, _lib.COUNT_SORTED)
            part.add_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, total, stream)
            part.prepare_lookup(stream)
            torch.cuda.synchronize()
            p_ms, p_kern, p_stats = stats_of(part)
            res["partitioned"] = {"abundance_stats": p_ms, "abund_kernel": p_kern}
            res["list_over_partitioned_lookup"] = round(l_ms / p_ms, 4)
            res["stats_equal"] = bool(res["stats_equal"] and p_stats == t_stats)
            del part
        _lib.lib().brx_devpool_trim()
        out["k%d" % k] = res
        print("k=%d: %s" % (k, json.dumps(res)), file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
