#!/usr/bin/env python3
"""The multi-GPU merge of counting tables (include/brx.h brx_exchange_table_merge / _spectrum / _table_finish) on bench.py's
synthetic workload -- 10 kb reads at 50x of a uniform random genome, device-resident, one batch -- at k = 25, in ONE process
at world 1 through real librccl: every entry of the table takes the split -> copy -> merge path there, so the kernels are
timed at full size although nothing crosses a link.  Prints ONE JSON line (and writes it to --out):

  kernels_ms_per_gbp   the brx_profile_* timers of the same run: tab_count (the yardstick for tab_merge: the same find-or-claim
                       and counter update, once per base instead of once per entry), tab_split (histogram + split pass; reads
                       what tab_select reads and writes 9 B per entry), tab_merge, tab_select (the yardstick for tab_split),
                       tab_spectrum, tab_zero
  calls_ms_per_gbp     host wall time of merge_table, spectrum and finish_table (each returns after its stream work is done)
  distinct             distinct k-mers in the table; link_bytes_per_rank_world8 = 7/8 x 9 B x distinct: what one rank WOULD send
                       at world 8 with this shard -- a count of bytes, not a rate: rates over real links need more than one card

One warm-up run, then --repeat runs with a fresh counter each; every figure is the median over the repeats.

    python tools/table_exchange_bench.py [--reads 100000] [--repeat 5] [--out profiles/table_exchange_bench.json]
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

TIMERS = ["tab_count", "tab_split", "tab_merge", "tab_select", "tab_spectrum", "tab_zero", "tab_rehash"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--read-len", type=int, default=10_000)
    ap.add_argument("--coverage", type=int, default=50)
    ap.add_argument("-k", type=int, default=25)
    ap.add_argument("--abundance", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default="", help="also write the line to this file")
    args = ap.parse_args()

    import torch
    import br_amd
    from br_amd import _lib, synth
    from br_amd import dist as D

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

    ex = D.AbiExchange(1, 0, dev)
    solid = br_amd.Pcon.new(k, dev)

    def one_run():
        _lib.profile_reset()
        cnt = br_amd.Counter(k, dev, _lib.COUNT_TABLE)
        cnt.add_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, total, stream)
        torch.cuda.synchronize()
        wall = {}
        t0 = time.perf_counter()
        ex.merge_table(cnt, stream)
        t1 = time.perf_counter()
        spec = ex.spectrum(cnt, stream)
        t2 = time.perf_counter()
        ex.finish_table(cnt, solid, a, stream)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        wall["merge_table"], wall["spectrum"], wall["finish_table"] = (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3
        prof = {nm: v["total_ms"] for nm, v in _lib.profile_all().items() if v["launches"] and nm in TIMERS}
        return wall, prof, cnt.table_info(stream), int(spec[1:].sum()), ex.last_stats(), solid.popcount()

    _lib.profile_enable(True)
    one_run()                                                                   # warm-up: code objects, pools, librccl
    runs = [one_run() for _ in range(max(1, args.repeat))]
    _lib.profile_enable(False)
    med = lambda xs: round(statistics.median(xs) / gbp, 3)
    wall = {nm: med([r[0][nm] for r in runs]) for nm in runs[0][0]}
    prof = {nm: med([r[1].get(nm, 0.0) for r in runs]) for nm in TIMERS if any(nm in r[1] for r in runs)}
    _, _, info, distinct, stats, n_solid = runs[-1]
    assert distinct == info["keys"] == stats["keys_counted_here"]              # every entry went through split and merge
    res = {"tool": "table_exchange_bench",
           "workload": "%d synthetic %d bp reads, %dx, k %d, abundance %d, device-resident, one batch; world 1 through librccl"
                       % (n_reads, read_len, args.coverage, k, a),
           "bases": int(total), "repeats": len(runs), "statistic": "median",
           "kernels_ms_per_gbp": prof, "calls_ms_per_gbp": wall,
           "split_over_select": round(prof.get("tab_split", 0.0) / max(prof.get("tab_select", 0.0), 1e-9), 3),
           "merge_over_count": round(prof.get("tab_merge", 0.0) / max(prof.get("tab_count", 0.0), 1e-9), 3),
           "distinct": distinct, "solid": int(n_solid), "merged_table": info,
           "link_bytes_per_rank_world8": distinct * 9 * 7 // 8}
    ex.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
