#!/usr/bin/env python3
"""The joint spectrum of two count lists against the merge it rides on, on bench.py's synthetic workload (10 kb reads at 50x
of a uniform random genome, device-resident) at k = 25: the two half-job shard lists of tools/countlist_bench.py's leg (d),
all legs in ONE process.  ONE JSON line, ms per Gbp of reads, median of --repeat with the spread (min .. max) beside it:

  compare           brx_counts_compare (CountList.joint): wall time, and the "count_joint" timer (split, the pass, the copy
                    out) with its share of the wall time
  size_only         brx_counts_combine_device with d_kout == NULL and cap == 0 over the same two lists: split + pass 1 + scan
                    under the "count_merge" timer, and wall time -- the yardstick: it reads the same 9 bytes per entry
  add               a + b (brx_counts_combine): wall time and the "count_merge" timer
  joint_over_size_only   the ratio of the two timers' medians
  spectrum          the joint's bins: how many are non-zero, the share of the keys in the LDS corner, the hottest bins
  equal             the joint's row sums against a.spectrum(), its column sums against b.spectrum(), |A n B| of the three legs

    python tools/count_compare_bench.py [--reads 100000] [--repeat 5] [--out profiles/count_compare_bench.json]
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


def shard_lists(args):
    """(the count lists of the two halves of the reads, Gbp of all the reads)"""
    import torch
    import br_amd
    from br_amd import _lib, synth

    dev = 0
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream().cuda_stream
    n_reads, read_len = args.reads, args.read_len
    genome_len = max(n_reads * read_len // args.coverage, read_len)
    cfg = synth.config(genome_len=genome_len, read_len=read_len)
    d_genome = torch.empty(genome_len, dtype=torch.uint8, device="cuda")
    synth.genome_device(cfg, dev, d_genome.data_ptr(), stream)
    half = n_reads // 2
    lists, bases = [], 0
    for first, n in ((0, half), (half, n_reads - half)):
        cap = int(n * read_len * 1.03) + (1 << 20)
        d_bases = torch.empty(cap, dtype=torch.uint8, device="cuda")
        d_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        total = synth.reads_device(cfg, dev, d_genome.data_ptr(), first, n, d_bases.data_ptr(), cap, d_off.data_ptr(), stream)
        torch.cuda.synchronize()
        cnt = br_amd.Counter(args.k, dev, _lib.COUNT_TABLE)
        cnt.add_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n, total, stream)
        torch.cuda.synchronize()
        lists.append(br_amd.CountList.from_counter(cnt))
        bases += total
        cnt = d_bases = d_off = None
    return lists[0], lists[1], bases / 1e9


def timed(fn, timer, repeat):
    """(wall ms, ms under the profile timer) of `repeat` runs of fn after one that is not taken, and the last result"""
    import torch
    from br_amd import _lib
    walls, kernels, res = [], [], None
    for i in range(repeat + 1):
        res = None
        _lib.profile_enable(True)
        _lib.profile_reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        kernel = _lib.profile_all()[timer]["total_ms"]
        _lib.profile_enable(False)
        if i:
            walls.append(ms)
            kernels.append(kernel)
    return walls, kernels, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--read-len", type=int, default=10_000)
    ap.add_argument("--coverage", type=int, default=50)
    ap.add_argument("-k", type=int, default=25)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default="", help="also write the line to this file")
    args = ap.parse_args()

    import numpy as np
    from br_amd import countops
    from br_amd.set import combine_counts_device

    a, b, gbp = shard_lists(args)

    def spread(xs):
        return {"median": round(statistics.median(xs) / gbp, 3), "min": round(min(xs) / gbp, 3), "max": round(max(xs) / gbp, 3)}

    (ka, ca, na), (kb, cb, nb) = a.device_arrays(), b.device_arrays()
    joint_wall, joint_kernel, J = timed(lambda: a.joint(b), "count_joint", args.repeat)
    size_wall, size_kernel, size_res = timed(lambda: combine_counts_device(ka, ca, na, kb, cb, nb, "add", None, None, 0), "count_merge",
                                             args.repeat)
    add_wall, add_kernel, added = timed(lambda: a + b, "count_merge", args.repeat)
    both_add, n_add = added.combine_stats["both"], added.n
    added = None

    corner = countops.JOINT_CORNER
    keys = int(J.sum()) - int(J[0, 0])
    flat = J.ravel().copy()
    flat[0] = 0
    hottest = [[int(x) >> 8, int(x) & 255, round(int(flat[x]) / keys, 4)] for x in np.argsort(flat)[::-1][:6]]
    ratio = statistics.median(joint_kernel) / statistics.median(size_kernel)
    out = {"tool": "count_compare_bench",
           "workload": "the two halves of %d synthetic %d bp reads, %dx, k=%d, device-resident" % (args.reads, args.read_len, args.coverage, args.k),
           "bases": int(round(gbp * 1e9)), "a": na, "b": nb, "both": a.compare_stats["both"], "either": keys,
           "unit": "ms per Gbp of reads, median (min, max) of %d" % args.repeat,
           "compare": {"wall": spread(joint_wall), "count_joint": spread(joint_kernel),
                       "kernel_share": round(statistics.median(joint_kernel) / statistics.median(joint_wall), 4),
                       "gb_per_s": round(9 * (na + nb) / 1e9 / (statistics.median(joint_kernel) / 1e3), 1)},
           "size_only": {"wall": spread(size_wall), "count_merge": spread(size_kernel),
                         "gb_per_s": round(9 * (na + nb) / 1e9 / (statistics.median(size_kernel) / 1e3), 1)},
           "add": {"wall": spread(add_wall), "count_merge": spread(add_kernel)},
           "joint_over_size_only": round(ratio, 4),
           "spectrum": {"bins": int(np.count_nonzero(flat)), "in_corner": round((int(J[:corner, :corner].sum()) - int(J[0, 0])) / keys, 6),
                        "hottest": hottest},
           "equal": {"rows_are_a_spectrum": bool(np.array_equal(J.sum(axis=1), a.spectrum())),
                     "columns_are_b_spectrum": bool(np.array_equal(J.sum(axis=0), b.spectrum())),
                     "both": bool(a.compare_stats["both"] == size_res[1][2] == both_add),
                     "either": bool(keys == n_add == size_res[0])}}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
