#!/usr/bin/env python3
"""Counting in parts against one counting table, on bench.py's synthetic workload (10 kb reads at 50x of a uniform random
genome, device-resident) at k = 25, all legs in ONE process.  ONE JSON line, ms per Gbp of reads, median of --repeat with the
spread (min .. max) beside it:

  unsliced          tab_count (brx_set_count_add_batch_device into a new table counter, one batch, under the profile timer)
                    + tab_select (finish(abundance), wall time); the table's peak bytes
  parts[P]          for P in --parts: one counter, P sweeps of reset / set_slice / one batch.  Summed over the sweeps: the
                    tab_count and tab_census (sizing pass) timers, the wall time of listing at min_count 1 and at 4, of the
                    balanced join of the lists of min_count 1; the largest table peak of a sweep, the bytes of the joined
                    list (9 per entry) and of the lists at min_count 4, the slice statistics; and
                    count_ratio = sum of the parts' tab_count / the unsliced tab_count (an uncompacted filter would sit near P)
  equal             per P: the joined list's finish(abundance) fingerprint and the summed spectrum against the unsliced ones

    python tools/sliced_count_bench.py [--reads 100000] [--repeat 5] [--parts 2,4,8,16] [--out profiles/sliced_count_bench.json]
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
    ap.add_argument("-k", type=int, default=25)
    ap.add_argument("--abundance", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--parts", default="2,4,8,16")
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

    def spread(xs):
        return {"median": round(statistics.median(xs) / gbp, 3), "min": round(min(xs) / gbp, 3), "max": round(max(xs) / gbp, 3)}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def timer(name):
        v = _lib.profile_all().get(name)
        return v["total_ms"] if v else 0.0

    def count(cnt):
        cnt.add_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, total, stream)
        torch.cuda.synchronize()

    _lib.profile_enable(True)
    # the unsliced count, a new counter every time
    t_count, t_select = [], []
    for i in range(args.repeat + 1):
        cnt = gs = None
        cnt = br_amd.Counter(k, dev, _lib.COUNT_TABLE)
        _lib.profile_reset()
        count(cnt)
        ms_c = timer("tab_count")
        ms_s, gs = wall(lambda: cnt.finish(a, stream))
        if i:
            t_count.append(ms_c)
            t_select.append(ms_s)
    fp, spec = gs.fingerprint(), cnt.spectrum()
    info = cnt.table_info()
    unsliced = {"tab_count": spread(t_count), "tab_select": spread(t_select), "keys": info["keys"], "solid": int(gs.popcount()),
                "log2_lines": info["log2_lines"], "peak_bytes": info["peak_bytes"]}
    cnt = gs = None
    _lib.lib().brx_devpool_trim()

    out_parts, equal = {}, {}
    for P in [int(x) for x in args.parts.split(",") if x]:
        rows = []
        cnt = br_amd.Counter(k, dev, _lib.COUNT_TABLE)
        for i in range(args.repeat + 1):
            row = {"tab_count": 0.0, "tab_census": 0.0, "list_1": 0.0, "list_4": 0.0, "join": 0.0}
            job_spec = np.zeros(256, dtype=np.uint64)
            stack, peak, bytes4, log2 = [], 0, 0, []
            stats = {"seen": 0, "walked": 0, "trips": 0, "waves": 0}
            for p in range(P):
                cnt.reset(stream)
                cnt.set_slice(p, P)
                _lib.profile_reset()
                count(cnt)
                row["tab_count"] += timer("tab_count")
                row["tab_census"] += timer("tab_census")
                ms, l4 = wall(lambda: br_amd.CountList.from_counter(cnt, 4))
                row["list_4"] += ms
                bytes4 += 9 * l4.n
                l4 = None
                ms, l1 = wall(lambda: br_amd.CountList.from_counter(cnt, 1))
                row["list_1"] += ms
                job_spec[1:] += cnt.spectrum()[1:]
                ti = cnt.table_info()
                peak = max(peak, ti["peak_bytes"])
                log2.append(ti["log2_lines"])
                for name, v in cnt.slice_stats().items():
                    stats[name] += v
                stack.append((0, l1))
                l1 = None
                while len(stack) > 1 and stack[-1][0] == stack[-2][0]:
                    (ra, x), (_, y) = stack.pop(), stack.pop()
                    ms, z = wall(lambda: y.maximum(x))
                    row["join"] += ms
                    stack.append((ra + 1, z))
                    x = y = z = None
            while len(stack) > 1:
                (ra, x), (_, y) = stack.pop(), stack.pop()
                ms, z = wall(lambda: y.maximum(x))
                row["join"] += ms
                stack.append((ra + 1, z))
                x = y = z = None
            joined = stack.pop()[1]
            if i:
                rows.append(row)
            else:
                job_spec[0] = np.uint64((1 << (2 * k - 1)) - int(job_spec[1:].sum()))
                equal[str(P)] = {"fingerprint": joined.finish(a).fingerprint() == fp, "spectrum": bool(np.array_equal(job_spec, spec)),
                                 "entries": joined.n == unsliced["keys"]}
                shape = {"table_peak_bytes": peak, "log2_lines": [min(log2), max(log2)], "list_bytes_min1": 9 * joined.n,
                         "list_bytes_min4": bytes4, "slice_stats": stats,
                         "dense": stats["trips"] <= stats["walked"] // 64 + stats["waves"]}
            joined = None
        cnt = None
        _lib.lib().brx_devpool_trim()
        res = {key: spread([r[key] for r in rows]) for key in rows[0]}
        res["count_ratio"] = round(statistics.median(r["tab_count"] for r in rows) / statistics.median(t_count), 4)
        res["count_and_census_ratio"] = round(statistics.median(r["tab_count"] + r["tab_census"] for r in rows) / statistics.median(t_count), 4)
        res.update(shape)
        out_parts[str(P)] = res
    _lib.profile_enable(False)

    out = {"tool": "sliced_count_bench",
           "workload": "%d synthetic %d bp reads, %dx, k=%d, abundance %d, device-resident" % (n_reads, read_len, args.coverage, k, a),
           "bases": int(round(gbp * 1e9)), "unit": "ms per Gbp of reads, median (min, max) of %d" % args.repeat,
           "unsliced": unsliced, "parts": out_parts, "equal": equal}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
