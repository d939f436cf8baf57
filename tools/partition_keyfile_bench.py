#!/usr/bin/env python3
"""Count files from the partitioned counter against the hash table's, on bench.py's synthetic workload (10 kb reads at 50x
of a uniform random genome, device-resident, one batch), at k = 19 and k = 21, both paths in ONE process.  ONE JSON line,
ms per Gbp of reads, median of --repeat, a new counter per repetition as a run of the command line has:

  partitioned  count (brx_set_count_add_batch_device into a new BRX_COUNT_SORTED counter), view (brx_counter_lookup_prepare:
               the radix levels 2..n + the view kernel), then Counter.save by the library's own clocks (stats8): key_list
               (the compaction of the view), key_pack, fd write
  table        count (tab_count, into a new BRX_COUNT_TABLE counter), then Counter.save: key_list + key_sort (one clock in
               stats8; their shares from the brx_profile_* timers of one more save), key_pack, fd write

sum = everything a `fasta --save-counts` pays for its count file on that path; `partitioned_over_table` decides which
counter the command line takes (br_amd/cli.py build_set).  The two files must be the same bytes.  compaction: the
kernels' time under key_list against the traffic the compaction cannot avoid -- 2 B + 1 B per position of the view and
8 B per bucket offset read, 9 B per kept key written (it reads the view twice, once to count and once to write: the
achieved rate is stated against the single read).

The files go to --dir (default /dev/shm where there is one: the fd write is then a copy, not a disk) and are removed.

    python tools/partition_keyfile_bench.py [--reads 100000] [--repeat 5] [--out profiles/partition_keyfile_bench.json]
"""
import argparse
import filecmp
import json
import os
import statistics
import sys
import tempfile
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
    ap.add_argument("--min-count", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--dir", default=None, help="where the files are written (default: /dev/shm, else the temporary directory)")
    ap.add_argument("--out", default="", help="also write the line to this file")
    args = ap.parse_args()

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
    cap = int(n_reads * read_len * 1.03) + (1 << 20)
    d_bases = torch.empty(cap, dtype=torch.uint8, device="cuda")
    d_off = torch.empty(n_reads + 1, dtype=torch.int64, device="cuda")
    total = synth.reads_device(cfg, dev, d_genome.data_ptr(), 0, n_reads, d_bases.data_ptr(), cap, d_off.data_ptr(), stream)
    torch.cuda.synchronize()
    lens = (d_off[1:] - d_off[:-1]).cpu()
    gbp = total / 1e9
    med = lambda xs: round(statistics.median(xs) / gbp, 3)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def profiled(fn):
        torch.cuda.synchronize()
        _lib.profile_enable(True)
        _lib.profile_reset()
        fn()
        torch.cuda.synchronize()
        prof = {nm: round(v["total_ms"] / gbp, 3) for nm, v in _lib.profile_all().items() if v["launches"]}
        _lib.profile_enable(False)
        return prof

    def leg(k, strategy, path):
        """a new counter per repetition: count, (view,) save; then one more save and one more view under the kernel timers"""
        part = strategy == _lib.COUNT_SORTED
        rows, st, cnt = [], None, None
        for i in range(args.repeat + 1):
            cnt = None
            cnt = br_amd.Counter(k, dev, strategy)
            row = {"count": wall(lambda: cnt.add_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, total, stream))}
            if part:
                row["view"] = wall(lambda: cnt.prepare_lookup(stream))
            with open(path, "wb") as f:
                st = cnt.save(f, args.min_count)
            row["key_list" if part else "key_list_sort"] = st["ns_list_sort"] / 1e6
            row["key_pack"] = st["ns_pack"] / 1e6
            row["fd"] = st["ns_fd"] / 1e6
            row["save_wall"] = st["ns_wall"] / 1e6
            if i:
                rows.append(row)
        res = {key: med([r[key] for r in rows]) for key in rows[0]}
        res["sum"] = round(sum(v for key, v in res.items() if key != "save_wall"), 3)
        with open(path, "wb") as f:
            res["save_kernels"] = profiled(lambda: cnt.save(f, args.min_count))
        if part:
            cnt.drop_lookup()
            res["view_kernels"] = profiled(lambda: cnt.prepare_lookup(stream))
        else:
            res["table"] = cnt.table_info(stream)
        cnt = None
        _lib.lib().brx_devpool_trim()
        return res, st

    if args.dir is None and os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK):
        args.dir = "/dev/shm"
    tmp = tempfile.mkdtemp(prefix="partition_keyfile_bench_", dir=args.dir)
    ppath, tpath = os.path.join(tmp, "part.keys"), os.path.join(tmp, "table.keys")
    out = {"tool": "partition_keyfile_bench",
           "workload": "%d synthetic %d bp reads, %dx, min_count %d, device-resident, one batch" % (n_reads, read_len, args.coverage,
                                                                                                   args.min_count),
           "bases": int(total), "unit": "ms per Gbp of reads, median of %d" % args.repeat, "files_on": args.dir or tempfile.gettempdir()}
    try:
        for k in args.k or [19, 21]:
            res_p, st_p = leg(k, _lib.COUNT_SORTED, ppath)
            res_t, st_t = leg(k, _lib.COUNT_TABLE, tpath)
            equal = filecmp.cmp(ppath, tpath, shallow=False)
            assert equal, "k=%d: the partitioned counter's file differs from the table counter's" % k
            positions = int((lens - (k - 1)).clamp(min=0).sum())  # (the synthetic reads hold no N: a k-mer per position)
            n_buckets = 1 << (2 * k - 1 - 12)
            traffic = 3 * positions + 8 * (n_buckets + 1) + 9 * st_p["keys"]
            list_ms = res_p["save_kernels"].get("key_list", 0.0) * gbp
            out["k%d" % k] = {
                "keys": st_p["keys"], "bytes": st_p["bytes"], "bytes_per_key": round(st_p["bytes"] / max(st_p["keys"], 1), 3),
                "files_equal": bool(equal and st_p["keys"] == st_t["keys"] and st_p["bytes"] == st_t["bytes"]),
                "partitioned": res_p, "table": res_t,
                "partitioned_over_table": round(res_p["sum"] / res_t["sum"], 4),
                "partitioned_wins": bool(res_p["sum"] < res_t["sum"]),
                "compaction": {"positions": positions, "buckets": n_buckets, "traffic_bytes": traffic, "kernels_ms": round(list_ms, 3),
                               "gb_per_s": round(traffic / 1e9 / (list_ms / 1e3), 1) if list_ms else None}}
    finally:
        for p in (ppath, tpath):
            if os.path.exists(p):
                os.remove(p)
        os.rmdir(tmp)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
