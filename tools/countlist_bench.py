#!/usr/bin/env python3
"""Count lists against the counting table and against counting the reads again, on bench.py's synthetic workload (10 kb reads
at 50x of a uniform random genome, device-resident) at k = 25, all legs in ONE process.  ONE JSON line, ms per Gbp of reads,
median of --repeat with the spread (min .. max) beside it:

  a_list_route      CountList.from_keyfile -> finish(abundance): fd read, unpack (stats8 of the load), select, set build
                    (stats8 of the finish), and the wall time of both calls
  b_table_route     Counter.load into a new BRX_COUNT_TABLE counter -> finish(abundance), wall time
  c_count_again     tab_count (brx_set_count_add_batch_device into a new table counter, one batch) + tab_select (finish)
  d_shards_list     the count files of the two halves of the reads: two loads, add, finish -- wall time of each step
  e_shards_table    the same two files loaded into one table counter, finish
  count_merge       the add of (d) under the profile timer: ms, and GB/s of operand + result bytes (9 per entry)
  kernels           the brx_profile_* timers of one more run of (a) and of (d)
  equal             the fingerprints of the sets of (a), (b), (d), (e) against (c)'s, and the spectrum of the list against
                    the table counter's

The files go to --dir (default: /dev/shm where there is one, else the temporary directory) and are removed.

    python tools/countlist_bench.py [--reads 100000] [--repeat 5] [--out profiles/countlist_bench.json]
"""
import argparse
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
    ap.add_argument("-k", type=int, default=25)
    ap.add_argument("--abundance", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--dir", default=None, help="where the files are written (default: /dev/shm, else the temporary directory)")
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

    def batch(first, n):
        cap = int(n * read_len * 1.03) + (1 << 20)
        d_bases = torch.empty(cap, dtype=torch.uint8, device="cuda")
        d_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        total = synth.reads_device(cfg, dev, d_genome.data_ptr(), first, n, d_bases.data_ptr(), cap, d_off.data_ptr(), stream)
        torch.cuda.synchronize()
        return d_bases, d_off, n, total

    whole = batch(0, n_reads)
    gbp = whole[3] / 1e9

    def spread(xs):
        return {"median": round(statistics.median(xs) / gbp, 3), "min": round(min(xs) / gbp, 3), "max": round(max(xs) / gbp, 3)}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def counted(b):
        cnt = br_amd.Counter(k, dev, _lib.COUNT_TABLE)
        ms, _ = wall(lambda: cnt.add_batch_device(b[0].data_ptr(), b[1].data_ptr(), b[2], b[3], stream))
        return cnt, ms

    def profiled(fn):
        _lib.profile_enable(True)
        _lib.profile_reset()
        fn()
        torch.cuda.synchronize()
        prof = {nm: round(v["total_ms"] / gbp, 3) for nm, v in _lib.profile_all().items() if v["launches"]}
        _lib.profile_enable(False)
        return prof

    tmp = tempfile.mkdtemp(prefix="countlist_bench_", dir=args.dir or ("/dev/shm" if os.path.isdir("/dev/shm") else None))
    paths = {name: os.path.join(tmp, name + ".keys") for name in ("whole", "half0", "half1")}
    try:
        # (c) counting again, a new counter every time; the last one writes the whole job's file
        t_count, t_select = [], []
        for i in range(args.repeat + 1):
            cnt = gs = None
            cnt, ms_c = counted(whole)
            ms_s, gs = wall(lambda: cnt.finish(a, stream))
            if i:
                t_count.append(ms_c)
                t_select.append(ms_s)
        fp, spec = gs.fingerprint(), cnt.spectrum()
        with open(paths["whole"], "wb") as f:
            whole_stats = cnt.save(f)
        cnt = gs = None
        half = n_reads // 2
        for name, first, n in (("half0", 0, half), ("half1", half, n_reads - half)):
            b = batch(first, n)
            cnt, _ = counted(b)
            with open(paths[name], "wb") as f:
                cnt.save(f)
            cnt = b = None
        whole = None

        def load_list(path):
            with open(path, "rb") as f:
                return br_amd.CountList.from_keyfile(f, dev)

        def load_table(cnt, path):
            with open(path, "rb") as f:
                return cnt.load(f)

        # (a) the list route and (b) the table route, over the same file
        rows_a, rows_b = [], []
        same = {}
        for i in range(args.repeat + 1):
            ms_l, lst = wall(lambda: load_list(paths["whole"]))
            ms_f, gs = wall(lambda: lst.finish(a))
            if i:
                rows_a.append({"fd": lst.keyfile_stats["ns_fd"] / 1e6, "unpack": lst.keyfile_stats["ns_pack"] / 1e6,
                               "select": gs.finish_stats["ns_select"] / 1e6, "set_build": gs.finish_stats["ns_build"] / 1e6,
                               "load_wall": ms_l, "finish_wall": ms_f, "total": ms_l + ms_f})
            else:
                same["a_fingerprint"] = gs.fingerprint() == fp
                same["list_spectrum"] = bool(np.array_equal(lst.spectrum(), spec))
                entries = lst.n
            lst = gs = None
            cnt = br_amd.Counter(k, dev, _lib.COUNT_TABLE)
            ms_l, _ = wall(lambda: load_table(cnt, paths["whole"]))
            ms_f, gs = wall(lambda: cnt.finish(a, stream))
            if i:
                rows_b.append({"load_wall": ms_l, "finish_wall": ms_f, "total": ms_l + ms_f})
            else:
                same["b_fingerprint"] = gs.fingerprint() == fp
            cnt = gs = None

        # (d) two shards as lists and (e) into one table
        rows_d, rows_e, merge = [], [], {}
        for i in range(args.repeat + 1):
            ms_l0, l0 = wall(lambda: load_list(paths["half0"]))
            ms_l1, l1 = wall(lambda: load_list(paths["half1"]))
            ms_add, both = wall(lambda: l0 + l1)
            ms_f, gs = wall(lambda: both.finish(a))
            if i:
                rows_d.append({"loads": ms_l0 + ms_l1, "add": ms_add, "finish": ms_f, "total": ms_l0 + ms_l1 + ms_add + ms_f})
            else:
                same["d_fingerprint"] = gs.fingerprint() == fp
                same["d_entries"] = both.n == entries
                merge = {"a": l0.n, "b": l1.n, "both": both.combine_stats["both"], "result": both.n}
            l0 = l1 = both = gs = None
            cnt = br_amd.Counter(k, dev, _lib.COUNT_TABLE)
            ms_l0, _ = wall(lambda: load_table(cnt, paths["half0"]))
            ms_l1, _ = wall(lambda: load_table(cnt, paths["half1"]))
            ms_f, gs = wall(lambda: cnt.finish(a, stream))
            if i:
                rows_e.append({"loads": ms_l0 + ms_l1, "finish": ms_f, "total": ms_l0 + ms_l1 + ms_f})
            else:
                same["e_fingerprint"] = gs.fingerprint() == fp
            cnt = gs = None

        # the merge alone, under its timer
        l0, l1 = load_list(paths["half0"]), load_list(paths["half1"])
        merge_ms = []
        for i in range(args.repeat + 1):
            _lib.profile_enable(True)
            _lib.profile_reset()
            both = l0 + l1
            torch.cuda.synchronize()
            ms = _lib.profile_all()["count_merge"]["total_ms"]
            _lib.profile_enable(False)
            both = None
            if i:
                merge_ms.append(ms)
        l0 = l1 = None
        merge_bytes = 9 * (merge["a"] + merge["b"] + merge["result"])
        merge["ms_per_gbp"] = spread(merge_ms)
        merge["gb_per_s"] = round(merge_bytes / 1e9 / (statistics.median(merge_ms) / 1e3), 1)
        kernels = {"a_list_route": profiled(lambda: load_list(paths["whole"]).finish(a)),
                   "d_shards_list": profiled(lambda: (load_list(paths["half0"]) + load_list(paths["half1"])).finish(a))}
    finally:
        for p in paths.values():
            if os.path.exists(p):
                os.remove(p)
        os.rmdir(tmp)

    def legs(rows):
        return {key: spread([r[key] for r in rows]) for key in rows[0]}

    out = {"tool": "countlist_bench",
           "workload": "%d synthetic %d bp reads, %dx, k=%d, abundance %d, device-resident" % (n_reads, read_len, args.coverage, k, a),
           "bases": int(round(gbp * 1e9)), "entries": entries, "file_bytes": whole_stats["bytes"],
           "unit": "ms per Gbp of reads, median (min, max) of %d" % args.repeat,
           "a_list_route": legs(rows_a), "b_table_route": legs(rows_b),
           "c_count_again": {"tab_count": spread(t_count), "tab_select": spread(t_select),
                             "total": spread([x + y for x, y in zip(t_count, t_select)])},
           "d_shards_list": legs(rows_d), "e_shards_table": legs(rows_e), "count_merge": merge, "kernels": kernels,
           "a_over_b": round(statistics.median(r["total"] for r in rows_a) / statistics.median(r["total"] for r in rows_b), 4),
           "d_over_e": round(statistics.median(r["total"] for r in rows_d) / statistics.median(r["total"] for r in rows_e), 4),
           "equal": {key: bool(v) for key, v in same.items()}}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
