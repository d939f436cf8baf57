#!/usr/bin/env python3
"""Key files against counting the reads again, on bench.py's synthetic workload (10 kb reads at 50x of a uniform random
genome, device-resident, one batch) at k = 25, all legs in ONE process.  ONE JSON line, ms per Gbp of reads, median of
--repeat:

  counted_build   tab_count (brx_set_count_add_batch_device into a new BRX_COUNT_TABLE counter) + tab_select (finish with
                  --abundance): what every run pays today, the yardstick
  count_file      Counter.save: list + sort, pack, fd write (the library's own clocks, stats8), and the wall time
                  Counter.from_keyfile: fd read, unpack, merge into the table, and the wall time; then finish
  set_file        the same for the set finished above (Pcon.save_keys / Pcon.from_keyfile)
  kernels         the brx_profile_* timers of one more save and one more load
  bytes_per_key   of both files against the raw 9 (key + count) and 8 (key)
  round_trip      fingerprint of the finished set and the spectrum: loaded counter against the counted one

The files go to --dir (default: the system's temporary directory) and are removed.

    python tools/keyfile_bench.py [--reads 100000] [--repeat 5] [--out profiles/keyfile_bench.json]
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
    ap.add_argument("--dir", default=None, help="where the files are written (default: the temporary directory)")
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
    med = lambda xs: round(statistics.median(xs) / gbp, 3)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    # the yardstick: count the reads and select, a new counter every time as a run of the command line does
    t_count, t_select = [], []
    cnt = gs = None
    for i in range(args.repeat + 1):
        cnt = gs = None
        cnt = br_amd.Counter(k, dev, _lib.COUNT_TABLE)
        ms_c, _ = wall(lambda: cnt.add_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, total, stream))
        ms_s, gs = wall(lambda: cnt.finish(a, stream))
        if i:
            t_count.append(ms_c)
            t_select.append(ms_s)
    spec, fp = cnt.spectrum(), gs.fingerprint()

    def phases(stats):
        return {"list_sort": stats["ns_list_sort"] / 1e6, "pack_or_unpack": stats["ns_pack"] / 1e6, "fd": stats["ns_fd"] / 1e6,
                "wall": stats["ns_wall"] / 1e6}

    def profiled(fn):
        _lib.profile_enable(True)
        _lib.profile_reset()
        fn()
        torch.cuda.synchronize()
        prof = {nm: round(v["total_ms"] / gbp, 3) for nm, v in _lib.profile_all().items() if v["launches"]}
        _lib.profile_enable(False)
        return prof

    def file_leg(path, save, load, after_load=None):
        saves, loads, afters, st, obj = [], [], [], None, None
        for i in range(args.repeat + 1):
            with open(path, "wb") as f:
                st = save(f)
            obj = None
            with open(path, "rb") as f:
                ms_l, obj = wall(lambda: load(f))
            ms_a = wall(lambda: after_load(obj))[0] if after_load else 0.0
            if i:
                saves.append(phases(st))
                loads.append((ms_l, obj.keyfile_stats if hasattr(obj, "keyfile_stats") else obj.load_stats))
                afters.append(ms_a)
        res = {"keys": st["keys"], "bytes": st["bytes"], "blocks": st["blocks"], "max_width": st["max_width"],
               "save": {key: med([s[key] for s in saves]) for key in saves[0]},
               "load": {"fd": med([s["ns_fd"] / 1e6 for _, s in loads]), "unpack": med([s["ns_pack"] / 1e6 for _, s in loads]),
                        "merge_or_build": med([s["ns_list_sort"] / 1e6 for _, s in loads]), "wall": med([ms for ms, _ in loads])}}
        if after_load:
            res["finish_after_load"] = med(afters)
        with open(path, "wb") as f:
            res["save_kernels"] = profiled(lambda: save(f))
        with open(path, "rb") as f:
            res["load_kernels"] = profiled(lambda: load(f))
        return res, obj

    def load_counter(f):
        c = br_amd.Counter(k, dev, _lib.COUNT_TABLE)
        c.load_stats = c.load(f)
        return c

    tmp = tempfile.mkdtemp(prefix="keyfile_bench_", dir=args.dir)
    cpath, spath = os.path.join(tmp, "counts.keys"), os.path.join(tmp, "set.keys")
    try:
        count_res, back = file_leg(cpath, cnt.save, load_counter, lambda c: c.finish(a, stream))
        same_spec = bool(np.array_equal(back.spectrum(), spec))
        same_fp = back.finish(a).fingerprint() == fp
        back = None
        set_res, back_set = file_leg(spath, gs.save_keys, lambda f: br_amd.Pcon.from_keyfile(f, dev))
        same_set = back_set.fingerprint() == fp
        back_set = None
    finally:
        for p in (cpath, spath):
            if os.path.exists(p):
                os.remove(p)
        os.rmdir(tmp)
    counted = {"tab_count": med(t_count), "tab_select": med(t_select)}
    counted["total"] = round(counted["tab_count"] + counted["tab_select"], 3)
    reload_total = round(count_res["load"]["wall"] + count_res["finish_after_load"], 3)
    out = {"tool": "keyfile_bench",
           "workload": "%d synthetic %d bp reads, %dx, k=%d, abundance %d, device-resident, one batch" % (n_reads, read_len, args.coverage, k, a),
           "bases": int(total), "unit": "ms per Gbp of reads, median of %d" % args.repeat,
           "counted_build": counted, "count_file": count_res, "set_file": set_res,
           "load_plus_finish": reload_total, "load_plus_finish_over_counted_build": round(reload_total / counted["total"], 4),
           "set_load_over_counted_build": round(set_res["load"]["wall"] / counted["total"], 4),
           "bytes_per_key": {"count_file": round(count_res["bytes"] / max(count_res["keys"], 1), 3), "raw_pairs": 9,
                             "set_file": round(set_res["bytes"] / max(set_res["keys"], 1), 3), "raw_keys": 8},
           "round_trip": {"spectrum_equal": same_spec, "finish_fingerprint_equal": bool(same_fp), "set_fingerprint_equal": bool(same_set)}}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
