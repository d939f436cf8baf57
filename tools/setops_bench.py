#!/usr/bin/env python3
"""Set algebra on bench.py's synthetic workload (10 kb reads at 50x of a uniform random genome, device-resident, one batch)
at k = 19 and k = 25, all legs in ONE process.  A is the solid set of all reads (count > --abundance at k = 19, count > 3 at
k = 25), B the solid set of the second half of the reads under the same threshold.  ONE JSON line, ms per call, median of
--repeat:

  ops             union / intersection / difference / symmetric_difference (Pcon.combine) and compare:
                    stats8      list_sort, merge, build, wall -- the library's own clocks
                    kernels     the brx_profile_* timers of --repeat more calls: key_list, key_sort, set_merge and whatever
                                the build of the result launches
                    merge_gbps  set_merge over 8 (|A| + |B|) 2 + 8 |out| bytes (both passes read both lists)
  chained_difference  (A | B) - (A & B): the shapes of "difference" with both operands' key lists marked as sorted (results of
                  combines), so what the mark saves is the difference between the two rows
  key_sort_ms     what sorting the same keys costs inside those calls (both operands), from the same timers
  file_round_trip Pcon.save_keys + Pcon.from_keyfile of A alone through a file in memory (--dir, default /dev/shm where it
                  exists): combining two sets without this feature costs at least that twice, plus the host's merge

    python tools/setops_bench.py [--reads 100000] [--repeat 5] [--out profiles/setops_bench.json]
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
    ap.add_argument("--abundance", type=int, default=3, help="bench.py's threshold, used at k = 19")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--dir", default=None, help="where the round-trip file is written (default: /dev/shm, else the temporary directory)")
    ap.add_argument("--out", default="", help="also write the line to this file")
    args = ap.parse_args()

    import torch
    import br_amd
    from br_amd import _lib, setops, synth

    dev = 0
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream().cuda_stream
    n_reads, read_len = args.reads, args.read_len
    genome_len = max(n_reads * read_len // args.coverage, read_len)
    cfg = synth.config(genome_len=genome_len, read_len=read_len)
    d_genome = torch.empty(genome_len, dtype=torch.uint8, device="cuda")
    synth.genome_device(cfg, dev, d_genome.data_ptr(), stream)

    def reads(first, count):
        cap = int(count * read_len * 1.03) + (1 << 20)
        d_bases = torch.empty(cap, dtype=torch.uint8, device="cuda")
        d_off = torch.empty(count + 1, dtype=torch.int64, device="cuda")
        total = synth.reads_device(cfg, dev, d_genome.data_ptr(), first, count, d_bases.data_ptr(), cap, d_off.data_ptr(), stream)
        torch.cuda.synchronize()
        return d_bases, d_off, count, total

    batch_all, batch_half = reads(0, n_reads), reads(n_reads // 2, n_reads - n_reads // 2)
    med = lambda xs: round(statistics.median(xs), 3)

    def solid(k, a, batch):
        d_bases, d_off, count, total = batch
        cnt = br_amd.Counter(k, dev)
        cnt.add_batch_device(d_bases.data_ptr(), d_off.data_ptr(), count, total, stream)
        gs = cnt.finish(a, stream)
        torch.cuda.synchronize()
        return gs

    def profiled(fn):
        _lib.profile_enable(True)
        _lib.profile_reset()
        fn()
        torch.cuda.synchronize()
        prof = {nm: v["total_ms"] for nm, v in _lib.profile_all().items() if v["launches"]}
        _lib.profile_enable(False)
        return prof

    tmp_root = args.dir or ("/dev/shm" if os.path.isdir("/dev/shm") else None)
    per_k = {}
    for k, a in ((19, args.abundance), (25, 3)):
        A, B = solid(k, a, batch_all), solid(k, a, batch_half)
        res = {"threshold": a, "forms": {"a": A.bits_state(), "b": B.bits_state()}, "ops": {}}
        sort_ms = []
        for op in list(setops.OPS) + ["compare"]:
            call = (lambda: A.compare(B)) if op == "compare" else (lambda: A.combine(B, op))
            stats, walls, profs, out = [], [], [], None
            for i in range(args.repeat + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = call()
                ms = (time.perf_counter() - t0) * 1e3
                if i:
                    walls.append(ms)
                    if op != "compare":
                        stats.append(out.combine_stats)
            for i in range(args.repeat):
                profs.append(profiled(call))
            names = sorted(set().union(*profs))
            kernels = {nm: med([p.get(nm, 0.0) for p in profs]) for nm in names}
            sort_ms.append(kernels.get("key_sort", 0.0))
            if op == "compare":
                na, nb, n_out = out["a"], out["b"], 0
                entry = {"a": na, "b": nb, "both": out["both"], "jaccard": round(out["jaccard"], 6), "wall": med(walls)}
                merge_bytes = 8 * (na + nb)  # pass 1 alone
            else:
                st = stats[-1]
                na, nb, n_out = st["a"], st["b"], st["keys"]
                entry = {"a": na, "b": nb, "both": st["both"], "keys": n_out,
                         "stats8": {key: med([s["ns_" + key] / 1e6 for s in stats]) for key in ("list_sort", "merge", "build", "wall")},
                         "wall": med(walls)}
                merge_bytes = 8 * (na + nb) * 2 + 8 * n_out
            entry["kernels"] = kernels
            entry["merge_gbps"] = round(merge_bytes / (kernels["set_merge"] * 1e-3) / 1e9, 1) if kernels.get("set_merge") else None
            res["ops"][op] = entry
            out = None
        res["key_sort_ms"] = med(sort_ms)
        # operands whose key lists are known to be in order (results of combines): the same difference without the sorts
        U, I = A.combine(B, "union"), A.combine(B, "intersection")
        stats, profs = [], []
        for i in range(args.repeat + 1):
            out = U.combine(I, "difference")
            if i:
                stats.append(out.combine_stats)
        for i in range(args.repeat):
            profs.append(profiled(lambda: U.combine(I, "difference")))
        res["chained_difference"] = {
            "a": stats[-1]["a"], "b": stats[-1]["b"], "keys": stats[-1]["keys"],
            "stats8": {key: med([s["ns_" + key] / 1e6 for s in stats]) for key in ("list_sort", "merge", "build", "wall")},
            "kernels": {nm: med([p.get(nm, 0.0) for p in profs]) for nm in sorted(set().union(*profs))}}
        U = I = out = None
        # what the only route costs today, for A alone: its key file written and read back through memory
        tmp = tempfile.mkdtemp(prefix="setops_bench_", dir=tmp_root)
        path = os.path.join(tmp, "a.keys")
        saves, loads = [], []
        try:
            for i in range(args.repeat + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with open(path, "wb") as f:
                    A.save_keys(f)
                t1 = time.perf_counter()
                with open(path, "rb") as f:
                    back = br_amd.Pcon.from_keyfile(f, dev)
                t2 = time.perf_counter()
                if i:
                    saves.append((t1 - t0) * 1e3)
                    loads.append((t2 - t1) * 1e3)
            same = back.fingerprint() == A.fingerprint()
            back = None
            size = os.path.getsize(path)
        finally:
            if os.path.exists(path):
                os.remove(path)
            os.rmdir(tmp)
        res["file_round_trip"] = {"save": med(saves), "load": med(loads), "total": round(med(saves) + med(loads), 3), "bytes": size,
                                  "fingerprint_equal": bool(same)}
        per_k["k%d" % k] = res
        A = B = None

    out = {"tool": "setops_bench",
           "workload": "%d synthetic %d bp reads, %dx, device-resident, one batch; B = the second half of the reads" % (n_reads, read_len, args.coverage),
           "unit": "ms per call, median of %d" % args.repeat, "tile": setops.TILE, "per_thread": setops.PER_THREAD}
    out.update(per_k)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
