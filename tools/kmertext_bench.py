#!/usr/bin/env python3
"""K-mer text against the key file, on the count list of bench.py's synthetic workload (10 kb reads at 50x of a uniform random
genome, device-resident) at k = 25, all legs in ONE process.  ONE JSON line, ms per Gbp of reads, median of --repeat with the
spread (min .. max) beside it:

  dump        CountList.dump_text to a file: the host's wait for the device (formatting and copies that the fd does not
              hide), the fd, the wall time
  import      CountList.from_text of that file (lines in key order: the sort is skipped): parsing, sorting + summing, the fd,
              the wall time
  save, load  CountList.save / CountList.from_keyfile of the same list: the yardstick
  kernels     the brx_profile_* timers of one more dump and one more import
  expectation text_format below the dump's fd time, text_parse + text_runsum below the import's fd time
  equal       the imported list against the original: entries, spectrum, the fingerprint of finish(abundance)

The files go to --dir (default: /dev/shm where it has room for them, else the temporary directory) and are removed.

    python tools/kmertext_bench.py [--reads 100000] [--repeat 5] [--out profiles/kmertext_bench.json]
"""
import argparse
import json
import os
import shutil
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
    cap = int(n_reads * read_len * 1.03) + (1 << 20)
    d_bases = torch.empty(cap, dtype=torch.uint8, device="cuda")
    d_off = torch.empty(n_reads + 1, dtype=torch.int64, device="cuda")
    total = synth.reads_device(cfg, dev, d_genome.data_ptr(), 0, n_reads, d_bases.data_ptr(), cap, d_off.data_ptr(), stream)
    torch.cuda.synchronize()
    gbp = total / 1e9
    cnt = br_amd.Counter(k, dev, _lib.COUNT_TABLE)
    cnt.add_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, total, stream)
    torch.cuda.synchronize()
    lst = br_amd.CountList.from_counter(cnt)
    cnt = d_bases = d_off = d_genome = None
    entries = lst.n
    spec, fp = lst.spectrum(), lst.finish(a).fingerprint()

    def spread(xs):
        return {"median": round(statistics.median(xs) / gbp, 3), "min": round(min(xs) / gbp, 3), "max": round(max(xs) / gbp, 3)}

    def legs(rows):
        return {key: spread([r[key] for r in rows]) for key in rows[0]}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def profiled(fn):
        _lib.profile_enable(True)
        _lib.profile_reset()
        fn()
        torch.cuda.synchronize()
        prof = {nm: round(v["total_ms"] / gbp, 3) for nm, v in _lib.profile_all().items() if v["launches"]}
        _lib.profile_enable(False)
        return prof

    need = entries * (k + 6) + entries * 10  # the text and the key file, generously
    where = args.dir
    if not where:
        where = "/dev/shm" if os.path.isdir("/dev/shm") and shutil.disk_usage("/dev/shm").free > need else None
    tmp = tempfile.mkdtemp(prefix="kmertext_bench_", dir=where)
    text, keys = os.path.join(tmp, "list.tsv"), os.path.join(tmp, "list.keys")

    def dump():
        with open(text, "wb") as f:
            return lst.dump_text(f)

    def save():
        with open(keys, "wb") as f:
            return lst.save(f)

    def imported():
        with open(text, "rb") as f:
            return br_amd.CountList.from_text(f, None, 1, dev)

    def loaded():
        with open(keys, "rb") as f:
            return br_amd.CountList.from_keyfile(f, dev)

    try:
        rows = {"dump": [], "import": [], "save": [], "load": []}
        same = {}
        for i in range(args.repeat + 1):
            for p in (text, keys):  # (truncating the file of the repetition before is not part of a dump)
                if os.path.exists(p):
                    os.remove(p)
            ms, st = wall(dump)
            if i:
                rows["dump"].append({"device_wait": st["ns_format"] / 1e6, "fd": st["ns_fd"] / 1e6, "wall": ms})
            text_bytes = st["bytes"]
            ms, st = wall(save)
            if i:
                rows["save"].append({"pack": st["ns_pack"] / 1e6, "fd": st["ns_fd"] / 1e6, "wall": ms})
            file_bytes = st["bytes"]
            ms, back = wall(imported)
            st = back.text_stats
            if i:
                rows["import"].append({"parse": st["ns_parse"] / 1e6, "sort_sum": st["ns_sort_sum"] / 1e6, "fd": st["ns_fd"] / 1e6, "wall": ms})
            else:
                same = {"entries": back.n == entries, "k": back.k == k, "sort_skipped": not st["sorted"],
                        "spectrum": bool(np.array_equal(back.spectrum(), spec)), "fingerprint": back.finish(a).fingerprint() == fp}
            back = None
            ms, back = wall(loaded)
            st = back.keyfile_stats
            if i:
                rows["load"].append({"unpack": st["ns_pack"] / 1e6, "fd": st["ns_fd"] / 1e6, "wall": ms})
            back = None
            print("repetition %d of %d done" % (i, args.repeat), file=sys.stderr, flush=True)
        kernels = {"dump": profiled(dump), "import": profiled(imported)}
    finally:
        for p in (text, keys):
            if os.path.exists(p):
                os.remove(p)
        os.rmdir(tmp)

    res = {name: legs(r) for name, r in rows.items()}
    kd, ki = kernels["dump"], kernels["import"]
    expectation = {"text_format_below_dump_fd": kd.get("text_format", 0.0) < res["dump"]["fd"]["median"],
                   "text_parse_and_runsum_below_import_fd": ki.get("text_parse", 0.0) + ki.get("text_runsum", 0.0) < res["import"]["fd"]["median"]}
    out = {"tool": "kmertext_bench",
           "workload": "%d synthetic %d bp reads, %dx, k=%d, device-resident; files in %s" % (n_reads, read_len, args.coverage, k,
                                                                                             where or tempfile.gettempdir()),
           "bases": int(round(gbp * 1e9)), "entries": entries, "text_bytes": text_bytes, "file_bytes": file_bytes,
           "unit": "ms per Gbp of reads, median (min, max) of %d" % args.repeat,
           "dump": res["dump"], "import": res["import"], "save": res["save"], "load": res["load"], "kernels": kernels,
           "expectation": expectation, "dump_over_save": round(res["dump"]["wall"]["median"] / res["save"]["wall"]["median"], 3),
           "import_over_load": round(res["import"]["wall"]["median"] / res["load"]["wall"]["median"], 3),
           "equal": {key: bool(v) for key, v in same.items()}}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
