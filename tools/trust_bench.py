#!/usr/bin/env python3
"""Trusted stretches (include/brx.h "trusted stretches", br_amd/csrc/brx_trust.hip) on bench.py's configs[1] workload: 1e5
synthetic 10 kb reads at 50x, device-resident, with synthetic qualities (seeded: 1 % of the bases at Q2..Q19, the rest at
Q30..Q41) and 0.1 % of the bases turned into N.  Prints ONE JSON line:

  trust        the split call with -q 20, ACGT only, min_len = k: ms per Gbp of the profile timers "trust" (work list, pass 1,
               scans, pass 2) and "trust_copy" (keep, layout scans, copy, piece statistics), and of the whole call by HIP
               events (its own synchronisations and size read-backs included), best of --repeat; pieces and bytes kept
  cover_split  the yardstick, in the same process on the same batch: brx_set_cover_split_batch_device (min_len 0) against
               the set counted from the batch at k, abundance 3 -- timers "cover_tiles", "cover", "cover_runs", "cover_copy"
               and the whole call
  count        (--pipeline-reads N > 0) the first N reads as files in /dev/shm: Counter.count_reads(fastq, -q 20) against
               Counter.count_fasta of the same sequences at k = 19 and k = 25, seconds each, the slower of two runs after a
               warm-up, and the trust totals

    python tools/trust_bench.py [--reads 100000] [--repeat 3] [--pipeline-reads 20000]
"""
import argparse
import json
import os
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
    ap.add_argument("-k", type=int, default=19)
    ap.add_argument("--abundance", type=int, default=3)
    ap.add_argument("--min-quality", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--pipeline-reads", type=int, default=0)
    args = ap.parse_args()

    import ctypes as C
    import torch
    import br_amd
    from br_amd import _lib, synth
    from br_amd.set import trust_split_batch_device

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
    del d_genome
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20)
    d_quals = torch.empty(total, dtype=torch.uint8, device="cuda")
    step = 1 << 27
    for at in range(0, total, step):  # (in slices: the random draws are four bytes a base)
        m = min(step, total - at)
        u = torch.rand(m, generator=gen, device="cuda")
        v = torch.rand(m, generator=gen, device="cuda")
        d_quals[at:at + m] = torch.where(u < 0.01, 35 + (v * 18).to(torch.uint8), 63 + (v * 12).to(torch.uint8))
        d_bases[at:at + m][torch.rand(m, generator=gen, device="cuda") < 0.001] = ord("N")
        del u, v
    counter = br_amd.Counter(k, dev)
    counter.add_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, total, stream)
    gs = counter.finish(a, stream)
    del counter
    torch.cuda.synchronize()

    piece_cap = n_reads + total // (k + 1)
    d_out = torch.empty(total, dtype=torch.uint8, device="cuda")
    d_poff = torch.empty(piece_cap + 1, dtype=torch.int64, device="cuda")
    d_pread = torch.empty(piece_cap, dtype=torch.int32, device="cuda")
    d_pstart = torch.empty(piece_cap, dtype=torch.int64, device="cuda")
    d_stats = torch.empty((n_reads, 5), dtype=torch.int32, device="cuda")
    gbp = total / 1e9

    def timed(fn):
        best = None
        for _ in range(args.repeat):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            best = ms if best is None else min(best, ms)
        return best

    def profiled(fn, names):
        _lib.profile_enable(True)
        _lib.profile_reset()
        fn()
        torch.cuda.synchronize()
        prof = _lib.profile_all()
        _lib.profile_enable(False)
        return {nm: round(prof.get(nm, {}).get("total_ms", 0.0) / gbp, 3) for nm in names}

    sizes = {}

    def trust_call():
        sizes["trust"] = trust_split_batch_device(d_bases.data_ptr(), d_quals.data_ptr(), d_off.data_ptr(), n_reads, total, args.min_quality,
                                                  True, k, d_out.data_ptr(), total, d_poff.data_ptr(), d_pread.data_ptr(),
                                                  d_pstart.data_ptr(), piece_cap, d_stats.data_ptr(), dev, stream)
    np_, tot_ = C.c_uint32(0), C.c_uint64(0)

    def cover_call():
        _lib.check(_lib.lib().brx_set_cover_split_batch_device(gs._h, d_bases.data_ptr(), d_off.data_ptr(), n_reads, total, 0,
                                                               d_out.data_ptr(), d_out.numel(), d_poff.data_ptr(), d_pread.data_ptr(),
                                                               d_pstart.data_ptr(), piece_cap, C.byref(np_), C.byref(tot_), stream))
    trust_call()  # warm-up: the pool's blocks
    cover_call()
    res = {"tool": "trust_bench",
           "workload": "configs[1]: %d synthetic %d bp reads, %dx, k=%d, device-resident; 1 %% of the bases at Q2..Q19, 0.1 %% N; -q %d"
                       % (n_reads, read_len, args.coverage, k, args.min_quality),
           "bases": int(total)}
    t = profiled(trust_call, ("trust", "trust_copy"))
    res["trust"] = {"ms_per_gbp": dict(t, whole_call=round(timed(trust_call) / gbp, 3)), "pieces": sizes["trust"][0],
                    "bytes_kept": sizes["trust"][1]}
    s = d_stats.cpu().numpy().astype("int64").sum(axis=0)
    res["trust"]["totals"] = dict(zip(("bases", "non_acgt", "low_quality", "pieces", "kept_bases"), (int(x) for x in s)))
    c = profiled(cover_call, ("cover_tiles", "cover", "cover_runs", "cover_copy"))
    res["cover_split"] = {"ms_per_gbp": dict(c, whole_call=round(timed(cover_call) / gbp, 3)), "pieces": np_.value, "bytes_kept": tot_.value,
                          "abundance": a}
    res["trust_over_cover_split"] = {"timers": round(sum(t.values()) / max(sum(c.values()), 1e-9), 4),
                                     "whole_call": round(res["trust"]["ms_per_gbp"]["whole_call"] /
                                                         max(res["cover_split"]["ms_per_gbp"]["whole_call"], 1e-9), 4)}
    if args.pipeline_reads > 0:
        res["count"] = count_files(args, d_bases, d_quals, d_off, min(args.pipeline_reads, n_reads))
    print(json.dumps(res))


def count_files(args, d_bases, d_quals, d_off, n):
    import br_amd
    tmp = "/dev/shm" if os.path.isdir("/dev/shm") else "/tmp"
    fq = os.path.join(tmp, "brx_trust_bench_%d.fastq" % os.getpid())
    fa = os.path.join(tmp, "brx_trust_bench_%d.fasta" % os.getpid())
    ho = d_off[:n + 1].cpu().numpy()
    tot = int(ho[n])
    hb, hq = d_bases[:tot].cpu().numpy(), d_quals[:tot].cpu().numpy()
    out = {"reads": n, "bases": tot}
    try:
        with open(fq, "wb") as f, open(fa, "wb") as g:
            for r in range(n):
                s = hb[int(ho[r]):int(ho[r + 1])].tobytes()
                f.write(b"@r%d\n%s\n+\n%s\n" % (r, s, hq[int(ho[r]):int(ho[r + 1])].tobytes()))
                g.write(b">r%d\n%s\n" % (r, s))
        for k in (19, 25):
            row = {}
            for rnd in range(3):  # the first round warms the pools; the slower of the other two counts
                for name, path in (("count_fasta", fa), ("count_reads_fastq", fq)):
                    c = br_amd.Counter(k)
                    t0 = time.perf_counter()
                    with open(path, "rb") as f:
                        st = c.count_fasta(f) if name == "count_fasta" else c.count_reads(f, "fastq", args.min_quality, True)
                    dt = time.perf_counter() - t0
                    if rnd:
                        row[name + "_s"] = round(max(dt, row.get(name + "_s", dt)), 4)
                        if "trust" in st:
                            row["trust_totals"] = st["trust"]
                    del c
            row["fastq_over_fasta"] = round(row["count_reads_fastq_s"] / row["count_fasta_s"], 4)
            out["k%d" % k] = row
    finally:
        for p in (fq, fa):
            if os.path.exists(p):
                os.remove(p)
    return out


if __name__ == "__main__":
    main()
