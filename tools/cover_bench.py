#!/usr/bin/env python3
"""Solid coverage (include/brx.h "coverage", br_amd/csrc/brx_cover.hip) on bench.py's configs[1] workload: 1e5 synthetic
10 kb reads at 50x, k = 19, abundance 3, device-resident.  Prints ONE JSON line:

  ms_per_gbp         the flags + stats call, the masked call (in place) and the split call (min_len 0), by HIP events
                     around the whole call (work list, kernels, the call's own synchronisation), best of --repeat
  fractions          solid k-mers / k-mers and covered bases / bases, before and after correct::one (forward + reverse)
  kernel             the cover kernel alone (profile timer "cover") against lane_mask_kernel<true> (timer "lane_mask") of
                     a Graph forward pass of this process on the same batch: both ask one probe per position through the
                     probe index; ns per position and their ratio
  pipeline           (--pipeline-reads N > 0) FASTA -> FASTA through run_correction on the first N reads, /dev/shm: plain,
                     mask and split, Gbases/s each in this one call, the slower of two runs

    python tools/cover_bench.py [--reads 100000] [--repeat 3] [--pipeline-reads 20000]
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
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--pipeline-reads", type=int, default=0)
    args = ap.parse_args()

    import ctypes as C
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
    del d_genome
    counter = br_amd.Counter(k, dev)
    counter.add_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, total, stream)
    gs = counter.finish(a, stream)
    del counter
    d_out = torch.empty(int(total * 1.05) + (1 << 20), dtype=torch.uint8, device="cuda")
    d_out_off = torch.empty(n_reads + 1, dtype=torch.int64, device="cuda")
    chain = br_amd.Chain(gs, [("one", 5, 7)], two_side=False)
    out_total = chain.correct_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, total, d_out.data_ptr(), d_out.numel(),
                                           d_out_off.data_ptr(), stream)
    torch.cuda.synchronize()
    bits_state = gs.bits_state()  # (1: the cover calls below answer from the key list's probe index, the bit vector unwritten)

    d_flags = torch.empty(max(total, out_total), dtype=torch.uint8, device="cuda")
    d_stats = torch.empty((n_reads, 4), dtype=torch.int32, device="cuda")
    d_scratch = torch.empty(max(total, out_total), dtype=torch.uint8, device="cuda")
    piece_cap = n_reads + total // (k + 1)
    d_poff = torch.empty(piece_cap + 1, dtype=torch.int64, device="cuda")
    d_pread = torch.empty(piece_cap, dtype=torch.int32, device="cuda")
    d_pstart = torch.empty(piece_cap, dtype=torch.int64, device="cuda")

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

    def stats_of(bases, offs, tot):
        gs.cover_batch_device(bases.data_ptr(), offs.data_ptr(), n_reads, tot, None, None, d_stats.data_ptr(), stream)
        torch.cuda.synchronize()
        s = d_stats.cpu().numpy().view(np.uint32).astype(np.int64).sum(axis=0)
        return {"bases": int(tot), "kmers": int(s[0]), "solid": int(s[1]), "covered": int(s[2]), "runs": int(s[3]),
                "solid_fraction": round(float(s[1]) / max(int(s[0]), 1), 5), "covered_fraction": round(float(s[2]) / max(tot, 1), 5)}

    gbp = total / 1e9
    gs.cover_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, total, d_flags.data_ptr(), None, d_stats.data_ptr(), stream)  # warm-up
    ms_flags = timed(lambda: gs.cover_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, total, d_flags.data_ptr(), None,
                                                   d_stats.data_ptr(), stream))
    d_scratch[:total].copy_(d_bases[:total])
    ms_mask = timed(lambda: gs.cover_batch_device(d_scratch.data_ptr(), d_off.data_ptr(), n_reads, total, None, d_scratch.data_ptr(), None,
                                                  stream))
    np_, tot_ = C.c_uint32(0), C.c_uint64(0)

    def split():
        _lib.check(_lib.lib().brx_set_cover_split_batch_device(gs._h, d_bases.data_ptr(), d_off.data_ptr(), n_reads, total, 0,
                                                               d_scratch.data_ptr(), d_scratch.numel(), d_poff.data_ptr(),
                                                               d_pread.data_ptr(), d_pstart.data_ptr(), piece_cap, C.byref(np_),
                                                               C.byref(tot_), stream))
    ms_split = timed(split)
    before = stats_of(d_bases, d_off, total)
    after = stats_of(d_out, d_out_off, out_total)

    # the kernel alone against lane_mask_kernel<true> of a Graph forward pass on the same batch
    _lib.profile_enable(True)
    _lib.profile_reset()
    gs.cover_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, total, d_flags.data_ptr(), None, d_stats.data_ptr(), stream)
    graph = br_amd.Chain(gs, [("graph", 5, 7)], two_side=True)  # (-s: forward pass only)
    graph.correct_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, total, d_out.data_ptr(), d_out.numel(),
                               d_out_off.data_ptr(), stream)
    torch.cuda.synchronize()
    prof = _lib.profile_all()
    _lib.profile_enable(False)
    cov_ms, cov_n = prof.get("cover", {}).get("total_ms", 0.0), prof.get("cover", {}).get("launches", 0)
    lm_ms, lm_n = prof.get("lane_mask", {}).get("total_ms", 0.0), prof.get("lane_mask", {}).get("launches", 0)
    kernel = {"cover_ms": round(cov_ms, 3), "cover_launches": cov_n, "lane_mask_ms": round(lm_ms, 3), "lane_mask_launches": lm_n,
              "cover_tiles_ms": round(prof.get("cover_tiles", {}).get("total_ms", 0.0), 3)}
    if cov_n and lm_n:
        kernel["cover_ns_per_position"] = round(cov_ms / cov_n * 1e6 / total, 5)
        kernel["lane_mask_ns_per_position"] = round(lm_ms / lm_n * 1e6 / total, 5)
        kernel["ratio_cover_over_lane_mask"] = round((cov_ms / cov_n) / (lm_ms / lm_n), 3)

    res = {"tool": "cover_bench", "workload": "configs[1]: %d synthetic %d bp reads, %dx, k=%d, abundance %d, device-resident"
                                              % (n_reads, read_len, args.coverage, k, a),
           "bases": int(total), "index": gs.index_info(), "bits_state_during_cover": bits_state,
           "ms_per_gbp": {"flags_stats": round(ms_flags / gbp, 3), "masked_in_place": round(ms_mask / gbp, 3),
                          "split_min_len_0": round(ms_split / gbp, 3)},
           "split": {"pieces": np_.value, "bytes": tot_.value},
           "before_one": before, "after_one": after, "kernel": kernel}

    if args.pipeline_reads > 0:
        res["pipeline"] = pipeline(args, gs, d_bases, d_off, min(args.pipeline_reads, n_reads))
    print(json.dumps(res))


def pipeline(args, gs, d_bases, d_off, n):
    import br_amd
    from br_amd.driver import run_correction
    tmp = "/dev/shm" if os.path.isdir("/dev/shm") else "/tmp"
    src = os.path.join(tmp, "brx_cover_bench_%d_in.fasta" % os.getpid())
    dst = os.path.join(tmp, "brx_cover_bench_%d_out.fasta" % os.getpid())
    ho = d_off[:n + 1].cpu().numpy()
    tot = int(ho[n])
    hb = d_bases[:tot].cpu().numpy()
    out = {"reads": n, "bases": tot}
    try:
        with open(src, "wb") as f:
            for r in range(n):
                f.write(b">r%d\n" % r)
                f.write(hb[int(ho[r]):int(ho[r + 1])].tobytes())
                f.write(b"\n")
        methods = br_amd.build_methods(["one"], gs, 5, 7)
        for rnd in range(3):  # the first round warms the pools; the slower of the other two counts
            for mode in ("plain", "mask", "split"):
                if os.path.exists(dst):
                    os.remove(dst)
                t0 = time.perf_counter()
                with open(src, "rb") as fi, open(dst, "wb") as fo:
                    run_correction([fi], [fo], methods, False, native=True, output_mode=mode)
                rate = tot / (time.perf_counter() - t0) / 1e9
                if rnd:
                    out[mode + "_gbases_per_s"] = round(min(rate, out.get(mode + "_gbases_per_s", rate)), 4)
                    out[mode + "_out_bytes"] = os.path.getsize(dst)
        out["mask_over_plain"] = round(out["mask_gbases_per_s"] / out["plain_gbases_per_s"], 4)
        out["split_over_plain"] = round(out["split_gbases_per_s"] / out["plain_gbases_per_s"], 4)
    finally:
        for p in (src, dst):
            if os.path.exists(p):
                os.remove(p)
    return out


if __name__ == "__main__":
    main()
