#!/usr/bin/env python3
"""bench.py -- corrected Gbases/s at k=19 on synthetic 10 kb ONT-error reads (BASELINE.json).

One STEP = one whole job of the hot path on data already resident in HBM:
    zero the counter -> count canonical k-mers of every read -> (N>1: exchange) -> threshold into
    the solid set -> correct every read with the method chain, forward + reverse pass.
value = bases corrected by all ranks / wall time (max over ranks), i.e. set build INCLUDED.
The correction-only and build-only rates are reported next to it in "phases".

Workloads (`--config`, BASELINE.json configs[i]; synthetic: 50x coverage of a uniform random genome,
2 % sub / 1.5 % ins / 1.5 % del, 10 kb reads):
  1  1e5 reads (1 Gbp), k=19, `fasta -a 3` build + `-c one`                       -- default at N = 1 (the metric)
  2  1e6 reads (10 Gbp), k=19, `-c greedy`, one GPU
  3  625 000 reads per GPU (50 Gbp over 8), k=19, `-c one`, reads sharded          -- default at N > 1 (not for rehearsals)
  4  625 000 reads per GPU, k=21 (sparse set), `-c graph -c gap-size`, reads sharded
N > 1: every rank owns its block of the reads of ONE genome (N x reads x 10 kb / 50 long); the set is built
from ALL ranks' reads (one exchange step over RCCL), then replicated; correction needs no communication.

`python bench.py --gpus N` started by hand spawns its N ranks itself (one fresh child process per GPU,
before anything touches the GPU); under `python -m torch.distributed.run` it is one of the ranks.

A plain run sets up, warms up, times --steps steps and prints the result line (with the per-kernel timers, phases and
self-checks of those same steps).  `--full` adds what takes runs of its own: the CPU baseline with its read-by-read
parity check against the oracle (exit 3 on a mismatch), the host-buffer batches (`host_8192`) and the FASTA file to
FASTA file leg (`e2e`), as switched by --no-cpu-baseline / --no-e2e.  `--dump-outputs DIR` writes what the last timed
step computed as .npy files (float32 / float64, under 64 MB in all; see dump_outputs) for comparing two builds.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X spec, /opt/skills/guides/MI355X_MICROARCH.md

CONFIGS = {  # reads per GPU, k, method chain
    1: dict(reads=100_000, k=19, methods=["one"]),
    2: dict(reads=1_000_000, k=19, methods=["greedy"]),
    3: dict(reads=625_000, k=19, methods=["one"]),
    4: dict(reads=625_000, k=21, methods=["graph", "gap_size"]),
}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", type=int, default=0, choices=[0, 1, 2, 3, 4],
                    help="BASELINE.json configs[i]; 0 = 1 at --gpus 1, 3 otherwise")
    ap.add_argument("--reads", type=int, default=0, help="reads per GPU (10 kb each); 0 = the config's")
    ap.add_argument("--read-len", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=0, help="0 = the config's")
    ap.add_argument("--abundance", type=int, default=3)
    ap.add_argument("--confirm", type=int, default=5)
    ap.add_argument("--coverage", type=int, default=50)
    ap.add_argument("--method", default="", help="comma-separated chain of one,two,graph,greedy,gap_size; '' = the config's")
    ap.add_argument("--strategy", default="auto", choices=["auto", "dense", "sorted"])
    ap.add_argument("--exchange", default="abi", choices=["abi", "torch"],
                    help="N > 1 set exchange: brx_exchange_* (librccl called from libbrx) or br_amd/dist.py over torch.distributed")
    ap.add_argument("--full", action="store_true",
                    help="also the CPU baseline (with its parity check against the oracle), the host-buffer batches and "
                         "the FASTA-file-in -> FASTA-file-out figure; off: only the timed steps and what they measure")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write the last timed step's outputs to DIR/<name>.npy (float32 / float64, < 64 MB in all)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-e2e", action="store_true", help="with --full: skip the host-buffer and FASTA-file-in -> "
                                                          "FASTA-file-out figures")
    ap.add_argument("--progress", action="store_true", help="timestamps of the stages on stderr (big configurations)")
    ap.add_argument("--rehearse-on-one-gpu", action="store_true",
                    help="N > 1 ranks all on cuda:0 with the gloo backend: checks the multi-rank code path where only one "
                         "card is available (RCCL cannot put two ranks on one GPU); the rate it prints means nothing")
    ap.add_argument("--force-exchange", action="store_true",
                    help="debug: run the multi-GPU exchange step even with one rank (RCCL, world_size 1)")
    ap.add_argument("--cpu-reads", type=int, default=0, help="reads in the CPU-baseline sample (0 = auto)")
    ap.add_argument("--cpu-threads", type=int, default=0, help="threads of the CPU baseline (0 = every core)")
    ap.add_argument("--traffic-json", default=os.path.join(ROOT, "profiles", "traffic_latest.json"),
                    help="PMC-derived HBM bytes per launch of an EARLIER run of this workload (profiles/collect_pmc.sh)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    # (a rehearsal puts every rank on ONE card: configs[1]'s 1 Gbp per rank fits it, configs[3]'s 6.25 Gbp per rank does not)
    args.config = args.config or (1 if (args.gpus == 1 or args.rehearse_on_one_gpu) else 3)
    cfg = CONFIGS[args.config]
    args.reads = args.reads or cfg["reads"]
    args.k = args.k or cfg["k"]
    args.methods = [m.strip().replace("-", "_") for m in args.method.split(",") if m.strip()] or list(cfg["methods"])
    for m in args.methods:
        if m not in ("one", "two", "graph", "greedy", "gap_size"):
            ap.error("unknown method %r" % m)
    return args


def spawn_ranks(args) -> int:
    """--gpus N without a launcher: N fresh children, one per GPU, each a rank of this same script.
    Nothing in this parent touches the GPU (no torch import, no HIP call)."""
    n = args.gpus
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL))
    # Every child is watched: a rank that dies before or inside a collective leaves the others waiting for ever, and
    # rank 0 with them -- so the first non-zero exit (or the overall limit) ends all of them (they are exactly the
    # children started above).  Rank 0's stdout is drained by a thread so that a long line cannot block it.
    import threading
    chunks = []
    reader = threading.Thread(target=lambda: chunks.append(procs[0].stdout.read()), daemon=True)
    reader.start()
    limit = time.time() + float(os.environ.get("BRX_BENCH_TIMEOUT", "3000"))
    rcs = [None] * n
    while any(rc is None for rc in rcs):
        for r, p in enumerate(procs):
            if rcs[r] is None:
                rcs[r] = p.poll()
        failed = [r for r, rc in enumerate(rcs) if rc not in (None, 0)]
        if failed or time.time() > limit:
            for r, p in enumerate(procs):
                if rcs[r] is None:
                    p.kill()
                    rcs[r] = p.wait()
            if not failed:
                print("bench.py: ranks still running at the time limit were stopped", file=sys.stderr)
            break
        time.sleep(0.05)
    reader.join(timeout=10)
    sys.stdout.write(b"".join(c for c in chunks if c).decode(errors="replace"))
    sys.stdout.flush()
    bad = [(r, rc) for r, rc in enumerate(rcs) if rc != 0]
    if bad:
        print("bench.py: ranks failed (rank, exit code): %s" % bad, file=sys.stderr)
        return 1
    return 0


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}", file=sys.stderr)
        sys.exit(2)

    import torch
    import torch.distributed as dist
    import br_amd
    from br_amd import _lib, synth

    t_prog = time.perf_counter()
    dev = 0 if args.rehearse_on_one_gpu else local_rank
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream().cuda_stream

    k, a = args.k, args.abundance
    n_reads, read_len = args.reads, args.read_len
    genome_len = max(world * n_reads * read_len // args.coverage, read_len)
    cfg = synth.config(genome_len=genome_len, read_len=read_len)

    # ---- synthetic input, resident in HBM before the timed region --------------------------------
    d_genome = torch.empty(genome_len, dtype=torch.uint8, device="cuda")
    synth.genome_device(cfg, dev, d_genome.data_ptr(), stream)
    cap = int(n_reads * read_len * 1.03) + (1 << 20)
    d_bases = torch.empty(cap, dtype=torch.uint8, device="cuda")
    d_off = torch.empty(n_reads + 1, dtype=torch.int64, device="cuda")
    total = synth.reads_device(cfg, dev, d_genome.data_ptr(), rank * n_reads, n_reads, d_bases.data_ptr(), cap,
                               d_off.data_ptr(), stream)
    del d_genome
    d_out = torch.empty(int(total * 1.05) + (1 << 20), dtype=torch.uint8, device="cuda")
    d_out_off = torch.empty(n_reads + 1, dtype=torch.int64, device="cuda")

    strategy = {"auto": _lib.COUNT_AUTO, "dense": _lib.COUNT_DENSE, "sorted": _lib.COUNT_SORTED}[args.strategy]
    counter = br_amd.Counter(k, dev, strategy)
    gs = br_amd.Pcon.new(k, dev)
    chain = br_amd.Chain(gs, [(m, args.confirm, 7) for m in args.methods], two_side=False)

    # The process group is created AFTER the big HBM allocations above (measured: buffers allocated
    # after RCCL's communicator exists stream at a fraction of the bandwidth on this stack).
    multi = world > 1 or args.force_exchange
    if multi:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        if args.rehearse_on_one_gpu:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
    from br_amd import dist as brx_dist
    exchanger = None
    exchange_kind = None
    if multi:
        use_abi = args.exchange == "abi" and not args.rehearse_on_one_gpu
        exchange_kind = "brx_exchange_* (librccl from libbrx.so)" if use_abi else "br_amd/dist.py over torch.distributed"
        exchanger = brx_dist.AbiExchange(world, rank, dev) if use_abi else brx_dist.SetExchange(world, rank)
    partitioned = multi and (args.strategy == "sorted" or (args.strategy == "auto" and k >= 15))

    phase_ms = {"build": 0.0, "correct": 0.0, "exchange": 0.0}

    def note(msg):
        if args.progress and rank == 0:
            print("[bench %8.2f s] %s" % (time.perf_counter() - t_prog, msg), file=sys.stderr, flush=True)

    note("input resident: %d reads, %d bases" % (n_reads, total))

    def step(timed: bool):
        t0 = time.perf_counter()
        counter.reset(stream)
        counter.add_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, total, stream)
        if exchanger is not None:
            if timed:
                torch.cuda.synchronize()
            tx = time.perf_counter()
            if partitioned:
                exchanger.build_partitioned(counter, gs, a, stream)   # keys to their owner, solid set back
            else:
                exchanger.reduce_counts(counter, a, stream)           # dense: u8 all-reduce
                counter.finish_into(a, gs, stream)
            if timed:
                torch.cuda.synchronize()
                phase_ms["exchange"] += (time.perf_counter() - tx) * 1e3
        else:
            counter.finish_into(a, gs, stream)
        if timed:
            torch.cuda.synchronize()
        t1 = time.perf_counter()
        note("set built (%.1f ms)" % ((t1 - t0) * 1e3))
        out_total = chain.correct_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, total,
                                               d_out.data_ptr(), d_out.numel(), d_out_off.data_ptr(), stream)
        if timed:
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            phase_ms["build"] += (t1 - t0) * 1e3
            phase_ms["correct"] += (t2 - t1) * 1e3
            note("corrected (%.1f ms)" % ((t2 - t1) * 1e3))
        return out_total

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step(False)
    _lib.profile_enable(True)
    _lib.profile_reset()
    barrier()
    t0 = time.perf_counter()
    out_total = 0
    for _ in range(args.steps):
        out_total = step(True)
    barrier()
    elapsed = time.perf_counter() - t0
    _lib.profile_enable(False)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, gs, d_out, d_out_off, n_reads, read_len, stream)

    def reduce_scalar(v, op, dtype=torch.float64):
        if world == 1:
            return v
        t = torch.tensor([v], dtype=dtype, device="cpu" if args.rehearse_on_one_gpu else "cuda")
        dist.all_reduce(t, op=op)
        return t.item()

    elapsed = float(reduce_scalar(elapsed, dist.ReduceOp.MAX))
    total_all = int(reduce_scalar(total, dist.ReduceOp.SUM, torch.int64))

    prof = _lib.profile_all()
    stats = chain.last_stats()
    solid_bits = gs.popcount()
    # cheap self-checks of the job (a wrong set shows up here long before anyone diffs FASTA files):
    # every rank must hold the same set, and roughly one solid k-mer per genome position and strand-pair
    checks = {"solid_per_genome_base": round(solid_bits / genome_len, 3)}
    if world > 1:
        # Every rank must end with THE SAME set -- the one thing the exchange is for.  One all-gather of a fingerprint per
        # rank: popcount plus two order-independent 64-bit folds of the set's members (wrapping sums of the hashes and of
        # their squares, whatever holds the set on this rank: list, chained table of a sparse set, bit vector).  The
        # gather runs over the job's own backend, so the ranks that answer are also the count of ranks RCCL really joined.
        n_fp, f1, f2 = gs.fingerprint(stream)     # (brx_set_fingerprint: list, chained table or bit vector -- same numbers)
        how = "brx_set_fingerprint"
        assert n_fp == solid_bits, (n_fp, solid_bits)
        to_i64 = lambda v: v - (1 << 64) if v >= (1 << 63) else v
        mine = torch.tensor([to_i64(int(solid_bits)), to_i64(f1 & ((1 << 64) - 1)), to_i64(f2 & ((1 << 64) - 1))], dtype=torch.int64,
                            device="cpu" if args.rehearse_on_one_gpu else "cuda")
        gathered = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(gathered, mine)
        prints = [tuple(int(x) for x in g.cpu().tolist()) for g in gathered]
        checks["set_agree"] = bool(all(p_ == prints[0] for p_ in prints))
        checks["set_fingerprint"] = {"of": how, "popcount": prints[0][0], "fold_sum": prints[0][1] & ((1 << 64) - 1),
                                     "fold_sum_sq": prints[0][2] & ((1 << 64) - 1)}
        checks["set_popcount_identical_across_ranks"] = bool(len({p_[0] for p_ in prints}) == 1)
        checks["rccl_ranks"] = (len(prints) if dist.get_backend() == "nccl" else 0)
    min_fixes = 0.01 * total if args.methods == ["one"] else 0  # One repairs most isolated errors; Greedy few
    checks["plausible"] = bool(0.9 < solid_bits / genome_len < 1.3 and stats["fixes"] > min_fixes)

    # ---- roofline of the dominant kernel ---------------------------------------------------------
    n_table = 1 << (2 * k - 1)
    alg_bytes = {  # ALGORITHMIC bytes per launch (SURVEY 8(d) per-unit figure x units per launch)
        "correct_pass": 66.0 * total,                 # 1 B in + 1 B out + one 64 B probe per base, per pass
        "correct_pass_two": 66.0 * total, "correct_pass_graph": 66.0 * total, "correct_pass_greedy": 66.0 * total,
        "correct_pass_gap_size": 66.0 * total,        # same figure for every method
        "count_dense": 129.0 * total,                 # 1 B in + 64 B counter line read + 64 B write-back
        "count_keys": 9.0 * total,                    # 1 B in + 8 B key out
        "threshold": float(n_table + n_table // 8),   # stream the u8 table, write the bitset
        "count_zero": float(n_table),
        "compact": 2.0 * total,
    }
    dominant, best = None, -1.0
    for name, v in prof.items():
        if name in alg_bytes and v["launches"] > 0 and v["total_ms"] > best:
            dominant, best = name, v["total_ms"]
    roofline = None
    # A forward pass in lane form is several launches (unit tables + packed copy, sync points, the automaton, the replay
    # of its fixes, the few reads handed back; the successor table of a set for the walking methods): their time belongs
    # to the pass, so the launch average below is (everything the passes cost) / (passes)
    LANE_AUX = ("lane_units", "lane_mask", "lane_sync", "lane_apply", "lane_redo", "succ_build")
    aux_ms = sum(prof[n_]["total_ms"] for n_ in LANE_AUX if n_ in prof)
    if dominant:
        pass_ms = prof[dominant]["total_ms"] + (aux_ms if dominant.startswith("correct_pass") else 0.0)
        avg_ms = pass_ms / prof[dominant]["launches"]
        achieved = alg_bytes[dominant] / (avg_ms * 1e-3) / 1e9
        # HBM bytes per launch from the PMC counters cannot be collected inside this process (they need their own
        # rocprofv3 passes): the figure is the one profiles/collect_pmc.sh measured for this same kernel and
        # workload in an earlier run, and says so
        traffic, traffic_source = None, None
        try:
            with open(args.traffic_json) as f:
                tj = json.load(f)
            if tj.get("kernel") == dominant and tj.get("bases_per_launch") == total and args.methods == ["one"]:
                traffic = tj.get("hbm_bytes_per_launch")
                traffic_source = "%s (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of an earlier run of this workload; " \
                                 "not measured by this run)" % os.path.relpath(args.traffic_json, ROOT)
        except Exception:
            pass
        roofline = {"kernel": dominant, "bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS,
                    "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic,
                    "traffic_source": traffic_source,
                    # the real HBM rate of the kernel: measured bytes / launch time / peak (the contract's `frac` counts
                    # 64 B per probe whether or not neighbouring probes shared the line)
                    "frac_traffic": round(traffic / (avg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if traffic else None,
                    "avg_launch_ms": round(avg_ms, 4), "algorithmic_bytes_per_launch": alg_bytes[dominant],
                    "launches": prof[dominant]["launches"],
                    "launch_is": "one scan pass over every read; the forward pass's helper kernels (%s) are counted into it: "
                                 "%.3f ms per step" % (", ".join(n_ for n_ in LANE_AUX if n_ in prof), aux_ms / max(args.steps, 1))}

    cpu = e2e = host = None
    if args.full and rank == 0 and world == 1:
        # free the bench's own HBM/host buffers are not needed any more; the legs below bring their own
        # the file-to-file leg first: behind the CPU baseline (16 threads for ~20 s, an 8 GiB table allocated and freed) its
        # host stages measured 3-8x slower on the same box (build 1.0 s instead of 0.16 s per Gbp)
        if not args.no_e2e and args.config == 1 and n_reads <= 200_000:
            host = host_8192(args, d_bases, d_off, n_reads, gs)
            # the reference's batch size is a flag (`-b`, record_buffer_len, src/cli.rs): four times the records per call
            # amortise what an 82 Mbp batch cannot -- the passes' fixed latency (profiles/r4f_host_batch_stages.txt)
            host_big = host_8192(args, d_bases, d_off, n_reads, gs, per=32768, n_b=2)
            if host is not None and host_big is not None:
                host["records_32768"] = {k_: host_big.get(k_) for k_ in ("pinned", "pinned_async_3_chains", "error") if k_ in host_big}
            e2e = e2e_fasta(args, d_bases, d_off, n_reads, total, k, a)
        if not args.no_cpu_baseline:
            cpu = cpu_baseline(args, cfg, gs, k, n_reads, d_out, d_out_off)
            if cpu and "parity" in cpu:
                # the CPU leg corrects its sample anyway: every read of it is compared with what the timed GPU step wrote
                checks["parity_reads"] = cpu["parity"]["reads_compared"]
                checks["parity_mismatches"] = cpu["parity"]["mismatches"]
                if cpu["parity"]["reads_compared"] == n_reads:
                    checks["parity_fixes_equal"] = bool(int(stats["fixes"]) == cpu["parity"]["oracle_fixes"])
                if cpu["parity"]["mismatches"]:
                    print("bench.py: %d of %d reads differ from the oracle (first: read %s)" %
                          (cpu["parity"]["mismatches"], cpu["parity"]["reads_compared"], cpu["parity"]["first_mismatching_read"]),
                          file=sys.stderr)

    if rank == 0:
        value = total_all * args.steps / elapsed / 1e9
        mdesc = " + ".join("correct::%s" % m for m in args.methods)
        line = {
            "metric": "corrected Gbases/sec at k=%d, 10 kb ONT-error reads" % k,
            "value": round(value, 4), "unit": "Gbases/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u64 k-mers / 1-bit set",
            "data": "synthetic", "full": args.full,
            "config": {"workload": "BASELINE configs[%d]: synthetic %.2f Gbp/GPU ONT-error %d bp reads, k=%d, set build "
                                   "(-a %d) + %s (-C %d) fwd+rev" % (args.config, total / 1e9, read_len, k, a, mdesc, args.confirm),
                       "reads_per_gpu": n_reads, "bases_per_gpu": total, "genome_len": genome_len,
                       "strategy": args.strategy, "parallelism": "reads sharded x%d" % world,
                       **({"set_exchange": exchange_kind} if multi else {}),
                       **({"rehearsal": "all ranks on cuda:0 over gloo: code-path check, not a measurement"}
                          if args.rehearse_on_one_gpu else {})},
            "phases": {"build_ms_per_step": round(phase_ms["build"] / args.steps, 3),
                       "correct_ms_per_step": round(phase_ms["correct"] / args.steps, 3),
                       **({"exchange_ms_per_step": round(phase_ms["exchange"] / args.steps, 3)} if multi else {}),
                       "correct_only_gbases_per_s": round(total * args.steps / (phase_ms["correct"] * 1e-3) / 1e9, 3)
                       if phase_ms["correct"] > 0 else None,
                       "build_only_gbases_per_s": round(total * args.steps / (phase_ms["build"] * 1e-3) / 1e9, 3)
                       if phase_ms["build"] > 0 else None,
                       **build_roofline(prof, total, args.steps, phase_ms["build"])},
            "kernels": {n: {"avg_ms": round(v["total_ms"] / max(v["launches"], 1), 4), "launches": v["launches"]}
                        for n, v in prof.items() if v["launches"]},
            "correct_stats": {**{k_: int(v) for k_, v in stats.items()}, "out_bases": int(out_total),
                              "solid_kmers": int(solid_bits)},
            "probe_index": gs.index_info(),
            "checks": checks,
            "roofline": roofline,
            "cpu_baseline": cpu,
            "e2e": e2e,
            "host_8192": host,
        }
        print(json.dumps(line), flush=True)
        if checks.get("parity_mismatches"):
            sys.exit(3)  # a rate for bytes that differ from the reference's is not a result
    # N > 1: a job whose ranks do not hold the same set, or that RCCL did not carry with all N ranks, has no rate either
    # (every rank computes the same verdict from the same gather: all of them leave with it)
    if world > 1 and (not checks.get("set_agree") or (not args.rehearse_on_one_gpu and checks.get("rccl_ranks") != world)):
        print("bench.py: rank %d: the ranks' sets differ or RCCL ranks != %d: %s" % (rank, world, checks), file=sys.stderr)
        if exchanger is not None and hasattr(exchanger, "close"):
            exchanger.close()
        dist.destroy_process_group()
        sys.exit(4)
    if exchanger is not None and hasattr(exchanger, "close"):
        exchanger.close()
    if multi:
        dist.destroy_process_group()


def usable_cpus():
    """host cores this process may really use: the affinity mask, cut down to the cgroup's CPU quota when the box is
    shared (a one-GPU lease of an 8-GPU host sees all its cores in nproc but is scheduled on its share of them)"""
    n = os.cpu_count() or 1
    how = "nproc"
    try:
        a = len(os.sched_getaffinity(0))
        if a < n:
            n, how = a, "sched_getaffinity"
    except AttributeError:
        pass
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            with open(path) as f:
                txt = f.read().split()
            if path.endswith("cpu.max"):
                quota, period = txt[0], int(txt[1])
            else:
                quota = txt[0]
                with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f2:
                    period = int(f2.read())
            if quota not in ("max", "-1"):
                q = max(1, int(int(quota) / period + 0.5))
                if q < n:
                    n, how = q, "cgroup cpu quota (%s)" % path
            break
        except (OSError, ValueError, IndexError):
            continue
    return n, how


def cpu_baseline(args, cfg, gs, k, n_reads, d_out=None, d_out_off=None):
    """Times the CPU oracle (restatement of the reference's path; the Rust reference itself cannot be built
    offline) on a bounded sample of the same workload, with pthread workers on every core of the box
    (oracle/br_oracle.c: bro_correct_batch_mt / bro_count_batch_mt, the shape of the reference's rayon path):
      correction: the method chain fwd+rev over the first S reads against the same k-mer set (exported from HBM
                  for k <= 19; a sparse oracle set rebuilt from the sample's own k-mers otherwise);
      set build:  Counter<u8> over the first reads at the largest k whose 2^(2k-1)-byte table is reasonable on a
                  host (k=17: 8 GiB; the metric's k=19 needs 128 GiB) -- a random 1-byte RMW per base at either k."""
    import numpy as np
    from br_amd import synth
    from oracle import oracle as O

    usable, how = usable_cpus()
    cores = args.cpu_threads or usable
    per_read_s = {"one": 1.6e-3, "two": 4e-3, "graph": 3e-3, "greedy": 6e-3, "gap_size": 3e-3}
    want_s = 12.0
    est = sum(per_read_s.get(m, 3e-3) for m in args.methods)
    S = args.cpu_reads or int(min(n_reads, max(256, want_s * cores / est), 1 << 30 if k <= 19 else 4096))
    g = synth.genome_host(cfg)
    bases, offs = synth.reads_host(cfg, g, 0, S)
    if k <= 19:
        bits = gs.export_bits()                       # 2^(2k-4) bytes, D2H once
        solid = O.Solid.wrap(k, bits)
        set_desc = "the GPU-built k=%d set" % k
    else:
        # no bit vector at k >= 21: the baseline probes a sparse oracle set holding the GPU set's members among the
        # sample's k-mers (every probe the correctors can make hits a k-mer near the sample's reads or an absent one)
        reads = [bases[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(S)]
        hs = np.unique(np.concatenate([O.hashes(k, r) for r in reads]))
        canon = (hs << np.uint64(1)) | (np.bitwise_count(hs).astype(np.uint64) & np.uint64(1))  # even-popcount member
        keep = np.ascontiguousarray(hs[gs.get_many(canon)], dtype=np.uint64)
        solid = O.Solid(k, _h=O.lib().bro_solid_new_sparse(k, keep.ctypes.data, keep.size))
        set_desc = "the GPU-built sparse k=%d set restricted to the sample's k-mers" % k
    # what the GPU wrote for the same reads in the last timed step (the oracle here is the checker of that output, never
    # a source of it): compared read by read inside the workers, after each read's correction
    expect = expect_off = None
    if d_out is not None and d_out_off is not None:
        expect_off = d_out_off[:S + 1].cpu().numpy().astype(np.uint64)
        expect = d_out[:int(expect_off[-1])].cpu().numpy()
    t0 = time.perf_counter()
    _, out_bytes, fixes, n_bad, first_bad = O.correct_batch_mt_check(solid, args.methods, bases, offs, expect, expect_off,
                                                                      args.confirm, 7, False, cores)
    dt = time.perf_counter() - t0
    nb = int(offs[S])
    res = {"value": round(nb / dt / 1e9, 5), "unit": "Gbases/s", "cores": cores, "nproc": os.cpu_count(),
           "cores_how": how, "kind": "port",
           "sample": "%s fwd+rev of the first %d reads (%.1f Mbp) against %s; correction phase only, %d pthreads "
                     "pulling 16-record blocks, %.1f s, %d fixes" % (" + ".join(args.methods), S, nb / 1e6, set_desc, cores, dt, fixes)}
    if expect_off is not None:
        res["parity"] = {"reads_compared": S, "mismatches": n_bad, "first_mismatching_read": first_bad,
                         "oracle_fixes": fixes, "oracle_out_bases": out_bytes, "gpu_out_bases": int(expect_off[-1]),
                         "what": "every read of the sample: bytes of the timed GPU step's output vs the oracle's"}
    # set-build leg
    kb = min(k, 17)
    Sb = int(min(S, 1600 * cores))     # ~0.1 ms per 10 kb read on one thread (DRAM-latency-bound RMW): a few seconds, so that
    #                                    the fixed 2^(2k-1)-byte zero fill + threshold pass does not swamp the counting
    try:
        t0 = time.perf_counter()
        counts = O.count_reads_mt(kb, bases[:int(offs[Sb])], offs[:Sb + 1], cores)
        t1 = time.perf_counter()
        sol = O.Solid.from_count(kb, counts, args.abundance)
        t2 = time.perf_counter()
        nbb = int(offs[Sb])
        res["set_build"] = {"value": round(nbb / (t2 - t0) / 1e9, 5), "unit": "Gbases/s counted", "k": kb, "cores": cores,
                            "sample": "Counter<u8> (%d pthreads, saturating atomic cells, %.1f GiB table incl. its zero fill) over "
                                      "the first %d reads (%.1f Mbp): %.2f s, + Solid::from_count %.2f s; %d solid k-mers"
                                      % (cores, (1 << (2 * kb - 1)) / 2**30, Sb, nbb / 1e6, t1 - t0, t2 - t1, sol.popcount())}
        del counts, sol
    except MemoryError:
        res["set_build"] = {"value": None, "sample": "host table of k=%d did not fit" % kb}
    return res


DUMP_SEED = 0x5EED_B3C4
DUMP_SAMPLE_BASES = 8 << 20   # corrected bases of the sampled reads, as float32: 32 MiB at most
DUMP_LENGTH_READS = 2 << 20   # corrected lengths of the first 2 Mi reads, as float64: 16 MiB at most


def dump_outputs(out_dir, gs, d_out, d_out_off, n_reads, read_len, stream):
    """What a caller of the timed path receives from its last step, as .npy files that a run of another build with the
    same arguments (hence the same synthetic input) can be compared with file for file:
      corrected_lengths.npy       float64  length of every corrected read (of the first 2 Mi reads in a bigger batch)
      corrected_sample_reads.npy  float64  indices of a fixed, seeded sample of reads, chosen from n_reads and read_len
                                           alone so that every build samples the same reads
      corrected_sample_bases.npy  float32  those reads' corrected bases (ASCII codes), concatenated in index order and
                                           cut at 8 Mi bases
      solid_set.npy               float64  the solid set: members, then the two order-independent 64-bit folds of
                                           brx_set_fingerprint as 32-bit halves, high half first
    At most 48 MiB and a few kB in all; rank 0's reads only at N > 1 (every rank holds the same set)."""
    import numpy as np
    import torch
    os.makedirs(out_dir, exist_ok=True)
    torch.cuda.synchronize()
    off = d_out_off[:n_reads + 1].cpu().numpy()
    lengths = np.diff(off[:min(n_reads, DUMP_LENGTH_READS) + 1]).astype(np.float64)
    n_s = max(1, min(n_reads, DUMP_SAMPLE_BASES // max(read_len, 1)))
    idx = np.sort(np.random.default_rng(DUMP_SEED).choice(n_reads, size=n_s, replace=False))
    sample = torch.cat([d_out[int(off[i]):int(off[i + 1])] for i in idx])[:DUMP_SAMPLE_BASES]
    members, f1, f2 = gs.fingerprint(stream)
    halves = lambda v: [float((v >> 32) & 0xFFFFFFFF), float(v & 0xFFFFFFFF)]
    arrays = {"corrected_lengths": lengths,
              "corrected_sample_reads": idx.astype(np.float64),
              "corrected_sample_bases": sample.cpu().numpy().astype(np.float32),
              "solid_set": np.array([float(members)] + halves(f1) + halves(f2), dtype=np.float64)}
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def build_roofline(prof, total, steps, build_ms):
    """The set build against the bytes its own passes must move: the partitioned build reads the
    bases twice at level 1 (histogram, scatter: 1 B each) and writes a 4-byte key per k-mer, reads the keys twice and
    writes them once at every further level (12 B), and reads them once more in the final count (4 B); the index
    build and the threshold output are a few bytes per SOLID k-mer, not per base, and are left out.  SURVEY 8(d)'s
    figure for the set build -- 129 B per base, one 64-byte counter line read and written back per k-mer -- is the
    dense-counter algorithm's; it is quoted beside it."""
    levels = sum(1 for n_ in prof if n_.startswith("part_l") and n_.endswith("_scatter") and prof[n_]["launches"])
    if not levels or build_ms <= 0:
        return {}
    per_base = 2 + 4 + 12 * (levels - 1) + 4
    rate = per_base * total * steps / (build_ms * 1e-3) / 1e9
    return {"build_bytes_per_base": per_base, "build_levels": levels, "build_gbs": round(rate, 1),
            "build_frac": round(rate / HBM_PEAK_GBS, 4),
            "build_frac_survey_model": round(129 * total * steps / (build_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}


def host_8192(args, d_bases, d_off, n_reads, gs, per=8192, n_b=4):
    """The boundary the reference would call: brx_chain_correct_batch on HOST buffers of 8192 records, the batch size
    of run_correction / populate_buffer (src/lib.rs:90,168-188) -- upload, both passes, download, per call.  Twice: the
    batches in ordinary (pageable) memory, and in brx_host_alloc (page-locked) blocks.  PCIe-inclusive: never `value`."""
    import ctypes as C
    import numpy as np
    import br_amd
    from br_amd import _lib
    L = _lib.lib()
    if n_reads < per * (n_b + 1):
        return None
    try:
        off_all = d_off[:per * (n_b + 1) + 1].cpu().numpy().astype(np.uint64)
        bases_all = d_bases[:int(off_all[-1])].cpu().numpy()
        chain = br_amd.Chain(gs, [(m, args.confirm, 7) for m in args.methods], two_side=False)
        res = {"records_per_batch": per, "batches": n_b}
        for kind in ("pageable", "pinned"):
            bufs, keep = [], []
            for b in range(n_b + 1):
                lo, hi = int(off_all[b * per]), int(off_all[(b + 1) * per])
                offs = np.ascontiguousarray(off_all[b * per:(b + 1) * per + 1] - off_all[b * per])
                if kind == "pinned":
                    ptr = L.brx_host_alloc(hi - lo)
                    keep.append(ptr)
                    C.memmove(ptr, bases_all[lo:hi].ctypes.data, hi - lo)
                    bufs.append((ptr, offs, hi - lo))
                else:
                    piece = bases_all[lo:hi].copy()
                    bufs.append((piece.ctypes.data, offs, hi - lo, piece))
            ob, oo = C.POINTER(C.c_uint8)(), C.POINTER(C.c_uint64)()
            def one(bf):
                _lib.check(L.brx_chain_correct_batch(chain._h, bf[0], bf[1].ctypes.data, per, C.byref(ob), C.byref(oo)))
                L.brx_buf_free(ob)
                L.brx_buf_free(oo)
            one(bufs[n_b])  # warm-up: workspace, page-locked pool
            t0 = time.perf_counter()
            for b in range(n_b):
                one(bufs[b])
            dt = time.perf_counter() - t0
            nb = sum(bf[2] for bf in bufs[:n_b])
            res[kind] = {"gbases_per_s": round(nb / dt / 1e9, 3), "ms_per_batch": round(dt / n_b * 1e3, 2)}
            for ptr in keep:
                L.brx_host_free(ptr)
        # the same batches, page-locked, through brx_chain_correct_batch_async / _wait: ONE host thread rotating over
        # three chains of the set, so that a batch's upload, another's passes and a third's download overlap
        # (the double-buffered form of run_correction's batch loop)
        n_ch, rounds = 3, 3
        chains = [br_amd.Chain(gs, [(m, args.confirm, 7) for m in args.methods], two_side=False) for _ in range(n_ch)]
        bufs, keep = [], []
        for b in range(n_b + 1):
            lo, hi = int(off_all[b * per]), int(off_all[(b + 1) * per])
            offs = np.ascontiguousarray(off_all[b * per:(b + 1) * per + 1] - off_all[b * per])
            ptr = L.brx_host_alloc(hi - lo)
            keep.append(ptr)
            C.memmove(ptr, bases_all[lo:hi].ctypes.data, hi - lo)
            bufs.append((ptr, offs, hi - lo))
        ob, oo = C.POINTER(C.c_uint8)(), C.POINTER(C.c_uint64)()
        def submit(ch, bf):
            _lib.check(L.brx_chain_correct_batch_async(ch._h, bf[0], bf[1].ctypes.data, per))
        def collect(ch):
            _lib.check(L.brx_chain_correct_batch_wait(ch._h, C.byref(ob), C.byref(oo)))
            L.brx_buf_free(ob)
            L.brx_buf_free(oo)
        for ch in chains:                     # warm-up: every chain's workspace
            submit(ch, bufs[n_b])
        for ch in chains:
            collect(ch)
        seq = [bufs[b % n_b] for b in range(n_b * rounds)]
        t0 = time.perf_counter()
        for j, bf in enumerate(seq):
            ch = chains[j % n_ch]
            if j >= n_ch:
                collect(ch)
            submit(ch, bf)
        for j in range(min(n_ch, len(seq))):
            collect(chains[(len(seq) - min(n_ch, len(seq)) + j) % n_ch])
        dt = time.perf_counter() - t0
        nb = sum(bf[2] for bf in seq)
        res["pinned_async_3_chains"] = {"gbases_per_s": round(nb / dt / 1e9, 3), "ms_per_batch": round(dt / len(seq) * 1e3, 2),
                                        "batches": len(seq)}
        for ptr in keep:
            L.brx_host_free(ptr)
        del chains
        res["value"] = res["pinned_async_3_chains"]["gbases_per_s"]
        res["value_is"] = "page-locked batches, one host thread, three chains in flight (brx_chain_correct_batch_async / _wait); " \
                          "`pinned` is the single synchronous call"
        res["unit"] = "Gbases/s"
        return res
    except Exception as e:
        return {"value": None, "error": "%s: %s" % (type(e).__name__, e)}


def e2e_fasta(args, d_bases, d_off, n_reads, total, k, a):
    """SURVEY 8(d) "for honesty": the same job FASTA file in -> FASTA file out through the native host pipeline
    (brx_count_fasta_fd + brx_run_correction_fd, what `python -m br_amd ... fasta` runs), files in /dev/shm so
    that no disk is measured: parse + H2D + kernels + D2H + 80-column formatting + write.  Never `value`."""
    import br_amd
    from br_amd.driver import run_correction
    tmp = "/dev/shm" if os.path.isdir("/dev/shm") else "/tmp"
    src = os.path.join(tmp, "brx_bench_%d_in.fasta" % os.getpid())
    dst = os.path.join(tmp, "brx_bench_%d_out.fasta" % os.getpid())
    try:
        hb, ho = d_bases[:total].cpu().numpy(), d_off.cpu().numpy()
        with open(src, "wb") as f:
            for r in range(n_reads):
                f.write(b">r%d\n" % r)
                f.write(hb[int(ho[r]):int(ho[r + 1])].tobytes())
                f.write(b"\n")
        del hb
        res = {}
        # "cold": the first job of the process -- the library's device blocks (keys, count rows, probe index: ~12 GB at
        # 1 Gbp) are mapped by the driver for the first time, the input file's pages are touched for the first time; then
        # two runs in steady state (blocks come back from the library's pools), whose SLOWER one is the value
        for attempt in ("cold", "first", "second"):
            if os.path.exists(dst):
                os.remove(dst)                # (truncating the first run's 1 GB of tmpfs is not part of the second)
            t0 = time.perf_counter()
            cnt = br_amd.Counter(k, 0)
            ts0 = time.perf_counter()
            with open(src, "rb") as f:
                cnt.count_fasta(f)
            gs2 = cnt.finish(a)
            t1 = time.perf_counter()
            del cnt
            ts1 = time.perf_counter()
            methods = br_amd.build_methods(args.methods, gs2, args.confirm, 7)
            ts2 = time.perf_counter()
            with open(src, "rb") as fi, open(dst, "wb") as fo:
                st = run_correction([fi], [fo], methods, False, native=True)
            t2 = time.perf_counter()
            res[attempt] = {"build_gbases_per_s": round(total / (t1 - t0) / 1e9, 3),
                            "correct_gbases_per_s": round(total / (t2 - t1) / 1e9, 3),
                            "end_to_end_gbases_per_s": round(total / (t2 - t0) / 1e9, 3),
                            # creating the counter, dropping it, creating the chain: inside the legs above, listed apart
                            "setup_s": round((ts0 - t0) + (ts1 - t1) + (ts2 - ts1), 4),
                            "parse_s": round(st["ns_parse"] / 1e9, 3), "gpu_format_s_summed": round(st["ns_gpu"] / 1e9, 3),
                            "write_s": round(st["ns_write"] / 1e9, 3)}
            del methods, gs2
        steady_s = total / 1e9 / min(res["first"]["end_to_end_gbases_per_s"], res["second"]["end_to_end_gbases_per_s"])
        res["cold"]["extra_s_over_steady_state"] = round(total / 1e9 / res["cold"]["end_to_end_gbases_per_s"] - steady_s, 3)
        return {"value": min(res["first"]["end_to_end_gbases_per_s"], res["second"]["end_to_end_gbases_per_s"]), "unit": "Gbases/s",
                "what": "FASTA file -> count -> set -> correct -> 80-column FASTA file, /dev/shm, native host pipeline; "
                        "the SLOWER of two identical steady-state runs (both listed, and the process's first, cold run "
                        "beside them; each run creates its counter, set and chain anew, "
                        "page-locked and device blocks come from the library's pools)",
                "in_bytes": os.path.getsize(src),
                "out_bytes": os.path.getsize(dst), **res}
    except Exception as e:  # the honesty figure must not take the contract line down with it
        return {"value": None, "error": "%s: %s" % (type(e).__name__, e)}
    finally:
        for p in (src, dst):
            if os.path.exists(p):
                os.remove(p)


if __name__ == "__main__":
    main()
