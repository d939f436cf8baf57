"""One rank of a world-N run of the SHIPPED multi-GPU merge of counting tables (br_amd/csrc/brx_exchange.hip:
brx_exchange_table_merge / _spectrum / _table_finish) with all ranks on ONE card, in the manner of abi_exchange_worker.py:
the library's librccl calls are served by tests/libfake_rccl.so (BRX_RCCL_PATH, set by the test that starts this
process), the communicator id travels through a file, the results come back as a pickle.
usage: python table_exchange_worker.py RANK WORLD K ABUNDANCE N_READS OUT_PREFIX raw|sat
  raw  the first N_READS reads of the fixture, sharded; merge, spectrum, finish with ABUNDANCE, correction of the shard
  sat  poly-A counted 200 times and poly-C 60 times on each of two ranks; finish with four thresholds on one merged counter"""
import os
import pickle
import sys
import time

T_START = time.time()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
rank, world, k, a, n_reads = (int(x) for x in sys.argv[1:6])
out_prefix, mode = sys.argv[6], sys.argv[7]

import numpy as np
import br_amd
from br_amd import _lib, fasta
from br_amd import dist as bd


def phase(what):
    """to stderr, which the runner keeps per rank: where the time of a slow or a hung world went"""
    print("rank %d: %s at %.2f s" % (rank, what, time.time() - T_START), file=sys.stderr, flush=True)


phase("imports done")
if mode == "sat":
    reads = [b"A" * (k + 199), b"C" * (k + 59)] * 2
else:
    with open(os.path.join(ROOT, "tests", "golden", "raw.fasta"), "rb") as f:
        reads = [seq for _, _, seq in fasta.read_records(f)][:n_reads]
lo, hi = bd.shard_range(len(reads), world, rank)
mine = reads[lo:hi]                                   # may be empty: that rank still joins every collective

id_path = out_prefix + ".id"
if rank == 0:
    ident = bd.AbiExchange.unique_id()
    with open(id_path + ".tmp", "wb") as f:
        f.write(ident)
    os.rename(id_path + ".tmp", id_path)
else:
    t0 = time.time()
    while not os.path.exists(id_path):
        if time.time() - t0 > 120:
            sys.exit("rank %d: no communicator id after 120 s" % rank)
        time.sleep(0.05)
    with open(id_path, "rb") as f:
        ident = f.read()
phase("communicator id in hand")
ex = bd.AbiExchange(world, rank, 0, ident=ident)
phase("communicator up")
result = {"n_mine": len(mine)}
counter = br_amd.Counter(k, 0, _lib.COUNT_TABLE)
half = (len(mine) + 1) // 2
for part in (mine[:half], mine[half:]):               # any number of batches: two
    if part:
        counter.add_reads(part)
result["state_before"] = counter.merge_state()
phase("shard counted")
ex.merge_table(counter)
phase("merged")
result["state_after"] = counter.merge_state()
result["stats_merge"] = ex.last_stats()
result["keys"] = counter.table_info()["keys"]
result["spectrum"] = ex.spectrum(counter)
phase("spectrum")
solid = br_amd.Pcon.new(k)
if mode == "sat":
    probes = [br_amd.seq2bit(b"A" * k), br_amd.seq2bit(b"C" * k)]
    result["counts"] = [int(x) for x in counter.get_counts(probes)]
    result["finish"] = {}
    for thr in (254, 255, 119, 120):
        ex.finish_table(counter, solid, thr)
        result["finish"][thr] = ([bool(x) for x in solid.get_many(probes)], solid.fingerprint())
        phase("finished at threshold %d" % thr)
    result["state_end"] = counter.merge_state()
else:
    ex.finish_table(counter, solid, a)
    phase("finished")
    result["stats"] = ex.last_stats()
    result["popcount"] = solid.popcount()
    result["fingerprint"] = solid.fingerprint()
    result["index"] = solid.index_info()
    if k <= 15:
        result["solid_bytes"] = solid.to_solid_bytes()
    # every third k-mer of the first and the last read of the JOB, and two neighbours of each
    sample = []
    for r in (reads[0], reads[-1]):
        for j in range(0, len(r) - k + 1, 3):
            km = br_amd.seq2bit(r[j:j + k])
            sample += [km, km ^ 1, km ^ (3 << 10)]
    result["sample"] = sample
    result["members"] = [bool(x) for x in solid.get_many(sample)]
    result["counts"] = counter.get_counts(sample)
    chain = br_amd.Chain(solid, [("one", 5, 7), ("graph", 5, 7)], two_side=False)
    result["corrected"] = chain.correct_reads(mine) if mine else []
    del chain
    phase("shard corrected")
ex.close()
phase("communicator closed")
with open("%s.rank%d.pkl" % (out_prefix, rank), "wb") as f:
    pickle.dump(result, f)
