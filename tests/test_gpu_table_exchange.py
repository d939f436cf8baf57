"""Counted sets across ranks at any odd k up to 31: the counting tables of the ranks merged by owner
(br_amd/csrc/brx_exchange.hip brx_exchange_table_merge / _spectrum / _table_finish, the split and merge kernels of
brx_counttable.hip), run with world 2 and 3 for real in the manner of test_gpu_exchange_abi.py: `world` fresh processes
(tests/table_exchange_worker.py) share the one card, the library's librccl entry points are served by
tests/libfake_rccl.so.  Expected values: the CPU oracle's sets and corrections, and a table counter of this process
that counted all the reads at once -- what the ranks together must reproduce bin for bin.
Reference: no counterpart (one process, src/main.rs:30-33); src/lib.rs:72-139 is the loop being sharded."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import br_amd
from br_amd import _lib, synth
from br_amd import dist as D
from oracle import oracle as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FAKE = os.path.join(HERE, "libfake_rccl.so")
WORKER = os.path.join(HERE, "table_exchange_worker.py")
TABLE = _lib.COUNT_TABLE

_cache = {}


def _ref_set(k, reads, n, a):
    """the oracle's set, computed once per case and shared (never modified)"""
    key = (k, n, a)
    if key not in _cache:
        _cache[key] = O.Solid.from_count(k, O.count_reads(k, reads), a) if k <= 15 else O.Solid.sparse_from_count(k, reads, a)
    return _cache[key]


def _run_world(tmp_path, world, k, a, n_reads, mode, extra_env=None):
    assert os.path.exists(FAKE), "tests/libfake_rccl.so not built: __graft_entry__.build()"
    assert world + 1 <= 4                                         # processes that hold the GPU at once, this one included
    prefix = str(tmp_path / "x")
    env = dict(os.environ)
    env["BRX_RCCL_PATH"] = FAKE
    env["FAKE_RCCL_DIR"] = str(tmp_path)
    env["FAKE_RCCL_STATS"] = prefix + ".traffic"
    env.update(extra_env or {})
    procs = [subprocess.Popen([sys.executable, WORKER, str(r), str(world), str(k), str(a), str(n_reads), prefix, mode], env=env)
             for r in range(world)]
    try:
        codes = [p.wait(timeout=280) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert codes == [0] * world
    out = []
    for r in range(world):
        with open("%s.rank%d.pkl" % (prefix, r), "rb") as f:
            out.append(pickle.load(f))
        with open("%s.traffic.rank%d" % (prefix, r)) as f:
            out[-1]["msgs"], out[-1]["bytes"] = (int(x) for x in f.read().split())
    return out


def _check_job(res, world, k, a, reads, several_rounds):
    """everything the ranks of one job must reproduce: the single process's counter, the oracle's set and corrections"""
    ref = _ref_set(k, reads, len(reads), a)
    one = br_amd.Counter(k, 0, TABLE)
    one.add_reads(reads)
    spec = one.spectrum()
    whole = one.finish(a)
    fp = whole.fingerprint()
    assert fp[0] == ref.popcount() > 0
    om = O.build_methods(ref, ["one", "graph"], 5, 7)
    got = []
    for r, x in enumerate(res):
        assert x["state_before"] == (0, 0) and x["state_after"] == (world, r)
        assert np.array_equal(x["spectrum"], spec)                                   # all 256 bins, on every rank
        assert x["popcount"] == ref.popcount() and x["fingerprint"] == fp            # every rank holds the set of ALL reads
        want = [ref.get(q) for q in x["sample"]]
        assert x["members"] == want and any(want) and not all(want)
        # the merged counter answers for the k-mers its rank owns, with the counts of the whole job, and 0 for the rest
        owner = D.table_owner(np.array([O.khash(q, k) for q in x["sample"]], dtype=np.uint64), world)
        counts = one.get_counts(x["sample"])
        assert counts.max() > a and np.array_equal(x["counts"], np.where(owner == r, counts, 0))
        st, sm = x["stats"], x["stats_merge"]
        assert st["solid_job"] == ref.popcount()
        assert sm["keys_counted_here"] >= x["keys"] > 0 and sm["solid_here"] == 0
        if several_rounds:
            assert 0 < st["solid_here"] < st["solid_job"]
            assert sm["key_bytes_sent"] > 0 and sm["key_bytes_received"] > 0
            assert sm["largest_message_keys"] > 15000 and x["msgs"] > 4 * (world - 1)    # really several rounds
        if k >= 15:
            assert x["index"]["valid"]
        if k <= 15:
            assert x["solid_bytes"] == ref.to_bytes()
        assert x["corrected"] == [O.correct_record(om, s, False) for s in reads[slice(*D.shard_range(len(reads), world, r))]]
        got += x["corrected"]
    assert sum(x["keys"] for x in res) == one.table_info()["keys"]                    # every k-mer has ONE owner
    assert sum(x["stats"]["solid_here"] for x in res) == ref.popcount()
    assert len(got) == len(reads)                                                      # shards concatenate in input order
    return res


@pytest.mark.parametrize("world,k", [(2, 23), (3, 25), (3, 31)])
def test_table_exchange_large_k(tmp_path, raw_reads, world, k):
    """the feature: a counted set at k >= 23 over 2 / 3 ranks, several capped rounds of the pair all-to-all"""
    reads = raw_reads[:150]
    res = _run_world(tmp_path, world, k, 1, 150, "raw", {"BRX_A2A_CHUNK": "30000"})
    _check_job(res, world, k, 1, reads, True)
    assert res[0]["popcount"] > 1000


@pytest.mark.parametrize("world,k", [(2, 15), (2, 21)])
def test_table_exchange_bit_vector_and_smallest_sparse_k(tmp_path, raw_reads, world, k):
    """a destination with a bit vector (k = 15: to_solid_bytes against the dense oracle) and the smallest sparse k"""
    reads = raw_reads[:45]
    res = _run_world(tmp_path, world, k, 2, 45, "raw", {"BRX_A2A_CHUNK": "30000"})
    _check_job(res, world, k, 2, reads, False)


def test_table_exchange_sums_and_saturation(tmp_path):
    """each of two ranks counts poly-A 200 times and poly-C 60 times: the owner reads min(255, 400) and 120, the other
    rank 0; four thresholds on the same merged counter"""
    k = 25
    res = _run_world(tmp_path, 2, k, 0, 4, "sat")
    probes = [O.seq2bit(b"A" * k), O.seq2bit(b"C" * k)]
    owner = D.table_owner(np.array([O.khash(q, k) for q in probes], dtype=np.uint64), 2)
    for r, x in enumerate(res):
        assert x["counts"] == [255 if owner[0] == r else 0, 120 if owner[1] == r else 0]
        assert x["state_end"] == (2, r)
        for thr, want in ((254, [True, False]), (255, [False, False]), (119, [True, True]), (120, [True, False])):
            members, fp = x["finish"][thr]
            assert members == want, thr
            assert fp == res[0]["finish"][thr][1] and fp[0] == sum(want)          # both ranks agree on the set each time
    spec = res[0]["spectrum"]
    assert int(spec[255]) == 1 and int(spec[120]) == 1 and int(spec[1:].sum()) == 2
    assert np.array_equal(res[1]["spectrum"], spec)
    assert sum(x["keys"] for x in res) == 2


def test_table_exchange_with_an_empty_shard(tmp_path, raw_reads):
    """2 reads over 3 ranks: rank 0 counts nothing, joins every collective, owns its share and ends with the whole set"""
    k, a = 23, 0
    res = _run_world(tmp_path, 3, k, a, 2, "raw")
    assert [x["n_mine"] for x in res] == [0, 1, 1]
    _check_job(res, 3, k, a, raw_reads[:2], False)
    sm = res[0]["stats_merge"]
    assert sm["key_bytes_sent"] == 0 and sm["keys_counted_here"] > 0 and res[0]["keys"] > 0
    assert res[0]["stats"]["solid_here"] > 0


def test_table_exchange_world_one_through_librccl():
    """merge, spectrum and finish through REAL librccl (world 1 is all a one-GPU box can give it: every entry takes the
    split -> copy -> merge path), and the state rules of a merged counter"""
    k, a = 25, 3
    cfg = synth.config(genome_len=30_000, read_len=2_000)
    g = synth.genome_host(cfg)
    bases, offs = synth.reads_host(cfg, g, 0, 300)
    plain = br_amd.Counter(k, 0, TABLE)
    plain.add_batch(bases, offs)
    spec = plain.spectrum()
    fp = plain.finish(a).fingerprint()
    assert fp[0] > 0
    ex = D.AbiExchange(1, 0, 0)
    cnt = br_amd.Counter(k, 0, TABLE)
    cnt.add_batch(bases, offs)
    assert cnt.merge_state() == (0, 0)
    ex.merge_table(cnt)
    assert cnt.merge_state() == (1, 0)
    assert cnt.table_info()["keys"] == plain.table_info()["keys"] == ex.last_stats()["keys_counted_here"]
    assert np.array_equal(ex.spectrum(cnt), spec)
    solid = br_amd.Pcon.new(k)
    ex.finish_table(cnt, solid, a)
    assert solid.fingerprint() == fp
    ex.finish_table(cnt, solid, a + 1)                                                # the counter is left merged and untouched
    assert solid.fingerprint() == plain.finish(a + 1).fingerprint()
    with pytest.raises(_lib.BrxError) as e:
        cnt.add_reads([b"ACGT" * 20])
    assert e.value.status == _lib.BRX_ERR_ARG
    with pytest.raises(_lib.BrxError) as e:
        ex.merge_table(cnt)                                                           # a second merge
    assert e.value.status == _lib.BRX_ERR_ARG
    cnt.reset()                                                                       # reopens it
    assert cnt.merge_state() == (0, 0)
    cnt.add_batch(bases, offs)
    with pytest.raises(_lib.BrxError) as e:
        ex.spectrum(cnt)                                                              # not merged
    assert e.value.status == _lib.BRX_ERR_ARG
    solid2 = br_amd.Pcon.new(k)
    ex.build_table(cnt, solid2, a)                                                    # merge + finish
    assert solid2.fingerprint() == fp
    part = br_amd.Counter(15, 0, _lib.COUNT_SORTED)
    with pytest.raises(_lib.BrxError) as e:
        ex.merge_table(part)
    assert e.value.status == _lib.BRX_ERR_UNSUPPORTED
    cnt.reset()
    with pytest.raises(_lib.BrxError) as e:
        ex.build_partitioned(cnt, solid, a, None)                                     # still refused, as before
    assert e.value.status == _lib.BRX_ERR_UNSUPPORTED
    ex.close()
