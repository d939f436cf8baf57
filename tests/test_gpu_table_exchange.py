"""Counted sets across ranks at any odd k up to 31: the counting tables of the ranks merged by owner
(br_amd/csrc/brx_exchange.hip brx_exchange_table_merge / _spectrum / _table_finish, the split and merge kernels of
brx_counttable.hip), run with world 2, 3, 5, 7 and 8 for real in the manner of test_gpu_exchange_abi.py: `world` fresh
processes (tests/table_exchange_worker.py) share the one card, the library's librccl entry points are served by
tests/libfake_rccl.so.  Expected values: the CPU oracle's sets and corrections, the owners br_amd.dist.table_owner names, and
a table counter of this process that counted all the reads at once -- what the ranks together must reproduce bin for bin.
That the inputs do what they are for is asserted first, on the CPU (the tests without the gpu mark; tests/world_runner.py).
Reference: no counterpart (one process, src/main.rs:30-33); src/lib.rs:72-139 is the loop being sharded."""
import os

import numpy as np
import pytest

import br_amd
from br_amd import _lib, synth
from br_amd import dist as D
from oracle import oracle as O
from tests import world_runner as WR

gpu = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "table_exchange_worker.py")
TABLE = _lib.COUNT_TABLE

LARGE_K_SMALL = [(2, 23), (3, 25), (3, 31)]        # 150 reads, BRX_A2A_CHUNK 30000
LARGE_K_LARGE = [(5, 23), (8, 25), (7, 31)]        # 150 reads, BRX_A2A_CHUNK 8000: a third of the smallest of their largest messages
LARGE_K_READS = 150
EMPTY_8 = (8, 23, 0, 3)                            # world, k, a, reads

_cache = {}


def _ref_set(k, reads, n, a):
    """the oracle's set, computed once per case and shared (never modified)"""
    key = (k, n, a)
    if key not in _cache:
        _cache[key] = O.Solid.from_count(k, O.count_reads(k, reads), a) if k <= 15 else O.Solid.sparse_from_count(k, reads, a)
    return _cache[key]


def _large_k_chunk(world, k):
    return 8000 if (world, k) in LARGE_K_LARGE else 30000


def _run_world(tmp_path, world, k, a, n_reads, mode, extra_env=None):
    assert os.path.exists(WR.FAKE), "tests/libfake_rccl.so not built: __graft_entry__.build()"
    return WR.run_world(tmp_path, WORKER, world, [k, a, n_reads, mode], extra_env)


# ---- CPU: the inputs do what they are for ---------------------------------------------------------------------------

@pytest.mark.parametrize("world,k", LARGE_K_LARGE)
def test_large_worlds_take_several_rounds(world, k):
    """the largest per-peer message (entries) is at least 3 x BRX_A2A_CHUNK; every rank has reads and entries for every owner"""
    m = WR.table_messages(k, LARGE_K_READS, world)
    assert m.shape == (world, world) and m.min() > 0
    assert m.max() >= 3 * _large_k_chunk(world, k), (m.max(), _large_k_chunk(world, k))


@pytest.mark.parametrize("world,k", LARGE_K_LARGE)
def test_large_worlds_figures_are_their_own(world, k):
    """the exact per-rank key counts the GPU test asserts are not those of world - 1 owners, for any rank; and where the
    reads do not divide evenly the messages are not those of a sharding other than shard_range"""
    right = WR.table_keys_per_owner(k, LARGE_K_READS, world)
    fewer = WR.table_keys_per_owner(k, LARGE_K_READS, world - 1)
    assert right.sum() == fewer.sum() and all(right[r] != fewer[r] for r in range(world - 1))
    assert right.sum() == np.unique(np.concatenate(WR.read_hashes(k, LARGE_K_READS))).size
    if LARGE_K_READS % world:
        other = WR.table_messages(k, LARGE_K_READS, world, cuts=WR.even_cuts(LARGE_K_READS, world))
        assert not np.array_equal(WR.table_messages(k, LARGE_K_READS, world), other)
    else:
        assert (world, k) == (5, 23)                                                   # 150 = 5 x 30: only the owners tell


def test_three_reads_leave_five_ranks_without_any():
    world, k, _, n_reads = EMPTY_8
    cuts = WR.shard_cuts(n_reads, world)
    assert [hi - lo for lo, hi in zip(cuts, cuts[1:])] == [0, 0, 1, 0, 0, 1, 0, 1]
    m = WR.table_messages(k, n_reads, world)
    assert [int(x) for x in np.flatnonzero(m.sum(axis=1) == 0)] == [0, 1, 3, 4, 6]
    assert WR.table_keys_per_owner(k, n_reads, world).min() > 0                       # every rank owns k-mers all the same


def test_three_reads_figures_are_their_own():
    """the exact per-rank figures of the 3-read job are not those of 7 owners, for any rank"""
    world, k, _, n_reads = EMPTY_8
    right, fewer = WR.table_keys_per_owner(k, n_reads, world), WR.table_keys_per_owner(k, n_reads, world - 1)
    assert right.sum() == fewer.sum() and all(right[r] != fewer[r] for r in range(world - 1))
    m, mf = WR.table_messages(k, n_reads, world), WR.table_messages(k, n_reads, world, owners=world - 1)
    assert all(m[:, r].sum() != mf[:, r].sum() for r in range(world - 1))
    assert not np.array_equal(m, WR.table_messages(k, n_reads, world, cuts=WR.even_cuts(n_reads, world)))


# ---- GPU ------------------------------------------------------------------------------------------------------------

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


def _check_owners(res, world, k, a, n_reads):
    """the CPU's statement of who owns what, exactly: the keys of every merged counter, its solid ones, the merge's traffic"""
    keys = WR.table_keys_per_owner(k, n_reads, world)
    solid = WR.table_keys_per_owner(k, n_reads, world, a)
    m = WR.table_messages(k, n_reads, world)
    for r, x in enumerate(res):
        sm = x["stats_merge"]
        assert x["keys"] == keys[r], r                                                 # table_owner(h, world) == r and no others
        assert x["stats"]["solid_here"] == solid[r], r
        assert sm["keys_counted_here"] == m[:, r].sum(), r                             # one entry per source that has the key
        assert sm["key_bytes_sent"] == 9 * (m[r].sum() - m[r, r]), r
        assert sm["key_bytes_received"] == 9 * (m[:, r].sum() - m[r, r]), r
        assert sm["largest_message_keys"] == m.max(), r                                # the same on every rank: it sets the rounds
    return m


@gpu
@pytest.mark.parametrize("world,k", LARGE_K_SMALL + LARGE_K_LARGE)
def test_table_exchange_large_k(tmp_path, raw_reads, world, k):
    """the feature: a counted set at k >= 23 over 2 / 3 / 5 / 7 / 8 ranks, several capped rounds of the pair all-to-all"""
    reads = raw_reads[:LARGE_K_READS]
    chunk = _large_k_chunk(world, k)
    res = _run_world(tmp_path, world, k, 1, LARGE_K_READS, "raw", {"BRX_A2A_CHUNK": str(chunk)})
    _check_job(res, world, k, 1, reads, True)
    assert res[0]["popcount"] > 1000
    m = _check_owners(res, world, k, 1, LARGE_K_READS)
    assert m.max() >= (3 * chunk if (world, k) in LARGE_K_LARGE else chunk // 2)


@gpu
@pytest.mark.parametrize("world,k", [(2, 15), (2, 21)])
def test_table_exchange_bit_vector_and_smallest_sparse_k(tmp_path, raw_reads, world, k):
    """a destination with a bit vector (k = 15: to_solid_bytes against the dense oracle) and the smallest sparse k"""
    reads = raw_reads[:45]
    res = _run_world(tmp_path, world, k, 2, 45, "raw", {"BRX_A2A_CHUNK": "30000"})
    _check_job(res, world, k, 2, reads, False)


@gpu
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


@gpu
def test_table_exchange_with_an_empty_shard(tmp_path, raw_reads):
    """2 reads over 3 ranks: rank 0 counts nothing, joins every collective, owns its share and ends with the whole set"""
    k, a = 23, 0
    res = _run_world(tmp_path, 3, k, a, 2, "raw")
    assert [x["n_mine"] for x in res] == [0, 1, 1]
    _check_job(res, 3, k, a, raw_reads[:2], False)
    sm = res[0]["stats_merge"]
    assert sm["key_bytes_sent"] == 0 and sm["keys_counted_here"] > 0 and res[0]["keys"] > 0
    assert res[0]["stats"]["solid_here"] > 0


@gpu
def test_table_exchange_world_8_with_three_reads(tmp_path, raw_reads):
    """3 reads over 8 ranks: five ranks count nothing, join every collective, own their share and end with the whole set"""
    world, k, a, n_reads = EMPTY_8
    res = _run_world(tmp_path, world, k, a, n_reads, "raw")
    assert [x["n_mine"] for x in res] == [0, 0, 1, 0, 0, 1, 0, 1]
    _check_job(res, world, k, a, raw_reads[:n_reads], False)
    _check_owners(res, world, k, a, n_reads)
    for x in res:
        sm = x["stats_merge"]
        if not x["n_mine"]:
            assert sm["key_bytes_sent"] == 0 and sm["keys_counted_here"] > 0 and x["keys"] > 0
        assert x["stats"]["solid_here"] > 0


@gpu
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
