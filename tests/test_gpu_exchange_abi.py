"""The shipped multi-GPU exchange (br_amd/csrc/brx_exchange.hip: brx_comm_init, brx_exchange_build_partitioned,
brx_exchange_reduce_counts) run with world 2, 3, 5, 7 and 8 -- for real, not at world 1: `world` fresh processes share the
one card of the box, each drives the C ABI, and the library's ten librccl entry points are served by the test transport
tests/libfake_rccl.so (device -> host -> socket -> host -> device; selected with BRX_RCCL_PATH).  Everything above
those entry points -- owner bounds, per-peer send / recv counts, capped rounds, the clamped segment tables, the
finish of borrowed segments, the all-gather-v of the solid lists, the OR / index build from them, the clamp / widen /
narrow of the dense reduction, the status agreement -- is the product's code, checked bit for bit against the oracle.
Worlds 5, 7 and 8 are what the 8-GPU jobs run: owner bounds of 512 first digits are uneven at 5 and 7 and even at 8, the
tables are world x world, and the switch of the dense reduction is sat on from both sides.

That the inputs do what they are for -- messages of several rounds, ranks without reads, one rank with nearly all of
them, figures that another world or another sharding would not give -- is asserted first, on the CPU (the tests
without the gpu mark), from the oracle's hashes and the numpy statements of br_amd/dist.py (tests/world_runner.py).
Reference: there is no counterpart (one process, src/main.rs:30-33); src/lib.rs:72-139 is the loop being sharded."""
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
WORKER = os.path.join(HERE, "abi_exchange_worker.py")

# (world, k) of brx_exchange_build_partitioned.  k = 19 stays at worlds 2 and 3: eight ranks of a k = 19 set (2^37 hashes,
# the largest bit vector) on one card is a question of memory, not of the exchange, and not what this test is for.
PART_SMALL = [(2, 13), (3, 13), (2, 15), (3, 19), (2, 19), (2, 21), (3, 21)]     # 45 reads, BRX_A2A_CHUNK 30000
PART_LARGE = [(5, 13), (8, 13), (7, 15), (8, 15), (8, 21)]                        # all 206 reads, BRX_A2A_CHUNK 10000
FIVE_READS = (8, 15, 0, 5, None)                                                  # world, k, a, reads, cuts
SKEWED = (8, 15, 2, 157, (0, 150, 151, 152, 153, 154, 155, 156, 157))             # rank 0 holds 150 of 157 reads
SKEWED_CHUNK = 10000
FEW_SOLID = (8, 15, 4, 16)                                                        # world, k, a, reads: 4 solid k-mers in the job
# (world, a) of brx_exchange_reduce_counts: world * (a + 1) against 255
DENSE_SMALL = [(2, 2), (3, 2), (2, 200), (3, 100)]
DENSE_SWITCH = [(5, 50), (5, 51), (8, 30), (8, 31), (8, 2)]

_sets = {}


def _part_input(world, k):
    """(reads, BRX_A2A_CHUNK) of a (world, k) case"""
    return (206, 10000) if (world, k) in PART_LARGE else (45, 30000)


def _ref_set(k, n_reads, a):
    """the oracle's set of the first n_reads reads, computed once per (k, n_reads, a) and shared (never modified)"""
    key = (k, n_reads, a)
    if key not in _sets:
        reads = list(WR.fixture_reads()[:n_reads])
        _sets[key] = O.Solid.from_count(k, O.count_reads(k, reads), a) if k <= 15 else O.Solid.sparse_from_count(k, reads, a)
    return _sets[key]


def _run_world(tmp_path, world, k, a, n_reads, strategy, extra_env=None, cuts=None):
    assert os.path.exists(WR.FAKE), "tests/libfake_rccl.so not built: __graft_entry__.build()"
    argv = [k, a, n_reads, strategy] + ([",".join(str(c) for c in cuts)] if cuts else [])
    return WR.run_world(tmp_path, WORKER, world, argv, extra_env)


# ---- CPU: the inputs do what they are for ---------------------------------------------------------------------------

@pytest.mark.parametrize("world,k", PART_LARGE)
def test_large_worlds_take_several_rounds(world, k):
    """every case that claims several rounds: the largest per-peer message is at least 3 x BRX_A2A_CHUNK, every rank has
    reads and a message for every owner"""
    n_reads, chunk = _part_input(world, k)
    m = WR.part_messages(k, n_reads, world)
    assert m.shape == (world, world) and m.min() > 0
    assert m.max() >= 3 * chunk, (m.max(), chunk)
    assert m.sum() == sum(max(0, len(r) - k + 1) for r in WR.fixture_reads()[:n_reads])
    cuts = WR.shard_cuts(n_reads, world)
    assert all(hi > lo for lo, hi in zip(cuts, cuts[1:]))


@pytest.mark.parametrize("world,k", PART_LARGE)
def test_large_worlds_figures_are_their_own(world, k):
    """the exact per-rank figures the GPU test asserts would not come out of a job divided among world - 1 owners (for NO
    rank), nor -- where the reads do not divide evenly -- out of a sharding that is not shard_range"""
    n_reads, _ = _part_input(world, k)
    right = WR.part_messages(k, n_reads, world)
    fewer = WR.part_messages(k, n_reads, world, owners=world - 1)
    assert all(right[:, r].sum() != fewer[:, r].sum() for r in range(world - 1))
    assert right.max() != fewer.max()
    if n_reads % world:
        other = WR.part_messages(k, n_reads, world, cuts=WR.even_cuts(n_reads, world))
        assert WR.even_cuts(n_reads, world) != WR.shard_cuts(n_reads, world)
        assert not np.array_equal(right, other)
    b = D.owner_bounds(1 << WR.first_digit_bits(k), world)
    assert (len({hi - lo for lo, hi in zip(b, b[1:])}) > 1) == ((1 << WR.first_digit_bits(k)) % world != 0)


def test_owner_bounds_are_uneven_at_5_and_7_and_even_at_8():
    for world, even in ((5, False), (7, False), (8, True)):
        b = D.owner_bounds(512, world)
        assert (len({hi - lo for lo, hi in zip(b, b[1:])}) == 1) == even and b[0] == 0 and b[-1] == 512


def test_five_reads_leave_three_ranks_without_any():
    world, k, _, n_reads, _ = FIVE_READS
    cuts = WR.shard_cuts(n_reads, world)
    assert [hi - lo for lo, hi in zip(cuts, cuts[1:])] == [0, 1, 0, 1, 1, 0, 1, 1]
    m = WR.part_messages(k, n_reads, world)
    assert [int(x) for x in np.flatnonzero(m.sum(axis=1) == 0)] == [0, 2, 5]      # they send nothing ...
    assert m.sum(axis=0).min() > 0                                                # ... and own keys all the same


def test_one_rank_holds_the_largest_messages():
    """rank 0 holds 150 of 157 reads: the largest message anywhere is one of its, every one of them takes several rounds,
    and those of every other rank fit into one -- they must go through the rounds of rank 0 all the same"""
    world, k, _, n_reads, cuts = SKEWED
    m = WR.part_messages(k, n_reads, world, cuts)
    assert m.max() == m[0].max() and m[0].min() >= 3 * SKEWED_CHUNK
    assert 0 < m[1:].min() and m[1:].max() < SKEWED_CHUNK
    assert not np.array_equal(m, WR.part_messages(k, n_reads, world))             # shard_range would not give this


@pytest.mark.parametrize("case", ["five_reads", "skewed", "few_solid"])
def test_small_world_8_figures_are_their_own(case):
    """the cases with their own shards or thresholds, like the large ones: what the GPU tests assert for every rank is
    not what 7 owners would count (for NO rank), nor what another sharding would send"""
    world, k, a, n_reads = {"five_reads": FIVE_READS[:4], "skewed": SKEWED[:4], "few_solid": FEW_SOLID}[case]
    cuts = SKEWED[4] if case == "skewed" else None
    right = WR.part_messages(k, n_reads, world, cuts)
    fewer = WR.part_messages(k, n_reads, world, cuts, owners=world - 1)
    assert all(right[:, r].sum() != fewer[:, r].sum() for r in range(world - 1))
    assert right.max() != fewer.max()
    for other in (WR.even_cuts(n_reads, world), None if cuts is None else WR.shard_cuts(n_reads, world)):
        if other is not None and list(other) != WR.shard_cuts(n_reads, world, cuts):
            assert not np.array_equal(right, WR.part_messages(k, n_reads, world, cuts=other))
    if case == "few_solid":
        assert WR.part_solid_per_owner(k, n_reads, world, a)[:world - 1].tolist() != WR.part_solid_per_owner(k, n_reads, world - 1, a).tolist()
    # (16 reads divide evenly over 8 ranks: there only the owners tell; the other two did compare a sharding above)
    assert (WR.even_cuts(n_reads, world) != WR.shard_cuts(n_reads, world, cuts)) == (case != "few_solid")


def test_first_digit_widths():
    """the widths world_runner.first_digit_bits gives for every k in use here (the GPU tests compare them with the
    library's n_buckets): 128 first digits at k = 13, 512 from k = 15 on"""
    assert [WR.first_digit_bits(k) for k in (13, 15, 19, 21)] == [7, 9, 9, 9]


def test_few_solid_kmers_leave_owners_with_empty_lists():
    """16 reads, abundance 4: four owners find one solid k-mer each and four find none -- the list gather and the
    replication of the set run over eight lists of which half are empty"""
    world, k, a, n_reads = FEW_SOLID
    assert WR.part_solid_per_owner(k, n_reads, world, a).tolist() == [0, 1, 1, 0, 1, 0, 1, 0]
    assert _ref_set(k, n_reads, a).popcount() == 4


@pytest.mark.parametrize("world,a", DENSE_SMALL + DENSE_SWITCH)
def test_dense_cases_sit_where_they_say(world, a):
    exact = world * (a + 1) <= 255
    assert (D.exact_cap(a, world) is not None) == exact
    assert exact == ((world, a) in [(2, 2), (3, 2), (5, 50), (8, 30), (8, 2)])
    _, cnt = np.unique(np.concatenate(WR.read_hashes(11, 206)), return_counts=True)
    assert len(WR.fixture_reads()) == 206 and int((cnt > 255).sum()) == 5 and int(cnt.max()) == 1730


_STAND_IN = """
import os, pickle, sys, time
rank, world, prefix, mode = int(sys.argv[1]), int(sys.argv[2]), sys.argv[6], sys.argv[7]
if mode == "fail" and rank == 1:
    sys.exit("rank 1 gives up")
if mode in ("fail", "wait"):
    time.sleep(600)                    # a peer that waits for ever: the runner's to end
assert os.environ["BRX_DEVPOOL_GB"] == "1" and os.environ["BRX_HOSTPOOL_GB"] == "1"
open(prefix + ".traffic.rank%d" % rank, "w").write("3 %d" % (100 + rank))
pickle.dump({"rank": rank}, open(prefix + ".rank%d.pkl" % rank, "wb"))
"""


def test_the_runner_ends_a_world_whose_rank_failed_or_that_takes_too_long(tmp_path):
    """the supervision of tests/world_runner.py, on stand-in ranks without a GPU: a clean world comes back with every
    rank's pickle and traffic; once a rank has exited non-zero the others are killed after the grace period, and a world
    past its limit is killed too; both fail with every rank's exit code and the tail of its log, and nothing is retried"""
    script = tmp_path / "stand_in.py"
    script.write_text(_STAND_IN)
    (tmp_path / "ok").mkdir()
    res = WR.run_world(tmp_path / "ok", str(script), 8, [15, 0, 1, "ok"])
    assert [(x["rank"], x["msgs"], x["bytes"]) for x in res] == [(r, 3, 100 + r) for r in range(8)]
    with pytest.raises(AssertionError):
        WR.run_world(tmp_path, str(script), 9, [15, 0, 1, "ok"])                      # ten processes: refused before any starts
    for mode, kw, words in (("fail", {"grace": 0.3}, "a rank failed and its peers were still running"),
                            ("wait", {"limit": 0.3}, "did not end within")):
        (tmp_path / mode).mkdir()
        with pytest.raises(AssertionError) as e:
            WR.run_world(tmp_path / mode, str(script), 3, [15, 0, 1, mode], **kw)
        text = str(e.value)
        assert words in text and all("---- rank %d" % r in text for r in range(3))
        if mode == "fail":
            assert "[None, 1, None]" in text and "rank 1 gives up" in text
    assert [w[1] for w in WR.world_times[-3:]] == [8, 3, 3]


# ---- GPU ------------------------------------------------------------------------------------------------------------

def _check_set(res, ref, k):
    if k <= 15:
        assert res["solid_bytes"] == ref.to_bytes()               # every rank holds the set of ALL reads
    else:
        assert res["members"] == [ref.get(x) for x in res["sample"]]
        assert any(res["members"]) and not all(res["members"])


def _check_traffic(res, m, k, solid_here, chunk=None):
    """last_stats() of every rank against the CPU's message matrix m[s, r] (keys of shard s owned by rank r), exactly, and
    the messages the transport saw every rank send in its two builds: every capped round to every peer, and no more"""
    sent = WR.part_sent_messages(m, solid_here, chunk)
    assert [x["msgs"] for x in res] == sent.tolist()
    for r, x in enumerate(res):
        assert x["stats_0"]["solid_here"] == x["stats_1"]["solid_here"] == solid_here[r], r
        for st in (x["stats_0"], x["stats_1"]):
            assert st["keys_counted_here"] == m[:, r].sum(), r                         # the owner's digits and no others
            assert st["key_bytes_sent"] == 4 * (m[r].sum() - m[r, r]), r
            assert st["key_bytes_received"] == 4 * (m[:, r].sum() - m[r, r]), r
            assert st["largest_message_keys"] == m.max(), r                            # the same on every rank: it sets the rounds
        assert x["n_buckets"] == 1 << WR.first_digit_bits(k)


@gpu
@pytest.mark.parametrize("world,k", PART_SMALL + PART_LARGE)
def test_shipped_exchange_partitioned(tmp_path, raw_reads, world, k):
    """brx_exchange_build_partitioned at world 2 / 3 (uneven owner bounds: 512 first digits over 3 ranks) and at 5 / 7 / 8
    (uneven, uneven, even; 128 first digits at k = 13), several capped rounds of the key all-to-all and of the list
    gather (BRX_A2A_CHUNK far below the per-peer message).  The corrected reads are compared for every read up to 45
    reads and at (8, 15), for the first and the last read of every shard elsewhere."""
    a = 2
    n_reads, chunk = _part_input(world, k)
    res = _run_world(tmp_path, world, k, a, n_reads, "part", {"BRX_A2A_CHUNK": str(chunk)})
    reads = raw_reads[:n_reads]
    ref = _ref_set(k, n_reads, a)
    om = O.build_methods(ref, ["one", "graph"], 5, 7)
    cuts = WR.shard_cuts(n_reads, world)
    if n_reads <= 45 or (world, k) == (8, 15):
        which = list(range(n_reads))
    else:
        which = sorted({i for lo, hi in zip(cuts, cuts[1:]) for i in (lo, hi - 1)})
    expect = [O.correct_record(om, reads[i], False) for i in which]
    got = []
    n_kmers = sum(max(0, len(r) - k + 1) for r in reads)
    for r, x in enumerate(res):
        _check_set(x, ref, k)
        assert x["n_mine"] == cuts[r + 1] - cuts[r] == len(x["corrected_0"])
        assert x["corrected_0"] == x["corrected_1"]
        st = x["stats_1"]
        assert st["solid_job"] == x["popcount"] and 0 < st["solid_here"] < st["solid_job"]
        assert st["key_bytes_sent"] > 0 and st["key_bytes_received"] > 0
        assert st["largest_message_keys"] > 30000 and x["msgs"] > 4 * (world - 1)      # really several rounds
        if k >= 15:
            assert x["index"]["valid"]
        got += x["corrected_0"]
    assert sum(x["stats_1"]["keys_counted_here"] for x in res) == n_kmers              # every key reached ONE owner
    assert [got[i] for i in which] == expect and len(got) == n_reads                   # shards concatenate in input order
    m = WR.part_messages(k, n_reads, world)
    assert m.max() >= (3 * chunk if (world, k) in PART_LARGE else chunk)
    _check_traffic(res, m, k, WR.part_solid_per_owner(k, n_reads, world, a), chunk)


@gpu
def test_shipped_exchange_world_8_with_five_reads(tmp_path, raw_reads):
    """5 reads over 8 ranks: ranks 0, 2 and 5 count nothing, join every collective, own their digits and end with the
    whole set"""
    world, k, a, n_reads, _ = FIVE_READS
    res = _run_world(tmp_path, world, k, a, n_reads, "part")
    assert [x["n_mine"] for x in res] == [0, 1, 0, 1, 1, 0, 1, 1]
    ref = _ref_set(k, n_reads, a)
    m = WR.part_messages(k, n_reads, world)
    _check_traffic(res, m, k, WR.part_solid_per_owner(k, n_reads, world, a))
    for r, x in enumerate(res):
        _check_set(x, ref, k)
        st = x["stats_1"]
        assert x["popcount"] == st["solid_job"] and 0 < st["solid_here"] < st["solid_job"]
        assert x["index"]["valid"]
        if not x["n_mine"]:
            assert st["key_bytes_sent"] == 0 and st["keys_counted_here"] > 0 and x["corrected_0"] == []
    assert sum(x["stats_1"]["keys_counted_here"] for x in res) == sum(len(r) - k + 1 for r in raw_reads[:n_reads])


@gpu
def test_shipped_exchange_one_rank_holds_most_reads(tmp_path, raw_reads):
    """rank 0 holds 150 of 157 reads: the largest message anywhere is one of its, and the seven ranks whose own messages
    fit into one round go through every round of rank 0's.  Every rank's sent messages are counted exactly: rank 0 sends
    each peer one message in each of that peer's rounds, the others one key message per peer.  That the others also
    RECEIVED every round shows in what they end with: each owner's part of the set holds rank 0's keys of all its rounds
    (the bytes of every rank's set against the oracle, solid_here against the CPU's count), and a rank that posted
    fewer receives would leave rank 0's message of another size in front of its next receive: the transport aborts on
    that, the runner fails the world."""
    world, k, a, n_reads, cuts = SKEWED
    res = _run_world(tmp_path, world, k, a, n_reads, "part", {"BRX_A2A_CHUNK": str(SKEWED_CHUNK)}, cuts=cuts)
    assert [x["n_mine"] for x in res] == [150, 1, 1, 1, 1, 1, 1, 1]
    ref = _ref_set(k, n_reads, a)
    m = WR.part_messages(k, n_reads, world, cuts)
    solid_here = WR.part_solid_per_owner(k, n_reads, world, a)
    _check_traffic(res, m, k, solid_here, SKEWED_CHUNK)
    rounds = -(-int(m.max()) // SKEWED_CHUNK)
    per_build = 5 * (world - 1) + (world - 1) * -(-int(solid_here[1]) // (SKEWED_CHUNK // 2))
    assert res[1]["msgs"] == 2 * (per_build + (world - 1))                             # one key message per peer, no more
    om = O.build_methods(ref, ["one", "graph"], 5, 7)
    for r, x in enumerate(res):
        _check_set(x, ref, k)
        st = x["stats_1"]
        assert x["popcount"] == st["solid_job"] and 0 < st["solid_here"] < st["solid_job"]
        assert x["index"]["valid"] and x["corrected_0"] == x["corrected_1"]
        first, last = cuts[r], cuts[r + 1] - 1
        assert x["corrected_0"][0] == O.correct_record(om, raw_reads[first], False)
        assert x["corrected_0"][-1] == O.correct_record(om, raw_reads[last], False)
    assert rounds >= 3 and res[0]["msgs"] >= 2 * rounds * (world - 1)                  # both builds: every round, every peer


@gpu
def test_shipped_exchange_owners_with_empty_solid_lists(tmp_path, raw_reads):
    """four solid k-mers in the whole job, one each at four of the eight owners: every rank ends with exactly those four"""
    world, k, a, n_reads = FEW_SOLID
    res = _run_world(tmp_path, world, k, a, n_reads, "part")
    ref = _ref_set(k, n_reads, a)
    here = WR.part_solid_per_owner(k, n_reads, world, a)
    _check_traffic(res, WR.part_messages(k, n_reads, world), k, here)
    for r, x in enumerate(res):
        _check_set(x, ref, k)
        assert x["popcount"] == 4 and x["corrected_0"] == x["corrected_1"]
        for st in (x["stats_0"], x["stats_1"]):
            assert st["solid_job"] == 4, r


@gpu
def test_shipped_exchange_with_an_empty_shard(tmp_path, raw_reads):
    """2 reads over 3 ranks: rank 0 counts nothing and must still join every collective (it used to leave its peers
    waiting in the first all-gather), own a digit range, and end with the whole set."""
    k, a = 15, 0
    res = _run_world(tmp_path, 3, k, a, 2, "part")
    assert [x["n_mine"] for x in res] == [0, 1, 1]
    ref = O.Solid.from_count(k, O.count_reads(k, raw_reads[:2]), a)
    for x in res:
        _check_set(x, ref, k)
        assert x["popcount"] == x["stats_1"]["solid_job"]
    assert res[0]["stats_1"]["key_bytes_sent"] == 0 and res[0]["stats_1"]["keys_counted_here"] > 0


@gpu
@pytest.mark.parametrize("world,a", DENSE_SMALL + DENSE_SWITCH)
def test_shipped_exchange_dense_reduce(tmp_path, raw_reads, world, a):
    """brx_exchange_reduce_counts, north_star's form (all-reduce of the u8 count vector, then every rank thresholds):
    exact u8 sums while world * (a + 1) <= 255 -- against a transport whose u8 SUM wraps like RCCL's -- and int32
    slices beyond (a = 200, and 3 x 101 = 303).  k = 11 on the whole fixture: five k-mers are counted 256 ... 1730 times.
    Worlds 5 and 8 sit on the switch: 5 x 51 = 255 (u8, at equality), 5 x 52 = 260 (int32), 8 x 31 = 248, 8 x 32 = 256.
    Which path ran shows in the bytes a rank sent: the 2^21-byte table once to every peer, or four times that."""
    k = 11
    res = _run_world(tmp_path, world, k, a, len(raw_reads), "dense")
    ref = _ref_set(k, len(raw_reads), a)
    table_bytes = 1 << (2 * k - 1)
    width = 1 if D.exact_cap(a, world) is not None else 4
    for x in res:
        assert x["solid_bytes"] == ref.to_bytes()
        # the table to every peer, and a status word or two: nothing near another table
        assert 0 <= x["bytes"] - width * table_bytes * (world - 1) < 4096, (x["bytes"], width)
    assert res[0]["popcount"] > 0


@gpu
def test_dense_reduce_wide_path_at_world_one(monkeypatch):
    """the widen -> int32 all-reduce -> saturating narrow path through REAL librccl (world 1 is all a one-GPU box can
    give it), forced with BRX_EXCHANGE_FORCE_WIDE: the table must come back unchanged"""
    from br_amd import dist as D
    k, a = 13, 3
    cfg = synth.config(genome_len=30_000, read_len=2_000)
    g = synth.genome_host(cfg)
    bases, offs = synth.reads_host(cfg, g, 0, 300)
    plain = br_amd.Counter(k, 0, _lib.COUNT_DENSE)
    plain.add_batch(bases, offs)
    ref = plain.finish(a)
    monkeypatch.setenv("BRX_EXCHANGE_FORCE_WIDE", "1")
    ex = D.AbiExchange(1, 0, 0)
    cnt = br_amd.Counter(k, 0, _lib.COUNT_DENSE)
    cnt.add_batch(bases, offs)
    ex.reduce_counts(cnt, a, None)
    assert cnt.finish(a).to_solid_bytes() == ref.to_solid_bytes()
    ex.close()
