"""The chain executes what plan_pass (br_amd/csrc/brx_plan.hpp) decides, from ONE reading of the switches per batch, taken
on the thread that calls the library: the form a pass took shows in Chain.last_stats() and in the profile timers, the
bytes are the oracle's whatever the form.  The rule itself is checked without a GPU by test_pass_plan_cpu.py."""
import functools

import pytest

import br_amd
from br_amd import _lib, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CONFIRM, MAX_SEARCH = 2, 7


@pytest.fixture(scope="module")
def reads(raw_reads):
    return tuple(r[:2000] for r in raw_reads[:25])


@pytest.fixture(scope="module")
def expected(reads, solid_fixture_bytes):
    ref = O.Solid.from_bytes(solid_fixture_bytes)

    @functools.lru_cache(maxsize=None)
    def of(names, two_side):
        om = O.build_methods(ref, list(names), CONFIRM, MAX_SEARCH)
        return [O.correct_record(om, r, two_side) for r in reads]
    return of


def chain_of(gs, names, two_side):
    return br_amd.Chain(gs, [(m, CONFIRM, MAX_SEARCH) for m in names], two_side=two_side)


def test_one_takes_the_lane_form_unless_switched_off(monkeypatch, reads, expected, solid_fixture_bytes):
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    monkeypatch.delenv("BRX_LANE", raising=False)
    chain = chain_of(gs, ("one",), True)
    assert chain.correct_reads(reads) == expected(("one",), True)
    assert chain.last_stats()["lane_units"] > 0
    monkeypatch.setenv("BRX_LANE", "0")
    chain = chain_of(gs, ("one",), True)
    assert chain.correct_reads(reads) == expected(("one",), True)
    assert chain.last_stats()["lane_units"] == 0


def test_graph_reverse_pass_is_lean_unless_switched_off(monkeypatch, reads, expected, solid_fixture_bytes):
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    _lib.profile_enable(True)
    try:
        for lean, launched in ((None, True), ("0", False)):
            if lean is None:
                monkeypatch.delenv("BRX_REV_LEAN", raising=False)
            else:
                monkeypatch.setenv("BRX_REV_LEAN", lean)
            _lib.profile_reset()
            assert chain_of(gs, ("graph",), False).correct_reads(reads) == expected(("graph",), False)
            assert _lib.profile_get("correct_pass_graph")[1] > 0
            assert (_lib.profile_get("rev_verify")[1] > 0) == launched, lean
    finally:
        _lib.profile_enable(False)


def test_switches_are_read_per_batch_not_per_chain(monkeypatch, reads, expected, solid_fixture_bytes):
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    chain = chain_of(gs, ("one",), True)
    monkeypatch.setenv("BRX_LANE", "0")
    assert chain.correct_reads(reads) == expected(("one",), True)
    assert chain.last_stats()["lane_units"] == 0
    monkeypatch.delenv("BRX_LANE")
    assert chain.correct_reads(reads) == expected(("one",), True)
    assert chain.last_stats()["lane_units"] > 0


def test_async_batch_runs_under_the_switches_of_the_call(monkeypatch, reads, expected, solid_fixture_bytes):
    """the record is taken by brx_chain_correct_batch_async itself, on the calling thread: what the host does to its
    environment once the call has returned does not reach the batch"""
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    chain = chain_of(gs, ("one",), True)
    bases, offs = br_amd.pack_reads(reads)
    monkeypatch.setenv("BRX_LANE", "0")
    chain.correct_batch_async(bases, offs)
    monkeypatch.delenv("BRX_LANE")
    out, oo = chain.correct_batch_wait()
    got = [out[int(oo[i]):int(oo[i + 1])].tobytes() for i in range(len(reads))]
    assert got == expected(("one",), True)
    assert chain.last_stats()["lane_units"] == 0


# ---- every launch route of the group kernels (brx_group.hip, brx_one.hip, brx_revscan.hip) ------------------------------
# All forms of a pass give the same bytes, so a launch that went to another kernel than the planned one shows in no
# comparison with the oracle.  What does tell the forms apart: lane_units (the lane form ran), the rev_verify / rev_redo
# timers (the lean reverse form ran), lane_redone_reads (the list form had work), and `rounds`, which the group kernels
# count per GROUP: a trigger-free stretch of L positions is ceil(L / G) SCAN rounds of a G-lane group, while the rounds a
# trigger costs (ALTS, SCEN, MORE, a walk step) do not grow with G -- so over reads of kilobases the count falls strictly
# with every doubling of the width, and a launch that took another width than the one asked for breaks the order.

ROUTE_SWITCHES = ("BRX_GROUP", "BRX_GROUP_REV", "BRX_GROUP_WALK", "BRX_LANE", "BRX_LANE_WALK", "BRX_LANE_REV", "BRX_LANE_CHUNK",
                  "BRX_LANE_SYNC", "BRX_REV_LEAN", "BRX_REV_LEAN_ONE", "BRX_REV_VERIFY_G", "BRX_ONE_V1")


@pytest.fixture
def switches(monkeypatch):
    def set_(**env):
        for key in ROUTE_SWITCHES:
            monkeypatch.delenv(key, raising=False)
        for key, v in env.items():
            monkeypatch.setenv(key, str(v))
    return set_


@pytest.fixture(scope="module")
def fixture_case(raw_reads, solid_fixture_bytes):
    """the 206 records of raw.fasta against the reference's k = 11 set (the kernels' general-k instantiation); the
    oracle's answer once per chain"""
    ref = O.Solid.from_bytes(solid_fixture_bytes)

    @functools.lru_cache(maxsize=None)
    def want(names, two_side):
        om = O.build_methods(ref, list(names), CONFIRM, MAX_SEARCH)
        return [O.correct_record(om, r, two_side) for r in raw_reads]
    return br_amd.Pcon.from_pcon_solid(solid_fixture_bytes), tuple(raw_reads), want


@functools.lru_cache(maxsize=None)
def synthetic_case(k):
    """test_gpu_lane.py's synthetic reads against their own counted set: k = 19 and k = 21 are the instantiations the
    kernels have beside the general one"""
    cfg = synth.config(genome_len=40_000, read_len=3_000)
    bases, offs = synth.reads_host(cfg, synth.genome_host(cfg), 0, 300)
    reads = tuple(bases[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(300))
    om = O.build_methods(O.Solid.sparse_from_count(k, reads, 2), ["one"], CONFIRM, MAX_SEARCH)
    return br_amd.Pcon.from_count(list(reads), k, 2), reads, {True: [O.correct_record(om, r, True) for r in reads],
                                                              False: [O.correct_record(om, r, False) for r in reads]}


def rounds_by_width(switches, gs, names, reads, want, widths, **env):
    """the chain at every width, lane form off, forward + reverse: every read the oracle's; the rounds of each run"""
    rounds = []
    for w in widths:
        switches(BRX_LANE=0, BRX_GROUP=w, BRX_GROUP_WALK=w, **env)
        chain = chain_of(gs, names, False)
        got = chain.correct_reads(reads)
        bad = [i for i in range(len(reads)) if got[i] != want[i]]
        assert not bad, (w, bad[:5])
        st = chain.last_stats()
        assert st["lane_units"] == 0 and st["fixes"] > 0, (w, st)
        rounds.append(st["rounds"])
    return rounds


@pytest.mark.parametrize("method,widths,env", [
    ("one", (4, 8, 16, 64), {}),                                  # one_kernel<4 | 8 | 16 | 64>
    ("one", (8, 16, 32, 64), {"BRX_ONE_V1": 1}),                  # correct_kernel<8 | 16 | 32 | 64, One>
    ("two", (16, 32, 64), {}),
    ("graph", (4, 8, 16, 32, 64), {"BRX_REV_LEAN": 0}),           # (BRX_GROUP_WALK: 4 and 8 lanes are its widths)
    ("greedy", (16, 32, 64), {}),
    ("gap_size", (4, 8, 16, 32, 64), {"BRX_REV_LEAN": 0}),
], ids=["one", "one_v1", "two", "graph", "greedy", "gap_size"])
def test_group_kernel_runs_at_the_width_asked_for(switches, fixture_case, method, widths, env):
    gs, reads, want = fixture_case
    rounds = rounds_by_width(switches, gs, (method,), reads, want((method,), False), widths, **env)
    print(method, env, dict(zip(widths, rounds)))
    assert all(a > b for a, b in zip(rounds, rounds[1:])), dict(zip(widths, rounds))


@pytest.mark.parametrize("k", [19, 21])
def test_one_kernel_runs_at_the_width_asked_for_at_k19_and_k21(switches, k):
    gs, reads, want = synthetic_case(k)
    widths = (4, 8, 16, 64)
    rounds = rounds_by_width(switches, gs, ("one",), reads, want[False], widths)
    print(k, dict(zip(widths, rounds)))
    assert all(a > b for a, b in zip(rounds, rounds[1:])), dict(zip(widths, rounds))


@functools.lru_cache(maxsize=None)
def handback_case(k):
    """Reads that One's lane form cannot stitch, at any k.  A read is a sequence G; the set holds H, which is G with every
    seventh base changed, and every k-mer of G but the ones that END at such a site.  The sequential scan triggers at the
    first site, finds H's base the one solid alternative, and from there on carries a k-mer of H: it triggers and fixes at
    every site, and its state never is the ORIGINAL k-mer that a unit behind a sync point starts from (the original k-mers
    between two sites are solid, so there are sync points) -- every prediction misses, and three misses in a row hand the
    read back."""
    import numpy as np
    rng = np.random.default_rng(k)
    alpha = np.frombuffer(b"ACGT", dtype=np.uint8)
    reads, in_set = [], []
    for _ in range(60):
        g = rng.choice(alpha, 700).tobytes()
        sites = list(range(k + 3, len(g) - k, 7))
        h = bytearray(g)
        for s in sites:
            h[s] = b"ACGT"[(b"ACGT".index(g[s]) + 1) % 4]
        reads.append(g)
        in_set.append(bytes(h))
        in_set.append(g[:sites[0]])
        in_set += [g[a - k + 2:b] for a, b in zip(sites, sites[1:] + [len(g)])]
    # (confirm 5: with fewer look-aheads two scenarios tie now and then, One declines, and the scan falls back onto G)
    om = O.build_methods(O.Solid.sparse_from_count(k, in_set, 0), ["one"], 5, MAX_SEARCH)
    return br_amd.Pcon.from_fasta(in_set, k), tuple(reads), [O.correct_record(om, r, True) for r in reads]


@pytest.mark.parametrize("k", [11, 19, 21])
def test_one_list_form_takes_the_reads_the_lanes_hand_back(switches, fixture_case, k):
    """one_kernel<8, k, LIST>: the fixture reads in 64-base units behind a single solid k-mer (k = 11: a dense set, some
    reads miss three predictions in a row), and reads built to miss every prediction (k = 19, 21)"""
    switches(BRX_LANE_CHUNK=64, BRX_LANE_SYNC=1)
    if k == 11:
        gs, reads, want = fixture_case
        want = want(("one",), True)
    else:
        gs, reads, want = handback_case(k)
        assert sum(a != b for a, b in zip(want, reads)) == len(reads)  # (the oracle does fix them)
    chain = br_amd.Chain(gs, [("one", CONFIRM if k == 11 else 5, MAX_SEARCH)], two_side=True)
    got = chain.correct_reads(reads)
    bad = [i for i in range(len(reads)) if got[i] != want[i]]
    assert not bad, bad[:5]
    st = chain.last_stats()
    print(k, st)
    assert st["lane_units"] > 0 and st["lane_redone_reads"] > 0, st


def test_one_reverse_pass_is_lean_when_asked_for(switches, fixture_case):
    """BRX_REV_LEAN_ONE: rev_scan_kernel<k, One>, correct_kernel<8, One, 2> over the triggers it left open, one_kernel's
    list form over the reads handed back"""
    gs, reads, want = fixture_case
    _lib.profile_enable(True)
    try:
        for lean in (None, 1):
            switches(**({} if lean is None else {"BRX_REV_LEAN_ONE": lean}))
            _lib.profile_reset()
            assert chain_of(gs, ("one",), False).correct_reads(reads) == want(("one",), False)
            assert _lib.profile_get("correct_pass")[1] > 0
            assert (_lib.profile_get("rev_verify")[1] > 0) == (lean == 1), lean
            assert (_lib.profile_get("rev_redo")[1] > 0) == (lean == 1), lean
    finally:
        _lib.profile_enable(False)
