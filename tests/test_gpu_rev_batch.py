"""The 64-lane reverse scans (one_kernel<64>, correct_kernel<64>, rev_scan_kernel in br_amd/csrc/brx_one.hip, brx_group.hip, brx_revscan.hip) take
their trigger-free rounds REV_BLOCK = 4 at a time (rev_block_rounds, brx_correct.hpp): every round filters its 64
positions through the index's occupancy bits, the survivors wait in a queue and are probed together, and the trigger
test runs over the block's answer words.  These inputs aim at that loop: reverse passes that correct for their living
(triggers in every round of a block, a queue that fills before the block ends), read lengths on both sides of every
entry threshold, solid runs across round and block boundaries, index lines that overflow, and the switches.

The expected bytes are the oracle's, for every read.  That the inputs do what they are for is asserted first, on the
CPU (the tests without the gpu mark)."""
import functools
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import br_amd
from oracle import oracle as O

R = 4            # BRX_REV_BLOCK of the default build
CONFIRM = 2
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def genome_a():
    return np.random.default_rng(5).choice(ACGT, 8_000).tobytes()


@functools.lru_cache(maxsize=None)
def oracle_set(k, seqs):
    """presence-only set of the sequences' k-mers: the bit vector up to k = 15, the sorted hash array beyond"""
    if k > 15:
        return O.Solid.sparse_from_count(k, list(seqs), 0)
    ref = O.Solid(k)
    for s in seqs:
        ref.set_seq(s)
    return ref


def gpu_set(k, seqs, monkeypatch, counted=True):
    """the same set on the GPU, with an index whose minimizers leave at most 8 windows (the block loop's range).
    counted: built from a key list (occupancy bits, lazy bit vector); else inserted k-mer by k-mer"""
    if k >= 19:
        monkeypatch.setenv("BRX_INDEX_M", "15")  # w = 5 at k = 19, 7 at k = 21, as at the benchmark's sizes
    if counted and k > 15:
        return br_amd.Pcon.from_count(list(seqs), k, 0)
    return br_amd.Pcon.from_fasta(list(seqs), k)


def plant(read, kind, positions, rng):
    r = bytearray(read)
    for pos in sorted(positions, reverse=True):
        if kind == "sub":
            r[pos] = int(rng.choice([c for c in b"ACGT" if c != r[pos]]))
        elif kind == "del":
            del r[pos]
        else:
            r.insert(pos, int(rng.choice(ACGT)))
    return bytes(r)


@functools.lru_cache(maxsize=None)
def working_reads(kind, n_reads, seed=5):
    """stretches of A, 144 ... 700 bases, an error of one kind every 29 ... 40 bases.  With only the REVERSED genome solid
    the forward scan meets no solid k-mer, and the scan over the reversed read follows the reversed genome and
    corrects: every k-mer passes the occupancy filter and triggers fall everywhere"""
    rng = np.random.default_rng(seed)
    g = genome_a()
    reads = []
    for _ in range(n_reads):
        n = int(rng.integers(144, 701))
        s = int(rng.integers(0, len(g) - n))
        pos, at = int(rng.integers(20, 41)), []
        while pos < n - 20:
            at.append(pos)
            pos += int(rng.integers(29, 41))
        reads.append(plant(g[s:s + n], kind, at, rng))
    return tuple(reads)


@functools.lru_cache(maxsize=None)
def expected(k, seqs, reads, names, two_side=False):
    om = O.build_methods(oracle_set(k, seqs), list(names), CONFIRM, 7)
    return tuple(O.correct_record(om, r, two_side) for r in reads)


def check(gs, k, seqs, reads, names):
    chain = br_amd.Chain(gs, [(m, CONFIRM, 7) for m in names], two_side=False)
    got = chain.correct_reads(list(reads))
    want = expected(k, seqs, reads, names)
    bad = [i for i, (x, y) in enumerate(zip(got, want)) if x != y]
    assert not bad, (names, k, bad[:10], [len(reads[i]) for i in bad[:10]])
    # the index the passes probed is one the block loop takes (rev_block_applies, brx_correct.hpp: at most 8 windows and
    # 2^26 lines; the occupancy bits come with every index built from a key list): the reads above did go through it
    info = gs.index_info()
    assert info["valid"] and 1 <= k - info["m"] + 1 <= 8 and info["log2_lines"] <= 26, info
    return got


# ---- CPU: the inputs do what they are for ---------------------------------------------------------------------------

def test_reversed_genome_makes_the_reverse_pass_work():
    k, seqs = 15, (genome_a()[::-1],)
    reads = working_reads("sub", 60)
    fwd = expected(k, seqs, reads, ("one",), True)
    assert all(f == r for f, r in zip(fwd, reads)), "the forward scan alone must return every read unchanged"
    both = expected(k, seqs, reads, ("one",))
    residues, rounds, total = set(), set(), 0
    for r, o in zip(reads, both):
        assert len(o) == len(r)
        at = [p for p in range(len(r)) if r[::-1][p] != o[::-1][p]]  # positions of the reversed read, as the scan counts
        assert at, "every read is corrected by the reversed scan"
        total += len(at)
        residues.update(p % 64 for p in at)
        rounds.update(((p - k) // 64) % R for p in at if p >= k)  # the scan's first round starts at position k
    assert total > 400 and residues == set(range(64)) and rounds == set(range(R)), (total, sorted(residues), rounds)


@pytest.mark.parametrize("kind", ["ins", "del"])
def test_reversed_genome_indels_are_corrected(kind):
    k, seqs = 15, (genome_a()[::-1],)
    reads = working_reads(kind, 12)
    assert all(f == r for f, r in zip(expected(k, seqs, reads, ("one",), True), reads))
    assert all(o != r for o, r in zip(expected(k, seqs, reads, ("one",)), reads))


def threshold_lengths(k):
    ls = list(range(k + 60, k + 71))
    for blocks in (1, 2, 3):
        ls += list(range(64 * R * blocks + k - 4, 64 * R * blocks + k + 5))
    return ls


@functools.lru_cache(maxsize=None)
def threshold_reads(k):
    """reads of A at every length around the block loop's entry thresholds (n - i >= 64 R + 1 with i = k, 64 R + k,
    128 R + k), clean and with one substitution near the middle, odd and even lengths"""
    rng = np.random.default_rng(17 + k)
    g = genome_a()
    reads = []
    for n in threshold_lengths(k):
        s = int(rng.integers(0, len(g) - n))
        reads.append(g[s:s + n])
        reads.append(plant(g[s + 1:s + 1 + n], "sub", [n // 2], rng))
    return tuple(reads)


def test_threshold_lengths_pass_every_bound_from_both_sides():
    for k in (15, 19):
        ls = set(threshold_lengths(k))
        for blocks in (1, 2, 3):
            edge = 64 * R * blocks + k + 1  # the shortest read whose scan still enters a block of R rounds at i = k + 64 R (blocks - 1)
            assert {edge - 1, edge, edge + 1} <= ls
        assert {n & 1 for n in ls} == {0, 1} and {k + 64, k + 65, k + 66} <= ls


@functools.lru_cache(maxsize=None)
def straddling_reads():
    """700 bases of A with substitutions 3, 19 and 64 bases apart: with A and its reverse both solid the reversed scan
    sees solid runs and triggers across round and block boundaries"""
    rng = np.random.default_rng(23)
    g = genome_a()
    reads = []
    for gap in (3, 19, 64):
        for first in (15, 40, 63, 64, 65):
            s = int(rng.integers(0, len(g) - 700))
            reads.append(plant(g[s:s + 700], "sub", range(first, 690, gap), rng))
    return tuple(reads)


@functools.lru_cache(maxsize=None)
def repeat_genome():
    rng = np.random.default_rng(11)
    parts = []
    for period in range(2, 8):
        unit = rng.choice(ACGT, period).tobytes()
        parts += [rng.choice(ACGT, 200).tobytes(), unit * (600 // period)]
    return b"".join(parts) + rng.choice(ACGT, 200).tobytes()


@functools.lru_cache(maxsize=None)
def repeat_reads():
    """low-complexity reads: stretches of tandem repeats of period 2 ... 7 (their k-mers share a handful of minimizers,
    whose index lines overflow) with a few errors of every kind"""
    rng = np.random.default_rng(12)
    g = repeat_genome()
    reads = []
    for _ in range(24):
        s = int(rng.integers(0, len(g) - 640))
        r = g[s:s + 640]
        for kind in ("sub", "ins", "del"):
            r = plant(r, kind, rng.integers(25, len(r) - 25, size=3).tolist(), rng)
        reads.append(r)
    return tuple(reads)


# ---- GPU --------------------------------------------------------------------------------------------------------------

METHOD_CASES = [(("one",), ""), (("two",), ""), (("greedy",), ""), (("graph",), "1"), (("graph",), "0"), (("gap_size",), "1"),
                (("gap_size",), "0")]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [15, 19])
@pytest.mark.parametrize("kind", ["sub", "ins", "del"])
@pytest.mark.parametrize("names,lean", METHOD_CASES)
def test_working_reverse_pass(monkeypatch, k, kind, names, lean):
    """only the reversed genome is solid: the reverse pass corrects, with triggers in every round of a block and a
    queue that fills before the block ends.  Graph / GapSize with and without the lean form (rev_scan_kernel and
    correct_kernel<64> both run the block loop); Greedy's group kernel is compiled without it and runs the one-round
    loop over the same reads"""
    if lean:
        monkeypatch.setenv("BRX_REV_LEAN", lean)
    seqs = (genome_a()[::-1],)
    reads = working_reads(kind, 60 if (names == ("one",) and kind == "sub") else 12)
    gs = gpu_set(k, seqs, monkeypatch)
    got = check(gs, k, seqs, reads, names)
    if names == ("one",):
        assert sum(x != r for x, r in zip(got, reads)) == len(reads)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [15, 19])
@pytest.mark.parametrize("names,lean", [(("one",), ""), (("graph",), "1"), (("gap_size",), "0")])
def test_entry_and_exit_lengths(monkeypatch, k, names, lean):
    if lean:
        monkeypatch.setenv("BRX_REV_LEAN", lean)
    seqs = (genome_a(),)
    check(gpu_set(k, seqs, monkeypatch), k, seqs, threshold_reads(k), names)


@pytest.mark.gpu
@pytest.mark.parametrize("names,lean", [(("one",), ""), (("graph",), "1"), (("gap_size",), "0"), (("two",), "")])
def test_solid_runs_across_rounds_and_blocks(monkeypatch, names, lean):
    if lean:
        monkeypatch.setenv("BRX_REV_LEAN", lean)
    k, seqs = 15, (genome_a(), genome_a()[::-1])
    check(gpu_set(k, seqs, monkeypatch), k, seqs, straddling_reads(), names)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [15, 21])
@pytest.mark.parametrize("names,lean", [(("one",), ""), (("gap_size",), "1"), (("graph",), "0")])
def test_cannot_say_in_the_drain(monkeypatch, k, names, lean):
    """overflowing lines: settled through the bit vector at k = 15, along the chain of the sparse set at k = 21"""
    if lean:
        monkeypatch.setenv("BRX_REV_LEAN", lean)
    seqs = (repeat_genome(), repeat_genome()[::-1])
    gs = gpu_set(k, seqs, monkeypatch)
    assert gs.is_sparse() == (k == 21)
    check(gs, k, seqs, repeat_reads(), names)
    info = gs.index_info()
    assert info["overflow_keys"] > 0, info


_CHILD = """
import pickle, sys
import br_amd
k, seqs, reads, confirm = pickle.load(open(sys.argv[1], "rb"))
gs = br_amd.Pcon.from_fasta(list(seqs), k)
out = br_amd.Chain(gs, [("one", confirm, 7)], two_side=False).correct_reads(list(reads))
pickle.dump(out, open(sys.argv[2], "wb"))
"""


@pytest.mark.gpu
def test_switches(monkeypatch, tmp_path):
    """BRX_REV_BATCH=0 (the one-round loop everywhere) and builds with 2 and 8 rounds per block, where tools/ab_build.sh
    has made them (br_amd/lib/ab/libbrx_block{2,8}.so), give the default's bytes"""
    k, seqs = 15, (genome_a()[::-1],)
    reads = working_reads("sub", 60)
    default = check(gpu_set(k, seqs, monkeypatch), k, seqs, reads, ("one",))
    monkeypatch.setenv("BRX_REV_BATCH", "0")
    assert check(gpu_set(k, seqs, monkeypatch), k, seqs, reads, ("one",)) == default
    monkeypatch.delenv("BRX_REV_BATCH")
    with open(tmp_path / "in.pkl", "wb") as f:
        pickle.dump((k, seqs, reads, CONFIRM), f)
    for name in ("block2", "block8"):
        lib = os.path.join(ROOT, "br_amd", "lib", "ab", f"libbrx_{name}.so")
        if not os.path.exists(lib):
            print(f"{name}: no such build here (tools/ab_build.sh {name} -DBRX_REV_BLOCK=...), not compared")
            continue
        env = dict(os.environ, BRX_LIB_PATH=lib, PYTHONPATH=ROOT)
        subprocess.run([sys.executable, "-c", _CHILD, str(tmp_path / "in.pkl"), str(tmp_path / f"{name}.pkl")], env=env, check=True,
                       cwd=ROOT, timeout=120)
        with open(tmp_path / f"{name}.pkl", "rb") as f:
            assert pickle.load(f) == default, name


@functools.lru_cache(maxsize=None)
def long_genome():
    return np.random.default_rng(31).choice(ACGT, 60_000).tobytes()


@functools.lru_cache(maxsize=None)
def long_reads():
    """20 000 ... 40 000 bases with a substitution every few hundred: 300 ... 600 rounds of the reverse scan in ONE wave
    (a read has a wave of its own until a batch outgrows the grid), with a chance trigger now and then whose general
    rounds shift where the blocks fall against the wave's 255-round counter flushes"""
    rng = np.random.default_rng(32)
    g = long_genome()
    reads = []
    for _ in range(24):
        n = int(rng.integers(20_000, 40_001))
        s = int(rng.integers(0, len(g) - n))
        reads.append(plant(g[s:s + n], "sub", range(int(rng.integers(50, 400)), n - 50, int(rng.integers(150, 700))), rng))
    return tuple(reads)


@pytest.mark.gpu
@pytest.mark.parametrize("names", [("one",), ("graph",), ("two",)])
def test_counters_are_those_of_the_one_round_loop(monkeypatch, names):
    """triggers and fixes of Chain.last_stats() with the block loop and with BRX_REV_BATCH=0.  one_kernel packs rounds,
    probes, triggers and fixes into 8-bit fields that it flushes every 255 rounds, and a block adds its rounds at once:
    a field that passes 255 carries into the next one, rounds into probes, probes into triggers.  Triggers and fixes
    are the same in every run of a job; rounds and probes are not (the forward pass's share depends on how its units
    were dealt: the parent's own result lines in profiles/r8_bench_ab.jsonl differ in both), so they are only
    required to be there"""
    k, seqs = 15, (long_genome(),)
    reads = long_reads()
    assert min(len(r) for r in reads) >= 255 * 64 + k
    stats = {}
    for batch in ("", "0"):
        if batch:
            monkeypatch.setenv("BRX_REV_BATCH", batch)
        gs = gpu_set(k, seqs, monkeypatch)
        chain = br_amd.Chain(gs, [(m, CONFIRM, 7) for m in names], two_side=False)
        got = chain.correct_reads(list(reads))
        assert list(got) == list(expected(k, seqs, reads, names))
        st = chain.last_stats()
        stats[batch] = {key: int(st[key]) for key in ("rounds", "probes", "triggers", "fixes")}
    print(names, stats)
    assert (stats[""]["triggers"], stats[""]["fixes"]) == (stats["0"]["triggers"], stats["0"]["fixes"]), stats
    assert stats[""]["triggers"] > 0 and stats[""]["rounds"] > 24 * 255 and stats[""]["probes"] > 64 * 24 * 255


@pytest.mark.gpu
@pytest.mark.parametrize("names,lean", [(("one",), ""), (("graph",), "1")])
def test_set_without_occupancy_bits_keeps_the_one_round_loop(monkeypatch, names, lean):
    """a sparse set filled k-mer by k-mer has no occupancy bits: its reverse scans take the old loop and still match"""
    if lean:
        monkeypatch.setenv("BRX_REV_LEAN", lean)
    k, seqs = 21, (genome_a()[::-1],)
    gs = gpu_set(k, seqs, monkeypatch, counted=False)
    assert gs.is_sparse()
    check(gs, k, seqs, working_reads("sub", 12), names)
