"""Counting hash table (include/brx.h BRX_COUNT_TABLE, br_amd/csrc/brx_counttable.hip): k-mer counts with an abundance
threshold for every odd k up to 31 -- the chained 64-byte-line table of sparse sets with a counter per slot beside it.
Every expected value comes from the CPU oracle: the dense one (and the reference's own .solid fixture) at small k, the
sparse one from k = 21 up."""
import os

import numpy as np
import pytest

import br_amd
from br_amd import _lib
from oracle import oracle as O

pytestmark = pytest.mark.gpu

METHODS = ["one", "two", "graph", "greedy", "gap_size"]
TABLE = _lib.COUNT_TABLE

_cache = {}


def _sparse_ref(tag, k, reads, a):
    """the sparse oracle's set, computed once per (reads, k, a) and shared (never modified)"""
    key = (tag, k, a)
    if key not in _cache:
        _cache[key] = O.Solid.sparse_from_count(k, reads, a)
    return _cache[key]


def _queries(k, reads, rng):
    fw = []
    for r in reads[:6]:
        for i in range(0, len(r) - k + 1, 3):
            w = r[i:i + k]
            if set(w) <= set(b"ACGT"):
                fw.append(O.seq2bit(w))
    fw = np.array(fw, dtype=np.uint64)
    mask = np.uint64((1 << (2 * k)) - 1)
    return np.concatenate([fw, fw ^ np.uint64(1), fw ^ (np.uint64(2) << np.uint64(2 * (k - 1))),
                           rng.integers(0, 1 << (2 * k), 5000, dtype=np.uint64)]) & mask


def _same_members(gs, ref, k, reads, seed):
    q = _queries(k, reads, np.random.default_rng(seed))
    want = np.array([ref.get(int(x)) for x in q])
    assert np.array_equal(gs.get_many(q), want)
    return want


# ---- 1. pinned by the reference's fixture -------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [8192, 7])
def test_fixture_k11_a2(raw_reads, solid_fixture_bytes, batch):
    """batch = 7: 30 batches, the table regrows several times on the way"""
    gs = br_amd.Pcon.from_count(raw_reads, 11, 2, batch=batch, strategy=TABLE)
    assert not gs.is_sparse()
    assert gs.to_solid_bytes() == solid_fixture_bytes


# ---- 2. small k against the dense oracle --------------------------------------------------------------------------------
@pytest.mark.parametrize("k,a", [(5, 0), (7, 1), (13, 3), (15, 2)])
def test_small_k_vs_dense_oracle(raw_reads, k, a):
    reads = raw_reads[:40] + [b"", b"ACG", b"N" * 40, b"acgtacgtacgtacgtacgtacgt"]
    gs = br_amd.Pcon.from_count(reads, k, a, strategy=TABLE)
    ref = O.Solid.from_count(k, O.count_reads(k, reads), a)
    assert gs.to_solid_bytes() == ref.to_bytes()


# ---- 3. saturation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [7, 25])
def test_saturation(k):
    """900 occurrences of the poly-A k-mer, 300 consecutive ones per read: the counter must read 255, not 900 % 256"""
    reads = [b"A" * (k + 299)] * 3 + [b"ACGTACGTAC"]
    cnt = br_amd.Counter(k, 0, TABLE)
    cnt.add_reads(reads)
    poly_a = 0  # A = 0: the forward k-mer of k As
    for a in (0, 200, 254, 255):
        gs = cnt.finish(a)
        if k == 25:
            assert gs.is_sparse()
            assert gs.get(poly_a) == (a < 255), a
        else:
            ref = O.Solid.from_count(k, O.count_reads(k, reads), a)
            assert ref.get(poly_a) == (a < 255)
            assert gs.to_solid_bytes() == ref.to_bytes(), a


# ---- 4. the feature itself ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", [1, 2])
@pytest.mark.parametrize("k", [23, 25, 31])
def test_large_k_counted_set_and_correctors(raw_reads, k, a):
    reads = raw_reads[:150]
    gs = br_amd.Pcon.from_count(reads, k, a)  # COUNT_AUTO
    assert gs.is_sparse() and gs.k() == k
    ref = _sparse_ref("raw150", k, reads, a)
    assert gs.popcount() == ref.popcount() > 1000
    want = _same_members(gs, ref, k, reads, k)
    assert want.any() and not want.all()
    changed = None
    for method in METHODS:
        om = O.build_methods(ref, [method], 5, 7)
        sub = reads[:25] if method == "greedy" else reads[:40]
        got = br_amd.Chain(gs, [(method, 5, 7)], two_side=False).correct_reads(sub)
        for r, g in zip(sub, got):
            assert g == O.correct_record(om, r, False), (k, a, method)
        if method == "one":
            changed = sum(g != r for r, g in zip(sub, got))
    # a set that triggered nothing (the presence set of the very reads) would pass everything above with 0 here
    assert changed >= 25


# ---- 5. regrow carries counts -------------------------------------------------------------------------------------------
def test_regrow_carries_counts(raw_reads):
    k, a = 25, 1
    reads = raw_reads[:150]
    one = br_amd.Pcon.from_count(reads, k, a)
    many = br_amd.Pcon.from_count(reads, k, a, batch=16)
    ref = _sparse_ref("raw150", k, reads, a)
    assert one.popcount() == ref.popcount()
    assert many.fingerprint() == one.fingerprint()
    assert many.fingerprint()[0] == ref.popcount()


# ---- 6. spectrum --------------------------------------------------------------------------------------------------------
def test_spectrum_k25(raw_reads):
    k = 25
    reads = raw_reads[:150]
    cnt = br_amd.Counter(k, 0)
    cnt.add_reads(reads)
    spec = cnt.spectrum()
    _, counts = np.unique(np.concatenate([O.hashes(k, r) for r in reads if len(r) >= k]), return_counts=True)
    exp = np.bincount(np.minimum(counts, 255), minlength=256)
    assert np.array_equal(spec[1:].astype(np.int64), exp[1:].astype(np.int64))
    assert int(spec[0]) == 2 ** 49 - counts.size
    assert cnt.table_info()["keys"] == counts.size


def test_spectrum_k11_equals_dense(raw_reads):
    spec = []
    for strategy in (TABLE, _lib.COUNT_DENSE):
        cnt = br_amd.Counter(11, 0, strategy)
        cnt.add_reads(raw_reads)
        spec.append(cnt.spectrum())
    assert np.array_equal(spec[0], spec[1])
    assert int(spec[0].sum()) == 1 << 21


# ---- 7. counter life cycle ----------------------------------------------------------------------------------------------
def test_counter_life_cycle(raw_reads):
    k = 25
    first, other = raw_reads[:150], raw_reads[100:200]
    cnt = br_amd.Counter(k, 0)
    cnt.add_reads(first)
    for a in (1, 3):
        gs = cnt.finish(a)
        ref = _sparse_ref("raw150", k, first, a)
        assert gs.popcount() == ref.popcount()
        _same_members(gs, ref, k, first, 70 + a)
    # a chain corrects with the set of abundance 1, then the counter -- reset, other reads -- is finished INTO that set:
    # the chain's next batch must see the new set (the old probe index is invalid)
    gs = cnt.finish(1)
    chain = br_amd.Chain(gs, [("one", 5, 7)], two_side=False)
    sub = raw_reads[:30]
    om = O.build_methods(_sparse_ref("raw150", k, first, 1), ["one"], 5, 7)
    for r, g in zip(sub, chain.correct_reads(sub)):
        assert g == O.correct_record(om, r, False)
    cnt.reset()
    cnt.add_reads(other)
    ref2 = _sparse_ref("raw100:200", k, other, 1)
    alone = cnt.finish(1)
    assert alone.popcount() == ref2.popcount()  # the reads counted before the reset are gone
    cnt.finish_into(1, gs)
    assert gs.popcount() == ref2.popcount() != _sparse_ref("raw150", k, first, 1).popcount()
    _same_members(gs, ref2, k, other, 77)
    om2 = O.build_methods(ref2, ["one"], 5, 7)
    got = chain.correct_reads(sub)
    differs = 0
    for r, g in zip(sub, got):
        assert g == O.correct_record(om2, r, False)
        differs += g != O.correct_record(om, r, False)
    assert differs > 0  # (the two sets do correct these reads differently)


# ---- 8. hot slots and loop trips ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocks", ["1", "3", "7"])
def test_hot_slots_and_loop_trips(raw_reads, monkeypatch, blocks):
    """BRX_READ_GRID shrinks the grid of every new kernel, so each block goes round its loop over tiles, lines or slots
    many times; poly-A / poly-T / poly-G and ACAC.. reads put whole waves onto one slot; short and empty reads put many
    boundaries into a tile"""
    monkeypatch.setenv("BRX_READ_GRID", blocks)
    k = 25
    rng = np.random.default_rng(100 + k)
    short = [bytes(rng.choice(list(b"ACGT"), size=int(n)).astype(np.uint8)) for n in rng.integers(0, 60, size=600)]
    reads = raw_reads[:30] + [b"A" * 9000, b"", b"ACACACACAC" * 700, b"T" * 5000] + short + raw_reads[30:45] + [b"G" * 4100]
    assert sum(len(r) for r in reads) > 20 * 4096
    cnt = br_amd.Counter(k, 0)
    cnt.add_reads(reads[:20])
    small = cnt.table_info()["log2_lines"]
    cnt.add_reads(reads[20:])  # the second batch does not fit the first one's table: the rehash kernel under the same switch
    assert cnt.table_info()["log2_lines"] > small
    allh = np.concatenate([O.hashes(k, r) for r in reads if len(r) >= k])
    _, counts = np.unique(allh, return_counts=True)
    for a in (0, 2):
        gs = cnt.finish(a)
        ref = _sparse_ref("hot", k, reads, a)
        assert gs.popcount() == ref.popcount() > 1000
        q = np.concatenate([_queries(k, reads, np.random.default_rng(a)),
                            _queries(k, [b"A" * 100, b"T" * 100, b"G" * 100, b"ACACACACAC" * 10], np.random.default_rng(a + 5))])
        want = np.array([ref.get(int(x)) for x in q])
        assert np.array_equal(gs.get_many(q), want)
    spec = cnt.spectrum()
    exp = np.bincount(np.minimum(counts, 255), minlength=256)
    assert exp[255] >= 3  # the homopolymers and the dinucleotide repeat
    assert np.array_equal(spec[1:].astype(np.int64), exp[1:].astype(np.int64))
    assert int(spec[0]) == 2 ** 49 - counts.size


# ---- 9. refusals --------------------------------------------------------------------------------------------------------
def test_refusals(raw_reads):
    cnt = br_amd.Counter(25, 0)
    cnt.add_reads(raw_reads[:3])
    for call in (cnt.device_counts, lambda: cnt.load_counts(0, b"\x01\x02"), lambda: cnt.clamp(3), cnt.l1_view):
        with pytest.raises(_lib.BrxError) as ei:
            call()
        assert "table count strategy" in str(ei.value)
    with pytest.raises(_lib.BrxError):
        br_amd.Counter(24)
    with pytest.raises(_lib.BrxError):
        br_amd.Counter(24, 0, TABLE)
    c21 = br_amd.Counter(21)
    c21.add_reads(raw_reads[:3])
    assert c21.l1_view()[3] > 0  # still the partitioned strategy
    with pytest.raises(_lib.BrxError):
        c21.table_info()


def test_k21_unchanged(raw_reads):
    k, a = 21, 1
    reads = raw_reads[:150]
    gs = br_amd.Pcon.from_count(reads, k, a)
    assert gs.is_sparse() and gs.k() == 21
    ref = _sparse_ref("raw150", k, reads, a)
    assert gs.popcount() == ref.popcount() > 1000
    want = _same_members(gs, ref, k, reads, 21)
    assert want.any() and not want.all()


# ---- 10. CLI ------------------------------------------------------------------------------------------------------------
def _oracle_hist(k, reads):
    _, counts = np.unique(np.concatenate([O.hashes(k, r) for r in reads if len(r) >= k]), return_counts=True)
    hist = np.bincount(np.minimum(counts, 255), minlength=256).astype(np.uint64)
    hist[0] = (1 << (2 * k - 1)) - counts.size
    return hist


def test_cli_fasta_k25(tmp_path, golden_dir, raw_reads):
    from br_amd import cli, fasta, spectrum
    raw = os.path.join(golden_dir, "raw.fasta")
    out25, out26, outm = (str(tmp_path / n) for n in ("c25.fasta", "c26.fasta", "cmin.fasta"))
    assert cli.main(["-i", raw, "-o", out25, "-c", "one", "-s", "fasta", "-i", raw, "-k", "25", "-a", "1"]) == 0
    om = O.build_methods(_sparse_ref("rawall", 25, raw_reads, 1), ["one"], 5, 7)
    got = list(fasta.read_records(open(out25, "rb")))
    assert len(got) == len(raw_reads)
    changed = 0
    for (_, _, seq), r in zip(got, raw_reads):
        assert seq == O.correct_record(om, r, True)  # (-s: no reverse pass)
        changed += seq != r
    assert changed > len(raw_reads) // 2
    # an even k is lowered by one, like the reference's Fasta::kmer_size
    assert cli.main(["-i", raw, "-o", out26, "-c", "one", "-s", "fasta", "-i", raw, "-k", "26", "-a", "1"]) == 0
    assert open(out26, "rb").read() == open(out25, "rb").read()
    # threshold from the spectrum
    thr = spectrum.get_threshold(_oracle_hist(25, raw_reads), "first-minimum")
    assert thr is not None
    assert cli.main(["-i", raw, "-o", outm, "-c", "one", "-s", "fasta", "-i", raw, "-k", "25", "first-minimum"]) == 0
    om = O.build_methods(_sparse_ref("rawall", 25, raw_reads, thr), ["one"], 5, 7)
    got = list(fasta.read_records(open(outm, "rb")))
    assert len(got) == len(raw_reads)
    for (_, _, seq), r in zip(got, raw_reads):
        assert seq == O.correct_record(om, r, True)
