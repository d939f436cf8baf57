"""K-mer abundance of reads on the GPU (include/brx.h "abundance", br_amd/csrc/brx_abundance.hip): per-base counts, per-read
histograms and statistics from a dense or a table counter.  Every expected value comes from br_amd/abundance.py -- numpy
over the CPU oracle's canonical hashes -- and every comparison is exact."""
import numpy as np
import pytest

import br_amd
from br_amd import _lib, cover
from br_amd import abundance as ab
from br_amd.set import pack_reads
from oracle import oracle as O

pytestmark = pytest.mark.gpu

TABLE, DENSE = _lib.COUNT_TABLE, _lib.COUNT_DENSE

_cache = {}


def _hashes(tag, k, reads):
    """the oracle's hashes of a list of reads, computed once per (tag, k) and shared (never modified)"""
    if (tag, k) not in _cache:
        _cache[(tag, k)] = [O.hashes(k, r) for r in reads]
    return _cache[(tag, k)]


def expect(k, counted_h, query, query_h, a):
    """(profile bytes of the batch, hist[n, 256], stats[n]) from abundance.py"""
    counts = ab.profile_from_hashes(counted_h, query_h)
    prof = np.concatenate([ab.profile_bytes(c, len(r)) for c, r in zip(counts, query)]) if query else np.zeros(0, np.uint8)
    hist = np.array([ab.hist_from_profile(c) for c in counts], dtype=np.uint32).reshape(len(query), 256)
    return prof, hist, ab.stats_array(counts, a)


def same_stats(got, want):
    for name in ab.STATS_DTYPE.names:
        bad = np.flatnonzero(got[name] != want[name])
        assert not bad.size, (name, bad[:5].tolist(), got[name][bad[:5]].tolist(), want[name][bad[:5]].tolist())


def check(cnt, k, counted_h, query, query_h, a):
    bases, offs = pack_reads(query)
    prof, hist, st = cnt.abundance_batch(bases, offs, a, profile=True, hist=True)
    wp, wh, ws = expect(k, counted_h, query, query_h, a)
    bad = np.flatnonzero(prof != wp)
    assert not bad.size, (bad[:8].tolist(), prof[bad[:8]].tolist(), wp[bad[:8]].tolist())
    assert np.array_equal(hist, wh)
    same_stats(st, ws)
    return st


def raw_call(cnt, bases, offs, a, want):
    """brx_counter_abundance_batch with exactly the outputs named in `want`, the others NULL"""
    n = offs.size - 1
    pr = np.full(bases.size, 0xEE, dtype=np.uint8) if "profile" in want else None
    hi = np.full((n, 256), 0xEEEEEEEE, dtype=np.uint32) if "hist" in want else None
    st = np.zeros(n, dtype=ab.STATS_DTYPE) if "stats" in want else None
    if st is not None:
        st.view(np.uint8)[:] = 0xEE
    ptr = lambda x: x.ctypes.data if x is not None else None
    _lib.check(_lib.lib().brx_counter_abundance_batch(cnt._h, bases.ctypes.data, offs.ctypes.data, n, a, ptr(pr), ptr(hi), ptr(st)))
    return pr, hi, st


def rand_seq(rng, n):
    return rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(n))


def noisy(rng, genome, start, n, rate=0.03):
    """n bases of the (circular) genome from `start` on, with substitutions"""
    r = genome[(start + np.arange(int(n))) % genome.size].copy()
    hit = rng.random(r.size) < rate
    r[hit] = rand_seq(rng, int(hit.sum()))
    return r.tobytes()


# ---- 1. the reference's fixture -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy", [DENSE, TABLE])
def test_fixture_k11(raw_reads, strategy):
    k, a = 11, 2
    cnt = br_amd.Counter(k, 0, strategy)
    cnt.add_reads(raw_reads)
    h = _hashes("raw", k, raw_reads)
    st = check(cnt, k, h, raw_reads, h, a)
    assert int(st["kmers"].astype(np.int64).sum()) == 2_517_532 and int(st["min"].min()) >= 1 and int(st["max"].max()) > 40
    # each output alone, the other two NULL
    query = raw_reads[:25] + [b"", raw_reads[30][:k - 1], raw_reads[31][:k]]
    qh = h[:25] + [O.hashes(k, r) for r in query[25:]]
    bases, offs = pack_reads(query)
    wp, wh, ws = expect(k, h, query, qh, a)
    pr, hi, s = raw_call(cnt, bases, offs, a, ("profile",))
    assert hi is None and s is None and np.array_equal(pr, wp)
    pr, hi, s = raw_call(cnt, bases, offs, a, ("hist",))
    assert pr is None and s is None and np.array_equal(hi, wh)
    pr, hi, s = raw_call(cnt, bases, offs, a, ("stats",))
    assert pr is None and hi is None
    same_stats(s, ws)
    pr, hi, s = raw_call(cnt, bases, offs, a, ())  # nothing asked for: nothing done, no error
    # the k-mers the reference's fixture calls solid are the ones counted more than twice
    assert np.array_equal(cnt.finish(a).cover_reads(query)[1]["solid"], ws["above"])


# ---- 2. tile boundaries -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,grid", [(15, None), (31, None), (15, "1")])
def test_tile_boundaries(monkeypatch, k, grid):
    """every length at which a tile, a step of 64 or the k-1 bases behind a tile begin or end; grid = "1": the helper
    kernels whose blocks loop over reads go round their loops"""
    if grid:
        monkeypatch.setenv("BRX_READ_GRID", grid)
    rng = np.random.default_rng(1000 + k)
    genome = rand_seq(rng, 3000)
    lengths = [0, k - 1, k, k + 1, 63, 64, 65, 1023, 1024, 1025, 1024 + k - 1, 1024 + k, 2048, 2049 + k, 5003]
    counted = [noisy(rng, genome, rng.integers(0, 3000), n) for n in lengths]
    counted += [noisy(rng, genome, rng.integers(0, 3000), 500) for _ in range(85)]  # about 20x of the genome in all
    other = [noisy(rng, genome, rng.integers(0, 3000), n) if i % 2 else rand_seq(rng, n).tobytes() for i, n in enumerate(lengths)]
    cnt = br_amd.Counter(k, 0, TABLE)
    cnt.add_reads(counted)
    ch = [O.hashes(k, r) for r in counted]
    st = check(cnt, k, ch, counted[:len(lengths)], ch[:len(lengths)], 3)
    assert st["kmers"].tolist() == [max(n - k + 1, 0) for n in lengths]
    assert int(st["min"][st["kmers"] > 0].min()) >= 1 and 5 < int(st["max"].max()) < 255  # counted reads: never absent
    st = check(cnt, k, ch, other, [O.hashes(k, r) for r in other], 3)
    assert int(st["absent"].astype(np.int64).sum()) > 5000 and int(st["max"].max()) > 3  # random halves, genome halves


# ---- 3. chains ----------------------------------------------------------------------------------------------------------
def test_long_overflow_chains():
    """the canonical m-mer of A^m is 0 for every m up to 16, the smallest hash there is: every k-mer that holds A^16 has the
    same home line, and the lookup follows the overflow chain hundreds of lines deep -- also for the k-mers that hold the
    minimizer and were never counted"""
    k = 25
    rng = np.random.default_rng(25)

    def form():
        return rand_seq(rng, rng.integers(20, 60)).tobytes() + b"A" * 16 + rand_seq(rng, rng.integers(20, 60)).tobytes()

    counted = [form() for _ in range(300)]
    never = [form() for _ in range(200)]
    cnt = br_amd.Counter(k, 0, TABLE)
    cnt.add_reads(counted + counted[:50])
    info = cnt.table_info()
    ch = [O.hashes(k, r) for r in counted + counted[:50]]
    assert sum(1 for r in counted for i in range(len(r) - k + 1) if b"A" * 16 in r[i:i + k]) > 7 * 300  # > 300 lines of one chain
    st = check(cnt, k, ch, counted, ch[:300], 1)
    assert set(st["min"][:50].tolist()) == {2} and int(st["absent"].max()) == 0
    st = check(cnt, k, ch, never, [O.hashes(k, r) for r in never], 1)
    assert int(st["absent"].astype(np.int64).sum()) > 0.9 * int(st["kmers"].astype(np.int64).sum())
    assert cnt.table_info() == info  # a lookup claims nothing


# ---- 4. saturation and regrow -------------------------------------------------------------------------------------------
def test_saturation():
    k = 25
    read = rand_seq(np.random.default_rng(4), 200).tobytes()
    for strategy, kk in ((TABLE, k), (DENSE, 13)):
        cnt = br_amd.Counter(kk, 0, strategy)
        cnt.add_reads([read] * 300)
        prof, st = cnt.abundance_reads([read, read[:kk] + b"ACGT"], 254)
        assert prof[0].size == 200 - kk + 1 and (prof[0] == 255).all()
        assert tuple(int(v) for v in st[0]) == (prof[0].size, 0, prof[0].size, 255, 255, 255, 255 * prof[0].size)
        assert prof[1][0] == 255 and int(cnt.abundance_reads([read], 255)[1]["above"][0]) == 0
        assert int(cnt.spectrum()[255]) == len(set(O.hashes(kk, read).tolist()))


def test_regrow_between_profiles(raw_reads):
    k = 25
    cnt = br_amd.Counter(k, 0, TABLE)
    query = raw_reads[:6] + raw_reads[100:104] + [raw_reads[149][:2000]]
    qh = [O.hashes(k, r) for r in query]
    all_h = _hashes("raw", k, raw_reads)
    sizes, done = [], 0
    for upto in (3, 20, 70, 150):
        cnt.add_reads(raw_reads[done:upto])
        done = upto
        sizes.append(cnt.table_info()["log2_lines"])
        st = check(cnt, k, all_h[:done], query, qh, 1)
        # reads 100..103 are counted by the last batch only: k-mers of their own before it, none absent after it
        assert (st["absent"][6:10] == 0).all() if done >= 104 else (st["absent"][6:10] > 0).all()
    assert sizes[-1] > sizes[0] and sorted(sizes) == sizes  # the table has regrown between the profiles


# ---- 5. cross-check with coverage ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,strategy", [(15, TABLE), (11, DENSE)])
def test_above_equals_cover_solid(raw_reads, k, strategy):
    reads = raw_reads[:60]
    query = raw_reads[:12] + raw_reads[80:84]
    cnt = br_amd.Counter(k, 0, strategy)
    cnt.add_reads(reads)
    spec = cnt.spectrum()
    prints = {a: cnt.finish(a).fingerprint() for a in (0, 2, 7)}
    for a in (0, 2, 7):
        _, st = cnt.abundance_reads(query, a)
        _, cst = cnt.finish(a).cover_reads(query)
        assert np.array_equal(st["above"], cst["solid"]) and np.array_equal(st["kmers"], cst["kmers"])
        assert int(st["above"].sum()) > 0
    assert np.array_equal(cnt.spectrum(), spec)
    for a in (0, 2, 7):
        assert cnt.finish(a).fingerprint() == prints[a]


# ---- 6. lookup ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,strategy", [(25, TABLE), (11, DENSE), (31, TABLE)])
def test_get_counts(raw_reads, k, strategy):
    reads = raw_reads[:30]
    cnt = br_amd.Counter(k, 0, strategy)
    cnt.add_reads(reads)
    table = ab.count_table([O.hashes(k, r) for r in reads])
    sample = [raw_reads[2][:400], raw_reads[40][:400], rand_seq(np.random.default_rng(k), 300).tobytes()]
    fwd = np.concatenate([cover.kmers_of(r, k) for r in sample])
    want = np.concatenate([ab.lookup(table, O.hashes(k, r)) for r in sample])
    rc = np.array([O.revcomp(int(x), k) for x in fwd], dtype=np.uint64)
    got = cnt.get_counts(fwd)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(cnt.get_counts(rc), want)
    assert want[:300].min() >= 1 and (want == 0).any()
    assert cnt.get_counts(np.zeros(0, dtype=np.uint64)).size == 0


# ---- 7. refusals and empty inputs ---------------------------------------------------------------------------------------
def test_refusals_and_empty(raw_reads):
    c21 = br_amd.Counter(21)  # the partitioned strategy
    c21.add_reads(raw_reads[:3])
    bases, offs = pack_reads(raw_reads[:2])
    for call in (lambda: c21.abundance_batch(bases, offs), lambda: c21.get_counts([1, 2, 3])):
        with pytest.raises(_lib.BrxError) as ei:
            call()
        assert ei.value.status == _lib.BRX_ERR_UNSUPPORTED and "BRX_COUNT_TABLE" in str(ei.value)
    # a table counter that has counted nothing: zeros
    k = 25
    cnt = br_amd.Counter(k, 0, TABLE)
    query = [raw_reads[0][:3000], b"ACGT", b"", raw_reads[1][:k]]
    qb, qo = pack_reads(query)
    prof, hist, st = cnt.abundance_batch(qb, qo, 0, profile=True, hist=True)
    assert not prof.any() and st["kmers"].tolist() == [3000 - k + 1, 0, 0, 1]
    assert np.array_equal(st["absent"], st["kmers"]) and np.array_equal(hist[:, 0], st["kmers"]) and not hist[:, 1:].any()
    assert not any(st[f].any() for f in ("above", "min", "median", "max", "sum"))
    assert not cnt.get_counts(cover.kmers_of(query[0][:100], k)).any()
    assert cnt.table_info()["log2_lines"] == 0  # and it still has no table
    # no reads, and reads without bases
    cnt.add_reads(raw_reads[:2])
    for c in (cnt, br_amd.Counter(11, 0, DENSE)):
        prof, hist, st = c.abundance_batch(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), 0, profile=True, hist=True)
        assert prof.size == 0 and hist.shape == (0, 256) and st.size == 0
        _lib.check(_lib.lib().brx_counter_abundance_batch_device(c._h, None, None, 0, 0, 0, None, None, None, None))
        pr, hi, s = raw_call(c, np.zeros(0, dtype=np.uint8), np.zeros(4, dtype=np.uint64), 0, ("profile", "hist", "stats"))
        assert not hi.any() and not s.view(np.uint8).any()


# ---- 8. CLI -------------------------------------------------------------------------------------------------------------
def test_cli_abundance_report(tmp_path):
    from br_amd import cli
    k, a = 15, 2
    rng = np.random.default_rng(8)
    genome = rand_seq(rng, 2000)
    reads = [noisy(rng, genome, rng.integers(0, 2000), rng.integers(100, 600)) for _ in range(60)] + [b"ACGTACGT", rand_seq(rng, 300).tobytes()]
    src = tmp_path / "reads.fasta"
    with open(src, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b">read%d some description\n" % i + r + b"\n")
    plain, with_rep, rep = (str(tmp_path / n) for n in ("plain.fasta", "rep.fasta", "abund.tsv"))
    tail = ["-c", "one", "-b", "7", "fasta", "-i", str(src), "-k", str(k), "-a", str(a)]
    assert cli.main(["-i", str(src), "-o", plain] + tail) == 0
    assert cli.main(["-i", str(src), "-o", with_rep, "--abundance-report", rep] + tail) == 0
    assert open(with_rep, "rb").read() == open(plain, "rb").read()
    hs = [O.hashes(k, r) for r in reads]
    want = ab.REPORT_HEADER + b"".join(ab.report_line(b"read%d" % i, len(r), ab.stats_from_profile(p, a))
                                      for i, (r, p) in enumerate(zip(reads, ab.profile_from_hashes(hs))))
    assert open(rep, "rb").read() == want
    assert want.count(b"\n") == len(reads) + 1 and b"\t0\t0\t0\t0\t0\t0\t0.000\n" in want
    # no counter behind `solid`: refused before anything is read
    with pytest.raises(SystemExit) as ei:
        cli.main(["-i", str(src), "-o", plain, "--abundance-report", rep, "solid", "-i", "none.solid", "-f", "solid"])
    assert ei.value.code not in (0, None)
