"""K-mer abundance from the partitioned counter (BRX_COUNT_SORTED): Counter.prepare_lookup turns the last-level buckets into
a sorted count view (br_amd/csrc/brx_partbuild.hip: final_view_kernel) and the abundance calls and get_counts answer from it
(brx_abundance.hip: SRC_PART).  Every expected value comes from br_amd/abundance.py -- numpy over the CPU oracle's
canonical hashes -- and every comparison is exact.  Every test calls prepare_lookup."""
import numpy as np
import pytest

import br_amd
from br_amd import _lib, cover
from br_amd import abundance as ab
from br_amd.set import pack_reads
from oracle import oracle as O
from tests.test_gpu_abundance import check, noisy, rand_seq

pytestmark = pytest.mark.gpu

SORTED, TABLE, DENSE = _lib.COUNT_SORTED, _lib.COUNT_TABLE, _lib.COUNT_DENSE

_cache = {}


def shared(key, make):
    """a reference computed once and shared between the tests that need it (never modified)"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def prepared(k, reads, strategy=SORTED):
    cnt = br_amd.Counter(k, 0, strategy)
    cnt.add_reads(reads)
    cnt.prepare_lookup()
    assert cnt.lookup_ready
    return cnt


def outputs(cnt, query, a):
    bases, offs = pack_reads(query)
    return cnt.abundance_batch(bases, offs, a, profile=True, hist=True)


def same_outputs(x, y):
    assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2].tobytes() == y[2].tobytes()


def forward_of_hash(h):
    """the forward k-mer that is its own canonical form and has canonical hash h: h << 1 with the parity bit that makes the
    popcount even"""
    x = np.asarray(h, dtype=np.uint64) << np.uint64(1)
    par = x.copy()
    for sh in (32, 16, 8, 4, 2, 1):
        par ^= par >> np.uint64(sh)
    return x | (par & np.uint64(1))


def revcomp_np(x, k):
    x = np.asarray(x, dtype=np.uint64) ^ np.uint64(int("10" * k, 2))
    rc = np.zeros_like(x)
    for _ in range(k):
        rc = (rc << np.uint64(2)) | (x & np.uint64(3))
        x = x >> np.uint64(2)
    return rc


# ---- 1. the reference's fixture -----------------------------------------------------------------------------------------
def test_fixture_k11(raw_reads):
    k, a = 11, 2
    h = shared(("raw", k), lambda: [O.hashes(k, r) for r in raw_reads])
    cnt = prepared(k, raw_reads)
    st = check(cnt, k, h, raw_reads, h, a)
    assert int(st["kmers"].astype(np.int64).sum()) == 2_517_532 and int(st["min"].min()) >= 1 and int(st["max"].max()) > 40
    dense = br_amd.Counter(k, 0, DENSE)
    dense.add_reads(raw_reads)
    same_outputs(outputs(cnt, raw_reads, a), outputs(dense, raw_reads, a))


# ---- 2. every plan shape ------------------------------------------------------------------------------------------------
def plan_case(k):
    """(counted reads, their hashes, queries, their hashes): 80 noisy reads of a 3 000-base genome; the counted reads,
    unrelated random reads and the lengths around k and around a tile of 1024 positions as queries"""
    def make():
        rng = np.random.default_rng(2000 + k)
        genome = rand_seq(rng, 3000)
        counted = [noisy(rng, genome, rng.integers(0, 3000), rng.integers(100, 601)) for _ in range(80)]
        query = counted + [rand_seq(rng, n).tobytes() for n in (300, 500, 0, k - 1, k, 1025)]
        query += [noisy(rng, genome, rng.integers(0, 3000), 1025), b"", counted[0][:k - 1], counted[1][:k]]
        ch = [O.hashes(k, r) for r in counted]
        return counted, ch, query, ch + [O.hashes(k, r) for r in query[len(counted):]]
    return shared(("plan", k), make)


def run_plan_case(k):
    counted, ch, query, qh = plan_case(k)
    a = 3
    cnt = prepared(k, counted)
    st = check(cnt, k, ch, query, qh, a)
    assert int(st["min"][:80].min()) >= 1 and int(st["max"].max()) > 5  # counted reads: never absent
    assert int(st["absent"][80:82].sum()) > (700 if k >= 13 else 0)  # random reads: (at k >= 13) nearly all absent
    assert st["kmers"][82:86].tolist() == [0, 0, 1, 1025 - k + 1]
    if k >= 15:
        same_outputs(outputs(cnt, query, a), outputs(prepared(k, counted, TABLE), query, a))


# k = 7 is the smallest k the partitioned counter takes (13 hash bits: one to partition away, a zero-bit second digit);
# 9 and 13: two levels; 15: two levels of 9 and 8 bits; 19: three levels; 21: four levels, u32 keys at their limit
@pytest.mark.parametrize("k", [7, 9, 13, 15, 19, 21])
def test_plan_shapes(k):
    run_plan_case(k)


# ---- 3. a full bucket ---------------------------------------------------------------------------------------------------
def full_case():
    def make():
        k = 9
        rng = np.random.default_rng(9)
        reads = [rand_seq(rng, 1000).tobytes() for _ in range(300)]
        table = ab.count_table([O.hashes(k, r) for r in reads])
        fwd = np.arange(4 ** k, dtype=np.uint64)
        want = ab.lookup(table, np.array([O.khash(int(x), k) for x in fwd], dtype=np.uint64))
        return reads, table, fwd, want
    return shared("full", make)


def run_full_bucket():
    """k = 9: 32 buckets of 4096 hashes, ~9 300 keys each -- far more than are staged, nearly every hash present: the
    deepest search, and the first and the last entry of every bucket"""
    k = 9
    reads, table, fwd, want = full_case()
    uniq, _ = table
    per_bucket = np.bincount((uniq >> np.uint64(12)).astype(np.int64), minlength=32)
    assert per_bucket.size == 32 and per_bucket.min() > 3500
    cnt = prepared(k, reads)
    got = cnt.get_counts(fwd)
    bad = np.flatnonzero(got != want)
    assert not bad.size, (bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
    assert want.max() > 5 and (want == 0).any()


def test_full_bucket():
    run_full_bucket()


# ---- 4. saturation and one heavy key ------------------------------------------------------------------------------------
def test_saturation_and_heavy_key():
    k = 15
    rng = np.random.default_rng(4)
    kmers = []
    while len(kmers) < 4:
        s = rand_seq(rng, k).tobytes()
        if int(O.hashes(k, s)[0]) not in [int(O.hashes(k, t)[0]) for t in kmers]:
            kmers.append(s)
    times = (254, 255, 256, 300)
    poly = b"A" * 70_000  # one hash, 69 986 times: more than a 16-bit counter holds
    reads = [poly] + [s for s, n in zip(kmers, times) for _ in range(n)]
    cnt = prepared(k, reads)
    fwd = np.array([int(cover.kmers_of(s, k)[0]) for s in kmers] + [0], dtype=np.uint64)
    assert cnt.get_counts(fwd).tolist() == [254, 255, 255, 255, 255]
    prof, st = cnt.abundance_reads(kmers + [poly[:2000]], 254)
    assert [int(p[0]) for p in prof[:4]] == [254, 255, 255, 255] and (prof[4] == 255).all() and prof[4].size == 2000 - k + 1
    assert st["above"].tolist() == [0, 1, 1, 1, 2000 - k + 1]
    ch = [O.hashes(k, poly)] + [np.repeat(O.hashes(k, s), n) for s, n in zip(kmers, times)]
    query = kmers + [poly[:1500], rand_seq(rng, 400).tobytes()]
    check(cnt, k, ch, query, [O.hashes(k, q) for q in query], 254)


# ---- 5. absent keys and edges -------------------------------------------------------------------------------------------
def test_absent_keys_and_edges():
    k = 21
    top = (1 << (2 * k - 1)) - 1  # 2^41 - 1, the largest hash
    rng = np.random.default_rng(5)
    genome = rand_seq(rng, 3000)
    reads = [noisy(rng, genome, rng.integers(0, 3000), rng.integers(100, 601)) for _ in range(20)]
    table = ab.count_table([O.hashes(k, r) for r in reads])
    uniq, _ = table
    u = uniq.astype(np.int64)
    buckets = np.unique(u >> 12)
    near = np.unique(np.concatenate([buckets - 1, buckets, buckets + 1]))
    q = np.concatenate([u, u - 1, u + 1, [0, top], near << 12, (near << 12) + 4095])
    q = np.unique(q[(q >= 0) & (q <= top)]).astype(np.uint64)
    want = ab.lookup(table, q)
    assert (want > 0).sum() == uniq.size and (want == 0).sum() > uniq.size
    cnt = prepared(k, reads)
    x = forward_of_hash(q)
    assert all(O.khash(int(v), k) == int(h) for v, h in zip(x[:50], q[:50]))  # x is its own canonical form
    got = cnt.get_counts(x)
    bad = np.flatnonzero(got != want)
    assert not bad.size, (q[bad[:8]].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
    assert np.array_equal(cnt.get_counts(revcomp_np(x, k)), want)


# ---- 6. batches and the view's life -------------------------------------------------------------------------------------
def test_batches_and_view_life():
    k, a = 15, 2
    counted, ch, query, qh = plan_case(k)
    more = [r[::-1] for r in counted[:30]]
    one = prepared(k, counted)
    ref = outputs(one, query, a)
    cnt = br_amd.Counter(k, 0, SORTED)
    assert not cnt.lookup_ready
    for lo, hi in ((0, 3), (3, 50), (50, 80)):
        cnt.add_reads(counted[lo:hi])
    cnt.prepare_lookup()
    same_outputs(outputs(cnt, query, a), ref)
    # anything that touches the batches drops the view, and the calls refuse as they do without one
    cnt.add_reads(more)
    assert not cnt.lookup_ready
    bases, offs = pack_reads(query)
    for call in (lambda: cnt.abundance_batch(bases, offs), lambda: cnt.get_counts([1, 2, 3])):
        with pytest.raises(_lib.BrxError) as ei:
            call()
        assert ei.value.status == _lib.BRX_ERR_UNSUPPORTED and "BRX_COUNT_TABLE" in str(ei.value)
    cnt.prepare_lookup()
    check(cnt, k, ch + [O.hashes(k, r) for r in more], query, qh, a)
    for drop in (cnt.spectrum, lambda: cnt.finish(a), cnt.drop_lookup, cnt.reset):
        cnt.prepare_lookup()
        assert cnt.lookup_ready
        drop()
        assert not cnt.lookup_ready
    cnt.prepare_lookup()  # after reset: nothing counted
    prof, hist, st = outputs(cnt, query, a)
    assert cnt.lookup_ready and not prof.any() and np.array_equal(st["absent"], st["kmers"]) and not st["max"].any()
    assert np.array_equal(hist[:, 0], st["kmers"]) and not hist[:, 1:].any()
    assert not cnt.get_counts(cover.kmers_of(counted[0], k)).any()
    # the other counters: always ready, prepare and drop change nothing
    for strategy, kk in ((DENSE, 11), (TABLE, 15)):
        c2 = br_amd.Counter(kk, 0, strategy)
        c2.add_reads(counted)
        assert c2.lookup_ready
        before = outputs(c2, query, a)
        c2.prepare_lookup()
        c2.drop_lookup()
        assert c2.lookup_ready
        same_outputs(outputs(c2, query, a), before)


# ---- 7. the counter is untouched ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [15, 21])
def test_counter_untouched(k):
    counted, ch, query, qh = plan_case(k)
    twin = br_amd.Counter(k, 0, SORTED)
    twin.add_reads(counted)
    cnt = prepared(k, counted)
    above = {}
    for a in (0, 2, 5):
        cnt.prepare_lookup()
        above[a] = cnt.abundance_reads(query, a)[1]
        cnt.get_counts(cover.kmers_of(counted[0], k))
        assert np.array_equal(cnt.spectrum(), twin.spectrum())
        cnt.prepare_lookup()
        got, want = cnt.finish(a), twin.finish(a)
        if k == 15:
            assert got.to_solid_bytes() == want.to_solid_bytes()
        else:
            assert got.fingerprint() == want.fingerprint() and got.fingerprint()[0] > 0
        cst = got.cover_reads(query)[1]
        assert np.array_equal(above[a]["above"], cst["solid"]) and np.array_equal(above[a]["kmers"], cst["kmers"])
    assert int(above[0]["above"].sum()) > int(above[5]["above"].sum()) > 0


# ---- 8. grid trips ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["1", "3"])
@pytest.mark.parametrize("case", ["plan15", "plan21", "full"])
def test_grid_trips(monkeypatch, case, grid):
    """BRX_READ_GRID: one block (three blocks) of the view kernel take all the buckets in turn, and the helper kernels of
    the lookup their reads"""
    monkeypatch.setenv("BRX_READ_GRID", grid)
    if case == "full":
        run_full_bucket()
    else:
        run_plan_case(int(case[4:]))


# ---- 9. CLI -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [["-a", "2"], ["first-minimum"]])
def test_cli_abundance_report_k21(tmp_path, method):
    """--abundance-report at k = 21.  The command line still counts into the hash table when the report is asked for (the
    partitioned counter's count + view + lookup measured slower: DESIGN.md section 10.11), so no timer is asserted here;
    the same report written from a partitioned counter after prepare_lookup must be the same bytes"""
    from br_amd import cli, spectrum
    k = 21
    rng = np.random.default_rng(21)
    genome = rand_seq(rng, 2000)
    reads = [noisy(rng, genome, rng.integers(0, 2000), rng.integers(100, 600)) for _ in range(60)] + [b"ACGTACGT", rand_seq(rng, 300).tobytes()]
    src = tmp_path / "reads.fasta"
    with open(src, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b">read%d some description\n" % i + r + b"\n")
    hs = [O.hashes(k, r) for r in reads]
    if method[0] == "-a":
        a = 2
    else:
        _, counts = np.unique(np.concatenate(hs), return_counts=True)
        hist = np.bincount(np.minimum(counts, 255), minlength=256).astype(np.uint64)
        hist[0] = (1 << (2 * k - 1)) - counts.size
        a = spectrum.get_threshold(hist, "first-minimum")
        assert a is not None
    plain, with_rep, rep, rep_part = (str(tmp_path / n) for n in ("plain.fasta", "rep.fasta", "abund.tsv", "abund_part.tsv"))
    tail = ["-c", "one", "-b", "7", "fasta", "-i", str(src), "-k", str(k)] + method
    assert cli.main(["-i", str(src), "-o", plain] + tail) == 0
    assert cli.main(["-i", str(src), "-o", with_rep, "--abundance-report", rep] + tail) == 0
    assert open(with_rep, "rb").read() == open(plain, "rb").read()
    want = ab.REPORT_HEADER + b"".join(ab.report_line(b"read%d" % i, len(r), ab.stats_from_profile(p, a))
                                      for i, (r, p) in enumerate(zip(reads, ab.profile_from_hashes(hs))))
    assert open(rep, "rb").read() == want
    assert want.count(b"\n") == len(reads) + 1 and b"\t0\t0\t0\t0\t0\t0\t0.000\n" in want
    # the counter `fasta` builds without the flag, through the report writer of the command line
    cnt = br_amd.Counter(k)
    with open(src, "rb") as f:
        cnt.count_fasta(f)
    assert not cnt.lookup_ready
    cnt.finish(a)
    cnt.prepare_lookup()
    with open(src, "rb") as f, open(rep_part, "wb") as out:
        cli.write_abundance_report(cnt, a, f, out, 7)
    assert open(rep_part, "rb").read() == want
