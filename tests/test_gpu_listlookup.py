"""Lookups in a count list (include/brx.h "lookups in a count list"): CountList.prepare_lookup builds the bucket directory
(br_amd/csrc/brx_listlookup.hip) and the abundance calls and get_counts answer from it (brx_abundance.hip: SRC_LIST).  Every
expected value comes from numpy -- br_amd/abundance.py over the CPU oracle's canonical hashes, br_amd/countops.py for the
directory and the lookup -- and every comparison is exact."""
import io
import os
import threading

import numpy as np
import pytest

import br_amd
from br_amd import _lib, countops, dist, keyfile, parts
from br_amd import abundance as ab
from br_amd.set import CountList, pack_reads
from oracle import oracle as O
from tests.test_gpu_abundance import check, noisy, rand_seq, same_stats
from tests.test_gpu_partition_lookup import forward_of_hash, revcomp_np

pytestmark = pytest.mark.gpu

TABLE = _lib.COUNT_TABLE

_cache = {}


def shared(key, make):
    """a reference computed once and shared between the tests that need it (never modified)"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def table_counter(k, reads):
    cnt = br_amd.Counter(k, 0, TABLE)
    cnt.add_reads(reads)
    return cnt


def list_of(k, keys, counts, floor=1):
    return CountList.from_keyfile(io.BytesIO(keyfile.encode(k, keys, counts, floor=floor)))


def counts_for(keys):
    """a count byte per key, 1 .. 255, all values taken"""
    return (np.arange(len(keys)) % 255 + 1).astype(np.uint8)


def outputs(obj, query, a):
    bases, offs = pack_reads(query)
    return obj.abundance_batch(bases, offs, a, profile=True, hist=True)


def same_outputs(x, y):
    assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2].tobytes() == y[2].tobytes()


def expect_from_list(k, keys, counts, query, a):
    """(profile, hist, stats) of `query` from the list itself, by countops.lookup"""
    cs = [countops.lookup(keys, counts, O.hashes(k, r)) for r in query]
    prof = np.concatenate([ab.profile_bytes(c, len(r)) for c, r in zip(cs, query)]) if query else np.zeros(0, np.uint8)
    hist = np.array([ab.hist_from_profile(c) for c in cs], dtype=np.uint32).reshape(len(query), 256)
    return prof, hist, ab.stats_array(cs, a)


def check_list(lst, k, keys, counts, query, a):
    got = outputs(lst, query, a)
    wp, wh, ws = expect_from_list(k, keys, counts, query, a)
    assert np.array_equal(got[0], wp) and np.array_equal(got[1], wh)
    same_stats(got[2], ws)
    return got


def check_directory(lst, k, keys, d):
    info = lst.lookup_info()
    want = countops.directory(keys, k, d)
    assert info["ready"] and lst.lookup_ready and info["log2_buckets"] == d and info["directory_bytes"] == 8 * ((1 << d) + 1)
    assert np.array_equal(lst.lookup_directory(), want)
    assert info["fullest_bucket"] == int(np.diff(want.astype(np.int64)).max())
    return want


def refused(call):
    with pytest.raises(_lib.BrxError) as ei:
        call()
    assert ei.value.status == _lib.BRX_ERR_UNSUPPORTED and "brx_counts_lookup_prepare" in str(ei.value)


# ---- 1. the reference's fixture -----------------------------------------------------------------------------------------
def test_fixture_k11(raw_reads):
    k, a = 11, 2
    cnt = table_counter(k, raw_reads)
    lst = CountList.from_counter(cnt)
    assert not lst.lookup_ready
    lst.prepare_lookup()
    h = shared(("raw", k), lambda: [O.hashes(k, r) for r in raw_reads])
    st = check(lst, k, h, raw_reads, h, a)
    assert int(st["kmers"].astype(np.int64).sum()) == 2_517_532 and int(st["min"].min()) >= 1 and int(st["max"].max()) > 40
    same_outputs(outputs(lst, raw_reads, a), outputs(cnt, raw_reads, a))
    keys, _ = lst.to_numpy()
    check_directory(lst, k, keys, countops.auto_log2_buckets(keys.size, k))


# ---- 2. plan shapes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [15, 21, 25, 31])
def test_plan_shapes(k):
    rng = np.random.default_rng(2000 + k)
    genome = rand_seq(rng, 3000)
    counted = [noisy(rng, genome, rng.integers(0, 3000), 300) for _ in range(80)]
    query = counted[:20] + [rand_seq(rng, 300).tobytes() for _ in range(10)]
    query += [b"", rand_seq(rng, k - 1).tobytes(), noisy(rng, genome, 5, k), noisy(rng, genome, 100, 1025)]
    ch, qh = [O.hashes(k, r) for r in counted], [O.hashes(k, r) for r in query]
    cnt = table_counter(k, counted)
    lst = CountList.from_counter(cnt)
    keys, counts = lst.to_numpy()
    assert keys.size > 3000
    one_each = min(int(np.ceil(np.log2(keys.size))), countops.max_log2_buckets(k))
    first = None
    for d in (None, 0, one_each, min(2 * k - 1, 20)):
        lst.prepare_lookup(d)
        want_d = countops.auto_log2_buckets(keys.size, k) if d is None else d
        check_directory(lst, k, keys, want_d)
        got = outputs(lst, query, 3)
        if first is None:
            first = got
            st = check(lst, k, ch, query, qh, 3)
            assert st["kmers"].tolist()[-4:] == [0, 0, 1, 1025 - k + 1] and int(st["absent"][20:30].min()) > 200
            same_outputs(got, outputs(cnt, query, 3))
        same_outputs(got, first)
    assert np.array_equal(lst.get_counts(forward_of_hash(keys[:2000])), counts[:2000])


# ---- 3. borders ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,ds", [(5, (0, 3, 9)), (13, (0, 7, 25)), (31, (0, 12, 20))])
def test_bucket_borders(k, ds):
    top = 1 << (2 * k - 1)
    for d in ds:
        shift = 2 * k - 1 - d
        inside = {0, 1, top - 1}
        for b in sorted({1, 2, (1 << d) // 2, (1 << d) - 1} & set(range(1, 1 << d))):
            inside |= {b << shift, (b << shift) - 1}
        keys = np.array(sorted(inside), dtype=np.uint64)
        outside = np.array(sorted({x + s for x in inside for s in (-1, 1) if 0 <= x + s < top} - inside), dtype=np.uint64)
        counts = counts_for(keys)
        lst = list_of(k, keys, counts)
        lst.prepare_lookup(d)
        check_directory(lst, k, keys, d)
        fwd_in, fwd_out = forward_of_hash(keys), forward_of_hash(outside)
        assert np.array_equal(lst.get_counts(fwd_in), counts) and np.array_equal(lst.get_counts(revcomp_np(fwd_in, k)), counts)
        assert outside.size and not lst.get_counts(fwd_out).any() and not lst.get_counts(revcomp_np(fwd_out, k)).any()
    # a random list under the chosen directory: every key its count, every absent neighbour 0
    rng = np.random.default_rng(3000 + k)
    keys = np.unique(rng.integers(0, top, min(50_000, top // 2), dtype=np.uint64))
    counts = counts_for(keys)
    lst = list_of(k, keys, counts)
    lst.prepare_lookup()
    check_directory(lst, k, keys, countops.auto_log2_buckets(keys.size, k))
    assert np.array_equal(lst.get_counts(forward_of_hash(keys)), counts)
    near = np.concatenate([keys[keys < np.uint64(top - 1)] + np.uint64(1), keys[keys > 0] - np.uint64(1)])
    near = near[~np.isin(near, keys)]
    assert near.size > keys.size // 4 and not lst.get_counts(forward_of_hash(near)).any()
    assert not lst.get_counts(revcomp_np(forward_of_hash(near), k)).any()


# ---- 4. skew ------------------------------------------------------------------------------------------------------------
def test_skewed_buckets():
    k, d = 21, 4
    rng = np.random.default_rng(4)
    poly_a, ac = np.frombuffer(b"A" * 400, dtype=np.uint8), np.frombuffer(b"AC" * 200, dtype=np.uint8)

    def two_letter(base, rate):
        """`base` with some of its letters drawn afresh from A and C alone: the k-mers (and their reverse complements over G
        and T) begin with two of those letters, so half of the 16 buckets stay empty"""
        r = base.copy()
        hit = rng.random(r.size) < rate
        r[hit] = rng.choice(np.frombuffer(b"AC", dtype=np.uint8), size=int(hit.sum()))
        return r.tobytes()

    counted = [two_letter(poly_a, 0.05) for _ in range(30)] + [two_letter(ac, 0.05) for _ in range(30)]
    counted += [bytes(poly_a), bytes(ac)]
    query = counted[:10] + counted[30:40] + [rand_seq(rng, 500).tobytes(), bytes(poly_a), bytes(ac), noisy(rng, poly_a, 0, 1100, 0.01)]
    ch, qh = [O.hashes(k, r) for r in counted], [O.hashes(k, r) for r in query]
    lst = CountList.from_counter(table_counter(k, counted))
    keys, counts = lst.to_numpy()
    lst.prepare_lookup(d)
    sizes = np.diff(check_directory(lst, k, keys, d).astype(np.int64))
    assert (sizes == 0).any() and int(sizes.max()) >= 150  # buckets of hundreds of keys beside empty ones
    first = outputs(lst, query, 2)
    check(lst, k, ch, query, qh, 2)
    lst.prepare_lookup()
    same_outputs(outputs(lst, query, 2), first)
    # the same list with 6000 more keys in one bucket: larger than any fixed search depth would take
    shift = 2 * k - 1 - d
    more = np.uint64(5 << shift) + rng.integers(0, 1 << shift, 6000, dtype=np.uint64)
    keys2 = np.union1d(keys, more)
    counts2 = counts_for(keys2)
    big = list_of(k, keys2, counts2)
    big.prepare_lookup(d)
    sizes2 = np.diff(check_directory(big, k, keys2, d).astype(np.int64))
    assert int(sizes2[5]) > 4096 and big.lookup_info()["fullest_bucket"] == int(sizes2.max()) > 4096
    assert np.array_equal(big.get_counts(forward_of_hash(keys2)), counts2)
    gone = np.setdiff1d(np.uint64(5 << shift) + rng.integers(0, 1 << shift, 3000, dtype=np.uint64), keys2)
    assert gone.size > 2000 and not big.get_counts(forward_of_hash(gone)).any()
    check_list(big, k, keys2, counts2, query, 2)


# ---- 5. small and floored -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 16, 17])
def test_small_lists(n):
    k = 21
    rng = np.random.default_rng(50 + n)
    keys = np.unique(rng.integers(0, 1 << (2 * k - 1), 64, dtype=np.uint64))[:n]
    counts = counts_for(keys)
    lst = list_of(k, keys, counts)
    refused(lambda: lst.get_counts([0]))
    lst.prepare_lookup()
    d = {0: 0, 1: 0, 16: 0, 17: 1}[n]
    check_directory(lst, k, keys, d) if n else None
    info = lst.lookup_info()
    assert info["ready"] and info["log2_buckets"] == d and info["fullest_bucket"] <= n
    assert np.array_equal(lst.lookup_directory(), countops.directory(keys, k, d))
    asked = np.concatenate([keys, keys + np.uint64(1), np.array([0, (1 << (2 * k - 1)) - 1], dtype=np.uint64)])
    assert np.array_equal(lst.get_counts(forward_of_hash(asked)), countops.lookup(keys, counts, asked))
    query = [rand_seq(rng, 200).tobytes(), b"", b"ACGT"]
    prof, hist, st = check_list(lst, k, keys, counts, query, 0)
    assert not prof.any() and st["kmers"].tolist() == [200 - k + 1, 0, 0] and st["absent"].tolist() == [200 - k + 1, 0, 0]


def test_floored_list():
    k = 15
    rng = np.random.default_rng(5)
    genome = rand_seq(rng, 2000)
    counted = [noisy(rng, genome, rng.integers(0, 2000), 250) for _ in range(60)]
    cnt = table_counter(k, counted)
    full, lst = CountList.from_counter(cnt), CountList.from_counter(cnt, 3)
    keys, counts = full.to_numpy()
    keep = counts >= 3
    assert lst.floor == 3 and 0 < lst.n == int(keep.sum()) < full.n
    lst.prepare_lookup()
    query = counted[:15] + [rand_seq(rng, 250).tobytes()]
    for a in (2, 5):
        got = check_list(lst, k, keys[keep], counts[keep], query, a)
        assert int(got[2]["above"].sum()) > 0
    # what the floor dropped answers 0, the rest as the counter answers
    fwd = forward_of_hash(keys)
    want = np.where(keep, counts, 0).astype(np.uint8)
    assert np.array_equal(lst.get_counts(fwd), want) and np.array_equal(cnt.get_counts(fwd), counts) and (want == 0).any()


# ---- 6. state -----------------------------------------------------------------------------------------------------------
def saved(lst, min_count=1):
    f = io.BytesIO()
    lst.save(f, min_count)
    return f.getvalue()


def test_state():
    k = 25
    rng = np.random.default_rng(6)
    genome = rand_seq(rng, 2000)
    counted = [noisy(rng, genome, rng.integers(0, 2000), 250) for _ in range(40)]
    lst = CountList.from_counter(table_counter(k, counted))
    other = CountList.from_counter(table_counter(k, counted[:10]))
    keys, counts = lst.to_numpy()
    bases, offs = pack_reads(counted[:3])
    before = {"file": saved(lst), "file3": saved(lst, 3), "spectrum": lst.spectrum(), "set": lst.finish(2).fingerprint(),
              "sum": saved(lst + other), "diff": saved(lst - other)}
    assert not lst.lookup_ready and lst.lookup_info() == {"ready": False, "log2_buckets": 0, "directory_bytes": 0, "fullest_bucket": 0}
    for call in (lambda: lst.get_counts(forward_of_hash(keys[:4])), lambda: lst.abundance_batch(bases, offs, 2), lst.lookup_directory,
                 lambda: lst.abundance_batch_device(None, None, 0, 0)):
        refused(call)
    lst.prepare_lookup()
    d0 = countops.auto_log2_buckets(keys.size, k)
    dir0 = check_directory(lst, k, keys, d0)
    first = outputs(lst, counted[:12], 2)
    lst.prepare_lookup()       # the same d: nothing happens
    lst.prepare_lookup(d0)
    assert np.array_equal(lst.lookup_directory(), dir0)
    lst.prepare_lookup(d0 + 3)  # another d: rebuilt
    assert not np.array_equal(check_directory(lst, k, keys, d0 + 3), dir0)
    same_outputs(outputs(lst, counted[:12], 2), first)
    for bad in (31, 50, countops.max_log2_buckets(k) + 1):
        with pytest.raises(_lib.BrxError) as ei:
            lst.prepare_lookup(bad)
        assert ei.value.status == _lib.BRX_ERR_ARG
    check_directory(lst, k, keys, d0 + 3)  # (a refused d leaves the directory in place)
    # every other entry ignores the directory
    both = lst + other
    after = {"file": saved(lst), "file3": saved(lst, 3), "spectrum": lst.spectrum(), "set": lst.finish(2).fingerprint(),
             "sum": saved(both), "diff": saved(lst - other)}
    assert all(np.array_equal(before[name], after[name]) for name in before)
    assert not both.lookup_ready and lst.lookup_ready
    refused(lambda: both.get_counts(forward_of_hash(keys[:4])))
    lst.drop_lookup()
    assert not lst.lookup_ready
    refused(lambda: lst.get_counts(forward_of_hash(keys[:4])))
    refused(lambda: lst.abundance_batch(bases, offs, 2))
    lst.drop_lookup()  # (twice is harmless)
    lst.prepare_lookup()
    same_outputs(outputs(lst, counted[:12], 2), first)


# ---- 7. slices ----------------------------------------------------------------------------------------------------------
def test_slices(tmp_path, raw_reads):
    k, n_parts = 25, 3
    reads = raw_reads[:30]
    src = str(tmp_path / "reads.fa")
    with open(src, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b">r%d\n%s\n" % (i, r))
    joined, _, _ = parts.count_in_parts([src], k, n_parts)
    cnt = table_counter(k, reads)
    joined.prepare_lookup()
    query = reads[:10] + raw_reads[200:203]
    same_outputs(outputs(joined, query, 2), outputs(cnt, query, 2))
    # one slice's list knows its own k-mers and answers 0 for the other parts'
    part = br_amd.Counter(k, 0, TABLE)
    part.set_slice(1, n_parts)
    part.add_reads(reads)
    mine = CountList.from_counter(part)
    mine.prepare_lookup()
    keys, counts = joined.to_numpy()
    own = dist.table_owner(keys, n_parts) == np.uint32(1)
    assert 0 < int(own.sum()) == mine.n < keys.size
    assert np.array_equal(mine.get_counts(forward_of_hash(keys)), np.where(own, counts, 0).astype(np.uint8))


# ---- 8. threads and streams ---------------------------------------------------------------------------------------------
def test_two_host_threads():
    k = 21
    rng = np.random.default_rng(8)
    genome = rand_seq(rng, 3000)
    counted = [noisy(rng, genome, rng.integers(0, 3000), 400) for _ in range(60)]
    lst = CountList.from_counter(table_counter(k, counted))
    lst.prepare_lookup()
    keys, counts = lst.to_numpy()
    want = outputs(lst, counted, 2)
    got, errors = {}, []

    def work(tag):
        try:
            got[tag] = [(outputs(lst, counted, 2), lst.get_counts(forward_of_hash(keys))) for _ in range(3)]
        except Exception as e:  # noqa: BLE001 (reported below)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in ("a", "b")]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors and sorted(got) == ["a", "b"]
    for tag in got:
        for out, c in got[tag]:
            same_outputs(out, want)
            assert np.array_equal(c, counts)


def test_device_entry_on_a_busy_stream():
    """the inputs hold a decoy until a delay queued on the caller's non-blocking stream has run, and become the real batch
    only in that stream's order: the entry must answer for the real batch"""
    import torch
    k, a = 21, 2
    rng = np.random.default_rng(9)
    genome = rand_seq(rng, 3000)
    counted = [noisy(rng, genome, rng.integers(0, 3000), 500) for _ in range(40)]
    decoy = [rand_seq(rng, 500).tobytes() for _ in range(40)]
    lst = CountList.from_counter(table_counter(k, counted))
    lst.prepare_lookup()
    want = outputs(lst, counted, a)
    assert not np.array_equal(want[0], outputs(lst, decoy, a)[0])
    (rb, ro), (db, do) = pack_reads(counted), pack_reads(decoy)
    assert np.array_equal(ro, do)
    n, total = len(counted), int(rb.size)
    dev = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).cuda()
    d_bases, d_off, real_bases = dev(db.copy()), dev(do.copy()), dev(rb.copy())
    d_prof = torch.full((total,), 0xEE, dtype=torch.uint8, device="cuda")
    d_hist = torch.full((n, 256), -1, dtype=torch.int32, device="cuda")
    d_stats = torch.full((n, ab.STATS_DTYPE.itemsize), 0xEE, dtype=torch.uint8, device="cuda")
    ballast = torch.randint(0, 1 << 30, (1 << 24,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        x = ballast
        for _ in range(32):
            x = torch.sort(x).values.flip(0)
        gate = torch.cuda.Event()
        gate.record()
        d_bases.copy_(real_bases, non_blocking=True)
    pending = not gate.query()
    lst.abundance_batch_device(d_bases.data_ptr(), d_off.data_ptr(), n, total, a, d_prof.data_ptr(), d_hist.data_ptr(), d_stats.data_ptr(),
                               s.cuda_stream)
    # complete on return: read back on another stream's order, after nothing but the call itself
    assert gate.query()
    torch.cuda.synchronize()
    assert pending, "the delay ran out before the call was issued: the probe has no teeth"
    assert np.array_equal(d_prof.cpu().numpy(), want[0])
    assert np.array_equal(d_hist.cpu().numpy().view(np.uint32), want[1])
    assert d_stats.cpu().numpy().tobytes() == want[2].tobytes()


# ---- 9 - 11. command line -----------------------------------------------------------------------------------------------
def small_fasta(path, reads, first=0):
    with open(path, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b">read%d some words\n%s\n" % (first + i, r))
    return path


def same_file(x, y):
    with open(x, "rb") as f, open(y, "rb") as g:
        a, b = f.read(), g.read()
    return a == b and len(a) > 100


def test_cli_count_parts(tmp_path, raw_reads):
    from br_amd import cli
    p = lambda name: str(tmp_path / name)
    src = small_fasta(p("reads.fa"), raw_reads[:30])
    head = ["-i", src, "-c", "one", "-s"]
    tail = ["fasta", "-i", src, "-k", "25", "-a", "2"]

    def run(tag, flags, more):
        files = ["-o", p(tag + ".out"), "--abundance-report", p(tag + ".tsv"), "--save-set", p(tag + ".set"), "--save-counts", p(tag + ".cnt"),
                 "--save-min-count", "2"]
        assert cli.main(head + files + flags + tail + more) == 0

    run("a", [], [])
    run("b", ["--list-lookup"], ["--count-parts", "3"])
    for ext in (".tsv", ".set", ".cnt", ".out"):
        assert same_file(p("a" + ext), p("b" + ext)), ext
    with open(p("b.tsv"), "rb") as f:
        lines = f.read().splitlines()
    assert lines[0] + b"\n" == ab.REPORT_HEADER and len(lines) == 31 and lines[1].startswith(b"read0\t")
    # (the report counts the k-mers seen once too, which neither -a 2 nor --save-min-count 2 keep: absent = 0 for counted reads)
    assert all(line.split(b"\t")[3] == b"0" for line in lines[1:])


def test_cli_count(tmp_path, raw_reads):
    from br_amd import cli
    k = 15
    p = lambda name: str(tmp_path / name)
    src = small_fasta(p("reads.fa"), raw_reads[:24])
    for name, reads in (("a.keys", raw_reads[:12]), ("b.keys", raw_reads[12:24])):
        with open(p(name), "wb") as f:
            f.write(keyfile.encode(k, *ab.count_table([O.hashes(k, r) for r in reads]), floor=1))
    head = ["-i", src, "-c", "one", "-s"]
    assert cli.main(head + ["-o", p("1.out"), "--list-lookup", "--abundance-report", p("r1.tsv"), "count", "-i", p("a.keys"), "--counts-add",
                            p("b.keys"), "-a", "2", "--save-counts", p("job.keys")]) == 0
    assert cli.main(head + ["-o", p("2.out"), "--abundance-report", p("r2.tsv"), "count", "-i", p("job.keys"), "-a", "2"]) == 0
    assert same_file(p("r1.tsv"), p("r2.tsv")) and same_file(p("1.out"), p("2.out"))
    # the flag alone sends `count` down the list route: the same set, the same corrected reads
    assert cli.main(head + ["-o", p("3.out"), "--save-set", p("3.set"), "--list-lookup", "count", "-i", p("job.keys"), "-a", "2"]) == 0
    assert cli.main(head + ["-o", p("4.out"), "--save-set", p("4.set"), "count", "-i", p("job.keys"), "-a", "2"]) == 0
    assert same_file(p("3.set"), p("4.set")) and same_file(p("3.out"), p("4.out")) and same_file(p("3.out"), p("1.out"))


def test_cli_errors(tmp_path, raw_reads):
    from br_amd import cli
    p = lambda name: str(tmp_path / name)
    src = small_fasta(p("reads.fa"), raw_reads[:2])
    with pytest.raises(SystemExit) as ei:
        cli.main(["-i", src, "-o", p("x.out"), "--list-lookup", "solid", "-i", src, "-f", "fasta", "-k", "15"])
    assert "--list-lookup" in str(ei.value) and "`solid`" in str(ei.value) and not os.path.exists(p("x.out"))
    with pytest.raises(SystemExit) as ei:
        cli.main(["-i", src, "-o", p("y.out"), "--list-lookup", "fasta", "-i", src, "-k", "15", "-a", "1"])
    assert "--list-lookup" in str(ei.value) and "--count-parts" in str(ei.value)
