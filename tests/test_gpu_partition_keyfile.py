"""Count files from the partitioned counter (BRX_COUNT_SORTED): brx_counter_save_fd compacts the count view that
Counter.prepare_lookup built (br_amd/csrc/brx_keyfile.hip: view_compact_kernel) and packs it -- no listing from table slots,
no sort.  Every expected file is keyfile.encode over abundance.count_table of the CPU oracle's hashes, every comparison is
exact, and where a table counter takes the k its file of the same reads must be the same bytes."""
import gzip
import io
import os
import threading

import numpy as np
import pytest

import br_amd
from br_amd import _lib, abundance, cover, keyfile
from oracle import oracle as O
from tests.test_gpu_abundance import noisy, rand_seq
from tests.test_gpu_partition_lookup import full_case, outputs, plan_case, same_outputs, shared

pytestmark = pytest.mark.gpu

SORTED, TABLE = _lib.COUNT_SORTED, _lib.COUNT_TABLE


def table_of(key, k, reads):
    """(keys, counts clipped at 255) of the reads, in numpy over the oracle's hashes; computed once, never modified"""
    return shared(("keyfile table",) + tuple(key), lambda: abundance.count_table([O.hashes(k, r) for r in reads]))


def expected(table, k, min_count):
    keys, counts = table
    floor = max(min_count, 1)
    keep = counts >= floor
    return keyfile.encode(k, keys[keep], counts[keep], floor=floor)


def counter(k, reads, strategy=SORTED, pieces=None):
    cnt = br_amd.Counter(k, 0, strategy)
    for lo, hi in pieces or [(0, len(reads))]:
        cnt.add_reads(reads[lo:hi])
    cnt.prepare_lookup()
    return cnt


def saved(cnt, min_count=1):
    f = io.BytesIO()
    st = cnt.save(f, min_count)
    data = f.getvalue()
    assert st["bytes"] == len(data) and st["blocks"] == (st["keys"] + 255) // 256
    return data


def refused(call):
    with pytest.raises(_lib.BrxError) as ei:
        call()
    assert ei.value.status == _lib.BRX_ERR_UNSUPPORTED
    for word in ("partitioned", "BRX_COUNT_TABLE", "brx_counter_lookup_prepare"):
        assert word in str(ei.value), str(ei.value)


# ---- 1. the reference's fixture -----------------------------------------------------------------------------------------
def test_fixture_k11(raw_reads):
    k = 11
    table = table_of(("raw", k), k, raw_reads)
    cnt = counter(k, raw_reads)
    tab = counter(k, raw_reads, TABLE)
    for min_count in (1, 2, 3):
        want = expected(table, k, min_count)
        assert saved(cnt, min_count) == want, min_count
        assert saved(tab, min_count) == want, min_count
    assert table[0].size > 100_000 and len(want) < len(expected(table, k, 1))


# ---- 2. every plan shape ------------------------------------------------------------------------------------------------
def run_plan_case(k):
    counted, ch, _, _ = plan_case(k)
    table = shared(("keyfile plan", k), lambda: abundance.count_table(ch))
    cnt = counter(k, counted)
    tab = counter(k, counted, TABLE) if k >= 15 else None
    for min_count in (1, 3):
        want = expected(table, k, min_count)
        got = saved(cnt, min_count)
        assert got == want, (k, min_count)
        assert keyfile.decode(got)[1].size > (50 if k >= 9 else 0)  # (something is kept at 3 too)
        if tab is not None:
            assert saved(tab, min_count) == want, (k, min_count)


# 7: the smallest plan (two buckets); 9, 13, 15: two levels; 19: three; 21: four levels, 2^29 buckets, nearly all empty
@pytest.mark.parametrize("k", [7, 9, 13, 15, 19, 21])
def test_plan_shapes(k):
    run_plan_case(k)


# ---- 3. full buckets ----------------------------------------------------------------------------------------------------
def run_full_buckets():
    """k = 9: 32 buckets of more than 3 500 distinct keys each, the wave-per-bucket walk over ~9 300 positions a bucket; the
    first and the last entry of every bucket are in the file, and the keys either side of every bucket edge"""
    k = 9
    reads, table, _, _ = full_case()
    keys, counts = table
    per_bucket = np.bincount((keys >> np.uint64(12)).astype(np.int64), minlength=32)
    assert per_bucket.size == 32 and per_bucket.min() > 3500
    cnt = counter(k, reads)
    for min_count in (1, 3):
        got = saved(cnt, min_count)
        assert got == expected(table, k, min_count), min_count
    kk, gk, gc, floor = keyfile.decode(saved(cnt))
    assert (kk, floor) == (k, 1) and np.array_equal(gk, keys) and np.array_equal(gc, counts)
    edges = np.flatnonzero(np.diff((gk >> np.uint64(12)).astype(np.int64))) # last entry of a bucket, the next one's first follows
    assert edges.size == 31 and np.array_equal(gk[edges + 1], keys[edges + 1]) and np.array_equal(gk[edges], keys[edges])


def test_full_buckets():
    run_full_buckets()


# ---- 4. saturation and one heavy key ------------------------------------------------------------------------------------
def test_saturation_and_heavy_key():
    k = 15
    rng = np.random.default_rng(4)
    kmers = []
    while len(kmers) < 4:
        s = rand_seq(rng, k).tobytes()
        if int(O.hashes(k, s)[0]) not in [int(O.hashes(k, t)[0]) for t in kmers] + [0]:
            kmers.append(s)
    times = (254, 255, 256, 300)
    poly = b"A" * 70_000  # one hash, 69 986 times: a bucket range of 69 986 positions holding one key, then padding
    reads = [poly] + [s for s, n in zip(kmers, times) for _ in range(n)]
    table = abundance.count_table([O.hashes(k, poly)] + [np.repeat(O.hashes(k, s), n) for s, n in zip(kmers, times)])
    cnt = counter(k, reads)
    data = saved(cnt)
    assert data == expected(table, k, 1)
    _, keys, counts, _ = keyfile.decode(data)
    by_key = dict(zip(keys.tolist(), counts.tolist()))
    assert [by_key[int(O.hashes(k, s)[0])] for s in kmers] == [254, 255, 255, 255] and by_key[0] == 255 and len(by_key) == 5
    top = saved(cnt, 255)
    assert top == expected(table, k, 255)
    _, keys, counts, floor = keyfile.decode(top)
    assert keys.size == 4 and floor == 255 and (counts == 255).all()
    assert saved(cnt, 0) == data  # 0 means 1
    assert saved(counter(k, reads, TABLE), 255) == top


# ---- 5. the life of the view --------------------------------------------------------------------------------------------
def test_view_life():
    k = 15
    counted, ch, _, _ = plan_case(k)
    table = shared(("keyfile plan", k), lambda: abundance.count_table(ch))
    want = expected(table, k, 1)
    cnt = br_amd.Counter(k, 0, SORTED)
    refused(lambda: cnt.save(io.BytesIO()))  # an empty counter without a view
    for lo, hi in ((0, 3), (3, 50), (50, 80)):  # three batches give the file of one
        cnt.add_reads(counted[lo:hi])
    refused(lambda: cnt.save(io.BytesIO()))  # nothing prepares the view implicitly
    assert not cnt.lookup_ready
    cnt.prepare_lookup()
    assert saved(cnt) == want
    for drop in (cnt.spectrum, lambda: cnt.finish(2), cnt.drop_lookup):
        cnt.prepare_lookup()
        assert saved(cnt) == want
        drop()
        refused(lambda: cnt.save(io.BytesIO()))
    cnt.prepare_lookup()
    cnt.add_reads(counted[:5])
    refused(lambda: cnt.save(io.BytesIO()))
    cnt.prepare_lookup()
    assert saved(cnt) == expected(abundance.count_table(ch + ch[:5]), k, 1)
    cnt.reset()
    refused(lambda: cnt.save(io.BytesIO()))
    cnt.prepare_lookup()  # after reset: nothing counted, the header-only count file
    empty = saved(cnt, 3)
    assert len(empty) == 32 and empty == keyfile.encode(k, np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint8), floor=3)
    assert cnt.floor == 1
    # a counter that never counted anything, with a view
    fresh = br_amd.Counter(9, 0, SORTED)
    fresh.prepare_lookup()
    assert saved(fresh) == keyfile.encode(9, np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint8), floor=1)
    # loading into a partitioned counter stays refused, view or not
    with pytest.raises(_lib.BrxError) as ei:
        fresh.load(io.BytesIO(empty))
    assert ei.value.status == _lib.BRX_ERR_UNSUPPORTED and "BRX_COUNT_TABLE" in str(ei.value)


# ---- 6. the counter is untouched ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [15, 21])
def test_counter_untouched(k):
    counted, ch, query, _ = plan_case(k)
    table = shared(("keyfile plan", k), lambda: abundance.count_table(ch))
    twin = counter(k, counted)
    cnt = counter(k, counted)
    for min_count in (1, 3):
        assert saved(cnt, min_count) == expected(table, k, min_count)
        assert cnt.lookup_ready
    for a in (0, 2):
        same_outputs(outputs(cnt, query, a), outputs(twin, query, a))
    fwd = cover.kmers_of(counted[0], k)
    assert np.array_equal(cnt.get_counts(fwd), twin.get_counts(fwd)) and cnt.get_counts(fwd).all()
    assert saved(cnt) == expected(table, k, 1)
    assert np.array_equal(cnt.spectrum(), twin.spectrum())
    for a in (0, 2):
        cnt.prepare_lookup()
        saved(cnt)
        got, want = cnt.finish(a), twin.finish(a)
        if k == 15:
            assert got.to_solid_bytes() == want.to_solid_bytes()
        else:
            assert got.fingerprint() == want.fingerprint() and got.fingerprint()[0] > 0


# ---- 7. round trip ------------------------------------------------------------------------------------------------------
def test_round_trip():
    k = 19
    counted, ch, _, _ = plan_case(k)
    cnt = counter(k, counted)
    data = saved(cnt)
    back = br_amd.Counter.from_keyfile(io.BytesIO(data))
    fwd = np.concatenate([cover.kmers_of(r, k) for r in counted[:10]])
    got = back.get_counts(fwd)
    assert np.array_equal(got, cnt.get_counts(fwd)) and got.all() and int(got.max()) > 5
    assert saved(back) == data  # and the table counter saves the same file
    assert br_amd.Pcon.from_keyfile(io.BytesIO(data)).fingerprint() == cnt.finish(0).fingerprint()
    # two partitioned shards saved apart, loaded into one table counter
    both = br_amd.Counter(k, 0, TABLE)
    for lo, hi in ((0, 30), (30, 80)):
        both.load(io.BytesIO(saved(counter(k, counted[lo:hi]))))
    assert saved(both) == saved(counter(k, counted, TABLE)) == data


# ---- 8. no sort, and the pieces -----------------------------------------------------------------------------------------
def test_no_sort_and_pieces(monkeypatch, tmp_path):
    k = 19
    counted, ch, _, _ = plan_case(k)
    want = expected(shared(("keyfile plan", k), lambda: abundance.count_table(ch)), k, 1)
    cnt = counter(k, counted)
    _lib.profile_enable(True)
    try:
        _lib.profile_reset()
        data = saved(cnt)
        prof = _lib.profile_all()
    finally:
        _lib.profile_enable(False)
    assert data == want
    assert prof["key_list"]["launches"] >= 2 and prof["key_pack"]["launches"] >= 2
    assert prof.get("key_sort", {"launches": 0})["launches"] == 0
    monkeypatch.setenv("BRX_KEYFILE_SLICE_KB", "4")
    assert len(want) > 3 * 4096 and saved(cnt) == want
    monkeypatch.delenv("BRX_KEYFILE_SLICE_KB")
    path = str(tmp_path / "counts.keys.gz")
    with gzip.open(path, "wb") as f:
        cnt.save(f)
    assert gzip.open(path, "rb").read() == want
    r, w = os.pipe()
    got = []
    t = threading.Thread(target=lambda: got.append(os.fdopen(r, "rb").read()))
    t.start()
    with os.fdopen(w, "wb") as wf:
        cnt.save(wf)
    t.join()
    assert got[0] == want


# ---- 9. grid trips ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["1", "3"])
@pytest.mark.parametrize("case", ["plan15", "plan21", "full"])
def test_grid_trips(monkeypatch, case, grid):
    """BRX_READ_GRID: one block (three blocks) of the compaction take all the chunks of buckets in turn"""
    monkeypatch.setenv("BRX_READ_GRID", grid)
    if case == "full":
        run_full_buckets()
    else:
        run_plan_case(int(case[4:]))


def test_wide_groups(monkeypatch):
    """BRX_VIEW_WIDE_SPAN=1: every group of buckets takes the path of one that spans 2^32 positions, bucket by bucket with
    no 32-bit distances; 300: only the groups that hold more positions than that"""
    for span in ("1", "300"):
        monkeypatch.setenv("BRX_VIEW_WIDE_SPAN", span)
        run_plan_case(15)
        run_plan_case(21)
        run_full_buckets()


# ---- 10. command line ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,tail,min_count", [(19, ["-a", "2"], None), (21, ["first-minimum"], 2)])
def test_cli_save_counts(tmp_path, k, tail, min_count):
    """`fasta --save-counts` at k = 19 and 21 without --abundance-report: the file is the numpy statement and the corrected
    output is that of the run without the flag.  The command line keeps the partitioned counter there (its path measured
    faster at both k: profiles/partition_keyfile_bench.json), so nothing runs under tab_count and nothing is sorted"""
    from br_amd import cli
    rng = np.random.default_rng(k)
    genome = rand_seq(rng, 2000)
    reads = [noisy(rng, genome, rng.integers(0, 2000), rng.integers(100, 600)) for _ in range(60)] + [b"ACGTACGT", rand_seq(rng, 300).tobytes()]
    src = tmp_path / "reads.fasta"
    with open(src, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b">read%d some description\n" % i + r + b"\n")
    plain, with_counts, cfile = (str(tmp_path / n) for n in ("plain.fasta", "counts.fasta", "C"))
    sub = ["-c", "one", "-b", "7", "fasta", "-i", str(src), "-k", str(k)] + tail
    flags = ["--save-counts", cfile] + (["--save-min-count", str(min_count)] if min_count else [])
    assert cli.main(["-i", str(src), "-o", plain] + sub) == 0
    _lib.profile_enable(True)
    try:
        _lib.profile_reset()
        assert cli.main(["-i", str(src), "-o", with_counts] + flags + sub) == 0
        prof = _lib.profile_all()
    finally:
        _lib.profile_enable(False)
    assert open(cfile, "rb").read() == expected(abundance.count_table([O.hashes(k, r) for r in reads]), k, min_count or 1)
    assert open(with_counts, "rb").read() == open(plain, "rb").read() and len(open(plain, "rb").read()) > 1000
    assert prof.get("tab_count", {"launches": 0})["launches"] == 0 and prof.get("key_sort", {"launches": 0})["launches"] == 0
    assert prof["key_list"]["launches"] >= 2 and prof["part_view"]["launches"] >= 1
    if k == 19:  # with --abundance-report the counter is the table, as before, and the file the same bytes
        _lib.profile_enable(True)
        try:
            _lib.profile_reset()
            assert cli.main(["-i", str(src), "-o", with_counts, "--abundance-report", str(tmp_path / "ab.tsv")] + flags + sub) == 0
            prof = _lib.profile_all()
        finally:
            _lib.profile_enable(False)
        assert open(cfile, "rb").read() == expected(abundance.count_table([O.hashes(k, r) for r in reads]), k, 1)
        assert prof["tab_count"]["launches"] >= 1 and prof["key_sort"]["launches"] >= 1
