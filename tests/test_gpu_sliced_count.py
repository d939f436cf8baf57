"""Sliced counting (include/brx.h "sliced counting", br_amd/parts.py): a table counter that counts only the k-mers one part
of P owns, the driver that counts a job part by part and joins the parts' lists, and `--count-parts`.  Expected values
come from the CPU oracle's hashes, dist.table_owner, parts.py and keyfile.encode."""
import gzip
import io

import numpy as np
import pytest

import br_amd
from br_amd import _lib, cli, dist, keyfile, parts
from br_amd.set import CountList
from oracle import oracle as O

pytestmark = pytest.mark.gpu

TABLE = _lib.COUNT_TABLE
K = 25
TILE = 4096  # k-mer start positions of a work item of the count kernels

_cache = {}


def _oracle(tag, k, reads):
    """(keys, min(255, count) u8, every occurrence's hash) of the reads, computed once per tag and never modified"""
    if tag not in _cache:
        hs = [O.hashes(k, r) for r in reads if len(r) >= k]
        allh = np.concatenate(hs) if hs else np.zeros(0, dtype=np.uint64)
        keys, cnt = np.unique(allh, return_counts=True)
        _cache[tag] = (keys.astype(np.uint64), np.minimum(cnt, 255).astype(np.uint8), allh)
    return _cache[tag]


def _dense(st):
    """the compaction's contract: only full waves walk, but for one last trip per wave"""
    assert st["trips"] <= st["walked"] // 64 + st["waves"], st


def _sliced(cnt, p, P):
    cnt.reset()
    cnt.set_slice(p, P)
    assert cnt.slice == (p if P > 1 else 0, P)
    return cnt


def _saved(obj, min_count=1):
    f = io.BytesIO()
    obj.save(f, min_count)
    return f.getvalue()


def _hot_reads(raw_reads):
    """test_hot_slots_and_loop_trips' mix (tests/test_gpu_count_table.py): whole waves on one slot, many boundaries in a tile"""
    rng = np.random.default_rng(100 + K)
    short = [bytes(rng.choice(list(b"ACGT"), size=int(n)).astype(np.uint8)) for n in rng.integers(0, 60, size=600)]
    return raw_reads[:30] + [b"A" * 9000, b"", b"ACACACACAC" * 700, b"T" * 5000] + short + raw_reads[30:45] + [b"G" * 4100]


# ---- 1. each part's list and file ---------------------------------------------------------------------------------------
def test_part_sizes_on_the_cpu(raw_reads):
    keys, _, _ = _oracle("r150", K, raw_reads[:150])
    n8 = np.bincount(dist.table_owner(keys, 8), minlength=8)
    n64 = np.bincount(dist.table_owner(keys, 64), minlength=64)
    assert (int(n8.min()), int(n8.max())) == (114184, 115004)
    assert (int(n64.min()), int(n64.max())) == (14004, 14632)


@pytest.mark.parametrize("P", [1, 2, 3, 5, 8])
def test_every_part_lists_its_slice(raw_reads, P):
    reads = raw_reads[:150]
    keys, counts, allh = _oracle("r150", K, reads)
    plain = br_amd.Counter(K, 0, TABLE)
    plain.add_reads(reads)
    assert plain.slice == (0, 1) and plain.slice_stats() == {"seen": 0, "walked": 0, "trips": 0, "waves": 0}
    cnt = br_amd.Counter(K, 0, TABLE)
    spec = np.zeros(256, dtype=np.uint64)
    lists = []
    for p in range(P):
        _sliced(cnt, p, P).add_reads(reads)
        sk, sc = parts.slice_of(keys, counts, p, P)
        assert sk.size > 0
        lst = CountList.from_counter(cnt)
        gk, gc = lst.to_numpy()
        assert np.array_equal(gk, sk) and np.array_equal(gc, sc)
        assert _saved(cnt, 1) == keyfile.encode(K, sk, sc, floor=1) == _saved(lst, 1)
        assert _saved(cnt, 3) == keyfile.encode(K, sk[sc >= 3], sc[sc >= 3], floor=3)
        h = cnt.spectrum()
        assert int(h[0]) == 2 ** (2 * K - 1) - sk.size and cnt.table_info()["keys"] == sk.size
        spec[1:] += h[1:]
        st = cnt.slice_stats()
        if P > 1:
            assert st["seen"] == allh.size and st["walked"] == int((dist.table_owner(allh, P) == p).sum()) and st["waves"] > 0
            _dense(st)
        else:
            assert st == {"seen": 0, "walked": 0, "trips": 0, "waves": 0}
        lists.append(lst)
    assert np.array_equal(spec[1:], plain.spectrum()[1:])
    joined = lists[0]
    for lst in lists[1:]:
        joined = joined.maximum(lst)
    assert _saved(joined) == _saved(plain) == keyfile.encode(K, keys, counts, floor=1)


# ---- 2. sizing ----------------------------------------------------------------------------------------------------------
def test_a_slice_sizes_its_table_for_its_share(raw_reads):
    reads = raw_reads[:150]
    _, _, allh = _oracle("r150", K, reads)
    own = dist.table_owner(allh, 8)
    plain = br_amd.Counter(K, 0, TABLE)
    plain.add_reads(reads)
    assert plain.table_info()["log2_lines"] == 20
    cnt = br_amd.Counter(K, 0, TABLE)
    for p in range(8):
        _sliced(cnt, p, 8).add_reads(reads)  # one batch
        occ = int((own == p).sum())
        info = cnt.table_info()
        assert info["log2_lines"] == parts.table_log2_lines(occ) == 17
        assert info["peak_bytes"] == 96 << 17  # (the peak starts again with every slice)
        st = cnt.slice_stats()
        assert st["seen"] == allh.size and st["walked"] == occ
        _dense(st)


# ---- 3. density under small grids ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocks", ["1", "3"])
def test_density_when_a_block_walks_many_tiles(raw_reads, monkeypatch, blocks):
    """BRX_READ_GRID 1: one block takes every tile, so its four queues live through the whole batch and at most four
    partial trips happen in all"""
    monkeypatch.setenv("BRX_READ_GRID", blocks)
    reads = raw_reads[:40]
    keys, counts, allh = _oracle("r40", K, reads)
    cnt = br_amd.Counter(K, 0, TABLE)
    for P in (2, 16):
        for p in (0, P - 1):
            _sliced(cnt, p, P).add_reads(reads)
            st = cnt.slice_stats()
            assert st["waves"] == 4 * int(blocks) and st["seen"] == allh.size
            assert st["walked"] == int((dist.table_owner(allh, P) == p).sum())
            assert st["walked"] // 64 <= st["trips"] <= st["walked"] // 64 + st["waves"]
            _dense(st)
            gk, gc = CountList.from_counter(cnt).to_numpy()
            sk, sc = parts.slice_of(keys, counts, p, P)
            assert np.array_equal(gk, sk) and np.array_equal(gc, sc)


# ---- 4. hard tiles ------------------------------------------------------------------------------------------------------
def _tile_census(k, batch, P):
    """[tiles, P] valid k-mers of every part per 4096-position tile of the batch's concatenated bases"""
    n_tiles = (sum(len(r) for r in batch) + TILE - 1) // TILE
    out = np.zeros((n_tiles, P), dtype=np.int64)
    at = 0
    for r in batch:
        if len(r) >= k:
            h = O.hashes(k, r)
            np.add.at(out, ((at + np.arange(h.size)) // TILE, dist.table_owner(h, P)), 1)
        at += len(r)
    return out


@pytest.mark.parametrize("P", [3, 5])
@pytest.mark.parametrize("blocks", ["1", "3", "7"])
def test_hard_tiles(raw_reads, monkeypatch, P, blocks):
    monkeypatch.setenv("BRX_READ_GRID", blocks)
    reads = _hot_reads(raw_reads)
    keys, counts, allh = _oracle("hot", K, reads)
    batches = (reads[:20], reads[20:])
    census = [_tile_census(K, b, P) for b in batches]
    # a whole tile inside poly-A belongs to one part: the others receive nothing from it, and its owner's queue takes all 4096
    assert any(((c == 0) & (c.sum(axis=1, keepdims=True) >= TILE - K)).any() for c in census)
    homo = dist.table_owner(np.array([O.khash(O.seq2bit(b"A" * K), K)], dtype=np.uint64), P)[0]
    cnt = br_amd.Counter(K, 0, TABLE)
    grew = []
    for p in range(P):
        _sliced(cnt, p, P)
        cnt.add_reads(batches[0])
        small = cnt.table_info()["log2_lines"]
        cnt.add_reads(batches[1])
        grew.append(cnt.table_info()["log2_lines"] > small)
        gk, gc = CountList.from_counter(cnt).to_numpy()
        sk, sc = parts.slice_of(keys, counts, p, P)
        assert np.array_equal(gk, sk) and np.array_equal(gc, sc)
        if p == homo:
            assert 255 in gc
        st = cnt.slice_stats()
        assert st["seen"] == allh.size and st["walked"] == int((dist.table_owner(allh, P) == p).sum())
        _dense(st)
    assert any(grew)  # the second batch regrew a sliced table


# ---- 5. tiny inputs -----------------------------------------------------------------------------------------------------
def test_tiny_inputs(raw_reads):
    one = raw_reads[0][:K]
    owner = int(dist.table_owner(O.hashes(K, one), 5)[0])
    cnt = br_amd.Counter(K, 0, TABLE)
    for p in range(5):
        _sliced(cnt, p, 5).add_reads([one])
        lst = CountList.from_counter(cnt)
        info = cnt.table_info()
        st = cnt.slice_stats()
        assert st["seen"] == 1
        _dense(st)
        gs = cnt.finish(0)
        if p == owner:
            assert lst.n == 1 and info["log2_lines"] == 12 and gs.popcount() == 1 and st["walked"] == 1
            assert bool(gs.get_many(np.array([O.seq2bit(one)], dtype=np.uint64))[0])
        else:
            assert lst.n == 0 and info["log2_lines"] == 0 and info["peak_bytes"] == 0 and st["walked"] == 0
            assert gs.popcount() == 0 and not gs.get_many(np.array([O.seq2bit(one)], dtype=np.uint64))[0]
            assert _saved(lst) == keyfile.encode(K, np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint8), floor=1)
    for p in range(5):  # a read of k - 1 bases holds no k-mer
        _sliced(cnt, p, 5).add_reads([one[:K - 1]])
        assert CountList.from_counter(cnt).n == 0 and cnt.table_info()["log2_lines"] == 0
        assert cnt.slice_stats() == {"seen": 0, "walked": 0, "trips": 0, "waves": 0}
    read = raw_reads[1][:90]
    keys, counts, allh = _oracle("r90", K, [read])
    total = 0
    for p in range(64):
        _sliced(cnt, p, 64).add_reads([read])
        gk, gc = CountList.from_counter(cnt).to_numpy()
        sk, sc = parts.slice_of(keys, counts, p, 64)
        assert np.array_equal(gk, sk) and np.array_equal(gc, sc)
        st = cnt.slice_stats()
        assert st["seen"] == 66 and st["walked"] == sk.size
        _dense(st)
        total += gk.size
    assert total == keys.size == 66


# ---- 6. life cycle and refusals -----------------------------------------------------------------------------------------
def test_life_cycle_and_refusals(raw_reads):
    reads = raw_reads[:6]
    keys, counts, allh = _oracle("r6", K, reads)
    cnt = br_amd.Counter(K, 0, TABLE)
    cnt.add_reads(reads)
    with pytest.raises(_lib.BrxError) as ei:
        cnt.set_slice(0, 2)
    assert ei.value.status == _lib.BRX_ERR_ARG and "k-mers" in str(ei.value) and "reset" in str(ei.value)
    assert cnt.slice == (0, 1)
    for strategy, k in ((_lib.COUNT_DENSE, 9), (_lib.COUNT_SORTED, 19)):
        with pytest.raises(_lib.BrxError) as ei:
            br_amd.Counter(k, 0, strategy).set_slice(0, 2)
        assert ei.value.status == _lib.BRX_ERR_UNSUPPORTED and "BRX_COUNT_TABLE" in str(ei.value)
    cnt.reset()
    for part, n in ((2, 2), (5, 3), (0, 0), (0, 4097)):
        with pytest.raises(_lib.BrxError) as ei:
            cnt.set_slice(part, n)
        assert ei.value.status == _lib.BRX_ERR_ARG
    cnt.set_slice(4095, 4096)
    cnt.set_slice(1, 3)
    with pytest.raises(_lib.BrxError) as ei:
        cnt.load(io.BytesIO(keyfile.encode(K, keys, counts, floor=1)))
    assert ei.value.status == _lib.BRX_ERR_ARG and "slice 1 of 3" in str(ei.value)
    cnt.add_reads(reads)
    sk, sc = parts.slice_of(keys, counts, 1, 3)
    assert cnt.table_info()["keys"] == sk.size
    # lookups: the count of the k-mers the part owns, 0 for the others
    fw = np.array([O.seq2bit(reads[0][i:i + K]) for i in range(0, 600, 3)], dtype=np.uint64)
    fh = np.array([O.khash(int(x), K) for x in fw], dtype=np.uint64)
    want = np.where(dist.table_owner(fh, 3) == 1, counts[np.searchsorted(keys, fh)], 0).astype(np.uint8)
    assert 0 < np.count_nonzero(want) < want.size
    assert np.array_equal(cnt.get_counts(fw), want)
    cnt.reset()  # keeps the slice
    assert cnt.slice == (1, 3) and cnt.slice_stats()["seen"] == 0
    cnt.add_reads(reads)
    gk, gc = CountList.from_counter(cnt).to_numpy()
    assert np.array_equal(gk, sk) and np.array_equal(gc, sc)
    _dense(cnt.slice_stats())
    cnt.reset()
    cnt.set_slice(0, 1)  # an ordinary counter again
    cnt.add_reads(reads)
    assert cnt.slice == (0, 1) and cnt.slice_stats() == {"seen": 0, "walked": 0, "trips": 0, "waves": 0}
    gk, gc = CountList.from_counter(cnt).to_numpy()
    assert np.array_equal(gk, keys) and np.array_equal(gc, counts)
    cnt.load(io.BytesIO(keyfile.encode(K, keys, counts, floor=1)))  # and it loads files again


def test_small_k_against_the_dense_oracle(raw_reads):
    k = 7
    reads = raw_reads[:10] + [b"", b"ACG", b"A" * 300]
    table = O.count_reads(k, reads)
    keys = np.flatnonzero(table).astype(np.uint64)
    counts = table[keys.astype(np.int64)]
    cnt = br_amd.Counter(k, 0, TABLE)
    seen = 0
    for p in range(3):
        _sliced(cnt, p, 3).add_reads(reads)
        gk, gc = CountList.from_counter(cnt).to_numpy()
        sk, sc = parts.slice_of(keys, counts, p, 3)
        assert np.array_equal(gk, sk) and np.array_equal(gc, sc)
        _dense(cnt.slice_stats())
        seen += gk.size
    assert seen == keys.size


# ---- 7. the driver ------------------------------------------------------------------------------------------------------
def _write_fasta(path, reads, gz=False):
    data = b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(reads))
    with open(path, "wb") as f:
        f.write(gzip.compress(data) if gz else data)
    return str(path)


def test_count_in_parts(raw_reads, tmp_path):
    a = _write_fasta(tmp_path / "a.fa", raw_reads[:40])
    b = _write_fasta(tmp_path / "b.fa.gz", raw_reads[40:70], gz=True)
    plain = br_amd.Counter(K, 0, TABLE)
    for path in (a, b):
        with cli.open_input(path) as f:
            plain.count_fasta(f)
    lst, spec, st = parts.count_in_parts([a, b], K, 3)
    assert _saved(lst) == _saved(plain)
    assert np.array_equal(spec, plain.spectrum())
    assert lst.finish(2).fingerprint() == plain.finish(2).fingerprint()
    assert [row["part"] for row in st["parts"]] == [0, 1, 2] and st["trust"] is None
    assert sum(row["keys"] for row in st["parts"]) == lst.n == sum(row["listed"] for row in st["parts"])
    for row in st["parts"]:
        _dense(row["slice_stats"])
        assert row["log2_lines"] < plain.table_info()["log2_lines"]
    lst3, spec3, st3 = parts.count_in_parts([a, b], K, 3, min_count=3)
    assert lst3.floor == 3 and _saved(lst3, 3) == _saved(CountList.from_counter(plain, 3), 3)
    assert np.array_equal(spec3, plain.spectrum())  # complete below the lists' floor too
    assert sum(row["listed"] for row in st3["parts"]) == lst3.n < lst.n


def _qualities(rng, n):
    """Phred+33 of n bases: 25..40, and one base in a hundred or so below any floor of 20"""
    q = rng.integers(25, 41, n)
    q[rng.integers(0, n, max(1, n // 100))] = 5
    return bytes((q + 33).astype(np.uint8))


def test_count_in_parts_fastq(raw_reads, tmp_path):
    rng = np.random.default_rng(5)
    recs = []
    for i, r in enumerate(raw_reads[:20]):
        seq = bytearray(r)
        for j in rng.integers(0, len(seq), 5):
            seq[j] = ord("N")
        q = _qualities(rng, len(seq))
        recs.append(b"@q%d\n%s\n+\n%s\n" % (i, bytes(seq), q))
    path = tmp_path / "x.fq"
    path.write_bytes(b"".join(recs))
    plain = br_amd.Counter(K, 0, TABLE)
    with open(path, "rb") as f:
        ref = plain.count_reads(f, "fastq", 20, True)
    lst, spec, st = parts.count_in_parts([str(path)], K, 4, fmt="fastq", min_quality=20, acgt_only=True)
    assert lst.n > 0 and _saved(lst) == _saved(plain)
    assert np.array_equal(spec, plain.spectrum())
    assert st["trust"] == ref["trust"]
    for row in st["parts"]:
        assert row["slice_stats"]["seen"] == ref["trust"]["kmers"]
        _dense(row["slice_stats"])


# ---- 8. command line ----------------------------------------------------------------------------------------------------
def test_cli_count_parts(raw_reads, tmp_path, capsys):
    """the reads to correct are the first 12 of the 60 that are counted (two files, one gzip): 60 reads are the fewest of
    the fixture whose 25-mer spectrum has a first minimum (2; worked out with the oracle's hashes)"""
    fix = _write_fasta(tmp_path / "fix.fa", raw_reads[:12])
    src = _write_fasta(tmp_path / "in.fa", raw_reads[:35])
    src2 = _write_fasta(tmp_path / "in2.fa.gz", raw_reads[35:60], gz=True)
    p = lambda name: str(tmp_path / name)
    same = lambda x, y: open(p(x), "rb").read() == open(p(y), "rb").read()
    head = ["-i", fix, "-c", "one"]
    assert cli.main(head + ["-o", p("a.out"), "--save-set", p("a.keys"), "fasta", "-i", src, "-i", src2, "-k", "25", "-a", "2"]) == 0
    assert cli.main(head + ["-o", p("b.out"), "--save-set", p("b.keys"), "fasta", "-i", src, "-i", src2, "-k", "25", "-a", "2", "--count-parts", "3"]) == 0
    assert same("a.out", "b.out") and same("a.keys", "b.keys")
    assert cli.main(head + ["-o", p("c.out"), "--save-set", p("c.keys"), "fasta", "-i", src, "-i", src2, "-k", "25", "first-minimum"]) == 0
    assert cli.main(head + ["-o", p("d.out"), "--save-set", p("d.keys"), "fasta", "-i", src, "-i", src2, "-k", "25", "--count-parts", "3",
                            "first-minimum"]) == 0
    assert same("c.out", "d.out") and same("c.keys", "d.keys")
    for n in ("1", "2"):
        tail = ["--save-counts", p("x%s.cnt" % n), "--save-min-count", n, "fasta", "-i", src, "-i", src2, "-k", "25", "-a", "2"]
        assert cli.main(head + ["-o", p("e.out")] + tail) == 0
        tail[1] = p("y%s.cnt" % n)
        assert cli.main(head + ["-o", p("f.out")] + tail + ["--count-parts", "3"]) == 0
        assert same("x%s.cnt" % n, "y%s.cnt" % n) and same("e.out", "f.out") and same("a.out", "f.out")
    with pytest.raises(SystemExit) as ei:
        cli.main(head + ["-o", p("g.out"), "--abundance-report", p("g.tsv"), "fasta", "-i", src, "-i", src2, "-k", "25", "-a", "2", "--count-parts", "3"])
    assert "lists, which answer no lookups" in str(ei.value)
    with pytest.raises(SystemExit) as ei:
        cli.main(head + ["-o", p("g.out"), "fasta", "-i", src, "-i", src2, "-k", "3", "-a", "2", "--count-parts", "3"])
    assert "k from 5 to 31" in str(ei.value)


def test_cli_count_parts_fastq(raw_reads, tmp_path, capsys):
    rng = np.random.default_rng(9)
    src = _write_fasta(tmp_path / "in.fa", raw_reads[:10])
    fq = tmp_path / "x.fq"
    fq.write_bytes(b"".join(b"@q%d\n%s\n+\n%s\n" % (i, r, _qualities(rng, len(r))) for i, r in enumerate(raw_reads[:25])))
    p = lambda name: str(tmp_path / name)
    tail = ["fastq", "-i", str(fq), "-k", "25", "-a", "1", "-q", "20"]
    assert cli.main(["-i", src, "-c", "one", "-o", p("a.out"), "--save-set", p("a.keys")] + tail) == 0
    err_a = capsys.readouterr().err
    assert cli.main(["-i", src, "-c", "one", "-o", p("b.out"), "--save-set", p("b.keys")] + tail + ["--count-parts", "2"]) == 0
    err_b = capsys.readouterr().err
    assert open(p("a.keys"), "rb").read() == open(p("b.keys"), "rb").read()
    assert open(p("a.out"), "rb").read() == open(p("b.out"), "rb").read()
    line = [l for l in err_a.splitlines() if l.startswith("fastq:")]
    assert len(line) == 1 and [l for l in err_b.splitlines() if l.startswith("fastq:")] == line  # the first sweep's totals, once
