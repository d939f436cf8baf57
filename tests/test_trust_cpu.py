"""Trusted stretches, without a GPU: br_amd/trust.py on cases worked by hand, the identities of the statistics, the bound on
the pieces, and the command-line surface of `fastq`, -q, --all-bytes and --skip-non-acgt."""
import numpy as np
import pytest

from br_amd import cli, trust
from br_amd.set import pack_reads


def q(*scores):
    return bytes(33 + s for s in scores)


def test_floor_at_and_below():
    seq = b"ACGTA"
    qual = q(20, 19, 21, 20, 0)
    assert trust.trusted_bits(seq, qual, 20).tolist() == [True, False, True, True, False]
    assert trust.trusted_bits(seq, qual, 0).tolist() == [True] * 5                        # no floor: nothing is asked
    assert trust.trusted_bits(seq, qual, 21).tolist() == [False, False, True, False, False]
    assert trust.trusted_bits(seq, None, 41).tolist() == [True] * 5                        # absent qualities pass any floor
    assert trust.split_read(seq, qual, 20) == [(0, b"A"), (2, b"GT")]
    # a quality byte below 33 fails any floor above 0 and passes none
    low = bytes([32, 10, 0, 33, 34])
    assert trust.trusted_bits(seq, low, 1).tolist() == [False, False, False, False, True]
    assert trust.trusted_bits(seq, low, 0).tolist() == [True] * 5
    # the highest floor: only '~' passes
    assert trust.trusted_bits(b"AC", bytes([125, 126]), 93).tolist() == [False, True]
    for bad in (-1, 94, 255):
        with pytest.raises(ValueError):
            trust.trusted_bits(seq, qual, bad)
    with pytest.raises(ValueError):
        trust.trusted_bits(seq, qual[:4], 5)


def test_letters():
    seq = b"acgtACGTN-RUn@"
    assert trust.letter_bits(seq).tolist() == [True] * 8 + [False] * 6
    assert trust.trusted_bits(seq).tolist() == [True] * 8 + [False] * 6
    assert trust.trusted_bits(seq, acgt_only=False).tolist() == [True] * 14
    assert trust.split_read(seq) == [(0, b"acgtACGT")]
    assert trust.split_read(seq, acgt_only=False) == [(0, seq)]
    # acgt_only off: only the floor bites, and the statistics still tell letters from the rest
    qual = q(*([30] * 8 + [30, 2, 30, 30, 30, 30]))
    assert trust.split_read(seq, qual, 20, acgt_only=False) == [(0, seq[:9]), (10, seq[10:])]
    assert trust.stats_of(seq, qual, 20, acgt_only=False) == (14, 6, 0, 2, 13)
    assert trust.stats_of(seq, qual, 20, acgt_only=True) == (14, 6, 0, 1, 8)


def test_ends_and_min_len():
    seq = b"NACGTNACN"
    assert trust.split_read(seq) == [(1, b"ACGT"), (6, b"AC")]          # untrusted at 0 and at n - 1
    assert trust.split_read(seq, min_len=0) == trust.split_read(seq, min_len=1)   # max(min_len, 1)
    assert trust.split_read(seq, min_len=2) == [(1, b"ACGT"), (6, b"AC")]          # at a stretch's length
    assert trust.split_read(seq, min_len=3) == [(1, b"ACGT")]                      # above the shorter one's
    assert trust.split_read(seq, min_len=4) == [(1, b"ACGT")]
    assert trust.split_read(seq, min_len=5) == []
    assert trust.stats_of(seq, min_len=3) == (9, 3, 0, 1, 4)
    assert trust.split_read(b"") == [] and trust.stats_of(b"") == (0, 0, 0, 0, 0)
    assert trust.split_read(b"NNN") == [] and trust.split_read(b"ACG") == [(0, b"ACG")]
    # low_quality counts letters only: the N with a low quality is non_acgt, not both
    assert trust.stats_of(b"ANAC", q(30, 2, 2, 30), 20) == (4, 1, 1, 2, 2)


def random_batch(seed, n_reads=40):
    rng = np.random.default_rng(seed)
    reads, quals = [], []
    for _ in range(n_reads):
        n = int(rng.integers(0, 200))
        s = rng.choice(np.frombuffer(b"ACGTacgtN-", np.uint8), n, p=[.2, .2, .2, .2, .04, .04, .04, .04, .02, .02])
        reads.append(s.tobytes())
        quals.append(rng.integers(33, 33 + 42, n).astype(np.uint8).tobytes())
    return reads, quals


@pytest.mark.parametrize("min_quality", [0, 2, 20, 41])
@pytest.mark.parametrize("min_len", [1, 11, 100])
def test_identities_and_bound(min_quality, min_len):
    reads, quals = random_batch(min_quality * 1000 + min_len)
    bases, offs = pack_reads(reads)
    qb, _ = pack_reads(quals)
    out, oo, pr, ps, st = trust.split_batch(bases, qb, offs, min_quality, True, min_len)
    lens = np.diff(oo.astype(np.int64))
    n_trusted = np.array([int(np.count_nonzero(trust.trusted_bits(r, qq, min_quality))) for r, qq in zip(reads, quals)])
    assert np.array_equal(n_trusted + st["non_acgt"] + st["low_quality"], st["bases"])      # with acgt_only
    assert np.array_equal(st["bases"], [len(r) for r in reads])
    assert int(st["kept_bases"].sum()) == int(lens.sum()) == out.size
    assert np.array_equal(np.bincount(pr, weights=lens, minlength=len(reads)).astype(np.int64), st["kept_bases"])
    assert np.array_equal(np.bincount(pr, minlength=len(reads)), st["pieces"])
    assert (lens >= max(min_len, 1)).all()
    assert pr.size <= trust.piece_bound(len(reads), bases.size, min_len) and out.size <= bases.size
    assert (np.diff(pr.astype(np.int64)) >= 0).all()                                        # reads in order
    same = np.flatnonzero(np.diff(pr.astype(np.int64)) == 0)
    assert (ps[same + 1] > ps[same]).all()                                                   # stretches in order of their start
    for i in range(pr.size):
        r, s = int(pr[i]), int(ps[i])
        assert out[int(oo[i]):int(oo[i + 1])].tobytes() == reads[r][s:s + int(lens[i])]
    # the k-mers of the pieces at min_len = k are the k-mers of the read that touch no untrusted base
    k = min_len
    if k > 1:
        want = 0
        for r, qq in zip(reads, quals):
            t = trust.trusted_bits(r, qq, min_quality).astype(np.int64)
            if t.size >= k:
                want += int(np.count_nonzero(np.convolve(t, np.ones(k, dtype=np.int64), "valid") == k))
        assert trust.kmers_of_pieces(st, k) == want


def test_everything_trusted_is_the_batch():
    reads, quals = random_batch(7)
    bases, offs = pack_reads(reads)
    qb, _ = pack_reads(quals)
    out, oo, pr, ps, st = trust.split_batch(bases, qb, offs, 0, False, 1)
    kept = [i for i, r in enumerate(reads) if r]
    assert out.tobytes() == bases.tobytes() and pr.tolist() == kept and not ps.any()
    assert np.array_equal(np.diff(oo.astype(np.int64)), [len(reads[i]) for i in kept])


def test_piece_bound_is_tight():
    """alternating stretches of min_len and single untrusted bases reach the bound"""
    for min_len in (1, 3, 11):
        seq = (b"A" * min_len + b"N") * 9 + b"A" * min_len
        pieces = trust.split_read(seq, min_len=min_len)
        assert len(pieces) == 10 == trust.piece_bound(1, len(seq), min_len)


def test_cli_fastq_and_flags():
    p = cli.parser()
    a = p.parse_args(["-i", "r.fa", "-o", "c.fa", "--save-set", "s.keys", "-c", "one", "fastq", "-i", "x.fq.gz", "-i", "y.fq", "-k", "21",
                      "-q", "20", "first-minimum"])
    assert a.subcommand == "fastq" and a.sub_inputs == ["x.fq.gz", "y.fq"] and a.kmer_size == 21
    assert a.min_quality == 20 and not a.all_bytes and a.abundance is None and a.abundance_selection == "first-minimum"
    assert not a.quiet                                              # the top level's -q is another flag
    a = p.parse_args(["-q", "fastq", "-i", "x.fq", "-k", "14", "-a", "2", "--all-bytes"])
    assert a.quiet and a.min_quality == 0 and a.all_bytes and a.abundance == 2 and cli.fasta_kmer_size(a.kmer_size) == 13
    a = p.parse_args(["fastq", "-i", "x.fq", "-k", "11", "-q", "93", "rarefaction", "0.1"])
    assert a.min_quality == 93 and a.percent == 0.1
    for bad in ("94", "-1", "x"):
        with pytest.raises(SystemExit):
            p.parse_args(["fastq", "-i", "x.fq", "-k", "11", "-a", "2", "-q", bad])
    with pytest.raises(SystemExit):
        p.parse_args(["fastq", "-k", "11", "-a", "2"])             # -i is required
    a = p.parse_args(["fasta", "-i", "r.fa", "-k", "11", "-a", "2"])
    assert not a.skip_non_acgt
    a = p.parse_args(["fasta", "-i", "r.fa", "-k", "11", "-a", "2", "--skip-non-acgt"])
    assert a.skip_non_acgt
    a = p.parse_args(["solid", "-i", "r.fq", "-f", "fastq", "-k", "11", "-q", "30", "--skip-non-acgt"])
    assert a.min_quality == 30 and a.skip_non_acgt
    a = p.parse_args(["large-kmer", "-i", "r.fq", "-f", "fastq", "-k", "25"])
    assert a.min_quality == 0 and not a.skip_non_acgt
    a = p.parse_args(["--save-counts", "c.keys", "fastq", "-i", "x.fq", "-k", "11", "-a", "2"])
    assert cli.save_counts_of(a) == "c.keys"                        # `fastq` builds a counter like `fasta`
    with pytest.raises(SystemExit):
        cli.presence_set("x.fa", "fasta", 11, 0, 20, False)        # -q needs qualities
    with pytest.raises(SystemExit):
        cli.presence_set("x.csv", "csv", 11, 0, 0, True)
