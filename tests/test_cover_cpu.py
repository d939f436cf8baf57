"""br_amd/cover.py -- the numpy statement of solid coverage (include/brx.h "coverage") -- against a brute-force loop over
the definitions and against the oracle's `Solid.mask`, and the command-line flags of the output forms.  No GPU."""
import numpy as np
import pytest

from br_amd import cli, cover
from oracle import oracle as O


def oracle_solid(ref, read):
    n = max(len(read) - ref.k + 1, 0)
    return np.unpackbits(ref.mask(read), bitorder="little")[:n].astype(bool)


def brute(ref, read):
    """(solid, covered, runs as (start, end)) straight from the definitions, one k-mer and one base at a time"""
    k, n = ref.k, len(read)
    solid = [ref.get(O.seq2bit(read[i:i + k])) for i in range(max(n - k + 1, 0))]
    covered = [any(solid[i] for i in range(max(j - k + 1, 0), min(j, n - k) + 1)) for j in range(n)]
    runs, j = [], 0
    while j < n:
        if covered[j]:
            s = j
            while j < n and covered[j]:
                j += 1
            runs.append((s, j))
        else:
            j += 1
    return solid, covered, runs


@pytest.fixture(scope="module")
def ref(solid_fixture_bytes):
    return O.Solid.from_bytes(solid_fixture_bytes)


def test_against_brute_force(raw_reads, ref):
    k = ref.k
    sample = [raw_reads[0][:3000], raw_reads[5][100:1500], raw_reads[17][:700].lower(), raw_reads[3][:40]]
    for read in sample:
        solid, covered, runs = brute(ref, read)
        assert oracle_solid(ref, read).tolist() == solid
        cov = cover.covered_from_solid(np.array(solid, dtype=bool), len(read), k)
        assert cov.tolist() == covered
        assert cover.runs_of(cov) == runs
        assert all(e - s >= k for s, e in runs)
        fl = cover.flags_from_solid(np.array(solid, dtype=bool), len(read), k)
        assert ((fl & cover.SOLID_START) != 0)[:len(solid)].tolist() == solid
        assert not (fl[len(solid):] & cover.SOLID_START).any()
        assert cover.stats_from_flags(fl, k) == (len(solid), sum(solid), sum(covered), len(runs))
        masked = cover.mask_read(read, cov)
        for j, (a, b) in enumerate(zip(read, masked)):
            assert b == (a & 0xDF if covered[j] else a | 0x20)
        assert [p for _, p in cover.split_read(read, cov, 0)] == [read[s:e] for s, e in runs]
        assert [p for _, p in cover.split_read(read, cov, 100)] == [read[s:e] for s, e in runs if e - s >= 100]


def test_kmers_of_matches_seq2bit():
    read = b"ACGTNacgtnTTGACCAGGATTACA"
    for k in (1, 5, 11, 21):
        assert cover.kmers_of(read, k).tolist() == [O.seq2bit(read[i:i + k]) for i in range(len(read) - k + 1)]
    assert cover.kmers_of(b"ACG", 5).size == 0


def test_fixture_totals_before_and_after_one(raw_reads, ref):
    """what the oracle gives on the fixture, all 206 reads, k = 11"""
    k = ref.k

    def totals(reads):
        t = np.zeros(4, dtype=np.int64)
        for r in reads:
            t += cover.stats_from_flags(cover.flags_from_solid(oracle_solid(ref, r), len(r), k), k)
        return t.tolist()

    assert len(raw_reads) == 206
    assert totals(raw_reads) == [2_517_532, 1_883_972, 2_424_946, 17_836]
    om = O.build_methods(ref, ["one"], 5, 7)
    corrected = [O.correct_record(om, r, False) for r in raw_reads]  # forward and reverse pass
    assert sum(len(r) for r in corrected) == 2_520_330
    assert totals(corrected)[1:] == [2_061_179, 2_440_124, 13_612]


def _one_solid(n, k, at):
    s = np.zeros(max(n - k + 1, 0), dtype=bool)
    for i in at:
        s[i] = True
    return s


def test_edge_cases(ref):
    k = 11
    # empty read, n = k-1: no k-mers, nothing covered, nothing comes out
    for read in (b"", b"ACGTACGTAC"):
        fl = cover.flags_from_solid(np.zeros(0, dtype=bool), len(read), k)
        assert fl.size == len(read) and not fl.any()
        assert cover.stats_from_flags(fl, k) == (0, 0, 0, 0)
        assert cover.mask_read(read, fl != 0) == read.lower()
        assert cover.split_read(read, fl != 0, 0) == []
    # n = k and n = k+1 with their k-mers solid or not
    assert cover.flags_from_solid(_one_solid(k, k, [0]), k, k).tolist() == [3] + [2] * (k - 1)
    assert not cover.flags_from_solid(_one_solid(k, k, []), k, k).any()
    assert cover.flags_from_solid(_one_solid(k + 1, k, [1]), k + 1, k).tolist() == [0, 3] + [2] * (k - 1)
    assert cover.flags_from_solid(_one_solid(k + 1, k, [0, 1]), k + 1, k).tolist() == [3, 3] + [2] * (k - 1)
    # a single solid k-mer at either end of a longer read
    n = 50
    first = cover.flags_from_solid(_one_solid(n, k, [0]), n, k)
    last = cover.flags_from_solid(_one_solid(n, k, [n - k]), n, k)
    assert cover.runs_of(first & 2) == [(0, k)] and cover.runs_of(last & 2) == [(n - k, n)]
    assert cover.stats_from_flags(first, k) == cover.stats_from_flags(last, k) == (n - k + 1, 1, k, 1)
    # a read of Ns is a read of the base coded (ord('N') >> 1) & 3 = 3, like any other
    ns = b"N" * 30
    assert oracle_solid(ref, ns).tolist() == [ref.get(O.seq2bit(b"G" * k))] * 20
    assert cover.kmers_of(ns, k).tolist() == [O.seq2bit(b"G" * k)] * 20


def test_masking(raw_reads, ref):
    k = ref.k
    read = raw_reads[2][:5000]
    cov = cover.covered_from_solid(oracle_solid(ref, read), len(read), k)
    assert cov.any() and not cov.all()
    masked = cover.mask_read(read, cov)
    assert masked.upper() == read.upper() and masked != read
    # lower-case input has the same k-mers, hence the same flags and the same masked form
    assert np.array_equal(oracle_solid(ref, read.lower()), oracle_solid(ref, read))
    assert cover.mask_read(read.lower(), cov) == masked
    # idempotent; covering a masked read again gives the same flags
    assert cover.mask_read(masked, cov) == masked
    assert np.array_equal(cover.flags_from_solid(oracle_solid(ref, masked), len(read), k),
                          cover.flags_from_solid(oracle_solid(ref, read), len(read), k))
    # bytes that are not letters stay
    assert cover.mask_read(b"AC-*t1", np.array([1, 0, 1, 0, 1, 0], dtype=bool)) == b"Ac-*T1"


def test_split_and_piece_names(raw_reads, ref):
    k = ref.k
    read = raw_reads[2][:5000]
    cov = cover.covered_from_solid(oracle_solid(ref, read), len(read), k)
    pieces = cover.split_read(read, cov, 0)
    assert len(pieces) > 1
    # the pieces of min_len = 0 concatenate to exactly the covered bases
    assert b"".join(p for _, p in pieces) == bytes(np.frombuffer(read, dtype=np.uint8)[cov])
    assert all(read[s:s + len(p)] == p for s, p in pieces)
    assert [s for s, _ in pieces] == sorted(s for s, _ in pieces)
    longest = max(len(p) for _, p in pieces)
    assert cover.split_read(read, cov, longest + 1) == []
    assert [len(p) for _, p in cover.split_read(read, cov, longest)] == [longest] * sum(len(p) == longest for _, p in pieces)
    # names: piece i, counted over the pieces emitted, of `name [description]` is `name_i [description]`
    assert cover.piece_name(b"read7", 1) == b"read7_1"
    assert cover.piece_name(b"read7 some words here", 12) == b"read7_12 some words here"
    recs = cover.split_record(b"r1 d e", read, cov, 100)
    assert [h for h, _ in recs] == [b"r1_%d d e" % (i + 1) for i in range(len(recs))]
    assert [p for _, p in recs] == [p for _, p in pieces if len(p) >= 100]


def test_cli_flags():
    base = ["solid", "-i", "x.solid", "-f", "solid"]
    p = cli.parser()
    a = p.parse_args(base)
    assert cli.output_form(a) == ("plain", 0, None)
    assert cli.output_form(p.parse_args(["--mask-weak"] + base)) == ("mask", 0, None)
    assert cli.output_form(p.parse_args(["--trim-split", "-s"] + base)) == ("split", 0, None)
    assert cli.output_form(p.parse_args(["--trim-split", "250"] + base)) == ("split", 250, None)
    assert cli.output_form(p.parse_args(["--trim-split=0", "--cover-report", "r.tsv"] + base)) == ("split", 0, ["r.tsv"])
    a = p.parse_args(["-o", "a.fa", "-o", "b.fa", "--cover-report", "a.tsv", "--cover-report", "b.tsv", "--mask-weak"] + base)
    assert cli.output_form(a) == ("mask", 0, ["a.tsv", "b.tsv"])
    # the two forms exclude each other
    with pytest.raises(SystemExit):
        p.parse_args(["--mask-weak", "--trim-split", "100"] + base)
    with pytest.raises(SystemExit):
        p.parse_args(["--trim-split", "-3"] + base)
    # one report per output
    with pytest.raises(SystemExit):
        cli.output_form(p.parse_args(["-o", "a.fa", "-o", "b.fa", "--cover-report", "a.tsv"] + base))
    with pytest.raises(SystemExit):
        cli.output_form(p.parse_args(["--cover-report", "a.tsv", "--cover-report", "b.tsv"] + base))
