"""br_amd/abundance.py -- the numpy statement of k-mer abundance (include/brx.h "abundance") -- against a brute-force
`dict` count of canonical k-mers over the oracle's hashes, the reference's .solid fixture, and the command-line flag.
No GPU."""
import collections

import numpy as np
import pytest

from br_amd import abundance as ab
from br_amd import cli
from oracle import oracle as O


def brute(k, counted, query, abundance):
    """(count[] per query read, stats tuple per query read) one k-mer at a time, from a dict"""
    table = collections.Counter()
    for r in counted:
        table.update(O.hashes(k, r).tolist())
    profiles, stats = [], []
    for r in query:
        c = [min(255, table.get(h, 0)) for h in O.hashes(k, r).tolist()]
        profiles.append(c)
        s = sorted(c)
        stats.append((len(c), c.count(0), sum(v > abundance for v in c), s[0], s[(len(s) - 1) // 2], s[-1], sum(c)) if c
                     else (0,) * 7)
    return profiles, stats


def check(k, counted, query, abundance):
    want_p, want_s = brute(k, counted, query, abundance)
    got = ab.profile_from_hashes([O.hashes(k, r) for r in counted], [O.hashes(k, r) for r in query])
    assert len(got) == len(query)
    for r, g, wp, ws in zip(query, got, want_p, want_s):
        assert g.dtype == np.uint8 and g.tolist() == wp
        assert ab.stats_from_profile(g, abundance) == ws
        h = ab.hist_from_profile(g)
        assert h.dtype == np.uint32 and h.sum() == len(wp) and h[0] == ws[1]
        assert h.tolist() == [wp.count(v) for v in range(256)]
        pb = ab.profile_bytes(g, len(r))
        assert pb.size == len(r) and pb[:len(wp)].tolist() == wp and not pb[len(wp):].any()
    st = ab.stats_array(got, abundance)
    assert st.dtype.itemsize == 32  # brx_abund_stats_t: six u32 and one u64
    assert [tuple(int(v) for v in row) for row in st] == want_s
    return got, want_s


def test_fixture_k11_against_dict(raw_reads):
    k = 11
    got, stats = check(k, raw_reads, raw_reads[:40] + [raw_reads[7][:k - 1], raw_reads[8][:k], b""], 2)
    assert max(s[5] for s in stats) > 40 and any(s[3] == 1 for s in stats)
    # profile_from_hashes without a query profiles the counted reads themselves
    own = ab.profile_from_hashes([O.hashes(k, r) for r in raw_reads[:20]])
    assert all(p.size == len(r) - k + 1 and p.min() >= 1 for p, r in zip(own, raw_reads[:20]))


@pytest.mark.parametrize("k", [5, 15, 25])
def test_random_reads_against_dict(k):
    rng = np.random.default_rng(k)
    genome = rng.choice(list(b"ACGT"), size=600).astype(np.uint8)
    reads = []
    for _ in range(40):
        s = int(rng.integers(0, 500))
        r = genome[s:s + int(rng.integers(30, 120))].copy()
        r[rng.random(r.size) < 0.03] = ord("A")
        reads.append(r.tobytes())
    full = reads[0]
    edge = [full[:k - 1], full[:k], full[:k + 1], b"", full[:40].lower(), full[:20] + b"N" + full[21:60], b"N" * (k + 3), b"n" * (k + 3)]
    got, stats = check(k, reads + edge, reads[:10] + edge + [bytes(rng.choice(list(b"ACGT"), size=80).astype(np.uint8))], 1)
    at = 10
    assert stats[at] == (0,) * 7 and stats[at + 3] == (0,) * 7          # shorter than k, empty
    assert stats[at + 1][0] == 1 and stats[at + 2][0] == 2               # exactly k, k + 1
    assert got[at + 4].size and got[at + 4].tolist() == got[0][:got[at + 4].size].tolist()  # lower case = upper case
    assert got[at + 6].tolist() == got[at + 7].tolist() and got[at + 6].min() >= 2  # N codes like G, n like N
    if k > 5:
        assert stats[-1][1] > 0  # a random read: absent k-mers


@pytest.mark.parametrize("k", [5, 11, 15, 25, 31])
def test_canonical_hashes_equal_the_oracles(raw_reads, k):
    for r in (raw_reads[0][:700], raw_reads[3][:300].lower(), b"ACGTNNNNACGTTTGACCAGGATTACAGGATCCAGGTTACCA", b"ACG"):
        assert np.array_equal(ab.canonical_hashes(r, k), O.hashes(k, r))


def test_median_convention():
    assert ab.stats_from_profile(np.array([], dtype=np.uint8), 0) == (0, 0, 0, 0, 0, 0, 0)       # kmers == 0
    assert ab.stats_from_profile(np.array([7], dtype=np.uint8), 6) == (1, 0, 1, 7, 7, 7, 7)         # kmers == 1
    assert ab.stats_from_profile(np.array([9, 1, 5], dtype=np.uint8), 5)[3:6] == (1, 5, 9)          # odd: the middle
    assert ab.stats_from_profile(np.array([9, 1, 5, 3], dtype=np.uint8), 5)[3:6] == (1, 3, 9)       # even: the LOWER one
    assert ab.stats_from_profile(np.array([0, 0, 4, 4], dtype=np.uint8), 0) == (4, 2, 2, 0, 0, 4, 8)
    assert ab.stats_from_profile(np.array([2, 2], dtype=np.uint8), 2)[2] == 0                        # above is strict


def test_saturation():
    k = 15
    read = b"A" * (k + 299)  # one k-mer, 300 times
    (p,) = ab.profile_from_hashes([O.hashes(k, read)])
    assert p.size == 300 and (p == 255).all()
    assert ab.stats_from_profile(p, 254) == (300, 0, 300, 255, 255, 255, 255 * 300)
    assert ab.stats_from_profile(p, 255)[2] == 0
    assert ab.hist_from_profile(p)[255] == 300


def test_report_line():
    assert ab.REPORT_HEADER == b"#name\tlen\tkmers\tabsent\tabove\tmin\tmedian\tmax\tmean\n"
    assert ab.report_line(b"r1", 40, (30, 2, 25, 0, 7, 19, 200)) == b"r1\t40\t30\t2\t25\t0\t7\t19\t6.667\n"
    assert ab.report_line(b"r2", 9, (0, 0, 0, 0, 0, 0, 0)) == b"r2\t9\t0\t0\t0\t0\t0\t0\t0.000\n"
    assert ab.report_line(b"r3", 12, (2, 0, 2, 1, 1, 2, 3)).endswith(b"\t1.500\n")
    assert ab.report_line(b"r4", 12, (3, 0, 3, 255, 255, 255, 765)).endswith(b"\t255.000\n")
    assert ab.report_line(b"r5", 9, (16, 0, 0, 0, 0, 1, 1)).endswith(b"\t0.063\n")  # 0.0625: half goes up
    st = ab.stats_array([np.array([1, 2, 4], dtype=np.uint8)], 1)
    assert ab.report_line(b"x", 13, st[0]) == b"x\t13\t3\t0\t2\t1\t2\t4\t2.333\n"


def test_pinned_by_the_references_fixture(raw_reads, solid_fixture_bytes):
    """the k-mers with a count above 2 on raw.fasta at k = 11 are exactly the bits of raw.k11.a2.solid"""
    k = 11
    assert solid_fixture_bytes[0] == k
    uniq, cnt = ab.count_table([O.hashes(k, r) for r in raw_reads])
    bits = np.unpackbits(np.frombuffer(solid_fixture_bytes[1:], dtype=np.uint8), bitorder="little")
    assert np.array_equal(np.flatnonzero(bits).astype(np.uint64), uniq[cnt > 2])
    # ... and through the per-position profile: a position's count is above 2 exactly where its k-mer's bit is set
    for r, p in zip(raw_reads[:30], ab.profile_from_hashes([O.hashes(k, r) for r in raw_reads])):
        assert np.array_equal(p > 2, bits[O.hashes(k, r).astype(np.int64)] != 0)


def test_cli_flag():
    p = cli.parser()
    fasta = ["fasta", "-i", "x.fa", "-k", "15", "-a", "2"]
    one = ["-i", "r.fa", "--abundance-report", "a.tsv"]
    assert cli.abundance_reports(p.parse_args(fasta)) is None
    assert cli.abundance_reports(p.parse_args(one + fasta)) == ["a.tsv"]
    a = p.parse_args(["-i", "r.fa", "-i", "s.fa", "-o", "a.fa", "-o", "b.fa", "--abundance-report", "a.tsv", "--abundance-report",
                      "b.tsv"] + fasta)
    assert cli.abundance_reports(a) == ["a.tsv", "b.tsv"]
    assert cli.abundance_reports(p.parse_args(one + ["count", "-i", "t.pcon", "-a", "2"])) == ["a.tsv"]
    with pytest.raises(SystemExit):  # one per output
        cli.abundance_reports(p.parse_args(["-i", "r.fa", "-i", "s.fa", "-o", "a.fa", "-o", "b.fa", "--abundance-report", "a.tsv"] + fasta))
    with pytest.raises(SystemExit):  # the records are read twice: not from stdin
        cli.abundance_reports(p.parse_args(["--abundance-report", "a.tsv"] + fasta))
    for sub in (["solid", "-i", "x.solid", "-f", "solid"], ["large-kmer", "-i", "x.fa", "-f", "fasta", "-k", "25"]):
        with pytest.raises(SystemExit) as ei:  # no counter to ask
            cli.abundance_reports(p.parse_args(one + sub))
        assert ei.value.code not in (0, None) and "counter" in str(ei.value.code)
    assert "--abundance-report" in p.format_help() and "BRX_COUNT_TABLE" in p.format_help()
