"""Lookups in a count list, the numpy statement (br_amd/countops.py: auto_log2_buckets, directory, lookup) and the command
line's --list-lookup flag.  No GPU and no library: every expected value is a loop or a dict."""
import numpy as np
import pytest

from br_amd import cli, countops


def test_auto_log2_buckets():
    k = 21
    assert [countops.auto_log2_buckets(n, k) for n in (0, 1, 16, 17, 32, 33, 64, 65)] == [0, 0, 0, 1, 1, 2, 2, 3]
    for d in range(0, 31):  # the smallest d with 16 * 2^d >= n, on both sides of every power
        assert countops.auto_log2_buckets(16 << d, 31) == d
        assert countops.auto_log2_buckets((16 << d) + 1, 31) == min(d + 1, 30)
    # the caps: 2k-1 where that is smaller, 30 otherwise
    assert countops.auto_log2_buckets(1 << 40, 5) == 9 == countops.max_log2_buckets(5)
    assert countops.auto_log2_buckets(1 << 60, 31) == 30 == countops.max_log2_buckets(31)
    assert countops.auto_log2_buckets(16 << 9, 5) == 9 and countops.auto_log2_buckets((16 << 9) + 1, 5) == 9
    assert countops.max_log2_buckets(15) == 29 and countops.max_log2_buckets(17) == 30


def brute_directory(keys, k, d):
    shift = 2 * k - 1 - d
    return np.array([sum(1 for x in keys if int(x) < (b << shift)) for b in range((1 << d) + 1)], dtype=np.uint64)


@pytest.mark.parametrize("k,d", [(5, 0), (5, 3), (5, 9), (7, 4), (13, 0), (13, 6), (31, 0), (31, 5)])
def test_directory_against_a_loop(k, d):
    rng = np.random.default_rng(100 * k + d)
    top = 1 << (2 * k - 1)
    shift = 2 * k - 1 - d
    lists = {
        "random": np.unique(rng.integers(0, top, 200, dtype=np.uint64)),
        "empty": np.zeros(0, dtype=np.uint64),
        "ends": np.array([0, top - 1], dtype=np.uint64),
        # one full bucket (the last), every other one empty
        "one bucket": np.unique((np.uint64(((1 << d) - 1) << shift) + rng.integers(0, min(1 << shift, 1 << 20), 60, dtype=np.uint64))),
        # the borders themselves and the keys just below them
        "borders": np.unique(np.array([b << shift for b in range(1 << d)] + [(b << shift) - 1 for b in range(1, (1 << d) + 1)],
                                      dtype=np.uint64)),
    }
    for name, keys in lists.items():
        got = countops.directory(keys, k, d)
        assert got.dtype == np.uint64 and got.size == (1 << d) + 1, name
        assert np.array_equal(got, brute_directory(keys, k, d)), name
        assert int(got[0]) == 0 and int(got[-1]) == keys.size, name
        # a bucket holds exactly the keys whose high bits name it
        for b in range(1 << d):
            assert all(int(x) >> shift == b for x in keys[int(got[b]):int(got[b + 1])]), (name, b)
    if d:
        assert (np.diff(countops.directory(lists["one bucket"], k, d).astype(np.int64))[:-1] == 0).all()  # empty buckets
    with pytest.raises(ValueError):
        countops.directory(lists["random"], k, countops.max_log2_buckets(k) + 1)
    with pytest.raises(ValueError):
        countops.directory(np.array([top], dtype=np.uint64), k, d)


def test_lookup_against_a_dict():
    rng = np.random.default_rng(7)
    keys = np.unique(rng.integers(0, 1 << 41, 3000, dtype=np.uint64))
    counts = rng.integers(1, 256, keys.size).astype(np.uint8)
    table = dict(zip(keys.tolist(), counts.tolist()))
    asked = np.concatenate([keys[::3], keys[::5] + np.uint64(1), keys[::7] - np.uint64(1), rng.integers(0, 1 << 41, 500, dtype=np.uint64),
                            np.array([0, (1 << 41) - 1, int(keys[0]), int(keys[-1]), int(keys[-1]) + 1], dtype=np.uint64)])
    got = countops.lookup(keys, counts, asked)
    assert got.dtype == np.uint8 and got.tolist() == [table.get(x, 0) for x in asked.tolist()]
    assert got[:keys[::3].size].all() and not got.all()
    none = countops.lookup(np.zeros(0, np.uint64), np.zeros(0, np.uint8), asked)
    assert none.size == asked.size and not none.any()
    assert countops.lookup(keys, counts, np.zeros(0, np.uint64)).size == 0
    one = countops.lookup(np.array([9], np.uint64), np.array([200], np.uint8), np.array([8, 9, 10], np.uint64))
    assert one.tolist() == [0, 200, 0]


def test_parser_takes_the_flag():
    p = cli.parser()
    a = p.parse_args(["-i", "r.fa", "-o", "c.fa", "--list-lookup", "--abundance-report", "r.tsv", "fasta", "-i", "r.fa", "-k", "25", "-a", "2",
                      "--count-parts", "3"])
    assert a.list_lookup is True and a.count_parts == 3 and a.abundance_report == ["r.tsv"]
    a = p.parse_args(["-i", "r.fa", "--list-lookup", "count", "-i", "a.keys", "-a", "2"])
    assert a.list_lookup is True and getattr(a, "count_ops", None) is None
    assert p.parse_args(["-i", "r.fa", "count", "-i", "a.keys", "-a", "2"]).list_lookup is False
    assert "--list-lookup" in cli.__doc__


def test_refusals_without_the_flag_keep_their_words():
    """the two refusals stand as they were, and each now names the flag"""
    head = ["-i", "r.fa", "-o", "c.fa", "--abundance-report", "r.tsv"]
    with pytest.raises(SystemExit) as ei:
        cli.main(head + ["fasta", "-i", "r.fa", "-k", "25", "-a", "2", "--count-parts", "3"])
    assert "lists, which answer no lookups" in str(ei.value) and "--list-lookup" in str(ei.value)
    with pytest.raises(SystemExit) as ei:
        cli.main(head + ["count", "-i", "a.keys", "--counts-add", "b.keys", "-a", "2"])
    msg = str(ei.value)
    assert "--abundance-report" in msg and "lookups" in msg and "lists, which answer no lookups" in msg and "--list-lookup" in msg


@pytest.mark.parametrize("tail", [["solid", "-i", "s.solid", "-f", "solid"], ["large-kmer", "-i", "r.fa", "-f", "fasta", "-k", "25"],
                                  ["fasta", "-i", "r.fa", "-k", "25", "-a", "2"], ["fastq", "-i", "r.fq", "-k", "25", "-a", "2"]])
def test_flag_where_no_list_is_kept(tail):
    with pytest.raises(SystemExit) as ei:
        cli.main(["-i", "r.fa", "-o", "c.fa", "--list-lookup"] + tail)
    assert "--list-lookup" in str(ei.value) and "list" in str(ei.value).replace("--list-lookup", "")
