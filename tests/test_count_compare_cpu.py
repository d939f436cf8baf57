"""Comparing two count lists without a GPU: countops.joint against a dict loop, its row and column sums against
countops.spectrum, compare_summary on a joint spectrum written by hand with every field worked out here, and the bytes of
compare_report."""
import math

import numpy as np
import pytest

from br_amd import cli, countops

TOP = (1 << 61) - 1


def arrays(d):
    keys = np.array(sorted(d), dtype=np.uint64)
    return keys, np.array([d[int(x)] for x in keys], dtype=np.uint8)


def by_dict(a, b):
    """J over {key: count} dicts, one key at a time"""
    J = np.zeros((256, 256), dtype=np.uint64)
    for key in set(a) | set(b):
        J[a.get(key, 0), b.get(key, 0)] += np.uint64(1)
    return J


def _operands():
    rng = np.random.default_rng(23)
    yield "both empty", {}, {}
    yield "a empty", {}, {3: 1, 9: 255}
    yield "b empty", {0: 7, TOP: 1}, {}
    same = {int(x): int(c) for x, c in zip(rng.choice(5000, 700, replace=False), rng.integers(1, 256, 700))}
    yield "equal lists", same, dict(same)
    yield "equal keys, other counts", same, {x: 1 + (c * 7) % 255 for x, c in same.items()}
    yield "disjoint lists", {2 * x: 1 + x % 9 for x in range(400)}, {2 * x + 1: 1 + x % 5 for x in range(300)}
    yield "counts of 255", {1: 255, 2: 255, 3: 1, TOP: 255}, {2: 255, 3: 255, 4: 255, TOP: 254}
    for n in (50, 3000):
        a = {int(x): int(c) for x, c in zip(rng.choice(4 * n, n, replace=False), rng.integers(1, 256, n))}
        b = {int(x): int(c) for x, c in zip(rng.choice(4 * n, n, replace=False), rng.integers(1, 6, n))}
        yield f"random, {n} keys each", a, b


@pytest.mark.parametrize("name,a,b", list(_operands()), ids=[c[0] for c in _operands()])
def test_joint_against_a_dict_loop(name, a, b):
    J = countops.joint(*arrays(a), *arrays(b))
    want = by_dict(a, b)
    assert J.dtype == np.uint64 and J.shape == (256, 256) and np.array_equal(J, want)
    assert int(J[0, 0]) == 0 and int(J.sum()) == len(set(a) | set(b))
    if name == "equal lists":
        assert np.array_equal(J, np.diag(np.diag(J))) and int(J.sum()) == len(a)
    if name == "disjoint lists":
        assert not J[1:, 1:].any() and int(J[1:, 0].sum()) == len(a) and int(J[0, 1:].sum()) == len(b)
    if name == "counts of 255":
        assert (int(J[255, 0]), int(J[255, 255]), int(J[1, 255]), int(J[0, 255]), int(J[255, 254])) == (1, 1, 1, 1, 1)
    # with J[0][0] filled in as brx_counts_compare does, the margins are the two spectra
    k = 31
    J[0, 0] = (1 << (2 * k - 1)) - len(set(a) | set(b))
    assert np.array_equal(J.sum(axis=1), countops.spectrum(k, arrays(a)[1]))
    assert np.array_equal(J.sum(axis=0), countops.spectrum(k, arrays(b)[1]))


def test_joint_refuses_what_is_no_list():
    with pytest.raises(ValueError):
        countops.joint([3, 2], [1, 1], [], [])
    with pytest.raises(ValueError):
        countops.joint([], [], [1, 2], [1, 0])
    with pytest.raises(ValueError):
        countops.compare_summary(np.zeros((256, 255), np.uint64), 5)
    with pytest.raises(ValueError):
        countops.compare_summary(np.zeros((256, 256), np.uint64), 5, min_a=0)


def hand_joint():
    """ten k-mers once in A alone, two three times in A alone, four once in B alone, three (1, 2), five (2, 3) and one
    saturated in both"""
    J = np.zeros((256, 256), dtype=np.uint64)
    for (ca, cb), n in {(1, 0): 10, (3, 0): 2, (0, 1): 4, (1, 2): 3, (2, 3): 5, (255, 255): 1}.items():
        J[ca, cb] = n
    return J


def test_summary_of_a_hand_written_joint():
    J = hand_joint()
    s = countops.compare_summary(J, 5)
    assert (s["a"], s["b"], s["both"], s["either"]) == (10 + 2 + 3 + 5 + 1, 4 + 3 + 5 + 1, 3 + 5 + 1, 25)
    assert s["jaccard"] == 9 / 25
    assert (s["a_solid"], s["b_solid"], s["both_solid"]) == (21, 13, 9) and s["completeness"] == 9 / 13
    assert (s["a_occ"], s["a_only_occ"]) == (10 * 1 + 2 * 3 + 3 * 1 + 5 * 2 + 255, 10 * 1 + 2 * 3) == (284, 16)
    assert s["error_rate"] == 1 - (1 - 16 / 284) ** (1 / 5) and s["qv"] == -10 * math.log10(s["error_rate"])
    assert abs(s["error_rate"] - 0.011530460314958) < 1e-13 and abs(s["qv"] - 19.3815335460852) < 1e-9
    assert all(type(s[name]) is int for name in countops.SUMMARY_INTS)
    # J[0][0] is never read
    J2 = J.copy()
    J2[0, 0] = (1 << 9) - 25
    assert countops.compare_summary(J2, 5) == s
    # thresholds above 1: A from 2 up is (3, 0), (2, 3), (255, 255); B from 3 up is (2, 3), (255, 255)
    s = countops.compare_summary(J, 5, min_a=2, min_b=3)
    assert (s["a"], s["b"], s["both"], s["either"], s["jaccard"]) == (21, 13, 9, 25, 9 / 25)
    assert (s["a_solid"], s["b_solid"], s["both_solid"], s["completeness"]) == (2 + 5 + 1, 5 + 1, 5 + 1, 1.0)
    assert (s["a_occ"], s["a_only_occ"]) == (2 * 3 + 5 * 2 + 255, 2 * 3) == (271, 6)
    assert s["error_rate"] == 1 - (1 - 6 / 271) ** (1 / 5) and abs(s["qv"] - 23.499073859152) < 1e-9
    # min_b = 3 takes the (1, 2) k-mers' vouching away, min_a = 1 keeps them in A
    s = countops.compare_summary(J, 5, min_a=1, min_b=3)
    assert (s["a_solid"], s["both_solid"], s["a_occ"], s["a_only_occ"]) == (21, 6, 284, 10 + 6 + 3)
    # nothing of A at 256
    s = countops.compare_summary(J, 5, min_a=256)
    assert (s["a_solid"], s["both_solid"], s["a_occ"], s["completeness"]) == (0, 0, 0, 0.0) and math.isnan(s["qv"])


def test_summary_edges():
    J = np.zeros((256, 256), dtype=np.uint64)
    s = countops.compare_summary(J, 25)  # two empty lists
    assert (s["a"], s["b"], s["both"], s["either"], s["jaccard"]) == (0, 0, 0, 0, 0.0)
    assert math.isnan(s["completeness"]) and math.isnan(s["error_rate"]) and math.isnan(s["qv"])
    J[0, 1] = 4  # an empty A
    s = countops.compare_summary(J, 25)
    assert (s["a"], s["b"], s["either"], s["jaccard"], s["completeness"], s["a_occ"]) == (0, 4, 4, 0.0, 0.0, 0)
    assert math.isnan(s["error_rate"]) and math.isnan(s["qv"])
    J[2, 3] = 5  # every k-mer of A vouched for
    s = countops.compare_summary(J, 25)
    assert (s["a"], s["both"], s["a_occ"], s["a_only_occ"]) == (5, 5, 10, 0)
    assert s["error_rate"] == 0.0 and s["qv"] == math.inf and s["jaccard"] == 5 / 9 and s["completeness"] == 5 / 9
    J[:] = 0
    J[7, 0] = 3  # an empty B: nothing vouched for
    s = countops.compare_summary(J, 25)
    assert (s["a_occ"], s["a_only_occ"], s["error_rate"], s["qv"]) == (21, 21, 1.0, 0.0) and math.isnan(s["completeness"])
    assert str(s["qv"]) == "0.0"
    # bins whose sum passes 2^64 are summed exactly
    J[:] = 0
    J[200, 1:17] = 1 << 60
    s = countops.compare_summary(J, 31)
    assert s["a"] == s["both"] == 1 << 64 and s["a_occ"] == 200 << 64 and s["qv"] == math.inf


REPORT = (b"#k\t5\n#floor_a\t1\n#floor_b\t3\n#min_a\t2\n#min_b\t3\n"
          b"#a\t21\n#b\t13\n#both\t9\n#either\t25\n#a_solid\t8\n#b_solid\t6\n#both_solid\t6\n#a_occ\t271\n#a_only_occ\t6\n"
          b"#jaccard\t0.360000\n#completeness\t1.000000\n#error_rate\t0.004467789\n#qv\t23.499\n"
          b"#ca\tcb\tkmers\n"
          b"0\t1\t4\n1\t0\t10\n1\t2\t3\n2\t3\t5\n3\t0\t2\n255\t255\t1\n")


def test_report_bytes():
    J = hand_joint()
    assert countops.compare_report(5, 1, 3, J, min_a=2, min_b=3) == REPORT
    J[0, 0] = 487  # [0][0] is not a line
    assert countops.compare_report(5, 1, 3, J, min_a=2, min_b=3) == REPORT
    head = countops.compare_report(5, 1, 1, hand_joint()).split(b"#ca\t")[0]
    assert b"#jaccard\t0.360000\n#completeness\t0.692308\n#error_rate\t0.011530460\n#qv\t19.382\n" in head
    # inf and nan by name; halves go up
    J = np.zeros((256, 256), dtype=np.uint64)
    J[2, 3], J[0, 1] = 5, 3
    rep = countops.compare_report(25, 1, 1, J)
    assert b"#jaccard\t0.625000\n" in rep and b"#error_rate\t0.000000000\n#qv\tinf\n" in rep and rep.endswith(b"#ca\tcb\tkmers\n0\t1\t3\n2\t3\t5\n")
    rep = countops.compare_report(25, 1, 1, np.zeros((256, 256), dtype=np.uint64))
    assert b"#jaccard\t0.000000\n#completeness\tnan\n#error_rate\tnan\n#qv\tnan\n" in rep and rep.endswith(b"#ca\tcb\tkmers\n")
    assert countops._fixed(0.0625, 3) == b"0.063" and countops._fixed(0.125, 2) == b"0.13" and countops._fixed(2.5, 0) == b"3"


def test_cli_flags_need_each_other():
    common = ["-i", "reads.fa", "-o", "out.fa", "count", "-i", "a.keys", "-a", "1"]
    for given, missing in (("--counts-compare", "--compare-report"), ("--compare-report", "--counts-compare")):
        with pytest.raises(SystemExit) as ei:
            cli.main(common + [given, "x"])
        assert str(ei.value).startswith("Error: ") and f"{given} was given without {missing}" in str(ei.value)
    args = cli.parser().parse_args(common + ["--counts-compare", "c.keys", "--compare-report", "r.tsv"])
    assert (args.counts_compare, args.compare_report) == ("c.keys", "r.tsv") and cli.compare_of(args)
    assert not cli.compare_of(cli.parser().parse_args(common))
