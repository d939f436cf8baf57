"""Counting in parts, the rules in numpy (br_amd/parts.py): which part owns a k-mer, how the parts' lists join, how a
sliced table is sized.  No GPU and no library."""
import numpy as np
import pytest

from br_amd import countops, dist, parts


def _random_list(rng, n, k=25):
    keys = np.unique(rng.integers(0, 1 << (2 * k - 1), n, dtype=np.uint64))
    return keys, rng.integers(1, 256, keys.size).astype(np.uint8)


@pytest.mark.parametrize("P", [1, 2, 3, 5, 8, 64, 4096])
def test_slices_partition_and_join_back(P):
    rng = np.random.default_rng(P)
    keys, counts = _random_list(rng, 20000)
    slices = [parts.slice_of(keys, counts, p, P) for p in range(P)]
    assert sum(s[0].size for s in slices) == keys.size
    own = dist.table_owner(keys, P)
    for p, (sk, sc) in enumerate(slices):
        assert np.array_equal(sk, keys[own == p]) and np.array_equal(sc, counts[own == p])
        assert sk.size < 2 or (sk[1:] > sk[:-1]).all()  # a slice keeps the list's order
    if P <= 8:
        assert min(s[0].size for s in slices) > 0
    jk, jc = parts.join(slices[::-1])  # in any order
    assert np.array_equal(jk, keys) and np.array_equal(jc, counts)
    assert jk.dtype == np.uint64 and jc.dtype == np.uint8


def test_join_refuses_a_shared_key():
    rng = np.random.default_rng(7)
    keys, counts = _random_list(rng, 500)
    a = parts.slice_of(keys, counts, 0, 2)
    b = parts.slice_of(keys, counts, 1, 2)
    b = (np.sort(np.append(b[0], a[0][3])), np.append(b[1], np.uint8(9)))
    with pytest.raises(ValueError, match="share the key %d" % int(a[0][3])):
        parts.join([a, b])
    jk, jc = parts.join([])
    assert jk.size == 0 and jc.size == 0
    with pytest.raises(ValueError):
        parts.slice_of(keys, counts, 2, 2)
    for bad in (0, 4097):
        with pytest.raises(ValueError):
            parts.slice_of(keys, counts, 0, bad)


def test_command_line_flag():
    from br_amd import cli
    head = ["-i", "r.fa", "-o", "c.fa"]
    for sub in (["fasta"], ["fastq", "-q", "20"]):
        args = cli.parser().parse_args(head + sub + ["-i", "r", "-k", "25", "-a", "2", "--count-parts", "4096"])
        assert args.count_parts == 4096
        assert cli.parser().parse_args(head + sub + ["-i", "r", "-k", "25", "-a", "2"]).count_parts is None
        for bad in ("0", "4097", "-1", "x"):
            with pytest.raises(SystemExit):
                cli.parser().parse_args(head + sub + ["-i", "r", "-k", "25", "-a", "2", "--count-parts", bad])
    assert "only solid k-mers are ever kept between sweeps" in cli.COUNT_PARTS_HELP
    with pytest.raises(SystemExit):  # the other sub-commands do not take it
        cli.parser().parse_args(head + ["count", "-i", "t", "-a", "2", "--count-parts", "2"])
    for k in (4, 32):
        with pytest.raises(ValueError):
            parts.count_in_parts(["r.fa"], k, 2)
    with pytest.raises(ValueError):
        parts.count_in_parts(["r.fa"], 25, 0)


def test_table_log2_lines_by_hand():
    """7 * 2^L slots against 3 * need: 2^12 lines hold 28672 slots, so up to 9557 keys (3 * 9557 = 28671); one more key
    doubles the table"""
    assert parts.table_log2_lines(0) == 12
    assert parts.table_log2_lines(1) == 12
    assert (1 << 12) * 7 // 3 == 9557
    assert parts.table_log2_lines(9557) == 12
    assert parts.table_log2_lines(9558) == 13
    step = (7 << 17) // 3  # 305834: the most keys of 2^17 lines
    assert step == 305834
    assert parts.table_log2_lines(step - 1) == 17
    assert parts.table_log2_lines(step) == 17
    assert parts.table_log2_lines(step + 1) == 18
    assert parts.table_log2_lines(1 << 62) == 30  # the largest table; the library refuses what does not fit it


@pytest.mark.parametrize("floors", [[1], [1, 1, 1], [3, 3, 3, 3, 3], [2, 5, 3], [255, 1]])
def test_floor_of_a_join_is_the_max_rule(floors):
    rng = np.random.default_rng(len(floors))
    keys, counts = _random_list(rng, 4000)
    P = len(floors)
    lists = []
    for p, f in enumerate(floors):
        sk, sc = parts.slice_of(keys, counts, p, P)
        lists.append((sk[sc >= f], sc[sc >= f]))
    want = floors[0]
    for f in floors[1:]:
        want = countops.result_floor("max", want, f)
    assert parts.join_floor(floors) == want == max(floors)
    # disjoint keys: the join is what folding countops' max over the lists gives
    jk, jc = parts.join(lists)
    fk, fc = lists[0]
    for sk, sc in lists[1:]:
        fk, fc = countops.combine(fk, fc, sk, sc, "max")
    assert np.array_equal(jk, fk) and np.array_equal(jc, fc)
    # and from its floor up the joined list is exact
    top = want
    assert np.array_equal(jk[jc >= top], keys[counts >= top]) and np.array_equal(jc[jc >= top], counts[counts >= top])
