"""Set algebra without a GPU: br_amd/setops.py against Python's own set arithmetic, the command-line flags, and "union"
pinned to the oracle's Solid.extend on the reference's fixture."""
import numpy as np
import pytest

from br_amd import cli, setops
from oracle import oracle as O

TOP = (1 << 61) - 1
PY = {"union": set.union, "intersection": set.intersection, "difference": set.difference,
      "symmetric_difference": set.symmetric_difference}


def _arr(values):
    return np.array(sorted(values), dtype=np.uint64)


def _cases():
    rng = np.random.default_rng(7)
    yield "both empty", [], []
    yield "a empty", [], [3, 9]
    yield "b empty", [0, TOP], []
    yield "equal", [1, 5, TOP], [1, 5, TOP]
    yield "disjoint, a below b", range(0, 50), range(50, 90)
    yield "disjoint, interleaved", range(0, 100, 2), range(1, 100, 2)
    yield "b inside a", range(0, 100), range(10, 100, 7)
    yield "a inside b", range(10, 100, 7), range(0, 100)
    yield "ends of the key range", [0, 7, TOP - 1, TOP], [0, 8, TOP]
    for i, (na, nb, hi) in enumerate([(200, 300, 1000), (3000, 2500, 4000), (500, 500, TOP + 1), (1, 4000, 5000)]):
        a = np.unique(rng.integers(0, hi, na, dtype=np.uint64))
        b = np.unique(rng.integers(0, hi, nb, dtype=np.uint64))
        if hi > 1 << 60:  # wide keys meet rarely by chance: share a third of them
            b = np.unique(np.concatenate([b, a[::3]]))
        yield f"random {i}", a.tolist(), b.tolist()


@pytest.mark.parametrize("name,a,b", list(_cases()), ids=[c[0] for c in _cases()])
def test_combine_and_sizes_against_python_sets(name, a, b):
    sa, sb = set(int(x) for x in a), set(int(x) for x in b)
    ka, kb = _arr(sa), _arr(sb)
    for op, number in setops.OPS.items():
        want = _arr(PY[op](sa, sb))
        for spelled in (op, number):
            got = setops.combine(ka, kb, spelled)
            assert got.dtype == np.uint64 and np.array_equal(got, want), (name, op)
    assert setops.sizes(ka, kb) == (len(sa), len(sb), len(sa & sb))
    union = len(sa | sb)
    assert setops.jaccard(*setops.sizes(ka, kb)) == (len(sa & sb) / union if union else 1.0)


def test_combine_refuses_what_is_no_set():
    good = _arr([1, 2, 3])
    for bad in ([2, 1], [1, 1], [[1, 2]]):
        with pytest.raises(ValueError):
            setops.combine(np.array(bad, dtype=np.uint64), good, "union")
        with pytest.raises(ValueError):
            setops.sizes(good, np.array(bad, dtype=np.uint64))
    for op in ("minus", 4, -1):
        with pytest.raises(ValueError):
            setops.combine(good, good, op)
    assert sorted(setops.OPS.values()) == [0, 1, 2, 3]
    assert setops.TILE == 256 * setops.PER_THREAD and setops.PER_THREAD >= 2


def test_parser_keeps_the_order_of_the_set_flags():
    p = cli.parser()
    tail = ["solid", "-i", "x.solid", "-f", "solid"]
    a = p.parse_args(["--set-or", "a.keys", "--set-minus", "b.solid.gz", "-c", "one", "--set-and", "c.keys", "--set-or", "d.keys",
                      "--set-minus", "e"] + tail)
    assert [(op, path) for op, _, path in a.set_ops] == [("union", "a.keys"), ("difference", "b.solid.gz"), ("intersection", "c.keys"),
                                                         ("union", "d.keys"), ("difference", "e")]
    assert [flag for _, flag, _ in a.set_ops] == ["--set-or", "--set-minus", "--set-and", "--set-or", "--set-minus"]
    assert a.corrections == ["one"]
    assert not p.parse_args(tail).set_ops          # no flag: nothing to apply
    assert not p.parse_args(["-c", "one"] + tail).set_ops
    # two parses do not share a list
    b = p.parse_args(["--set-and", "z"] + tail)
    assert [(op, path) for op, _, path in b.set_ops] == [("intersection", "z")]
    with pytest.raises(SystemExit):
        p.parse_args(["--set-or"] + tail[:1])


def test_union_is_the_oracles_extend(raw_reads, solid_fixture_bytes):
    """the reference's k = 11 fixture set extended by the presence set of the first ten reads, Solid.extend, holds exactly
    the bits of the numpy union of the two key lists"""
    k = 11
    fixture = O.Solid.from_bytes(solid_fixture_bytes)
    keys_a = np.flatnonzero(np.unpackbits(np.frombuffer(solid_fixture_bytes, dtype=np.uint8)[1:], bitorder="little")).astype(np.uint64)
    keys_b = np.unique(np.concatenate([O.hashes(k, r) for r in raw_reads[:10]]))
    assert 0 < setops.sizes(keys_a, keys_b)[2] < min(keys_a.size, keys_b.size)  # they overlap, neither holds the other
    fixture.extend(O.Solid.from_count(k, O.count_reads(k, raw_reads[:10]), 0))
    want = np.flatnonzero(np.unpackbits(fixture.bits(), bitorder="little")).astype(np.uint64)
    assert np.array_equal(setops.combine(keys_a, keys_b, "union"), want)
    assert fixture.popcount() == want.size
