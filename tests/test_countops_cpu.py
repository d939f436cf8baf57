"""Count lists without a GPU: br_amd/countops.py against a dict-based statement, the reference's k = 11 fixture from the
added count lists of two halves of its reads, spectrum, the floor rules, the key-file round trip and the command line's
flags."""
import numpy as np
import pytest

from br_amd import cli, countops, keyfile
from oracle import oracle as O

TOP = (1 << 61) - 1


def by_dict(a, b, op, min_count):
    """`a op b` over {key: count} dicts, written out case by case"""
    out = {}
    for key in set(a) | set(b):
        ca, cb = a.get(key, 0), b.get(key, 0)
        if op == "add":
            r = min(255, ca + cb)
        elif op == "max":
            r = max(ca, cb)
        elif op == "min":
            r = min(ca, cb)
        else:
            r = ca - cb
        if r >= max(1, min_count):
            out[key] = r
    return out


def arrays(d):
    keys = np.array(sorted(d), dtype=np.uint64)
    return keys, np.array([d[int(x)] for x in keys], dtype=np.uint8)


def _operands():
    rng = np.random.default_rng(11)
    yield "both empty", {}, {}
    yield "a empty", {}, {3: 1, 9: 255}
    yield "b empty", {0: 7, TOP: 1}, {}
    # 200 + 100 saturates, 55 + 200 is exactly 255, 9 - 9 is exactly 0, 9 - 10 is negative, 255 - 255 is 0
    yield "edges", {1: 200, 2: 55, 3: 9, 4: 9, 5: 255, 6: 1, TOP: 3}, {1: 100, 2: 200, 3: 9, 4: 10, 5: 255, 7: 1, TOP: 2}
    for i, (na, nb, hi) in enumerate([(300, 200, 600), (2500, 3000, 4000), (400, 400, TOP + 1)]):
        ka = np.unique(rng.integers(0, hi, na, dtype=np.uint64))
        kb = np.unique(rng.integers(0, hi, nb, dtype=np.uint64))
        if hi > 1 << 60:
            kb = np.unique(np.concatenate([kb, ka[::3]]))
        # small counts, so that sub meets 0 and negative values often, and a few large ones, so that add saturates
        ca = np.where(rng.random(ka.size) < 0.1, rng.integers(150, 256, ka.size), rng.integers(1, 5, ka.size))
        cb = np.where(rng.random(kb.size) < 0.1, rng.integers(150, 256, kb.size), rng.integers(1, 5, kb.size))
        yield f"random {i}", dict(zip(ka.tolist(), ca.tolist())), dict(zip(kb.tolist(), cb.tolist()))


@pytest.mark.parametrize("name,a,b", list(_operands()), ids=[c[0] for c in _operands()])
def test_combine_against_dicts(name, a, b):
    (ka, ca), (kb, cb) = arrays(a), arrays(b)
    for op, number in countops.OPS.items():
        for min_count in (1, 2, 255):
            want_k, want_c = arrays(by_dict(a, b, op, min_count))
            for spelled in (op, number):
                got_k, got_c = countops.combine(ka, ca, kb, cb, spelled, min_count)
                assert got_k.dtype == np.uint64 and got_c.dtype == np.uint8
                assert np.array_equal(got_k, want_k) and np.array_equal(got_c, want_c), (name, op, min_count)
        assert all(np.array_equal(x, y) for x, y in zip(countops.combine(ka, ca, kb, cb, op, 0), countops.combine(ka, ca, kb, cb, op, 1)))
    assert countops.sizes((ka, ca), (kb, cb)) == countops.sizes(ka, kb) == (len(a), len(b), len(set(a) & set(b)))
    if name == "edges":
        assert dict(zip(*[x.tolist() for x in countops.combine(ka, ca, kb, cb, "add")]))[1] == 255
        sub = dict(zip(*[x.tolist() for x in countops.combine(ka, ca, kb, cb, "sub")]))
        assert sub == {1: 100, 6: 1, TOP: 1}  # 9 - 9, 9 - 10 and 255 - 255 are gone, the key of B alone never appears


def test_combine_refuses_what_is_no_count_list():
    keys, counts = np.array([1, 2, 3], dtype=np.uint64), np.array([1, 1, 1], dtype=np.uint8)
    for bad_k, bad_c in (([2, 1, 3], [1, 1, 1]), ([1, 1, 3], [1, 1, 1]), ([1, 2, 3], [1, 0, 1]), ([1, 2, 3], [1, 1])):
        with pytest.raises(ValueError):
            countops.combine(np.array(bad_k, dtype=np.uint64), np.array(bad_c, dtype=np.uint8), keys, counts, "add")
        with pytest.raises(ValueError):
            countops.combine(keys, counts, np.array(bad_k, dtype=np.uint64), np.array(bad_c, dtype=np.uint8), "max")
    for op in ("minus", 4, -1):
        with pytest.raises(ValueError):
            countops.combine(keys, counts, keys, counts, op)
    assert sorted(countops.OPS.values()) == [0, 1, 2, 3] and (countops.ADD, countops.MAX, countops.MIN, countops.SUB) == (0, 1, 2, 3)
    assert countops.TILE == 256 * countops.PER_THREAD and countops.PER_THREAD >= 2


def _oracle_list(k, reads):
    table = np.asarray(O.count_reads(k, reads))
    keys = np.flatnonzero(table).astype(np.uint64)
    return keys, table[keys].astype(np.uint8)


def test_added_halves_reproduce_the_reference_fixture(raw_reads, solid_fixture_bytes):
    """the oracle's counts of the two halves of the reads, added as lists and thresholded at 2, are the bits of the
    reference's raw.k11.a2.solid"""
    k = 11
    half = len(raw_reads) // 2
    (ka, ca), (kb, cb) = _oracle_list(k, raw_reads[:half]), _oracle_list(k, raw_reads[half:])
    assert 0 < countops.sizes(ka, kb)[2] < min(ka.size, kb.size)
    keys, counts = countops.combine(ka, ca, kb, cb, "add")
    whole_k, whole_c = _oracle_list(k, raw_reads)
    assert np.array_equal(keys, whole_k) and np.array_equal(counts, whole_c)
    want = np.flatnonzero(np.unpackbits(np.frombuffer(solid_fixture_bytes, dtype=np.uint8)[1:], bitorder="little")).astype(np.uint64)
    assert want.size > 1000 and np.array_equal(countops.select(keys, counts, 2), want)
    assert not np.array_equal(countops.select(ka, ca, 2), want)  # (one half alone is not enough)


def test_spectrum_and_select():
    rng = np.random.default_rng(3)
    counts = rng.integers(1, 256, 5000).astype(np.uint8)
    keys = np.sort(rng.choice(1 << 25, size=5000, replace=False)).astype(np.uint64)
    h = countops.spectrum(13, counts)
    assert h.dtype == np.uint64 and h.shape == (256,)
    assert np.array_equal(h[1:], np.bincount(counts, minlength=256)[1:]) and int(h[0]) == (1 << 25) - 5000
    kept = counts[counts >= 4]
    hf = countops.spectrum(13, kept, floor=4)
    assert not hf[1:4].any() and np.array_equal(hf[4:], h[4:]) and int(hf[0]) == (1 << 25) - kept.size
    with pytest.raises(ValueError):
        countops.spectrum(13, counts, floor=4)
    assert int(countops.spectrum(31, [])[0]) == 1 << 61 and not countops.spectrum(31, [])[1:].any()
    for a in (0, 2, 254, 255):
        assert np.array_equal(countops.select(keys, counts, a), keys[counts.astype(int) > a])
    assert countops.select(keys, counts, 255).size == 0


def test_result_floor_every_combination():
    for fa in (1, 2, 3, 255):
        for fb in (1, 2, 3, 255):
            assert countops.result_floor("max", fa, fb) == countops.result_floor("min", fa, fb) == max(fa, fb)
            if fb == 1:
                assert countops.result_floor("sub", fa, fb) == countops.result_floor(countops.SUB, fa, fb) == fa
            else:
                with pytest.raises(ValueError):
                    countops.result_floor("sub", fa, fb)
            if fa == fb == 1:
                assert countops.result_floor("add", fa, fb) == 1
            else:
                with pytest.raises(ValueError):
                    countops.result_floor("add", fa, fb)
    for bad in ((0, 1), (1, 0), (256, 1)):
        with pytest.raises(ValueError):
            countops.result_floor("max", *bad)
    with pytest.raises(ValueError):
        countops.result_floor("plus", 1, 1)


def test_combined_list_round_trips_through_a_key_file():
    rng = np.random.default_rng(8)
    ka = np.sort(rng.choice(1 << 40, size=3000, replace=False)).astype(np.uint64)
    kb = np.unique(np.concatenate([ka[::4], rng.integers(0, 1 << 40, 2000, dtype=np.uint64)]))
    ca, cb = rng.integers(1, 200, ka.size).astype(np.uint8), rng.integers(1, 200, kb.size).astype(np.uint8)
    for op in countops.OPS:
        for min_count in (1, 3):
            keys, counts = countops.combine(ka, ca, kb, cb, op, min_count)
            assert keys.size > 100
            data = keyfile.encode(21, keys, counts, floor=min_count)
            k, keys2, counts2, floor = keyfile.decode(data)
            assert (k, floor) == (21, min_count) and np.array_equal(keys2, keys) and np.array_equal(counts2, counts)


def test_parser_keeps_the_order_of_the_count_flags():
    p = cli.parser()
    a = p.parse_args(["-i", "r.fa", "-o", "c.fa", "count", "-i", "a.keys", "--counts-add", "b.keys", "--counts-minus", "c.keys.gz",
                      "--counts-min", "d", "--counts-add", "e", "--counts-max", "f", "-a", "2", "--save-counts", "out.keys",
                      "--save-min-count", "3"])
    assert [(op, flag, path) for op, flag, path in a.count_ops] == [
        ("add", "--counts-add", "b.keys"), ("sub", "--counts-minus", "c.keys.gz"), ("min", "--counts-min", "d"), ("add", "--counts-add", "e"),
        ("max", "--counts-max", "f")]
    assert (a.sub_inputs, a.abundance, a.save_counts, a.save_min_count) == ("a.keys", 2, "out.keys", 3)
    # without the flags: nothing to apply, and the flags in front of the sub-command are kept
    b = p.parse_args(["--save-counts", "x.keys", "count", "-i", "a.keys", "-a", "2"])
    assert not b.count_ops and b.save_counts == "x.keys" and b.save_min_count is None
    assert not hasattr(p.parse_args(["solid", "-i", "x", "-f", "solid"]), "count_ops")
    with pytest.raises(SystemExit):  # they belong to `count`
        p.parse_args(["fasta", "-i", "r.fa", "-k", "11", "-a", "2", "--counts-add", "b.keys"])
