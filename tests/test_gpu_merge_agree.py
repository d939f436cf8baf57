"""Set algebra, the count merge and the joint spectrum are one merge (br_amd/csrc/brx_setops.hip tile_walk): over lists whose
every count byte is 1 the three raw entries -- brx_keys_combine_device, brx_counts_combine_device with min_count 1 and
brx_counts_joint_device -- must tell the same story about the same keys, and numpy's.  Every comparison is exact."""
import numpy as np
import pytest

from br_amd import countops
from tests.test_gpu_count_compare import run_joint
from tests.test_gpu_countops import _sample, _shape_cases, run_raw as run_counts, u64
from tests.test_gpu_setops import run_raw as run_keys

pytestmark = pytest.mark.gpu

TILE = countops.TILE


def _cases():
    yield from _shape_cases()
    for total in (TILE + 1, 3 * TILE + 5):
        rng = np.random.default_rng(total)
        yield f"sample of {total}, half and half", _sample(rng, total // 2, 2 * total), _sample(rng, total - total // 2, 2 * total)


@pytest.mark.parametrize("name,a,b", list(_cases()), ids=[c[0] for c in _cases()])
def test_three_consumers_tell_one_story(name, a, b):
    a, b = u64(a), u64(b)
    A, B = (a, np.ones(a.size, np.uint8)), (b, np.ones(b.size, np.uint8))
    union, inter, diff = np.union1d(a, b), np.intersect1d(a, b), np.setdiff1d(a, b)
    s3 = (a.size, b.size, inter.size)
    # each side against numpy
    keys = {}
    for op, want in (("union", union), ("intersection", inter), ("difference", diff)):
        keys[op], got_s3, _ = run_keys(a, b, op)
        assert got_s3 == s3 and np.array_equal(keys[op], want), (name, op)
    counted = {}
    for op, want in (("add", union), ("max", union), ("min", inter), ("sub", diff)):
        got_k, got_c, got_s3, _, _ = run_counts(A, B, op, 1)
        assert got_s3 == s3 and np.array_equal(got_k, want), (name, op)
        counted[op] = (got_k, got_c)
    J, got_s3 = run_joint(A, B)
    assert got_s3 == s3, name
    # the sides against each other
    assert np.array_equal(keys["union"], counted["add"][0]) and np.array_equal(keys["union"], counted["max"][0]), name
    assert np.array_equal(keys["intersection"], counted["min"][0]), name
    assert np.array_equal(keys["difference"], counted["sub"][0]), name  # (every pair subtracts to 0 and is dropped)
    assert (counted["min"][1] == 1).all() and (counted["max"][1] == 1).all() and (counted["sub"][1] == 1).all(), name
    assert np.array_equal(counted["add"][1], 1 + np.isin(counted["add"][0], keys["intersection"]).astype(np.uint8)), name
    assert int(J.sum()) == keys["union"].size and int(J[1, 1]) == keys["intersection"].size, name
    assert int(J[1, 0]) == keys["difference"].size and int(J[0, 1]) == b.size - inter.size == np.setdiff1d(b, a).size, name
    rest = J.copy()
    rest[:2, :2] = 0
    assert int(J[0, 0]) == 0 and not rest.any(), name
