"""The owner of a k-mer in the multi-GPU merge of counting tables (include/brx.h brx_exchange_table_owner, the host entry
that shares its one definition with the split kernel) against its numpy statement br_amd.dist.table_owner: equal, inside
the world, and balanced.  No GPU, no communicator.  Reference: no counterpart (one process, src/main.rs:30-33)."""
import ctypes as C

import numpy as np
import pytest

from br_amd import _lib
from br_amd import dist as D

WORLDS = [1, 2, 3, 5, 8, 64]
INPUTS = ["dense", "shifted", "random"]


@pytest.fixture(scope="module")
def inputs():
    low = np.arange(1 << 20, dtype=np.uint64)
    return {"dense": low, "shifted": low << np.uint64(20),
            "random": np.random.default_rng(1).integers(0, 1 << 61, 1 << 20, dtype=np.uint64)}


def _owner_abi(hashes, world):
    out = np.full(hashes.size, 0xFFFFFFFF, dtype=np.uint32)
    st = _lib.lib().brx_exchange_table_owner(hashes.ctypes.data, hashes.size, world, out.ctypes.data)
    return st, out


@pytest.mark.parametrize("name", INPUTS)
@pytest.mark.parametrize("world", WORLDS)
def test_owner_equals_its_numpy_statement(inputs, world, name):
    h = inputs[name]
    st, got = _owner_abi(h, world)
    assert st == 0
    want = D.table_owner(h, world)
    assert want.dtype == np.uint32 and np.array_equal(got, want)
    assert int(got.max()) < world
    # the formula of include/brx.h, in Python integers, on a few of them
    for x in h[:: 1 << 16].tolist() + [int(h[-1])]:
        assert int(want[np.nonzero(h == x)[0][0]]) == ((((x * 0x9E3779B97F4A7C15) % (1 << 64)) >> 32) * world) >> 32


@pytest.mark.parametrize("name", INPUTS)
@pytest.mark.parametrize("world", [2, 3, 8])
def test_owner_shares_are_balanced(inputs, world, name):
    h = inputs[name]
    st, got = _owner_abi(h, world)
    assert st == 0
    share = np.bincount(got, minlength=world) * world / h.size
    print("world %d %s: shares x world in [%.4f, %.4f]" % (world, name, share.min(), share.max()))
    assert share.size == world and share.min() >= 0.99 and share.max() <= 1.01


def test_owner_rejects_bad_arguments():
    h = np.arange(4, dtype=np.uint64)
    st, _ = _owner_abi(h, 0)
    assert st == _lib.BRX_ERR_ARG
    L = _lib.lib()
    out = np.zeros(4, dtype=np.uint32)
    assert L.brx_exchange_table_owner(None, 4, 2, out.ctypes.data) == _lib.BRX_ERR_ARG
    assert L.brx_exchange_table_owner(h.ctypes.data, 4, 2, None) == _lib.BRX_ERR_ARG
    with pytest.raises(ValueError):
        D.table_owner(h, 0)
