"""Set algebra on solid sets: the operations stated in numpy.

A set is its sorted keys (canonical(kmer) >> 1, the bit index the whole project uses; br_amd/keyfile.py), a strictly
increasing uint64 array.  `combine` is the expected value of the GPU path (include/brx.h "set algebra",
br_amd/csrc/brx_setops.hip: brx_keys_combine_device, brx_set_combine), `sizes` that of brx_set_compare -- as cover.py,
abundance.py and keyfile.py are for theirs: no GPU and no library needed.

The oracle's Solid.extend (a set grown by the k-mers of more reads) is a union in this sense: tests/test_setops_cpu.py pins
that on the reference's fixture."""
from __future__ import annotations

from typing import Tuple

import numpy as np

UNION, INTERSECT, DIFFERENCE, SYMDIFF = 0, 1, 2, 3          # BRX_SETOP_*
OPS = {"union": UNION, "intersection": INTERSECT, "difference": DIFFERENCE, "symmetric_difference": SYMDIFF}

# the merge kernel's tile: PER_THREAD consecutive positions of the merged sequence per thread, 256 threads
# (MERGE_PER_THREAD and MERGE_TILE of brx_setops.hip; the tests aim at the edges)
PER_THREAD = 8
TILE = 256 * PER_THREAD


def _keys(a) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.ndim != 1:
        raise ValueError("set algebra: keys are a one-dimensional array")
    if a.size > 1 and not (a[1:] > a[:-1]).all():
        raise ValueError("set algebra: keys must be strictly increasing")
    return a


def op_id(op) -> int:
    """BRX_SETOP_* of a name of OPS or of the number itself"""
    if isinstance(op, str):
        if op not in OPS:
            raise ValueError(f"set algebra: unknown operation {op!r} (one of {sorted(OPS)})")
        return OPS[op]
    if int(op) not in OPS.values():
        raise ValueError(f"set algebra: unknown operation {op!r}")
    return int(op)


def combine(a, b, op) -> np.ndarray:
    """the sorted keys of `a op b`; a and b strictly increasing uint64, op a name of OPS or a BRX_SETOP_* number"""
    a, b, op = _keys(a), _keys(b), op_id(op)
    if op == UNION:
        return np.union1d(a, b)
    in_b = np.isin(a, b, assume_unique=True)
    if op == INTERSECT:
        return a[in_b]
    if op == DIFFERENCE:
        return a[~in_b]
    return np.sort(np.concatenate([a[~in_b], b[~np.isin(b, a, assume_unique=True)]]))


def sizes(a, b) -> Tuple[int, int, int]:
    """(|A|, |B|, |A n B|)"""
    a, b = _keys(a), _keys(b)
    return int(a.size), int(b.size), int(np.isin(a, b, assume_unique=True).sum())


def jaccard(na: int, nb: int, both: int) -> float:
    """|A n B| / |A u B|; two empty sets are equal: 1.0"""
    union = na + nb - both
    return both / union if union else 1.0
