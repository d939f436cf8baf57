"""Count lists: add, max, min and subtract of sorted (key, count) lists, thresholds and spectra -- stated in numpy.

A count list is the content of a count file (br_amd/keyfile.py): `keys`, a strictly increasing uint64 array of bit indices
(canonical(kmer) >> 1), and `counts`, one uint8 per key, every count >= 1.  With ca, cb the counts of a key in A and in B (0
when it is absent):

    add   0   min(255, ca + cb)   every key of either list
    max   1   max(ca, cb)         every key of either list
    min   2   min(ca, cb)         the keys of both
    sub   3   ca - cb             the keys with ca > cb; a key of B alone never appears

After the operation a key is dropped when its result lies below `min_count` (0 means 1).  Counts are bytes as they are: 255
means "255 or more", so `sub` from or by a saturated count is a bound, not a value (255 - 5 = 250 says "at least 250"; 255 -
255 = 0 drops a k-mer whose true difference is unknown).

`combine` is the expected value of the GPU path (include/brx.h "count lists", br_amd/csrc/brx_setops.hip:
brx_counts_combine_device, brx_counts_combine), `spectrum` that of brx_counts_spectrum, `select` that of brx_counts_finish,
`result_floor` the floor rule of brx_counts_combine -- as setops.py is for set algebra: no GPU and no library needed.

A list answers lookups through a DIRECTORY of bucket offsets into its sorted keys (include/brx.h "lookups in a count list",
br_amd/csrc/brx_listlookup.hip): `auto_log2_buckets` is the bucket count brx_counts_lookup_prepare chooses, `directory` the
array it builds, `lookup` what brx_counts_get_counts and the abundance calls of a list answer."""
from __future__ import annotations

from typing import Tuple

import numpy as np

ADD, MAX, MIN, SUB = 0, 1, 2, 3          # BRX_COUNTOP_*
OPS = {"add": ADD, "max": MAX, "min": MIN, "sub": SUB}

# the merge kernel's tile, set algebra's: PER_THREAD consecutive positions of the merged sequence per thread, 256 threads
# (MERGE_PER_THREAD and MERGE_TILE of brx_setops.hip; the tests aim at the edges)
PER_THREAD = 8
TILE = 256 * PER_THREAD


def _list(keys, counts) -> Tuple[np.ndarray, np.ndarray]:
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    counts = np.ascontiguousarray(counts, dtype=np.uint8)
    if keys.ndim != 1 or counts.shape != keys.shape:
        raise ValueError("count list: keys and counts are one-dimensional arrays of one length")
    if keys.size > 1 and not (keys[1:] > keys[:-1]).all():
        raise ValueError("count list: keys must be strictly increasing")
    if counts.size and int(counts.min()) == 0:
        raise ValueError("count list: a count of 0 (a listed k-mer was seen at least once)")
    return keys, counts


def op_id(op) -> int:
    """BRX_COUNTOP_* of a name of OPS or of the number itself"""
    if isinstance(op, str):
        if op not in OPS:
            raise ValueError(f"count list: unknown operation {op!r} (one of {sorted(OPS)})")
        return OPS[op]
    if int(op) not in OPS.values():
        raise ValueError(f"count list: unknown operation {op!r}")
    return int(op)


def combine(a_keys, a_cnts, b_keys, b_cnts, op, min_count: int = 1) -> Tuple[np.ndarray, np.ndarray]:
    """(keys, counts) of `A op B` with the results below min_count (0 means 1) dropped; op a name of OPS or a BRX_COUNTOP_*
    number.  Counts saturate at 255 and are taken as they are: see the module's text on `sub`"""
    ka, ca = _list(a_keys, a_cnts)
    kb, cb = _list(b_keys, b_cnts)
    op = op_id(op)
    if not 0 <= int(min_count) <= 256:
        raise ValueError(f"count list: min_count={min_count}")
    keys = np.union1d(ka, kb)
    va = np.zeros(keys.size, dtype=np.int64)
    vb = np.zeros(keys.size, dtype=np.int64)
    va[np.searchsorted(keys, ka)] = ca
    vb[np.searchsorted(keys, kb)] = cb
    if op == ADD:
        r = np.minimum(255, va + vb)
    elif op == MAX:
        r = np.maximum(va, vb)
    elif op == MIN:
        r = np.minimum(va, vb)
    else:
        r = np.maximum(0, va - vb)
    keep = r >= max(1, int(min_count))
    return keys[keep], r[keep].astype(np.uint8)


def sizes(a, b) -> Tuple[int, int, int]:
    """(|A|, |B|, |A n B|) of two lists given as (keys, counts) or as their keys"""
    ka = np.ascontiguousarray(a[0] if isinstance(a, tuple) else a, dtype=np.uint64)
    kb = np.ascontiguousarray(b[0] if isinstance(b, tuple) else b, dtype=np.uint64)
    return int(ka.size), int(kb.size), int(np.isin(ka, kb, assume_unique=True).sum())


def spectrum(k: int, counts, floor: int = 1) -> np.ndarray:
    """uint64[256]: bin v >= 1 the entries with count v, bin 0 the k-mers not listed, 2^(2k-1) - n.  Bins 1 .. floor - 1 are 0,
    as a floored counter reports them; a count below the floor is an error"""
    counts = np.ascontiguousarray(counts, dtype=np.uint8)
    if counts.size and int(counts.min()) < max(1, int(floor)):
        raise ValueError(f"count list: a count below the floor {floor}")
    h = np.bincount(counts, minlength=256).astype(np.uint64)
    h[0] = (1 << (2 * k - 1)) - counts.size
    return h


def select(keys, counts, abundance: int) -> np.ndarray:
    """the keys with count > abundance (strict, as every finish of the project)"""
    keys, counts = _list(keys, counts)
    return keys[counts.astype(np.int64) > int(abundance)]


MAX_LOG2_BUCKETS = 30   # the largest directory a list takes: 2^30 + 1 offsets
KEYS_PER_BUCKET = 16    # the mean the chosen directory aims at: 16 u64 keys are one 128-byte request


def max_log2_buckets(k: int) -> int:
    """the largest log2 of the bucket count at this k: a bucket holds at least one possible key"""
    return min(2 * int(k) - 1, MAX_LOG2_BUCKETS)


def auto_log2_buckets(n: int, k: int) -> int:
    """the d brx_counts_lookup_prepare chooses for n keys: the smallest d >= 0 with 16 * 2^d >= n, capped at min(2k-1, 30)"""
    d = 0
    while d < max_log2_buckets(k) and (KEYS_PER_BUCKET << d) < int(n):
        d += 1
    return d


def directory(keys, k: int, log2_buckets: int) -> np.ndarray:
    """uint64[2^d + 1], the lookup directory of a list's ascending keys (all below 2^(2k-1)): entry b is the number of keys
    < (b << shift), shift = (2k-1) - d, so bucket b is keys[dir[b] : dir[b + 1]] and the last entry is n"""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    d = int(log2_buckets)
    if not 0 <= d <= max_log2_buckets(k):
        raise ValueError(f"count list: log2_buckets={log2_buckets} (0..{max_log2_buckets(k)} at k={k})")
    if keys.size and int(keys[-1]) >> (2 * int(k) - 1):
        raise ValueError(f"count list: a key of 2^{2 * int(k) - 1} or more at k={k}")
    shift = 2 * int(k) - 1 - d
    borders = np.arange((1 << d) + 1, dtype=np.uint64) << np.uint64(shift)
    return np.searchsorted(keys, borders, side="left").astype(np.uint64)


def lookup(keys, counts, hashes) -> np.ndarray:
    """uint8 per entry of `hashes` (canonical k-mer >> 1): the count beside that key, 0 where the list does not hold it --
    what brx_counts_get_counts and the abundance calls of a list answer, whatever the directory"""
    keys, counts = _list(keys, counts)
    hashes = np.ascontiguousarray(hashes, dtype=np.uint64)
    out = np.zeros(hashes.size, dtype=np.uint8)
    if keys.size:
        pos = np.minimum(np.searchsorted(keys, hashes, side="left"), keys.size - 1)
        hit = keys[pos] == hashes
        out[hit] = counts[pos[hit]]
    return out


def result_floor(op, floor_a: int, floor_b: int) -> int:
    """the floor of `A op B` before min_count, given the operands' floors (the smallest count each list kept, >= 1; k-mers
    seen fewer times are unknown to it).  The new list's floor is max(this, min_count).
        max, min   max(fa, fb), and the result is exact from there up: a value at or above it needs the key present with
                   that count in an operand (max) or in both (min)
        sub        needs fb == 1 -- the k-mers B no longer knows would be subtracted as 0; the floor is fa
        add        needs fa == fb == 1 -- two unknown parts could add up to a count that must be present
    ValueError on the refused cases"""
    op, fa, fb = op_id(op), int(floor_a), int(floor_b)
    if not (1 <= fa <= 255 and 1 <= fb <= 255):
        raise ValueError(f"count list: floors are 1..255 ({fa}, {fb})")
    if op in (MAX, MIN):
        return max(fa, fb)
    if op == SUB:
        if fb != 1:
            raise ValueError(f"count list: sub needs the subtracted list's floor to be 1 (it is {fb})")
        return fa
    if fa != 1 or fb != 1:
        raise ValueError(f"count list: add needs both floors to be 1 (they are {fa} and {fb})")
    return 1
