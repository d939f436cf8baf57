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


# the joint kernel keeps the bins ca, cb < JOINT_CORNER in LDS (JOINT_CORNER of brx_setops.hip; the tests aim at its edge)
JOINT_CORNER = 64


def joint(a_keys, a_cnts, b_keys, b_cnts) -> np.ndarray:
    """uint64[256][256], the joint spectrum: J[ca][cb] = keys of A u B with count byte ca in A and cb in B, 0 where the list
    does not hold the key; J[0][0] = 0 (brx_counts_joint_device; brx_counts_compare sets J[0][0] = 2^(2k-1) - |A u B|, so
    that the row sums are A's `spectrum` and the column sums B's).  Counts are bytes as they are: 255 is "255 or more"; a
    key a floored list does not hold falls in row or column 0"""
    ka, ca = _list(a_keys, a_cnts)
    kb, cb = _list(b_keys, b_cnts)
    keys = np.union1d(ka, kb)
    va = np.zeros(keys.size, dtype=np.int64)
    vb = np.zeros(keys.size, dtype=np.int64)
    va[np.searchsorted(keys, ka)] = ca
    vb[np.searchsorted(keys, kb)] = cb
    return np.bincount(va * 256 + vb, minlength=65536).astype(np.uint64).reshape(256, 256)


def _joint_of(J) -> np.ndarray:
    J = np.ascontiguousarray(J, dtype=np.uint64)
    if J.shape != (256, 256):
        raise ValueError("joint spectrum: a (256, 256) array")
    return J


def compare_summary(J, k: int, min_a: int = 1, min_b: int = 1) -> dict:
    """What two lists say about each other, from their joint spectrum alone (J[0][0] is never read); every integer field in
    exact integer arithmetic.
        a, b, both, either   distinct keys with ca >= 1, with cb >= 1, with both, with either (Pcon.compare's names)
        jaccard              both / either, 0.0 when either == 0
        a_solid, b_solid, both_solid   the same with ca >= min_a and cb >= min_b
        completeness         both_solid / b_solid: the share of B's k-mers at min_b or above that A holds at min_a or above;
                             nan when b_solid == 0
        a_occ                sum of ca * J[ca][cb] over ca >= min_a: occurrences in A (a saturated byte counts as 255, a
                             lower bound)
        a_only_occ           the part of a_occ with cb < min_b: occurrences in A of k-mers B does not vouch for
        error_rate, qv       1 - (1 - a_only_occ / a_occ) ** (1 / k) and -10 log10 of it: the k-mer survival formula Merqury
                             uses, taken over occurrences; qv = inf when a_only_occ == 0, both nan when a_occ == 0"""
    J = _joint_of(J)
    min_a, min_b, k = int(min_a), int(min_b), int(k)
    if not (1 <= min_a <= 256 and 1 <= min_b <= 256):
        raise ValueError(f"joint spectrum: min_a={min_a}, min_b={min_b} (1..256)")
    if k < 1:
        raise ValueError(f"joint spectrum: k={k}")

    def total(x) -> int:  # (a sum of bins may pass 2^64: the two halves of the bins apart, each sum below 2^48)
        return (int((x >> np.uint64(32)).sum()) << 32) + int((x & np.uint64(0xFFFFFFFF)).sum())

    a, b, both = total(J[1:, :]), total(J[:, 1:]), total(J[1:, 1:])
    either = a + b - both
    a_solid, b_solid, both_solid = total(J[min_a:, :]), total(J[:, min_b:]), total(J[min_a:, min_b:])
    a_occ = sum(ca * total(J[ca, :]) for ca in range(min_a, 256))
    a_only_occ = sum(ca * total(J[ca, :min_b]) for ca in range(min_a, 256))
    if a_occ == 0:
        error_rate = qv = float("nan")
    elif a_only_occ == 0:
        error_rate, qv = 0.0, float("inf")
    else:
        error_rate = 1.0 - (1.0 - a_only_occ / a_occ) ** (1.0 / k)
        qv = -10.0 * float(np.log10(error_rate)) + 0.0  # (+ 0.0: an error rate of 1 gives 0.0, not -0.0)
    return {"a": a, "b": b, "both": both, "either": either, "jaccard": both / either if either else 0.0,
            "a_solid": a_solid, "b_solid": b_solid, "both_solid": both_solid,
            "completeness": both_solid / b_solid if b_solid else float("nan"),
            "a_occ": a_occ, "a_only_occ": a_only_occ, "error_rate": error_rate, "qv": qv}


SUMMARY_INTS = ("a", "b", "both", "either", "a_solid", "b_solid", "both_solid", "a_occ", "a_only_occ")
SUMMARY_FLOATS = (("jaccard", 6), ("completeness", 6), ("error_rate", 9), ("qv", 3))  # the decimals the report prints


def _fixed(x: float, decimals: int) -> bytes:
    """x to a fixed number of decimals, halves up, from the shortest text that reads back as x; nan and inf by name"""
    from decimal import ROUND_HALF_UP, Decimal
    if x != x:
        return b"nan"
    if x in (float("inf"), float("-inf")):
        return b"inf" if x > 0 else b"-inf"
    return format(Decimal(repr(float(x))).quantize(Decimal(1).scaleb(-decimals), rounding=ROUND_HALF_UP), "f").encode()


def compare_report(k: int, floor_a: int, floor_b: int, J, min_a: int = 1, min_b: int = 1) -> bytes:
    """the bytes of --compare-report: `#name<TAB>value` lines for k, both floors, min_a, min_b and every field of
    compare_summary (floats to SUMMARY_FLOATS' decimals, halves up), then `#ca<TAB>cb<TAB>kmers` and one line per non-zero
    bin except [0][0], rows ascending and columns ascending within a row"""
    J = _joint_of(J)
    s = compare_summary(J, k, min_a, min_b)
    out = [b"#%s\t%d\n" % (name, v) for name, v in ((b"k", int(k)), (b"floor_a", int(floor_a)), (b"floor_b", int(floor_b)),
                                                    (b"min_a", int(min_a)), (b"min_b", int(min_b)))]
    out += [b"#%s\t%d\n" % (name.encode(), s[name]) for name in SUMMARY_INTS]
    out += [b"#%s\t%s\n" % (name.encode(), _fixed(s[name], decimals)) for name, decimals in SUMMARY_FLOATS]
    out.append(b"#ca\tcb\tkmers\n")
    flat = J.ravel()
    for x in np.flatnonzero(flat):
        if x:
            out.append(b"%d\t%d\t%d\n" % (x >> 8, x & 255, int(flat[x])))
    return b"".join(out)


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
