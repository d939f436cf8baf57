"""K-mer abundance of a read, stated in numpy: the definitions of include/brx.h ("abundance") in their readable form.

No counterpart in the reference.  For a read `s` of `n` bytes and a counter of k-mer length `k`:

  count[i]   0 <= i <= n-k: min(255, occurrences counted) of the canonical k-mer of s[i..i+k), 0 if never counted; every
             byte coded by (c >> 1) & 3, so a byte that is not ACGT is a base like any other and case does not matter
  profile    one byte per base: count[i] at base i, 0 at the last k-1 bases (every base of a read shorter than k)
  hist[v]    number of i with count[i] == v
  stats      kmers, absent = hist[0], above = #(count > abundance), min, lower median, max, sum -- all 0 without k-mers

Everything here starts from canonical hashes (canonical k-mer >> 1, what indexes the reference's count table), whoever
computed them: `canonical_hashes` below, or the tests' oracle.  This file never touches the GPU.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import cover

STATS_DTYPE = np.dtype([("kmers", np.uint32), ("absent", np.uint32), ("above", np.uint32), ("min", np.uint32),
                        ("median", np.uint32), ("max", np.uint32), ("sum", np.uint64)], align=True)  # brx_abund_stats_t

REPORT_HEADER = b"#name\tlen\tkmers\tabsent\tabove\tmin\tmedian\tmax\tmean\n"


def canonical_hashes(seq: bytes, k: int) -> np.ndarray:
    """canonical >> 1 of the k-mer at every position 0..n-k (odd k: the even-popcount member of {k-mer, revcomp})"""
    fwd = cover.kmers_of(seq, k)
    rc = np.zeros_like(fwd)
    x = fwd ^ np.uint64(int("10" * k, 2))  # complement = xor 0b10 per base
    for _ in range(k):
        rc = (rc << np.uint64(2)) | (x & np.uint64(3))
        x = x >> np.uint64(2)
    par = fwd.copy()
    for sh in (32, 16, 8, 4, 2, 1):
        par ^= par >> np.uint64(sh)
    odd = (par & np.uint64(1)).astype(bool)
    return np.where(odd, rc, fwd) >> np.uint64(1)


def count_table(hash_arrays: Sequence[np.ndarray]) -> Tuple[np.ndarray, np.ndarray]:
    """(sorted distinct hashes, their counts clipped to 255) of everything that was counted"""
    parts = [np.asarray(h, dtype=np.uint64) for h in hash_arrays if len(h)]
    allh = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)
    uniq, cnt = np.unique(allh, return_counts=True)
    return uniq, np.minimum(cnt, 255).astype(np.uint8)


def lookup(table: Tuple[np.ndarray, np.ndarray], hashes: np.ndarray) -> np.ndarray:
    """count[] of one read from its hashes"""
    uniq, cnt = table
    hashes = np.asarray(hashes, dtype=np.uint64)
    out = np.zeros(hashes.size, dtype=np.uint8)
    if uniq.size and hashes.size:
        at = np.minimum(np.searchsorted(uniq, hashes), uniq.size - 1)
        hit = uniq[at] == hashes
        out[hit] = cnt[at[hit]]
    return out


def profile_from_hashes(hash_arrays: Sequence[np.ndarray], query: Optional[Sequence[np.ndarray]] = None) -> List[np.ndarray]:
    """count[] (uint8, length kmers) of every read of `query` (default: the counted reads themselves) against the counts of
    `hash_arrays`, the hashes of the counted reads"""
    table = count_table(hash_arrays)
    return [lookup(table, h) for h in (hash_arrays if query is None else query)]


def profile_bytes(counts: np.ndarray, n: int) -> np.ndarray:
    """the profile of a read of n bases: its counts, then zeros"""
    out = np.zeros(n, dtype=np.uint8)
    out[:len(counts)] = counts
    return out


def hist_from_profile(counts: np.ndarray) -> np.ndarray:
    return np.bincount(np.asarray(counts, dtype=np.uint8), minlength=256).astype(np.uint32)


def stats_from_profile(counts: np.ndarray, abundance: int = 0) -> Tuple[int, int, int, int, int, int, int]:
    """(kmers, absent, above, min, median, max, sum) of one read's count[]"""
    c = np.sort(np.asarray(counts, dtype=np.int64))
    if not c.size:
        return (0, 0, 0, 0, 0, 0, 0)
    return (int(c.size), int(np.count_nonzero(c == 0)), int(np.count_nonzero(c > abundance)), int(c[0]),
            int(c[(c.size - 1) // 2]), int(c[-1]), int(c.sum()))


def stats_array(profiles: Sequence[np.ndarray], abundance: int = 0) -> np.ndarray:
    """STATS_DTYPE array of a list of count[] arrays"""
    out = np.zeros(len(profiles), dtype=STATS_DTYPE)
    for i, p in enumerate(profiles):
        out[i] = stats_from_profile(p, abundance)
    return out


def report_line(name: bytes, n: int, stats) -> bytes:
    """one TSV line of REPORT_HEADER; `stats` is a STATS_DTYPE record or the tuple of stats_from_profile"""
    kmers, absent, above, lo, med, hi, total = (int(v) for v in stats)
    # sum / kmers to three decimals, half up, in integers (no float formatting between the two paths that write reports)
    mean = b"0.000"
    if kmers:
        q = (total * 2000 + kmers) // (2 * kmers)
        mean = b"%d.%03d" % (q // 1000, q % 1000)
    return name + b"\t" + b"\t".join(str(v).encode() for v in (n, kmers, absent, above, lo, med, hi)) + b"\t" + mean + b"\n"


def unpack_profile(profile: np.ndarray, offsets: Sequence[int], k: int) -> List[np.ndarray]:
    """per-read count[] views (length kmers) of a batch's profile"""
    out = []
    for i in range(len(offsets) - 1):
        a, b = int(offsets[i]), int(offsets[i + 1])
        out.append(profile[a:a + max(b - a - k + 1, 0)])
    return out
