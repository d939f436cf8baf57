"""Trusted stretches of a read, stated in numpy: the definitions of include/brx.h ("trusted stretches") in their readable form.

No counterpart in the reference, which counts every k-mer of every record and codes every byte as a base.  For a read `s` of
`n` bytes, an optional quality string `q` of `n` bytes (Phred+33, the only encoding), a floor `min_quality` (0..93) and
`acgt_only`:

  letter[j]   s[j] is one of ACGTacgt
  good[j]     min_quality == 0, or q is absent, or q[j] >= 33 + min_quality (a byte below 33 fails any floor above 0)
  trusted[j]  (letter[j] or not acgt_only) and good[j]
  stretch     a maximal run of trusted bases
  split       the stretches of at least max(min_len, 1) bases, reads in order, the stretches of a read in order of their start

With min_len = k the k-mers of the pieces are exactly the k-mers of the read none of whose bases is untrusted.  The GPU path
(br_amd/csrc/brx_trust.hip) is held to this file bit for bit.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from .cover import runs_of

MAX_QUALITY = 93  # '~' is 33 + 93
STATS_DTYPE = np.dtype([("bases", np.uint32), ("non_acgt", np.uint32), ("low_quality", np.uint32), ("pieces", np.uint32),
                        ("kept_bases", np.uint32)])
TOTALS = ("bases", "non_acgt", "low_quality", "pieces", "kept_bases", "kmers")  # trust_totals8[0 .. 6) of the _fd entries

_LETTER = np.zeros(256, dtype=bool)
_LETTER[list(b"ACGTacgt")] = True


def _check(min_quality: int) -> int:
    if not 0 <= int(min_quality) <= MAX_QUALITY:
        raise ValueError(f"min_quality={min_quality} is not in 0..{MAX_QUALITY} (Phred+33)")
    return int(min_quality)


def letter_bits(seq: bytes) -> np.ndarray:
    return _LETTER[np.frombuffer(seq, dtype=np.uint8)]


def good_bits(n: int, qual: Optional[bytes], min_quality: int = 0) -> np.ndarray:
    mq = _check(min_quality)
    if mq == 0 or qual is None:
        return np.ones(n, dtype=bool)
    q = np.frombuffer(qual, dtype=np.uint8)
    if q.size != n:
        raise ValueError(f"{q.size} qualities for {n} bases")
    return q >= 33 + mq


def trusted_bits(seq: bytes, qual: Optional[bytes] = None, min_quality: int = 0, acgt_only: bool = True) -> np.ndarray:
    """trusted[0..n) of one read"""
    good = good_bits(len(seq), qual, min_quality)
    return (letter_bits(seq) & good) if acgt_only else good


def split_read(seq: bytes, qual: Optional[bytes] = None, min_quality: int = 0, acgt_only: bool = True,
               min_len: int = 1) -> List[Tuple[int, bytes]]:
    """the split form of one read: (start, bytes) of every stretch of at least max(min_len, 1) bases, in order"""
    floor = max(int(min_len), 1)
    return [(s, seq[s:e]) for s, e in runs_of(trusted_bits(seq, qual, min_quality, acgt_only)) if e - s >= floor]


def stats_of(seq: bytes, qual: Optional[bytes] = None, min_quality: int = 0, acgt_only: bool = True,
             min_len: int = 1) -> Tuple[int, int, int, int, int]:
    """(bases, non_acgt, low_quality, pieces, kept_bases) of one read; non_acgt and low_quality do not ask acgt_only"""
    letter, good = letter_bits(seq), good_bits(len(seq), qual, min_quality)
    pieces = split_read(seq, qual, min_quality, acgt_only, min_len)
    return (len(seq), int(np.count_nonzero(~letter)), int(np.count_nonzero(letter & ~good)), len(pieces),
            sum(len(p) for _, p in pieces))


def split_batch(bases: np.ndarray, quals: Optional[np.ndarray], offsets: Sequence[int], min_quality: int = 0,
                acgt_only: bool = True, min_len: int = 1):
    """(out uint8[], out_offsets uint64[p+1], piece_read uint32[p], piece_start uint64[p], stats STATS_DTYPE[n]) of a
    bases / offsets batch; `quals` (or None) is laid out like `bases`"""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    n = len(offsets) - 1
    out, lens, pr, ps = [], [], [], []
    st = np.zeros(n, dtype=STATS_DTYPE)
    for r in range(n):
        a, b = int(offsets[r]), int(offsets[r + 1])
        seq = bases[a:b].tobytes()
        qual = None if quals is None else np.ascontiguousarray(quals[a:b], dtype=np.uint8).tobytes()
        st[r] = stats_of(seq, qual, min_quality, acgt_only, min_len)
        for s, piece in split_read(seq, qual, min_quality, acgt_only, min_len):
            out.append(piece)
            lens.append(len(piece))
            pr.append(r)
            ps.append(s)
    oo = np.zeros(len(out) + 1, dtype=np.uint64)
    if out:
        oo[1:] = np.cumsum(lens, dtype=np.uint64)
    return (np.frombuffer(b"".join(out), dtype=np.uint8).copy(), oo, np.asarray(pr, dtype=np.uint32),
            np.asarray(ps, dtype=np.uint64), st)


def piece_bound(n_reads: int, total_bases: int, min_len: int = 1) -> int:
    """the bound of include/brx.h on the pieces of a batch: a caller allocates by it without a retry"""
    return n_reads + total_bases // (max(int(min_len), 1) + 1)


def kmers_of_pieces(stats: np.ndarray, k: int) -> int:
    """the k-mers a counter finds in the pieces of a split with min_len = k"""
    return int(stats["kept_bases"].astype(np.int64).sum() - stats["pieces"].astype(np.int64).sum() * (k - 1))


def totals(stats: np.ndarray) -> dict:
    """sums of a STATS_DTYPE array"""
    return {nm: int(stats[nm].astype(np.uint64).sum()) for nm in STATS_DTYPE.names}
