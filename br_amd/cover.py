"""Solid coverage of a read, stated in numpy: the definitions of include/brx.h ("coverage") in their readable form.

No counterpart in the reference.  For a read `s` of `n` bytes and a set of k-mer length `k`:

  solid[i]   0 <= i <= n-k: KmerSet::get of the forward k-mer s[i..i+k), every byte coded by (c >> 1) & 3
  covered[j] 0 <= j < n: some solid[i] holds with j-k+1 <= i <= j
  run        a maximal stretch of covered bases (at least k long)
  masked     letters in upper case where covered, in lower case where not; other bytes stay
  split      the runs of at least min_len bases, each a record of its own, `name_i [description]`

Everything here starts from the solid bits, whoever computed them (the GPU's flags, a KmerSet asked k-mer by k-mer,
the tests' oracle): this file never probes a set by itself except through `solid_bits`, which asks a KmerSet.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

SOLID_START = 1  # BRX_COVER_SOLID_START
COVERED = 2      # BRX_COVER_COVERED

STATS_DTYPE = np.dtype([("kmers", np.uint32), ("solid", np.uint32), ("covered", np.uint32), ("runs", np.uint32)])


def kmers_of(seq: bytes, k: int) -> np.ndarray:
    """the forward k-mer that starts at every position 0..n-k (uint64; 2k <= 62 bits)"""
    n = len(seq) - k + 1
    if n <= 0:
        return np.zeros(0, dtype=np.uint64)
    code = ((np.frombuffer(seq, dtype=np.uint8) >> 1) & 3).astype(np.uint64)
    km = np.zeros(n, dtype=np.uint64)
    for j in range(k):
        km = (km << np.uint64(2)) | code[j:j + n]
    return km


def solid_bits(kmer_set, seq: bytes) -> np.ndarray:
    """solid[] of a read from any KmerSet (br_amd.set.KmerSet: get / k; get_many when it has one)"""
    km = kmers_of(seq, kmer_set.k())
    if not km.size:
        return np.zeros(0, dtype=bool)
    if hasattr(kmer_set, "get_many"):
        return np.asarray(kmer_set.get_many(km), dtype=bool)
    return np.array([kmer_set.get(int(x)) for x in km], dtype=bool)


def covered_from_solid(solid: np.ndarray, n: int, k: int) -> np.ndarray:
    """covered[0..n): a base is covered if one of the (up to k) k-mers that contain it is solid"""
    solid = np.asarray(solid, dtype=bool)
    assert solid.size == max(n - k + 1, 0)
    cov = np.zeros(n, dtype=bool)
    if solid.size:
        # +1 where a solid k-mer starts, -1 behind its last base: covered where the running sum is positive
        d = np.zeros(n + 1, dtype=np.int64)
        idx = np.flatnonzero(solid)
        np.add.at(d, idx, 1)
        np.add.at(d, idx + k, -1)
        cov = np.cumsum(d[:n]) > 0
    return cov


def runs_of(covered: np.ndarray) -> List[Tuple[int, int]]:
    """the runs as (start, end) with end exclusive, in order"""
    c = (np.asarray(covered) != 0).astype(np.int8)
    if not c.size:
        return []
    edge = np.diff(np.concatenate(([0], c, [0])))
    return list(zip(np.flatnonzero(edge == 1).tolist(), np.flatnonzero(edge == -1).tolist()))


def flags_from_solid(solid: np.ndarray, n: int, k: int) -> np.ndarray:
    """one byte per base: SOLID_START | COVERED, as brx_set_cover_batch writes them"""
    fl = np.zeros(n, dtype=np.uint8)
    solid = np.asarray(solid, dtype=bool)
    fl[:solid.size][solid] |= SOLID_START
    fl[covered_from_solid(solid, n, k)] |= COVERED
    return fl


def stats_from_flags(flags: np.ndarray, k: int) -> Tuple[int, int, int, int]:
    """(kmers, solid, covered, runs) of one read"""
    flags = np.asarray(flags, dtype=np.uint8)
    cov = (flags & COVERED) != 0
    return (max(flags.size - k + 1, 0), int(np.count_nonzero(flags & SOLID_START)), int(np.count_nonzero(cov)),
            len(runs_of(cov)))


def mask_read(seq: bytes, covered: np.ndarray) -> bytes:
    """the masked form: letters upper case where covered, lower case where not"""
    b = np.frombuffer(seq, dtype=np.uint8)
    if not b.size:
        return b""
    low = b | 0x20
    letter = (low >= ord("a")) & (low <= ord("z"))
    cov = np.asarray(covered, dtype=bool)
    out = np.where(letter, np.where(cov, b & 0xDF, low), b).astype(np.uint8)
    return out.tobytes()


def split_read(seq: bytes, covered: np.ndarray, min_len: int = 0) -> List[Tuple[int, bytes]]:
    """the split form: (start, bytes) of every run of at least min_len bases, in order"""
    return [(s, seq[s:e]) for s, e in runs_of(covered) if e - s >= min_len]


def piece_name(header: bytes, i: int) -> bytes:
    """definition line (without '>') of piece i (1-based) of the record `name [description]`: `name_i [description]`"""
    name, sep, desc = header.partition(b" ")
    return name + b"_" + str(i).encode() + sep + desc


def split_record(header: bytes, seq: bytes, covered: np.ndarray, min_len: int = 0) -> List[Tuple[bytes, bytes]]:
    """(definition line, sequence) of the pieces of one record"""
    return [(piece_name(header, i + 1), piece) for i, (_, piece) in enumerate(split_read(seq, covered, min_len))]


def cover_read(kmer_set, seq: bytes) -> np.ndarray:
    """flags of one read, probed k-mer by k-mer through `kmer_set` (the record-by-record path)"""
    return flags_from_solid(solid_bits(kmer_set, seq), len(seq), kmer_set.k())


def unpack_flags(flags: np.ndarray, offsets: Sequence[int]) -> List[np.ndarray]:
    """per-read views of a batch's flags"""
    return [flags[int(offsets[i]):int(offsets[i + 1])] for i in range(len(offsets) - 1)]


def totals(stats: np.ndarray) -> Optional[dict]:
    """sums of a STATS_DTYPE array"""
    return {nm: int(stats[nm].astype(np.uint64).sum()) for nm in STATS_DTYPE.names}
