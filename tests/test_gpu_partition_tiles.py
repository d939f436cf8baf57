"""The partition passes of the sorted set build, where their tiles, ranges and prefetches can go wrong.

Level 1 cuts the flat base stream into 4096-position tiles and gives every block one contiguous range of them; each tile's
loads are issued one or two tiles ahead and consumed behind the k-mer loop of the tile before, the 256 read offsets that
come with them usually reach past the window (else the boundary loop goes back to memory), and the scan places whole
ranges, not tiles.  Levels >= 2 read one record per work item, a tile ahead.  Everything is compared with the oracle as
test_partitioned_level1_tile_ranges does: byte for byte up to k = 15, popcount and membership against the sparse oracle
above.
"""
import functools

import numpy as np
import pytest

import br_amd
from br_amd import _lib
from oracle import oracle as O

pytestmark = pytest.mark.gpu

TILE = 4096


def _rand(rng, n):
    return bytes(rng.choice(list(b"ACGT"), size=int(n)).astype(np.uint8))


def _kmers_of(reads, k):
    out = []
    for r in reads:
        for i in range(0, len(r) - k + 1, 5):
            out.append(O.seq2bit(r[i:i + k]))
    return np.array(out, dtype=np.uint64)


def _check(reads, k, probe, counts=None):
    """from_count(COUNT_SORTED) of `reads` at abundance 0 and 2 against the oracle; `counts`: count_reads(k, reads), k <= 15"""
    for a in (0, 2):
        gs = br_amd.Pcon.from_count(reads, k, a, strategy=_lib.COUNT_SORTED)
        if k <= 15:
            if counts is None:
                counts = O.count_reads(k, reads)
            assert gs.to_solid_bytes() == O.Solid.from_count(k, counts, a).to_bytes()
        else:
            ref = O.Solid.sparse_from_count(k, reads, a)
            assert gs.popcount() == ref.popcount() > 1000
            kmers = _kmers_of(probe, k)
            got = gs.get_many(kmers)
            assert np.array_equal(got, np.array([ref.get(int(x)) for x in kmers]))
            assert got.any() and (a == 0 or not got.all())


# ---------------------------------------------------------------- many read starts in one window ---------------------
@functools.lru_cache(maxsize=1)
def _crowded_reads():
    rng = np.random.default_rng(7001)
    tiny = [_rand(rng, n) for n in rng.integers(0, 15, size=9000)]
    # the long reads carry the k-mers; each of them twice (and the first eight a third time) so that abundance 2 keeps some
    base = [_rand(rng, n) for n in rng.integers(300, 3001, size=16)]
    long_ = base + base + base[:8]
    reads = tiny[:3000] + long_[:14] + tiny[3000:6000] + long_[14:28] + tiny[6000:] + long_[28:]
    offs = np.concatenate([[0], np.cumsum([len(r) for r in reads])])
    # read starts in the busiest window of 4096 + k positions that begins at a tile edge
    per_window = max(int(np.searchsorted(offs, g + TILE) - np.searchsorted(offs, g)) for g in range(0, int(offs[-1]), TILE))
    assert per_window > 512, per_window          # the boundary loop makes a second and a third trip
    assert len(reads) > 8192                     # from_count adds two batches to one counter
    assert any(len(r) == 0 for r in tiny)
    return reads, base


@functools.lru_cache(maxsize=1)
def _crowded_counts(k):
    return O.count_reads(k, _crowded_reads()[0])


@pytest.mark.parametrize("blocks", ["1", "3"])
@pytest.mark.parametrize("k", [13, 15, 19])
def test_many_read_starts_in_one_window(monkeypatch, k, blocks):
    monkeypatch.setenv("BRX_L1_GRID", blocks)
    reads, base = _crowded_reads()
    _check(reads, k, base[::3], _crowded_counts(k) if k <= 15 else None)


# ---------------------------------------------------------------- tile edges -----------------------------------------
@pytest.mark.parametrize("n", [1, 3])
def test_tile_edges(monkeypatch, n):
    """Batches that end one base before, at, and one base behind a tile edge, and k - 1 behind it (the last tile then holds
    no whole k-mer of its own), as one read and as two reads that meet at position 4095, 4096 or 4097; with one range, two,
    and five (more ranges than tiles: the number of ranges is clamped to the tiles)."""
    k = 13
    rng = np.random.default_rng(7100 + n)
    for total in (TILE * n - 1, TILE * n, TILE * n + 1, TILE * n + k - 1):
        seq = _rand(rng, total)
        for cut in (None, 4095, 4096, 4097):
            if cut is not None and cut > total:
                continue
            reads = [seq] if cut is None else [seq[:cut], seq[cut:]]
            counts = O.count_reads(k, reads)
            refs = {a: O.Solid.from_count(k, counts, a).to_bytes() for a in (0, 2)}
            for blocks in ("1", "2", "5"):
                monkeypatch.setenv("BRX_L1_GRID", blocks)
                for a in (0, 2):
                    gs = br_amd.Pcon.from_count(reads, k, a, strategy=_lib.COUNT_SORTED)
                    assert gs.to_solid_bytes() == refs[a], (total, cut, blocks, a)


# ---------------------------------------------------------------- ranges that do not divide; levels >= 2 -------------
@functools.lru_cache(maxsize=1)
def _lowcomplex_reads():
    """20 tiles.  A * 9000 (three times, and T * 5000, its reverse complement) puts whole tiles into one digit, so a carry
    and its phantoms cross range borders, and gives one level-1 bucket some 32 000 keys: several tiles of 8192 at the levels
    above, the last one partial, next to parents that are empty or hold a few hundred keys."""
    rng = np.random.default_rng(7200)
    low = [b"A" * 9000, b"T" * 5000, b"ACACACACAC" * 2000, b"A" * 9000, b"A" * 9000]
    base = [_rand(rng, n) for n in rng.integers(300, 1501, size=6)]
    reads = low[:2] + base + [b""] + low[2:3] + base + low[3:] + base[:3]
    left = 20 * TILE - 100 - sum(len(r) for r in reads)
    assert left > 0
    reads.append(_rand(rng, left))
    assert (sum(len(r) for r in reads) + TILE - 1) // TILE == 20
    return reads, base


@pytest.mark.parametrize("blocks", ["7", None])
@pytest.mark.parametrize("k", [13, 19])
def test_ranges_that_do_not_divide(monkeypatch, k, blocks):
    """20 tiles in 7 ranges (of 2 or 3 tiles), and in the default number of ranges (one tile each)."""
    if blocks is None:
        monkeypatch.delenv("BRX_L1_GRID", raising=False)
    else:
        monkeypatch.setenv("BRX_L1_GRID", blocks)
    reads, base = _lowcomplex_reads()
    _check(reads, k, base[::2] + [b"A" * 40, b"ACACACACAC" * 4])


@pytest.mark.parametrize("k,lazy", [(19, None), (19, "0"), (21, None)])
def test_upper_levels_big_and_small_parents(monkeypatch, k, lazy):
    """k = 19 ends in the hash count of the second level's buckets, with BRX_LAZY_BITS=0 it takes the third level and
    final_count; k = 21 is the sparse set behind four levels."""
    monkeypatch.setenv("BRX_L1_GRID", "3")
    if lazy is None:
        monkeypatch.delenv("BRX_LAZY_BITS", raising=False)
    else:
        monkeypatch.setenv("BRX_LAZY_BITS", lazy)
    reads, base = _lowcomplex_reads()
    _check(reads, k, base[::2] + [b"A" * 40, b"ACACACACAC" * 4])
