"""The probe index is built by regions (br_amd/csrc/brx_index.hip: keys ordered by the region of their home line, every
region's lines put together in LDS and written once, chains that leave their region placed afterwards).  Sets built from
explicit key lists must answer every probe like the Python key set does, and like the same set built the old way
(BRX_INDEX_BUILD=0: clear the table, insert one key at a time): same answers, same popcount, same fingerprint.

The shapes are the smallest at which each part of the build can go wrong: a table smaller than a region, exactly one
region, two, a nearly full table whose chains cross every region boundary and wrap from the last line to line 0, a
planted pile of keys on the last line of a region / of the table, sets with a bit vector (no chains), one key, no key."""
import numpy as np
import pytest
import torch

import br_amd
from br_amd import _lib

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
BUILDS = ("1", "0")  # by regions, the old way


def _u64(x):
    return np.uint64(x)


def _revcomp(x: np.ndarray, k: int) -> np.ndarray:
    y = x ^ _u64(0xAAAAAAAAAAAAAAAA)
    y = ((y >> _u64(2)) & _u64(0x3333333333333333)) | ((y & _u64(0x3333333333333333)) << _u64(2))
    y = ((y >> _u64(4)) & _u64(0x0F0F0F0F0F0F0F0F)) | ((y & _u64(0x0F0F0F0F0F0F0F0F)) << _u64(4))
    return y.byteswap() >> _u64(64 - 2 * k)


def _parity(x: np.ndarray) -> np.ndarray:
    p = x.copy()
    for s in (32, 16, 8, 4, 2, 1):
        p ^= p >> _u64(s)
    return p & _u64(1)


def _khash(fwd: np.ndarray, k: int) -> np.ndarray:
    """canonical (the even-popcount member of {k-mer, reverse complement}) >> 1: what the key lists hold"""
    return np.where(_parity(fwd) == 1, _revcomp(fwd, k), fwd) >> _u64(1)


def _canonical_of_key(h: np.ndarray) -> np.ndarray:
    return (h << _u64(1)) | _parity(h)


def _home_line(fwd: np.ndarray, k: int, m: int, log2_lines: int) -> np.ndarray:
    """brx_index.hpp minimizer_of + index_line_of"""
    w, mm = k - m + 1, _u64((1 << (2 * m)) - 1)
    rc = _revcomp(fwd, k)
    best = np.full(fwd.shape, 0xFFFFFFFF, dtype=np.uint64)
    for j in range(w):
        c = np.minimum((fwd >> _u64(2 * j)) & mm, (rc >> _u64(2 * (w - 1 - j))) & mm)
        best = np.minimum(best, (c * _u64(0x9E3779B1)) & _u64(0xFFFFFFFF))
    return ((best * _u64(0x85EBCA6B)) & _u64(0xFFFFFFFF)) >> _u64(32 - log2_lines)


def _fingerprint(keys: np.ndarray):
    s1 = sum(int(x) for x in keys) & M64
    s2 = sum(int(x) * int(x) for x in keys) & M64
    return int(keys.size), s1, s2


def _random_keys(k: int, n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    fwd = rng.integers(0, 1 << (2 * k), size=n + n // 8, dtype=np.uint64)
    keys = np.unique(_khash(fwd, k))
    return rng.permutation(keys)[:n]


def _sparse_set(k: int, monkeypatch) -> br_amd.Pcon:
    """a set without bit vector (chained table) at small k"""
    monkeypatch.setenv("BRX_FORCE_SPARSE", "1")
    try:
        c = br_amd.Counter(k, 0, _lib.COUNT_SORTED)
        c.add_reads([b"ACGTTGCATGCCGATAGCTAGGATCCAGTCAGTACCGATTAGC"])
        gs = c.finish(1)
    finally:
        monkeypatch.delenv("BRX_FORCE_SPARSE", raising=False)
    assert gs.is_sparse()
    return gs


def _queries(keys: np.ndarray, k: int, seed: int):
    """every key (as its canonical k-mer or the reverse complement, alternating) and as many k-mers not in the set"""
    rng = np.random.default_rng(seed)
    present = _canonical_of_key(keys)
    present[1::2] = _revcomp(present[1::2], k)
    rnd = rng.integers(0, 1 << (2 * k), size=max(keys.size, 64) * 2, dtype=np.uint64)
    absent = rnd[~np.isin(_khash(rnd, k), keys)][:max(keys.size, 64)]
    q = np.concatenate([present, absent])
    return q, np.isin(_khash(q, k), keys)


def _build_and_check(gs, keys, k, m, log2_lines, monkeypatch, seed=1):
    """builds the chained table from `keys` both ways; returns the two index_info dicts"""
    d_keys = torch.from_numpy(keys.astype(np.int64)).cuda() if keys.size else None
    q, want = _queries(keys, k, seed)
    fp_want = _fingerprint(keys)
    infos = []
    for build in BUILDS:
        monkeypatch.setenv("BRX_INDEX_BUILD", build)
        info = gs.index_build_from_keys_device(d_keys.data_ptr() if keys.size else None, int(keys.size), m, log2_lines)
        monkeypatch.delenv("BRX_INDEX_BUILD")
        assert info["valid"] and info["keys"] == keys.size
        got, _ = gs.get_batch_indexed(q)
        assert np.array_equal(got, want), (build, int((got != want).sum()))
        assert np.array_equal(gs.get_many(q), want), build
        assert gs.popcount() == keys.size
        assert gs.fingerprint() == fp_want, (build, gs.fingerprint(), fp_want)
        infos.append(info)
    assert infos[0]["log2_lines"] == infos[1]["log2_lines"] and infos[0]["m"] == infos[1]["m"]
    return infos


@pytest.fixture(scope="module")
def keys19():
    return _random_keys(19, 50_000, 19)


@pytest.mark.parametrize("log2_lines,expect", [(4, 14), (10, 14), (11, 14), (14, 14), (15, 15)])
def test_random_keys_tiny_one_and_two_regions(keys19, log2_lines, expect, monkeypatch):
    """50 000 keys need 2^14 lines of 7 slots: a request for fewer lines is grown, exactly as before, to 16 regions about
    half full.  The same keys cut down to fit the table asked for give the table smaller than a region (16 lines), exactly
    one region (2^10 lines) and two (2^11)."""
    gs = _sparse_set(19, monkeypatch)
    infos = _build_and_check(gs, keys19, 19, 0, log2_lines, monkeypatch)
    assert infos[0]["log2_lines"] == expect
    if log2_lines <= 11:
        fit = keys19[:(7 << log2_lines) * 4 // 5 - 1]  # (7 << log2_lines) >= n + n / 4 still holds: the table stays
        infos = _build_and_check(gs, fit, 19, 0, log2_lines, monkeypatch, seed=2)
        assert infos[0]["log2_lines"] == log2_lines
        assert infos[0]["overflow_keys"] > 0 and infos[1]["overflow_keys"] > 0


def test_k31_keys_too_wide_to_carry_their_region(monkeypatch):
    """at k = 31 a key fills 61 bits of its word: the region is sorted as a key of its own, the k-mer key as its value"""
    k = 31
    gs = br_amd.Pcon.from_count([b"ACGTTGCATGCCGATAGCTAGGATCCAGTCAGTACCGATTAGC"], k, 0)
    assert gs.is_sparse()
    infos = _build_and_check(gs, _random_keys(k, 20_000, 31), k, 0, 12, monkeypatch)
    assert infos[0]["log2_lines"] == 12 and infos[0]["overflow_keys"] > 0


def test_dense_table_long_chains_and_wrap(keys19, monkeypatch):
    """40 000 keys in 2^13 lines (57 344 slots, 70 % full): long chains, spills across all 8 regions, the wrap to line 0"""
    gs = _sparse_set(19, monkeypatch)
    keys = keys19[:40_000]
    infos = _build_and_check(gs, keys, 19, 0, 13, monkeypatch)
    assert infos[0]["log2_lines"] == 13
    assert infos[0]["overflow_keys"] > 1000 and infos[1]["overflow_keys"] > 1000


@pytest.mark.parametrize("where", ["last line of a region", "last line of the table"])
def test_planted_cluster_leaves_its_region(where, monkeypatch):
    """300 19-mers around one 15-mer whose hash is so small that it is their minimizer, with a home line that ends a
    region (2^12 lines = 4 regions): 7 stay, the others chain into the next region, or round to line 0"""
    k, m, log2_lines = 19, 15, 12
    rng = np.random.default_rng(1512)
    cand = rng.integers(0, 1 << (2 * m), size=1 << 22, dtype=np.uint64)
    cand = np.minimum(cand, _revcomp(cand, m))
    h = (cand * _u64(0x9E3779B1)) & _u64(0xFFFFFFFF)
    line = ((h * _u64(0x85EBCA6B)) & _u64(0xFFFFFFFF)) >> _u64(32 - log2_lines)
    ok = (line == 4095) if where == "last line of the table" else ((line & _u64(1023)) == 1023) & (line != 4095)
    pick = np.flatnonzero(ok)[np.argmin(h[ok])]
    core, core_line = cand[pick], int(line[pick])
    fwd = []
    for off in range(k - m + 1):  # the 15-mer at each of the 5 offsets, every flank
        flank = np.arange(1 << (2 * (k - m)), dtype=np.uint64)
        lo, hi = flank & _u64((1 << (2 * off)) - 1), flank >> _u64(2 * off)
        fwd.append((hi << _u64(2 * (off + m))) | (core << _u64(2 * off)) | lo)
    fwd = np.concatenate(fwd)
    fwd = fwd[_home_line(fwd, k, m, log2_lines) == core_line]
    planted = rng.permutation(np.unique(_khash(fwd, k)))[:300]
    assert planted.size == 300, planted.size
    keys = np.unique(np.concatenate([planted, _random_keys(k, 20_000, 5)]))
    gs = _sparse_set(k, monkeypatch)
    infos = _build_and_check(gs, rng.permutation(keys), k, m, log2_lines, monkeypatch)
    assert infos[0]["m"] == m and infos[0]["log2_lines"] == log2_lines
    assert infos[0]["overflow_keys"] >= 293 and infos[1]["overflow_keys"] >= 293


def test_one_key_and_empty_set(keys19, monkeypatch):
    """a single key goes through the build by regions; built over a table that was full, the empty set leaves nothing
    behind: every probe says absent"""
    gs = _sparse_set(19, monkeypatch)
    _build_and_check(gs, keys19[:1], 19, 0, 11, monkeypatch)
    _build_and_check(gs, keys19[:11_000], 19, 0, 11, monkeypatch)
    infos = _build_and_check(gs, keys19[:0], 19, 0, 11, monkeypatch)
    assert infos[0]["overflow_keys"] == 0
    q = _canonical_of_key(keys19[:11_000])
    got, n_fallback = gs.get_batch_indexed(q)
    assert not got.any() and n_fallback == 0


@pytest.fixture(scope="module")
def dense15(raw_reads):
    """the k = 15 set of tests/test_gpu_index.py (bit vector present) and its members, read back from the bit vector"""
    gs = br_amd.Pcon.from_count(raw_reads[:150], 15, 1, strategy=_lib.COUNT_DENSE)
    assert not gs.is_sparse() and gs.bits_state() == 0
    n = gs.popcount()
    d = torch.empty(n, dtype=torch.int64, device="cuda")
    assert gs.extract_keys_device(0, gs.n_hashes(), d.data_ptr(), n) == n
    torch.cuda.synchronize()
    return gs, d.cpu().numpy().astype(np.uint64)


@pytest.mark.parametrize("log2_lines", [4, 5, 6, 11])
def test_with_bit_vector_overflow_is_flagged_not_chained(dense15, raw_reads, log2_lines, monkeypatch):
    """k = 15 with its bit vector: a full line turns its keys away to the bits.  Which keys a line keeps depends on the
    order they arrive in, how many it turns away does not: the count is the same both ways.  16 and 32 lines are tables
    of less than one region, and of half an occupancy word and one; One's correction reads the occupancy bits."""
    k = 15
    gs, members = dense15
    rng = np.random.default_rng(log2_lines)
    rnd = rng.integers(0, 1 << (2 * k), size=30_000, dtype=np.uint64)
    q = np.concatenate([_canonical_of_key(members), _revcomp(_canonical_of_key(members), k), rnd])
    want = np.isin(_khash(q, k), members)
    assert np.array_equal(gs.get_many(q), want)
    out = {}
    for build in BUILDS:
        monkeypatch.setenv("BRX_INDEX_BUILD", build)
        info = gs.index_build(0, log2_lines)
        monkeypatch.delenv("BRX_INDEX_BUILD")
        assert info["valid"] and info["keys"] == members.size and info["log2_lines"] == log2_lines
        got, n_fallback = gs.get_batch_indexed(q)
        assert np.array_equal(got, want), build
        assert n_fallback > 0 and gs.popcount() == members.size
        chain = br_amd.Chain(gs, [("one", 5, 7)], two_side=False)
        out[build] = (info["overflow_keys"], gs.fingerprint(), chain.correct_reads(raw_reads[:60]))
        assert gs.index_info()["log2_lines"] == log2_lines  # the chain used this very table
    assert out["1"][0] == out["0"][0] > 0
    assert out["1"][1] == out["0"][1] == _fingerprint(members)
    assert out["1"][2] == out["0"][2]


def _timers_of(build):
    """names of the library's kernel timers that ran during build()"""
    _lib.profile_enable(True)
    try:
        _lib.profile_reset()
        build()
        return {name for name, v in _lib.profile_all().items() if v["launches"]}
    finally:
        _lib.profile_reset()
        _lib.profile_enable(False)


def test_refused_scratch_builds_the_old_way(keys19, monkeypatch):
    """BRX_INDEX_SCRATCH_PAD_GB makes the build ask for 2^50 bytes of scratch, which the runtime refuses: the build must
    go the old way (its timers say which way it went) and succeed, with the refusal left behind neither as the thread's
    last HIP error nor as the library's error text -- and the next build, with scratch, goes by regions again"""
    gs = _sparse_set(19, monkeypatch)
    keys = keys19[:40_000]
    d_keys = torch.from_numpy(keys.astype(np.int64)).cuda()
    q, want = _queries(keys, 19, 3)
    text_before = _lib.lib().brx_last_error()
    for pad, ran, ran_not in (("1048576", "index_zero", "index_lines"), ("", "index_lines", "index_zero")):
        if pad:
            monkeypatch.setenv("BRX_INDEX_SCRATCH_PAD_GB", pad)
        else:
            monkeypatch.delenv("BRX_INDEX_SCRATCH_PAD_GB")
        info = {}
        timers = _timers_of(lambda: info.update(gs.index_build_from_keys_device(d_keys.data_ptr(), int(keys.size), 0, 13)))
        assert ran in timers and ran_not not in timers, (pad, timers)
        assert info["valid"] and info["keys"] == keys.size and info["log2_lines"] == 13
        got, _ = gs.get_batch_indexed(q)
        assert np.array_equal(got, want)
        assert gs.fingerprint() == _fingerprint(keys)
        assert _lib.lib().brx_last_error() == text_before


def test_bit_vector_set_emptied_over_a_full_table(raw_reads, monkeypatch):
    """a set WITH bit vector, where One's correction goes through the occupancy bits: a table filled from a key list, then
    built again from the (empty, then nearly empty) bit vector in the same allocation.  Nothing of the full table may be
    left: every probe says absent and One's output is that of the old build; then three k-mers are there and the rest
    is not."""
    k = 15
    gs = br_amd.Pcon.new(k)
    assert not gs.is_sparse() and gs.popcount() == 0
    full = _random_keys(k, 11_000, 15)
    d_full = torch.from_numpy(full.astype(np.int64)).cuda()
    reads = raw_reads[:40]
    few = np.array([br_amd.set.seq2bit(reads[0][i:i + k]) for i in (0, 40, 80)], dtype=np.uint64)
    q = np.concatenate([_canonical_of_key(full), few, _revcomp(few, k)])
    for members in (few[:0], few):
        for km in members:
            gs.set(int(km), True)
        want = np.isin(_khash(q, k), _khash(members, k)) if members.size else np.zeros(q.size, dtype=bool)
        out = {}
        for build in BUILDS:
            gs.index_build_from_keys_device(d_full.data_ptr(), int(full.size), 0, 11)  # the table full of other keys
            monkeypatch.setenv("BRX_INDEX_BUILD", build)
            info = gs.index_build(0, 11)
            monkeypatch.delenv("BRX_INDEX_BUILD")
            assert info["valid"] and info["keys"] == np.unique(_khash(members, k)).size and info["overflow_keys"] == 0
            got, n_fallback = gs.get_batch_indexed(q)
            assert np.array_equal(got, want) and n_fallback == 0, build
            out[build] = br_amd.Chain(gs, [("one", 5, 7)], two_side=False).correct_reads(reads)
            assert gs.index_info()["log2_lines"] == 11
        assert out["1"] == out["0"]
