"""Count lists on the GPU path (include/brx.h "count lists", br_amd/csrc/brx_setops.hip, brx_keyfile.hip): the merge of two
sorted (key, count) lists against br_amd/countops.py at the shapes where a merge can go wrong, the objects against the
counters and the key files they replace, correction through a set finished from an added list against the oracle, stream
order of the raw entry and the command line.  Every comparison is exact."""
import gzip
import io
import os
import threading

import numpy as np
import pytest
import torch

import br_amd
from br_amd import _lib, abundance, countops, keyfile
from br_amd.set import CountList, combine_counts_device
from oracle import oracle as O
from tests.test_gpu_keyfile import _bad_files
from tests.test_gpu_setops import forward_kmers, pairs_on_diagonals
from tests.test_gpu_streams import Lane, decoy, fingerprint_of, lane, operation, probe, ptr, reads, solid_bytes_of  # noqa: F401

pytestmark = pytest.mark.gpu

TILE, PT = countops.TILE, countops.PER_THREAD
TOP = (1 << 61) - 1
OPS = list(countops.OPS)
KEY_SENTINEL = -0x1111111111111112  # 0xEEEE... as int64
CNT_SENTINEL = 0xEE
TABLE, SORTED, DENSE = _lib.COUNT_TABLE, _lib.COUNT_SORTED, _lib.COUNT_DENSE
_cache = {}


def u64(values):
    return np.ascontiguousarray(np.asarray(values, dtype=np.uint64))


def u8(values):
    return np.ascontiguousarray(np.asarray(values, dtype=np.uint8))


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy((a.view(np.int64) if a.dtype == np.uint64 else a).copy()).cuda()


def small_counts(keys, seed=0):
    """counts that make sub reach 0 and below often (1..4) and add saturate now and then (a tenth from 150 up)"""
    rng = np.random.default_rng(u64(keys).size + seed)
    n = u64(keys).size
    return np.where(rng.random(n) < 0.1, rng.integers(150, 256, n), rng.integers(1, 5, n)).astype(np.uint8)


def run_raw(a, b, op, min_count=1, cap=None, with_counts=True, stream=None):
    """(keys, counts or None, sizes3, the whole key array, the whole count array) of the raw entry; the output arrays are
    filled with the sentinels first"""
    (ka, ca), (kb, cb) = (u64(a[0]), u8(a[1])), (u64(b[0]), u8(b[1]))
    dka, dca, dkb, dcb = dev(ka), dev(ca), dev(kb), dev(cb)
    cap = ka.size + kb.size + 8 if cap is None else cap
    kout = torch.full((max(cap, 1),), KEY_SENTINEL, dtype=torch.int64, device="cuda")
    cout = torch.full((max(cap, 1),), CNT_SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        n, s3 = combine_counts_device(dka.data_ptr() if ka.size else None, dca.data_ptr() if ka.size else None, ka.size,
                                      dkb.data_ptr() if kb.size else None, dcb.data_ptr() if kb.size else None, kb.size, op,
                                      kout.data_ptr(), cout.data_ptr() if with_counts else None, cap, min_count, stream)
    finally:
        torch.cuda.synchronize()
        run_raw.left = (kout.cpu().numpy(), cout.cpu().numpy())
    wk, wc = run_raw.left
    return wk[:n].view(np.uint64), (wc[:n] if with_counts else None), s3, wk, wc


def check_raw(name, a, b, min_counts=(1,)):
    a, b = (u64(a[0]), u8(a[1])), (u64(b[0]), u8(b[1]))
    for op in OPS:
        for mc in min_counts:
            want_k, want_c = countops.combine(a[0], a[1], b[0], b[1], op, mc)
            got_k, got_c, s3, wk, wc = run_raw(a, b, op, mc)
            assert got_k.size == want_k.size and np.array_equal(got_k, want_k), (name, op, mc)
            assert np.array_equal(got_c, want_c), (name, op, mc)
            assert s3 == countops.sizes(a[0], b[0]), (name, op, mc)
            assert (wk[want_k.size:] == KEY_SENTINEL).all() and (wc[want_k.size:] == CNT_SENTINEL).all(), (name, op, mc, "written behind the result")


# ---- raw entry: shapes ---------------------------------------------------------------------------------------------------
def _sample(rng, n, hi):
    return np.sort(rng.choice(hi, size=n, replace=False)).astype(np.uint64)


@pytest.mark.parametrize("total", [0, 1, 2, PT - 1, PT + 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
def test_raw_sizes_around_thread_and_tile(total):
    rng = np.random.default_rng(total)
    for na in sorted({0, total // 3, total // 2, total}):
        nb = total - na
        hi = max(2 * total, 4)  # about half of the smaller list is in the other one
        ka, kb = _sample(rng, na, hi), _sample(rng, nb, hi)
        check_raw((total, na), (ka, small_counts(ka, 1)), (kb, small_counts(kb, 2)), (1, 2))


def pair_counts(a, b):
    """counts for two lists: for the i-th key they share, in turn (ca > cb, ca == cb, ca < cb), every sum above 255 and the
    values moving with i, so that add saturates, sub gives a positive value, 0 and a negative value, and min differs from max
    wherever the two counts differ; the keys of one list alone get 1 .. 5"""
    a, b = u64(a), u64(b)
    ca, cb = (1 + a % np.uint64(5)).astype(np.uint8), (1 + b % np.uint64(5)).astype(np.uint8)
    ia, ib = np.flatnonzero(np.isin(a, b)), np.flatnonzero(np.isin(b, a))
    i = np.arange(ia.size)
    big, small = 170 + i % 80, 130 - i % 40
    turn = i % 3
    ca[ia] = np.where(turn == 0, big, np.where(turn == 1, 128 + i % 100, small))
    cb[ib] = np.where(turn == 0, small, np.where(turn == 1, 128 + i % 100, big))
    return ca, cb


def _shape_cases():
    n = TILE + 100
    ar = np.arange
    yield "b empty", ar(TILE + 3), []
    yield "a empty", [], ar(2 * TILE + 1)
    yield "a below b: whole tiles from one list", ar(n), ar(n) + 10 * n
    yield "b below a: whole tiles from one list", ar(n) + 10 * n, ar(n)
    yield "a == b", ar(0, 3 * (TILE + 17), 3), ar(0, 3 * (TILE + 17), 3)
    yield "a inside b", ar(2 * TILE + 9)[::5], ar(2 * TILE + 9)
    yield "b inside a", ar(2 * TILE + 9), ar(2 * TILE + 9)[::7]
    yield "interleave", ar(0, 2 * TILE + 6, 2), ar(1, 2 * TILE + 6, 2)
    for shift in (0, 1):
        a, b = pairs_on_diagonals(2 * TILE + PT, shift)
        yield f"pairs on the diagonals, shift {shift}", a, b
        yield f"pairs on the diagonals, shift {shift}, lists swapped", b, a
    run = ar(2 * TILE) + 10
    yield "a run of equal pairs longer than a tile", np.concatenate([[1, 3], run]), np.concatenate([[2], run, [10 + 2 * TILE + 5]])
    yield "keys 0 and 2^61 - 1", [0, 5, TOP], [0, TOP - 1, TOP]
    yield "keys 0 and 2^61 - 1, long", np.concatenate([[0], ar(TILE) + 9, [TOP]]), np.concatenate([[0, 3], ar(0, TILE, 2) + 9, [TOP - 1, TOP]])


@pytest.mark.parametrize("name,a,b", list(_shape_cases()), ids=[c[0] for c in _shape_cases()])
def test_raw_shapes(name, a, b):
    a, b = u64(a), u64(b)
    ca, cb = pair_counts(a, b)
    if name == "pairs on the diagonals, shift 0":
        # the construction itself: A's key at the last position of every thread's share, B's equal key at the next one; and
        # what the counts of the pairs do
        merged = np.sort(np.concatenate([a, b]), kind="stable")
        m = np.arange(PT, merged.size - 1, PT)
        assert (merged[m - 1] == merged[m]).all() and m.size >= 2 * 256 and TILE in m
        xa, xb = ca[np.isin(a, b)].astype(int), cb[np.isin(b, a)].astype(int)
        assert (xa + xb > 255).all() and {-1, 0, 1} == set(np.sign(xa - xb).tolist())
        assert (np.sign(xa - xb)[:6] == [1, 0, -1, 1, 0, -1]).all()
    check_raw(name, (a, ca), (b, cb), (1, 2, 101))


def test_raw_one_array_for_both_inputs_and_equal_lists():
    a = u64(np.arange(0, 3 * TILE, 2))
    ca = small_counts(a)
    da, dc = dev(a), dev(ca)
    kout = torch.full((a.size,), KEY_SENTINEL, dtype=torch.int64, device="cuda")
    cout = torch.full((a.size,), CNT_SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for op in OPS:
        n, s3 = combine_counts_device(da.data_ptr(), dc.data_ptr(), a.size, da.data_ptr(), dc.data_ptr(), a.size, op, kout.data_ptr(),
                                      cout.data_ptr(), a.size)
        torch.cuda.synchronize()
        want_k, want_c = countops.combine(a, ca, a, ca, op)
        assert s3 == (a.size, a.size, a.size) and n == want_k.size == (0 if op == "sub" else a.size)
        if n:
            assert np.array_equal(kout.cpu().numpy().view(np.uint64), want_k) and np.array_equal(cout.cpu().numpy(), want_c)
    check_raw("equal lists, other counts", (a, ca), (a, small_counts(a, 7)), (1, 3))


def test_raw_min_count_that_drops_everything_and_keys_only():
    rng = np.random.default_rng(12)
    ka, kb = _sample(rng, TILE + 50, 3 * TILE), _sample(rng, TILE - 9, 3 * TILE)
    ca, cb = (1 + ka % np.uint64(4)).astype(np.uint8), (1 + kb % np.uint64(4)).astype(np.uint8)
    for op in OPS:
        got_k, got_c, s3, wk, wc = run_raw((ka, ca), (kb, cb), op, 255)
        assert got_k.size == 0 and s3 == countops.sizes(ka, kb)
        assert (wk == KEY_SENTINEL).all() and (wc == CNT_SENTINEL).all()
        # d_cout = NULL: the keys alone, the count array never touched
        want_k, _ = countops.combine(ka, ca, kb, cb, op, 2)
        got_k, got_c, s3, wk, wc = run_raw((ka, ca), (kb, cb), op, 2, with_counts=False)
        assert got_c is None and np.array_equal(got_k, want_k) and want_k.size > 100
        assert (wk[want_k.size:] == KEY_SENTINEL).all() and (wc == CNT_SENTINEL).all()


@pytest.mark.parametrize("grid", [1, 3, 7])
def test_raw_blocks_loop_over_tiles(monkeypatch, grid):
    """41 tiles through 1, 3 and 7 blocks (and through the grid's own cap in every other test)"""
    monkeypatch.setenv("BRX_READ_GRID", str(grid))
    if "trips" not in _cache:
        rng = np.random.default_rng(40)
        n = 40 * TILE + 77
        ka, kb = _sample(rng, n // 2, 2 * n), _sample(rng, n - n // 2, 2 * n)
        _cache["trips"] = ((ka, small_counts(ka, 3)), (kb, small_counts(kb, 4)))
    check_raw(("grid", grid), *_cache["trips"])


# ---- raw entry: refusals -------------------------------------------------------------------------------------------------
def _untouched_after(a, b, op, cap, min_count=1):
    """the refusal, and the sentinels still everywhere in both outputs"""
    with pytest.raises(_lib.BrxError) as ei:
        run_raw(a, b, op, min_count, cap)
    wk, wc = run_raw.left
    assert ei.value.status == _lib.BRX_ERR_ARG
    assert (wk == KEY_SENTINEL).all() and (wc == CNT_SENTINEL).all()
    return ei.value


def test_raw_cap_too_small_and_sizes_only():
    rng = np.random.default_rng(5)
    ka, kb = _sample(rng, TILE + 9, 3 * TILE), _sample(rng, TILE - 4, 3 * TILE)
    a, b = (ka, small_counts(ka)), (kb, small_counts(kb))
    for op in OPS:
        want_k, want_c = countops.combine(*a, *b, op)
        assert want_k.size > 1
        e = _untouched_after(a, b, op, want_k.size - 1)
        assert e.needed == want_k.size and str(want_k.size) in str(e)
        # the size-only form
        dka, dca, dkb, dcb = dev(a[0]), dev(a[1]), dev(b[0]), dev(b[1])
        torch.cuda.synchronize()
        n, s3 = combine_counts_device(dka.data_ptr(), dca.data_ptr(), ka.size, dkb.data_ptr(), dcb.data_ptr(), kb.size, op, None, None, 0)
        assert n == want_k.size and s3 == countops.sizes(ka, kb)
        # and exactly enough room is enough
        got_k, got_c, _, _, _ = run_raw(a, b, op, 1, want_k.size)
        assert np.array_equal(got_k, want_k) and np.array_equal(got_c, want_c)
    with pytest.raises(_lib.BrxError) as ei:  # a capacity without an array
        combine_counts_device(dev(ka).data_ptr(), dev(a[1]).data_ptr(), ka.size, None, None, 0, "add", None, None, 5)
    assert ei.value.status == _lib.BRX_ERR_ARG


def _broken_keys():
    good = np.arange(0, 6 * TILE, 2, dtype=np.uint64)  # 3 tiles' worth
    other = np.arange(1, 2 * TILE, 3, dtype=np.uint64)
    none = np.zeros(0, dtype=np.uint64)
    x = good.copy()
    x[1000], x[1001] = good[1001], good[1000]
    yield "unordered keys", x, other
    x = good.copy()
    x[777] = x[776]
    yield "a repeated key", x, other
    # with the other list empty, tile t of the merge is entries [TILE t, TILE t + TILE) of this one: the pair (TILE - 1, TILE)
    # lies across the edge of tiles 0 and 1 -- the second key meets the first one only as its halo
    x = good.copy()
    x[TILE] = x[TILE - 1]
    yield "a repeated key across a tile edge", x, none
    x = good.copy()
    x[2 * TILE - 1] = x[2 * TILE] + 1
    yield "descending across a tile edge", x, none


@pytest.mark.parametrize("name,bad,other", list(_broken_keys()), ids=[c[0] for c in _broken_keys()])
def test_raw_refuses_unordered_and_repeated_keys(name, bad, other):
    for op in OPS:
        for a, b in ((bad, other), (other, bad)):
            e = _untouched_after((a, np.ones(a.size, np.uint8)), (b, np.ones(b.size, np.uint8)), op, a.size + b.size + 8)
            assert "ascend" in str(e) and e.needed == 0, (name, op)


def test_raw_refuses_a_zero_count():
    good = np.arange(0, 6 * TILE, 2, dtype=np.uint64)
    other = np.arange(1, 2 * TILE, 3, dtype=np.uint64)
    none = (np.zeros(0, np.uint64), np.zeros(0, np.uint8))
    cases = []
    c = np.full(good.size, 3, np.uint8)
    c[1234] = 0
    cases.append(("in the middle of A", (good, c), (other, np.ones(other.size, np.uint8))))
    cases.append(("in the middle of B", (other, np.ones(other.size, np.uint8)), (good, c)))
    # A empty: tile 0 is B[0 .. TILE), and B[TILE] is the halo behind its piece
    c = np.full(good.size, 3, np.uint8)
    c[TILE] = 0
    cases.append(("the halo count behind B's piece, A empty", none, (good, c)))
    # equal key lists: tile 0 takes TILE / 2 entries of each, and B[TILE / 2] is the halo behind B's piece -- the count that
    # the pair of A's last key of the tile would not read, since that key's pair lies inside the tile
    c = np.full(good.size, 3, np.uint8)
    c[TILE // 2] = 0
    cases.append(("the halo count behind B's piece, equal keys", (good, np.full(good.size, 5, np.uint8)), (good, c)))
    for name, a, b in cases:
        for op in OPS:
            e = _untouched_after(a, b, op, a[0].size + b[0].size + 8)
            assert "count of 0" in str(e) and e.needed == 0, (name, op)


def test_raw_refuses_a_bad_op_and_overlap():
    a, b = (u64(np.arange(10)), np.ones(10, np.uint8)), (u64(np.arange(5, 15)), np.ones(10, np.uint8))
    for op in (4, -1, 77):
        e = _untouched_after(a, b, op, 32)
        assert "op=" in str(e)
    dk = dev(np.arange(4 * TILE, dtype=np.uint64))
    dc = torch.ones(4 * TILE, dtype=torch.uint8, device="cuda")
    spare_k = torch.zeros(3 * TILE, dtype=torch.int64, device="cuda")
    spare_c = torch.zeros(3 * TILE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    args = (dk.data_ptr(), dc.data_ptr(), 2 * TILE, dk.data_ptr() + 8 * 3 * TILE, dc.data_ptr() + 3 * TILE, TILE, "add")
    for kout, cout in ((dk.data_ptr() + 8 * TILE, spare_c.data_ptr()),   # the key output inside the keys of A
                       (spare_k.data_ptr(), dc.data_ptr() + TILE),       # the count output inside the counts of A
                       (spare_k.data_ptr(), dc.data_ptr() + 3 * TILE)):  # ... and over the counts of B
        with pytest.raises(_lib.BrxError) as ei:
            combine_counts_device(*args, kout, cout, 3 * TILE)
        assert ei.value.status == _lib.BRX_ERR_ARG and "overlap" in str(ei.value)
    # keys against counts is no overlap the entry looks for; disjoint arrays pass
    n, _ = combine_counts_device(*args, spare_k.data_ptr(), spare_c.data_ptr(), 3 * TILE)
    assert n == 3 * TILE


# ---- stream order of the raw entry ---------------------------------------------------------------------------------------
def test_raw_entry_reads_its_inputs_in_stream_order(lane, reads):
    """the four arrays hold a decoy of identical sizes until the lane's delay has run: the answer is the real one's"""
    k = 13
    ka, ca = abundance.count_table([abundance.canonical_hashes(r, k) for r in reads[:24]])
    kb, cb = abundance.count_table([abundance.canonical_hashes(r, k) for r in reads[12:36]])
    real = {"ka": ka, "ca": ca.astype(np.uint8), "kb": kb, "cb": cb.astype(np.uint8)}
    rng = np.random.default_rng(9)
    fake = {"ka": _sample(rng, ka.size, 1 << (2 * k - 1)), "ca": rng.integers(1, 200, ka.size).astype(np.uint8),
            "kb": _sample(rng, kb.size, 1 << (2 * k - 1)), "cb": rng.integers(1, 200, kb.size).astype(np.uint8)}

    def op_combine(op):
        @operation(lambda arrays: {"k": (arrays["ka"].size + arrays["kb"].size, "int64"), "c": (arrays["ka"].size + arrays["kb"].size, "uint8")})
        def run(ctx, inp, out):
            n, s3 = combine_counts_device(ptr(inp["ka"]), ptr(inp["ca"]), inp["ka"].numel(), ptr(inp["kb"]), ptr(inp["cb"]),
                                          inp["kb"].numel(), op, ptr(out["k"]), ptr(out["c"]), out["k"].numel(), 1, ctx.stream)
            return n, s3, ctx.fetch(out["k"])[:n].tobytes(), ctx.fetch(out["c"])[:n].tobytes()
        return run

    for op in ("add", "sub"):
        n, s3, keys, counts = probe(lane, op_combine(op), fake, real)
        want_k, want_c = countops.combine(real["ka"], real["ca"], real["kb"], real["cb"], op)
        assert n == want_k.size > 100 and s3 == countops.sizes(ka, kb) and keys == want_k.tobytes() and counts == want_c.tobytes()


# ---- objects -------------------------------------------------------------------------------------------------------------
N_READS = 40  # of the fixture's reads: counts up to the tens, some 300 000 k-mers at k = 25 (150 tiles)


def _table(raw_reads, k, lo=0, hi=N_READS):
    """(keys, counts clipped at 255) of raw_reads[lo:hi], in numpy; computed once and never modified"""
    key = ("table", k, lo, hi)
    if key not in _cache:
        keys, counts = abundance.count_table([abundance.canonical_hashes(r, k) for r in raw_reads[lo:hi]])
        _cache[key] = (keys, np.minimum(counts, 255).astype(np.uint8))
    return _cache[key]


def _count_file(raw_reads, k, min_count=1, lo=0, hi=N_READS):
    keys, counts = _table(raw_reads, k, lo, hi)
    keep = counts >= min_count
    return keyfile.encode(k, keys[keep], counts[keep], floor=min_count)


def _counter(reads_, k, strategy=TABLE):
    cnt = br_amd.Counter(k, 0, strategy)
    cnt.add_reads(reads_)
    if strategy == SORTED:
        cnt.prepare_lookup()
    return cnt


def _saved(obj, *args):
    f = io.BytesIO()
    obj.save(f, *args)
    return f.getvalue()


def _list(data):
    return CountList.from_keyfile(io.BytesIO(data))


def _list_of(keys, counts, k, floor=1):
    return _list(keyfile.encode(k, keys, counts, floor=floor))


def _same(x, y):
    return all(np.array_equal(p, q) for p, q in zip(x, y))


@pytest.mark.parametrize("k", [11, 19, 25, 31])
def test_load_then_save_is_the_file(raw_reads, k):
    for floor in (1, 3):
        data = _count_file(raw_reads, k, floor)
        lst = _list(data)
        keys, counts = _table(raw_reads, k)
        assert (lst.k, lst.n, lst.floor, len(lst)) == (k, int((counts >= floor).sum()), floor, lst.n) and (floor == 3 or lst.n > 1000)
        assert lst.keyfile_stats["keys"] == lst.n and lst.keyfile_stats["bytes"] == len(data)
        assert _saved(lst) == data and _saved(lst, floor) == data
        assert _same(lst.to_numpy(), (keys[counts >= floor], counts[counts >= floor]))
        # a min_count above the floor: one compaction, and the file of that floor
        assert _saved(lst, 4) == _count_file(raw_reads, k, 4)
        assert _saved(lst) == data  # (the list is as it was)
        # the device arrays are the list: handed to the raw entry, they come back
        d_keys, d_counts, n = lst.device_arrays()
        assert n == lst.n and (n == 0 or (d_keys and d_counts))
        if n:
            kout = torch.zeros(n, dtype=torch.int64, device="cuda")
            cout = torch.zeros(n, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            assert combine_counts_device(d_keys, d_counts, n, None, None, 0, "add", kout.data_ptr(), cout.data_ptr(), n)[0] == n
            torch.cuda.synchronize()
            assert _same((kout.cpu().numpy().view(np.uint64), cout.cpu().numpy()), lst.to_numpy())


def test_empty_list():
    data = keyfile.encode(25, np.zeros(0, np.uint64), np.zeros(0, np.uint8), floor=1)
    lst = _list(data)
    assert (lst.k, lst.n, lst.floor) == (25, 0, 1) and lst.device_arrays() == (0, 0, 0) and _saved(lst) == data
    assert int(lst.spectrum()[0]) == 1 << 49 and not lst.spectrum()[1:].any()
    assert (lst + lst).n == 0 and lst.finish(0).popcount() == 0


@pytest.mark.parametrize("k,strategy", [(25, TABLE), (19, SORTED), (11, TABLE)])
def test_from_counter_lists_what_the_counter_saves(raw_reads, k, strategy):
    cnt = _counter(raw_reads[:N_READS], k, strategy)
    spectrum = cnt.spectrum() if strategy == TABLE else None  # (a partitioned counter's spectrum drops its view)
    for min_count in (1, 2):
        lst = CountList.from_counter(cnt, min_count)
        assert (lst.k, lst.floor) == (k, min_count)
        assert _saved(lst) == _saved(cnt, min_count) == _count_file(raw_reads, k, min_count)
    assert cnt.lookup_ready
    keys, counts = _table(raw_reads, k)
    fw = forward_kmers(keys[::97])
    assert np.array_equal(cnt.get_counts(fw), counts[::97])  # the counter answers what it answered
    if strategy == TABLE:
        assert np.array_equal(cnt.spectrum(), spectrum)
        # a floored counter hands its floor on
        floored = br_amd.Counter.from_keyfile(io.BytesIO(_count_file(raw_reads, k, 3)))
        assert CountList.from_counter(floored).floor == 3 and CountList.from_counter(floored, 5).floor == 5
        assert _saved(CountList.from_counter(floored, 2)) == _count_file(raw_reads, k, 3)


def test_from_counter_refusals(raw_reads):
    for cnt, word in ((br_amd.Counter(11, 0, DENSE), "dense"), (br_amd.Counter(19, 0, SORTED), "brx_counter_lookup_prepare")):
        cnt.add_reads(raw_reads[:5])
        with pytest.raises(_lib.BrxError) as ei:
            CountList.from_counter(cnt)
        assert ei.value.status == _lib.BRX_ERR_UNSUPPORTED and word in str(ei.value)


@pytest.mark.parametrize("k,strategy", [(11, TABLE), (19, SORTED), (25, TABLE)])
def test_shards_added_are_the_whole_job(raw_reads, k, strategy):
    """the reads split three ways and counted apart; the lists added left to right and saved: byte for byte the file of one
    counter that counted everything (k = 19: partitioned counters, their count views)"""
    cuts = [(0, 12), (12, 30), (30, N_READS)]
    whole = _saved(_counter(raw_reads[:N_READS], k, strategy))
    assert whole == _count_file(raw_reads, k)
    shards = []
    for i, (lo, hi) in enumerate(cuts):
        cnt = _counter(raw_reads[lo:hi], k, strategy)
        shards.append(CountList.from_counter(cnt) if i % 2 == 0 else _list(_saved(cnt)))  # both ways into a list
    before = [s.to_numpy() for s in shards]
    total = shards[0] + shards[1] + shards[2]
    assert total.floor == 1 and _saved(total) == whole
    assert _saved(shards[0].add(shards[1]).add(shards[2], min_count=2), 1) == _count_file(raw_reads, k, 2)
    st = (shards[0] + shards[1]).combine_stats
    assert (st["a"], st["b"], st["both"]) == countops.sizes(before[0][0], before[1][0]) and st["entries"] == st["a"] + st["b"] - st["both"]
    assert all(_same(s.to_numpy(), b) for s, b in zip(shards, before))


@pytest.mark.parametrize("k", [11, 25])
def test_operations_against_numpy_and_operands_unchanged(raw_reads, k):
    a_np, b_np = _table(raw_reads, k, 0, 26), _table(raw_reads, k, 16, N_READS)
    a, b = _list_of(*a_np, k), _list_of(*b_np, k)
    assert 0 < countops.sizes(a_np[0], b_np[0])[2] < min(a.n, b.n)
    for op, method in (("add", a.add), ("max", a.maximum), ("min", a.minimum), ("sub", a.subtract)):
        for mc in (1, 2):
            res = method(b, mc)
            want = countops.combine(*a_np, *b_np, op, mc)
            assert (res.k, res.n, res.floor) == (k, want[0].size, mc) and _same(res.to_numpy(), want), (op, mc)
            assert _same(a.combine(b, countops.OPS[op], mc).to_numpy(), want)
    assert _same((a - b).to_numpy(), countops.combine(*a_np, *b_np, "sub")) and _same((b - a).to_numpy(), countops.combine(*b_np, *a_np, "sub"))
    # a list with itself
    assert _same((a + a).to_numpy(), (a_np[0], np.minimum(2 * a_np[1].astype(int), 255).astype(np.uint8)))
    assert _same(a.maximum(a).to_numpy(), a_np) and _same(a.minimum(a).to_numpy(), a_np)
    assert _same(a.to_numpy(), a_np) and _same(b.to_numpy(), b_np)  # only read
    with pytest.raises(TypeError):
        a.combine(br_amd.Pcon.new(k), "add")
    with pytest.raises(ValueError):
        a.combine(b, "plus")
    assert a.__add__(3) is NotImplemented


@pytest.mark.parametrize("k", [11, 25])
def test_sub_from_itself_is_an_empty_list(raw_reads, k):
    a = _list(_count_file(raw_reads, k))
    none = a - a
    assert none.n == 0 and none.floor == 1 and _saved(none) == keyfile.encode(k, np.zeros(0, np.uint64), np.zeros(0, np.uint8), floor=1)
    s = none.finish(0)
    model = br_amd.Pcon.from_keyfile(io.BytesIO(keyfile.encode(k, np.zeros(0, np.uint64))))
    assert s.k() == k and s.popcount() == 0 and s.fingerprint() == fingerprint_of(np.zeros(0, np.uint64))
    assert (s.bits_state(), s.is_sparse()) == (model.bits_state(), model.is_sparse())
    assert not s.get_many(forward_kmers(_table(raw_reads, k)[0][:300])).any()
    assert _saved(none + a) == _saved(a)  # an empty list is a list like any other


@pytest.mark.parametrize("k", [11, 25])
def test_spectrum_is_the_table_counters(raw_reads, k):
    for floor in (1, 3):
        data = _count_file(raw_reads, k, floor)
        lst, cnt = _list(data), br_amd.Counter.from_keyfile(io.BytesIO(data))
        keys, counts = _table(raw_reads, k)
        got = lst.spectrum()
        assert got.dtype == np.uint64 and np.array_equal(got, cnt.spectrum())
        assert np.array_equal(got, countops.spectrum(k, counts[counts >= floor], floor)) and int(got[3:].sum()) > 0
        assert not got[1:floor].any()
    # every count value, and a length that is no multiple of the 16 bytes a lane loads at once
    rng = np.random.default_rng(k)
    counts = np.concatenate([np.arange(1, 256), rng.integers(1, 256, 70001)]).astype(np.uint8)
    keys = np.sort(rng.choice(1 << 21, size=counts.size, replace=False)).astype(np.uint64)
    assert np.array_equal(_list_of(keys, counts, k).spectrum(), countops.spectrum(k, counts))


def _check_finished(res, k, want, model, others):
    assert res.k() == k and res.popcount() == want.size and res.fingerprint() == fingerprint_of(want)
    assert (res.bits_state(), res.is_sparse()) == (model.bits_state(), model.is_sparse()) == ((2, True) if k >= 21 else (0, False))
    info, minfo = res.index_info(), model.index_info()
    assert (info["keylist"], info["wanted"]) == (minfo["keylist"], minfo["wanted"])
    if k >= 21:
        assert info["valid"] and info["keys"] == want.size
    rng = np.random.default_rng(k)
    members = want[:: max(want.size // 500, 1)]
    outside = np.setdiff1d(np.concatenate([others[:: max(others.size // 500, 1)], others[:: max(others.size // 500, 1)] ^ np.uint64(1),
                                           rng.integers(0, 1 << (2 * k - 1), 500, dtype=np.uint64)]), want)
    assert res.get_many(forward_kmers(members)).all()
    assert not res.get_many(forward_kmers(outside)).any() and outside.size >= 400


@pytest.mark.parametrize("k", [11, 15, 25])
def test_finish_is_the_counters_finish(raw_reads, solid_fixture_bytes, k):
    data = _count_file(raw_reads, k)
    lst, cnt = _list(data), br_amd.Counter.from_keyfile(io.BytesIO(data))
    keys, counts = _table(raw_reads, k)
    for a in (0, 2, 254):
        want = countops.select(keys, counts, a)
        res = lst.finish(a)
        assert (res.finish_stats["entries"], res.finish_stats["kept"]) == (keys.size, want.size)
        assert res.fingerprint() == cnt.finish(a).fingerprint()
        model = br_amd.Pcon.from_keyfile(io.BytesIO(keyfile.encode(k, want)))
        _check_finished(res, k, want, model, keys)
        if k <= 15:
            assert res.to_solid_bytes() == solid_bytes_of(k, want)
    assert lst.finish(255).popcount() == 0
    assert _saved(lst) == data  # only read
    if k == 11:  # every read of the fixture, in two shards: the reference's own set
        whole = _list(_count_file(raw_reads, k, 1, 0, 150)) + _list(_count_file(raw_reads, k, 1, 150, None))
        assert whole.finish(2).to_solid_bytes() == solid_fixture_bytes


def test_floor_rules(raw_reads):
    k = 25
    full, b_np = _table(raw_reads, k, 0, 28), _table(raw_reads, k, 16, N_READS)
    keep = full[1] >= 3
    a3_np = (full[0][keep], full[1][keep])
    a3, b1, afull = _list_of(*a3_np, k, 3), _list_of(*b_np, k), _list_of(*full, k)
    assert (a3.floor, b1.floor) == (3, 1) and 100 < a3.n < afull.n
    for op in ("max", "min", "sub"):
        assert countops.result_floor(op, 3, 1) == 3
        res = a3.combine(b1, op)
        want = countops.combine(*a3_np, *b_np, op, 3)
        assert res.floor == 3 and _same(res.to_numpy(), want) and want[0].size > 10, op
        # exact: what the unfloored list gives from 3 up
        assert _same(res.to_numpy(), countops.combine(*full, *b_np, op, 3)), op
        assert _same(afull.combine(b1, op, 3).to_numpy(), want), op
        assert a3.combine(b1, op, 5).floor == 5 and _same(a3.combine(b1, op, 5).to_numpy(), countops.combine(*full, *b_np, op, 5))
        assert a3.combine(b1, op, 2).floor == 3  # min_count below the floor changes nothing
    for op in ("max", "min"):
        res = b1.combine(a3, op)
        assert res.floor == 3 and _same(res.to_numpy(), countops.combine(*b_np, *full, op, 3))
    for call, word in ((lambda: b1 - a3, "subtract"), (lambda: a3 + b1, "adding"), (lambda: b1 + a3, "adding"), (lambda: a3 + a3, "adding")):
        with pytest.raises(_lib.BrxError) as ei:
            call()
        assert ei.value.status == _lib.BRX_ERR_ARG and word in str(ei.value) and "3" in str(ei.value)
    for op in ("sub", "add"):
        with pytest.raises(ValueError):
            countops.result_floor(op, 1, 3)
    # finish below the floor
    for a in (0, 1):
        with pytest.raises(_lib.BrxError) as ei:
            a3.finish(a)
        assert ei.value.status == _lib.BRX_ERR_ARG
    assert a3.finish(2).fingerprint() == afull.finish(2).fingerprint() == fingerprint_of(a3_np[0])
    assert _same(a3.to_numpy(), a3_np) and _same(b1.to_numpy(), b_np)


def test_refused_operands_and_files(raw_reads):
    a11, a15 = _list(_count_file(raw_reads, 11, 1, 0, 10)), _list(_count_file(raw_reads, 15, 1, 0, 10))
    with pytest.raises(_lib.BrxError) as ei:
        a11 + a15
    assert ei.value.status == _lib.BRX_ERR_ARG and "k = 11" in str(ei.value) and "k = 15" in str(ei.value)
    with pytest.raises(_lib.BrxError) as ei:  # a set file
        _list(keyfile.encode(11, _table(raw_reads, 11)[0]))
    assert ei.value.status == _lib.BRX_ERR_FORMAT and "set file" in str(ei.value)
    h = _lib.C.c_void_p(0x1234)
    r, w = os.pipe()
    os.write(w, keyfile.encode(11, _table(raw_reads, 11)[0])[:4096])
    os.close(w)
    assert _lib.lib().brx_counts_load_fd(r, 0, _lib.C.byref(h), None) == _lib.BRX_ERR_FORMAT and h.value is None
    os.close(r)
    bad = {name: (data, word) for name, data, word in _bad_files()}
    for name in ("truncated", "key sum", "trailing", "magic"):
        data, word = bad[name]
        with pytest.raises(_lib.BrxError) as ei:
            _list(data)
        assert ei.value.status == _lib.BRX_ERR_FORMAT and word in str(ei.value), name
        # the counter's own refusal, word for word up to what it adds about itself
        with pytest.raises(_lib.BrxError) as ec:
            br_amd.Counter(9, 0, TABLE).load(io.BytesIO(data))
        assert str(ec.value).startswith(str(ei.value)), name
        h = _lib.C.c_void_p(0x1234)
        r, w = os.pipe()
        os.write(w, data)
        os.close(w)
        assert _lib.lib().brx_counts_load_fd(r, 0, _lib.C.byref(h), None) == _lib.BRX_ERR_FORMAT and h.value is None, name
        os.close(r)


def test_gzip_file_and_pipe(raw_reads, tmp_path):
    k = 25
    want = _count_file(raw_reads, k)
    lst = _list(want)
    path = str(tmp_path / "counts.keys.gz")
    with gzip.open(path, "wb") as f:
        lst.save(f)
    assert gzip.open(path, "rb").read() == want
    with gzip.open(path, "rb") as f:
        assert _saved(CountList.from_keyfile(f)) == want
    plain = str(tmp_path / "counts.keys")
    with open(plain, "wb") as f:
        lst.save(f)
    with open(plain, "rb") as f:
        assert _saved(CountList.from_keyfile(f)) == want
    # a pipe: the library writes to / reads from the descriptor itself
    r, w = os.pipe()
    got = []
    t = threading.Thread(target=lambda: got.append(os.fdopen(r, "rb").read()))
    t.start()
    with os.fdopen(w, "wb") as wf:
        lst.save(wf)
    t.join()
    assert got[0] == want
    r, w = os.pipe()

    def feed():
        with os.fdopen(w, "wb") as wf:
            wf.write(want)

    t = threading.Thread(target=feed)
    t.start()
    h, st = _lib.C.c_void_p(), (_lib.C.c_uint64 * 8)()
    _lib.check(_lib.lib().brx_counts_load_fd(r, 0, _lib.C.byref(h), st))
    os.close(r)
    t.join()
    back = CountList(h.value, 0)
    assert int(st[0]) == back.n == _table(raw_reads, k)[0].size and int(st[1]) == len(want) and _saved(back) == want


# ---- correction through a set finished from an added list -----------------------------------------------------------------
def test_k21_added_lists_correct_like_the_oracle(raw_reads):
    k = 21
    keys, counts = abundance.count_table([abundance.canonical_hashes(r, k) for r in raw_reads])
    want = keys[counts > 1]
    a = CountList.from_counter(_counter(raw_reads[:150], k))
    b = CountList.from_counter(_counter(raw_reads[150:], k))
    gs = (a + b).finish(1)
    assert gs.fingerprint() == fingerprint_of(want) and want.size > 1000 and gs.is_sparse()
    ref = O.Solid(k, _h=O.lib().bro_solid_new_sparse(k, want.ctypes.data, want.size))
    sub = raw_reads[:30]
    changed = 0
    for method in ("one", "graph"):
        om = O.build_methods(ref, [method], 5, 7)
        got = br_amd.Chain(gs, [(method, 5, 7)], two_side=False).correct_reads(sub)
        assert got == [O.correct_record(om, r, False) for r in sub], method
        changed += sum(g != r for g, r in zip(got, sub))
    assert changed >= 1  # (a set that nobody asks, or an empty one, changes no read: the comparison above would prove nothing)


# ---- command line --------------------------------------------------------------------------------------------------------
def _write(path, data, zipped=False):
    with (gzip.open(path, "wb") if zipped else open(path, "wb")) as f:
        f.write(data)
    return path


def test_cli_counts_flags(tmp_path, golden_dir, raw_reads):
    from br_amd import cli
    k = 15
    raw = os.path.join(golden_dir, "raw.fasta")
    p = lambda name: str(tmp_path / name)
    a_np, b_np, c_np = _table(raw_reads, k, 0, 24), _table(raw_reads, k, 24, N_READS), _table(raw_reads, k, 8, 14)
    _write(p("a.keys"), keyfile.encode(k, *a_np, floor=1))
    _write(p("b.keys.gz"), keyfile.encode(k, *b_np, floor=1), zipped=True)
    _write(p("c.keys"), keyfile.encode(k, *c_np, floor=1))
    common = ["-i", raw, "-c", "one", "-s"]
    assert cli.main(common + ["-o", p("1.fa"), "count", "-i", p("a.keys"), "--counts-add", p("b.keys.gz"), "--counts-minus", p("c.keys"),
                              "-a", "2", "--save-counts", p("out.keys")]) == 0
    want = countops.combine(*countops.combine(*a_np, *b_np, "add"), *c_np, "sub")
    assert open(p("out.keys"), "rb").read() == keyfile.encode(k, *want, floor=1) and want[0].size > 1000
    # the python composition: the same file, the same set, the same corrected reads
    lst = (_list(keyfile.encode(k, *a_np, floor=1)) + _list(keyfile.encode(k, *b_np, floor=1))) - _list(keyfile.encode(k, *c_np, floor=1))
    assert _saved(lst) == open(p("out.keys"), "rb").read()
    solid = lst.finish(2)
    assert solid.fingerprint() == fingerprint_of(countops.select(*want, 2))
    with open(p("set.keys"), "wb") as f:
        solid.save_keys(f)
    assert cli.main(common + ["-o", p("2.fa"), "solid", "-i", p("set.keys"), "-f", "keys"]) == 0
    assert open(p("1.fa"), "rb").read() == open(p("2.fa"), "rb").read() and os.path.getsize(p("1.fa")) > 1000
    # the order of the flags is the order applied; a threshold selector reads the list's spectrum; --save-min-count
    assert cli.main(common + ["-o", p("3.fa"), "--save-counts", p("out3.keys"), "--save-min-count", "2", "count", "-i", p("a.keys"),
                              "--counts-minus", p("c.keys"), "--counts-add", p("b.keys.gz"), "first-minimum"]) == 0
    want3 = countops.combine(*countops.combine(*a_np, *c_np, "sub"), *b_np, "add", 2)
    assert open(p("out3.keys"), "rb").read() == keyfile.encode(k, *want3, floor=2) != open(p("out.keys"), "rb").read()
    # refusals
    with pytest.raises(SystemExit) as ei:
        cli.main(common + ["-o", p("x.fa"), "--abundance-report", p("x.tsv"), "count", "-i", p("a.keys"), "--counts-add", p("c.keys"), "-a", "2"])
    assert "--abundance-report" in str(ei.value) and "lookups" in str(ei.value) and not os.path.exists(p("x.tsv"))
    table = bytes([11]) + np.asarray(O.count_reads(11, raw_reads[:5]), dtype=np.uint8).tobytes()
    _write(p("table.pcon"), table)
    with pytest.raises(SystemExit) as ei:
        cli.main(common + ["-o", p("y.fa"), "count", "-i", p("table.pcon"), "--counts-add", p("c.keys"), "-a", "2"])
    assert str(ei.value).startswith("Error: count -i %s: not a key file" % p("table.pcon"))
    _write(p("k11.keys"), _count_file(raw_reads, 11, 1, 0, 5))
    with pytest.raises(SystemExit) as ei:
        cli.main(common + ["-o", p("z.fa"), "count", "-i", p("a.keys"), "--counts-max", p("k11.keys"), "-a", "2"])
    assert str(ei.value) == "Error: --counts-max %s: k = 11, the counts in use have k = 15" % p("k11.keys")
    _write(p("cut.keys"), keyfile.encode(k, *c_np, floor=1)[:-3])
    with pytest.raises(SystemExit) as ei:
        cli.main(common + ["-o", p("w.fa"), "count", "-i", p("a.keys"), "--counts-min", p("cut.keys"), "-a", "2"])
    assert str(ei.value).startswith("Error: --counts-min %s: " % p("cut.keys")) and "truncated" in str(ei.value)
