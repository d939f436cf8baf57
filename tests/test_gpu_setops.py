"""Set algebra on the GPU path (include/brx.h "set algebra", br_amd/csrc/brx_setops.hip): the merge of two sorted key lists
against br_amd/setops.py at the shapes where a merge can go wrong, sets combined from every form that holds one, correction
through a combined set against the oracle, stream order of the raw entry and the command line.  Every comparison is exact."""
import gzip
import io
import os

import numpy as np
import pytest
import torch

import br_amd
from br_amd import _lib, abundance, keyfile, setops
from br_amd.set import combine_keys_device
from oracle import oracle as O
from tests.test_gpu_streams import Lane, decoy, fingerprint_of, lane, operation, probe, ptr, reads, solid_bytes_of  # noqa: F401

pytestmark = pytest.mark.gpu

TILE, PT = setops.TILE, setops.PER_THREAD
TOP = (1 << 61) - 1
OPS = list(setops.OPS)
SENTINEL = -0x1111111111111112  # 0xEEEE... as int64
METHODS = ["one", "two", "graph", "greedy", "gap_size"]
_cache = {}


def u64(values):
    return np.ascontiguousarray(np.asarray(values, dtype=np.uint64))


def dev(a):
    return torch.from_numpy(u64(a).view(np.int64).copy()).cuda()


def run_raw(a, b, op, cap=None, stream=None):
    """(result, sizes3, the whole output array) of the raw entry; the output array is filled with the sentinel first"""
    da, db = dev(a), dev(b)
    cap = a.size + b.size + 8 if cap is None else cap
    out = torch.full((max(cap, 1),), SENTINEL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    n, s3 = combine_keys_device(da.data_ptr() if a.size else None, a.size, db.data_ptr() if b.size else None, b.size, op,
                                out.data_ptr(), cap, stream)
    torch.cuda.synchronize()
    whole = out.cpu().numpy()
    return whole[:n].view(np.uint64), s3, whole


def check_raw(name, a, b):
    a, b = u64(a), u64(b)
    for op in OPS:
        want = setops.combine(a, b, op)
        got, s3, whole = run_raw(a, b, op)
        assert got.size == want.size and np.array_equal(got, want), (name, op)
        assert s3 == setops.sizes(a, b), (name, op)
        assert (whole[want.size:] == SENTINEL).all(), (name, op, "written behind the result")


# ---- raw entry: shapes ---------------------------------------------------------------------------------------------------
def _sample(rng, n, hi):
    return np.sort(rng.choice(hi, size=n, replace=False)).astype(np.uint64)


@pytest.mark.parametrize("total", [0, 1, 2, PT - 1, PT + 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
def test_raw_sizes_around_thread_and_tile(total):
    rng = np.random.default_rng(total)
    for na in sorted({0, total // 3, total // 2, total}):
        nb = total - na
        hi = max(2 * total, 4)  # about half of the smaller list is in the other one
        check_raw((total, na), _sample(rng, na, hi), _sample(rng, nb, hi))


def pairs_on_diagonals(n_pos, shift):
    """two lists whose merge has an equal pair -- the key of A, then the key of B -- at positions (m - 1 + shift, m + shift)
    for every multiple m of PER_THREAD: across every thread's diagonal and across the tile edges for shift 0, just behind
    them for shift 1"""
    a, b, key, pos = [], [], 5, 0
    while pos < n_pos:
        if (pos + 1 - shift) % PT == 0 and pos + 1 < n_pos:
            a.append(key)
            b.append(key)
            pos += 2
        else:
            (a if key % 2 else b).append(key)
            pos += 1
        key += 3
    return u64(a), u64(b)


def _shape_cases():
    n = TILE + 100
    ar = np.arange
    yield "b empty", ar(TILE + 3), []
    yield "a empty", [], ar(2 * TILE + 1)
    yield "a below b", ar(n), ar(n) + 10 * n
    yield "b below a", ar(n) + 10 * n, ar(n)
    yield "a == b", ar(0, 3 * (TILE + 17), 3), ar(0, 3 * (TILE + 17), 3)
    yield "a inside b", ar(2 * TILE + 9)[::5], ar(2 * TILE + 9)
    yield "b inside a", ar(2 * TILE + 9), ar(2 * TILE + 9)[::7]
    yield "interleave", ar(0, 2 * TILE + 6, 2), ar(1, 2 * TILE + 6, 2)
    for shift in (0, 1):
        a, b = pairs_on_diagonals(2 * TILE + PT, shift)
        yield f"pairs on the diagonals, shift {shift}", a, b
        yield f"pairs on the diagonals, shift {shift}, lists swapped", b, a
    run = ar(2 * TILE) + 10
    yield "a run of equal pairs", np.concatenate([[1, 3], run]), np.concatenate([[2], run, [10 + 2 * TILE + 5]])
    yield "ends of the key range", [0, 5, TOP], [0, TOP - 1, TOP]
    yield "ends of the key range, long", np.concatenate([[0], ar(TILE) + 9, [TOP]]), np.concatenate([[0, 3], ar(0, TILE, 2) + 9, [TOP - 1, TOP]])


@pytest.mark.parametrize("name,a,b", list(_shape_cases()), ids=[c[0] for c in _shape_cases()])
def test_raw_shapes(name, a, b):
    if name == "pairs on the diagonals, shift 0":
        # the construction itself: A's key at the last position of every thread's share, B's equal key at the next one
        merged = np.sort(np.concatenate([u64(a), u64(b)]), kind="stable")
        m = np.arange(PT, merged.size - 1, PT)
        assert (merged[m - 1] == merged[m]).all() and m.size >= 2 * 256 and TILE in m
    check_raw(name, a, b)


def test_raw_one_array_for_both_inputs():
    a = u64(np.arange(0, 3 * TILE, 2))
    da = dev(a)
    out = torch.full((a.size,), SENTINEL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for op in OPS:
        n, s3 = combine_keys_device(da.data_ptr(), a.size, da.data_ptr(), a.size, op, out.data_ptr(), a.size)
        assert s3 == (a.size, a.size, a.size)
        assert n == (a.size if op in ("union", "intersection") else 0)
        if n:
            assert np.array_equal(out.cpu().numpy().view(np.uint64), a)


# ---- raw entry: refusals -------------------------------------------------------------------------------------------------
def _refused(a, b, op, cap):
    with pytest.raises(_lib.BrxError) as ei:
        run_raw(u64(a), u64(b), op, cap)
    assert ei.value.status == _lib.BRX_ERR_ARG
    return ei.value


def _untouched_after(a, b, op, cap):
    """the refusal, and the sentinel still everywhere in d_out"""
    da, db = dev(a), dev(b)
    out = torch.full((max(cap, 1),), SENTINEL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(_lib.BrxError) as ei:
        combine_keys_device(da.data_ptr() if len(a) else None, len(a), db.data_ptr() if len(b) else None, len(b), op, out.data_ptr(), cap)
    torch.cuda.synchronize()
    assert ei.value.status == _lib.BRX_ERR_ARG
    assert (out.cpu().numpy() == SENTINEL).all()
    return ei.value


def test_raw_cap_too_small_and_sizes_only():
    rng = np.random.default_rng(5)
    a, b = _sample(rng, TILE + 9, 3 * TILE), _sample(rng, TILE - 4, 3 * TILE)
    for op in OPS:
        want = setops.combine(a, b, op)
        assert want.size > 1
        e = _untouched_after(a, b, op, want.size - 1)
        assert e.needed == want.size and str(want.size) in str(e)
        # the size-only form
        da, db = dev(a), dev(b)
        torch.cuda.synchronize()
        n, s3 = combine_keys_device(da.data_ptr(), a.size, db.data_ptr(), b.size, op, None, 0)
        assert n == want.size and s3 == setops.sizes(a, b)
        # and exactly enough room is enough
        got, _, _ = run_raw(a, b, op, want.size)
        assert np.array_equal(got, want)
    with pytest.raises(_lib.BrxError) as ei:  # a capacity without an array
        combine_keys_device(dev(a).data_ptr(), a.size, dev(b).data_ptr(), b.size, "union", None, 5)
    assert ei.value.status == _lib.BRX_ERR_ARG


def _broken_inputs():
    good = np.arange(0, 6 * TILE, 2, dtype=np.uint64)  # 3 tiles' worth
    other = np.arange(1, 2 * TILE, 3, dtype=np.uint64)
    x = good.copy()
    x[1000], x[1001] = good[1001], good[1000]
    yield "two keys swapped", x, other
    x = good.copy()
    x[777] = x[776]
    yield "a key twice", x, other
    x = good.copy()
    x[-1] = 0
    yield "the last key small", x, other
    x = good.copy()
    x[0] = TOP
    yield "the first key large", x, other
    # with the other list empty, tile t of the merge is keys [TILE t, TILE t + TILE) of this one: the pair (TILE - 1, TILE) lies
    # across the edge of tiles 0 and 1 -- the second key meets the first one only as its halo
    x = good.copy()
    x[TILE] = x[TILE - 1]
    yield "a key twice across a tile edge", x, np.zeros(0, dtype=np.uint64)
    x = good.copy()
    x[2 * TILE - 1] = x[2 * TILE] + 1
    yield "descending across a tile edge", x, np.zeros(0, dtype=np.uint64)
    yield "random keys", np.random.default_rng(2).integers(0, 1 << 40, 5 * TILE, dtype=np.uint64), other


@pytest.mark.parametrize("name,bad,other", list(_broken_inputs()), ids=[c[0] for c in _broken_inputs()])
def test_raw_refuses_unordered_and_repeated_keys(name, bad, other):
    for op in OPS:
        for a, b in ((bad, other), (other, bad)):
            e = _untouched_after(a, b, op, a.size + b.size + 8)
            assert "ascend" in str(e) and e.needed == 0, (name, op)


def test_raw_refuses_a_bad_op_and_overlap():
    a, b = u64(np.arange(10)), u64(np.arange(5, 15))
    for op in (4, -1, 77):
        e = _untouched_after(a, b, op, 32)
        assert "op=" in str(e)
    da = dev(np.arange(4 * TILE))
    with pytest.raises(_lib.BrxError) as ei:  # the output inside input A
        combine_keys_device(da.data_ptr(), 2 * TILE, da.data_ptr() + 8 * 3 * TILE, TILE, "union", da.data_ptr() + 8 * TILE, 3 * TILE)
    assert ei.value.status == _lib.BRX_ERR_ARG and "overlap" in str(ei.value)


# ---- grid trips ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [1, 3, 7])
def test_raw_blocks_loop_over_tiles(monkeypatch, grid):
    """41 tiles through 1, 3 and 7 blocks (and through the grid's own cap in every other test)"""
    monkeypatch.setenv("BRX_READ_GRID", str(grid))
    if "trips" not in _cache:
        rng = np.random.default_rng(40)
        n = 40 * TILE + 77
        _cache["trips"] = (_sample(rng, n // 2, 2 * n), _sample(rng, n - n // 2, 2 * n))
    check_raw(("grid", grid), *_cache["trips"])


# ---- sets in every form --------------------------------------------------------------------------------------------------
def _table(raw_reads, k, lo, hi):
    key = ("table", k, lo, hi)
    if key not in _cache:
        _cache[key] = abundance.count_table([abundance.canonical_hashes(r, k) for r in raw_reads[lo:hi]])
    return _cache[key]


def _solid_keys(raw_reads, k, a, lo, hi):
    keys, counts = _table(raw_reads, k, lo, hi)
    return keys[counts > a]


def from_keys(k, keys):
    return br_amd.Pcon.from_keyfile(io.BytesIO(keyfile.encode(k, keys)))


def keys_of_set(s):
    f = io.BytesIO()
    s.save_keys(f)
    k, keys, counts, _ = keyfile.decode(f.getvalue())
    assert k == s.k() and counts is None
    return keys


def forward_kmers(keys):
    """a forward k-mer whose canonical form >> 1 is the key: the canonical form is the one of even parity"""
    x = u64(keys) << np.uint64(1)
    parity = np.zeros(x.size, dtype=np.uint64)
    for shift in range(64):
        parity ^= (x >> np.uint64(shift)) & np.uint64(1)
    return x | parity


def state_of(s):
    fp = s.fingerprint()
    return fp, s.bits_state(), s.is_sparse(), s.index_info()


def operands(raw_reads, solid_fixture_bytes, k):
    """[(form, set, its sorted keys in numpy)] -- three sets of this k held in different ways, overlapping pairwise"""
    if k == 11:
        bits = np.unpackbits(np.frombuffer(solid_fixture_bytes, dtype=np.uint8)[1:], bitorder="little")
        pres = _table(raw_reads, k, 0, 10)[0]
        return [("solid bytes", br_amd.Pcon.from_pcon_solid(solid_fixture_bytes), np.flatnonzero(bits).astype(np.uint64)),
                ("key file", from_keys(k, pres), pres),
                ("dense count", br_amd.Pcon.from_count(raw_reads[20:60], k, 1, strategy=_lib.COUNT_DENSE), _solid_keys(raw_reads, k, 1, 20, 60))]
    if k == 15:
        kb = _solid_keys(raw_reads, k, 1, 100, 200)
        kc = _table(raw_reads, k, 140, 160)[0]
        return [("lazy", br_amd.Pcon.from_count(raw_reads[:150], k, 2), _solid_keys(raw_reads, k, 2, 0, 150)),
                ("solid bytes", br_amd.Pcon.from_pcon_solid(solid_bytes_of(k, kb)), kb),
                ("key file", from_keys(k, kc), kc)]
    if k == 19:
        kb = _solid_keys(raw_reads, k, 1, 100, 200)
        return [("lazy", br_amd.Pcon.from_count(raw_reads[:150], k, 2), _solid_keys(raw_reads, k, 2, 0, 150)),
                ("key file", from_keys(k, kb), kb),
                ("inserted bits", br_amd.Pcon.from_fasta(raw_reads[140:150], k), _table(raw_reads, k, 140, 150)[0])]
    kc = _solid_keys(raw_reads, k, 1, 100, 200)
    return [("sparse counted", br_amd.Pcon.from_count(raw_reads[:150], k, 1), _solid_keys(raw_reads, k, 1, 0, 150)),
            ("sparse inserted", br_amd.Pcon.from_fasta(raw_reads[120:170], k), _table(raw_reads, k, 120, 170)[0]),
            ("key file", from_keys(k, kc), kc)]


def check_result(res, k, want, others, model):
    """a combined set against the numpy keys `want`; others: keys of the operands (the non-members worth asking about);
    model: a from_keyfile set of this k, whose form the result must have"""
    assert res.k() == k
    assert np.array_equal(keys_of_set(res), want)
    assert res.fingerprint() == fingerprint_of(want)
    assert res.popcount() == want.size
    assert (res.bits_state(), res.is_sparse()) == (model.bits_state(), model.is_sparse()) == ((2, True) if k >= 21 else (0, False))
    info, minfo = res.index_info(), model.index_info()
    assert (info["keylist"], info["wanted"]) == (minfo["keylist"], minfo["wanted"])
    if k >= 21:
        assert info["valid"] and info["keys"] == want.size
    rng = np.random.default_rng(k)
    members = want[:: max(want.size // 500, 1)]
    outside = np.setdiff1d(np.concatenate([o[:: max(o.size // 500, 1)] for o in others] +
                                          [rng.integers(0, 1 << (2 * k - 1), 500, dtype=np.uint64)]), want)
    assert res.get_many(forward_kmers(members)).all()
    assert not res.get_many(forward_kmers(outside)).any() and outside.size >= 400
    if k <= 15:  # (the .solid stream of k = 19 is 16 GiB of host memory: its bits are asked about above instead)
        assert res.to_solid_bytes() == solid_bytes_of(k, want)


@pytest.mark.parametrize("k", [11, 15, 19, 21, 25, 31])
def test_sets_in_every_form(raw_reads, solid_fixture_bytes, k):
    assert int(O.khash(int(forward_kmers([12345])[0]), k)) == 12345
    sets = operands(raw_reads, solid_fixture_bytes, k)
    forms = [s.bits_state() for _, s, _ in sets]
    assert forms == {11: [0, 0, 0], 15: [1, 0, 0], 19: [1, 0, 0]}.get(k, [2, 2, 2])  # current, lazy, sparse
    before = [state_of(s) for _, s, _ in sets]
    for (_, s, keys), st in zip(sets, before):
        assert st[0] == fingerprint_of(keys) and keys.size > 1000
    model = from_keys(k, sets[0][2][:100])
    for i in range(3):
        (fa, a, ka), (fb, b, kb) = sets[i], sets[(i + 1) % 3]
        assert 0 < setops.sizes(ka, kb)[2] < min(ka.size, kb.size), (fa, fb)
        cmp = a.compare(b)
        na, nb, both = setops.sizes(ka, kb)
        assert cmp == {"a": na, "b": nb, "both": both, "jaccard": both / (na + nb - both)}
        for op in OPS:
            res = a.combine(b, op)
            want = setops.combine(ka, kb, op)
            check_result(res, k, want, [ka, kb], model)
            st = res.combine_stats
            assert (st["a"], st["b"], st["both"], st["keys"]) == (na, nb, both, want.size), (fa, fb, op)
    # the operands are as they were: the lazy one still lazy, index and key list in place, the same members
    assert [state_of(s) for _, s, _ in sets] == before


@pytest.mark.parametrize("k", [11, 25])
def test_empty_results_and_operands(raw_reads, k):
    ka = _table(raw_reads, k, 0, 10)[0]
    a = from_keys(k, ka)
    model = from_keys(k, ka[:10])
    none = np.zeros(0, dtype=np.uint64)
    empty = br_amd.Pcon.new(k)
    low, high = from_keys(k, ka[: ka.size // 2]), from_keys(k, ka[ka.size // 2:])
    cases = [(a - a, none), (a ^ a, none), (low & high, none), (empty & a, none), (a & empty, none), (empty | empty, none),
             (empty - a, none), (a | empty, ka), (empty | a, ka), (a - empty, ka), (empty ^ a, ka), (a | a, ka), (a & a, ka),
             (low | high, ka), (low ^ high, ka), (a - low, ka[ka.size // 2:])]
    for i, (res, want) in enumerate(cases):
        assert np.array_equal(keys_of_set(res), want), i
        assert res.fingerprint() == fingerprint_of(want) and res.popcount() == want.size
        assert (res.bits_state(), res.is_sparse()) == (model.bits_state(), model.is_sparse())
        gone = np.setdiff1d(ka, want)[:300]
        assert not gone.size or not res.get_many(forward_kmers(gone)).any()
        assert not want.size or res.get_many(forward_kmers(want[:300])).all()
        if k == 11:
            assert res.to_solid_bytes() == solid_bytes_of(k, want)
    # an empty result is a set like any other: it combines again
    nothing = a - a
    assert np.array_equal(keys_of_set(nothing | low), ka[: ka.size // 2])
    assert empty.compare(nothing) == {"a": 0, "b": 0, "both": 0, "jaccard": 1.0}
    assert a.compare(a) == {"a": ka.size, "b": ka.size, "both": ka.size, "jaccard": 1.0}
    assert low.compare(high) == {"a": ka.size // 2, "b": ka.size - ka.size // 2, "both": 0, "jaccard": 0.0}


def test_refused_operands(raw_reads):
    a11, a15 = br_amd.Pcon.new(11), br_amd.Pcon.new(15)
    for call in (lambda: a11 | a15, lambda: a15.compare(a11)):
        with pytest.raises(_lib.BrxError) as ei:
            call()
        assert ei.value.status == _lib.BRX_ERR_ARG and "k = 11" in str(ei.value) and "k = 15" in str(ei.value)
    for k in (12, 3):  # even k, and an odd k below the key files' range
        s = br_amd.Pcon.new(k)
        for call in (lambda: s | s, lambda: s.compare(s)):
            with pytest.raises(_lib.BrxError) as ei:
                call()
            assert ei.value.status == _lib.BRX_ERR_UNSUPPORTED and f"k={k}" in str(ei.value)
    for op in (9, "minus"):
        with pytest.raises(ValueError):
            a11.combine(a11, op)
    with pytest.raises(TypeError):
        a11 | {1, 2}


@pytest.mark.parametrize("k", [15, 25])
def test_chain_of_operations(raw_reads, k):
    ka, kb = _solid_keys(raw_reads, k, 1, 0, 150), _table(raw_reads, k, 120, 170)[0]
    kc, kd = _solid_keys(raw_reads, k, 1, 100, 200), _table(raw_reads, k, 0, 10)[0]
    a, b, c, d = br_amd.Pcon.from_count(raw_reads[:150], k, 1), br_amd.Pcon.from_fasta(raw_reads[120:170], k), from_keys(k, kc), from_keys(k, kd)
    got = (a | b) & c - d  # (python's precedence: - before &)
    want = setops.combine(setops.combine(ka, kb, "union"), setops.combine(kc, kd, "difference"), "intersection")
    assert want.size > 1000 and np.array_equal(keys_of_set(got), want)
    got = ((a | b) & c) - d
    want = setops.combine(setops.combine(setops.combine(ka, kb, "union"), kc, "intersection"), kd, "difference")
    assert want.size > 1000 and np.array_equal(keys_of_set(got), want)
    assert got.fingerprint() == fingerprint_of(want)
    assert np.array_equal(keys_of_set(a.union(b).intersection(c).difference(d).symmetric_difference(d)), setops.combine(want, kd, 3))


def _sort_launches(call):
    """(what call() returns, launches of the key sort's timer during it)"""
    _lib.profile_enable(True)
    _lib.profile_reset()
    try:
        res = call()
        torch.cuda.synchronize()
        return res, _lib.profile_all().get("key_sort", {"launches": 0})["launches"]
    finally:
        _lib.profile_enable(False)


@pytest.mark.parametrize("k", [15, 25])
def test_chain_skips_the_sort_of_lists_known_to_be_in_order(raw_reads, k):
    """a key list from a key file or from a combine is marked as sorted, and every writer of a key list takes the mark away:
    a stale mark would hand pass 1 an unordered list, which it refuses"""
    ka, kb, kc = _solid_keys(raw_reads, k, 1, 0, 150), _table(raw_reads, k, 120, 170)[0], _solid_keys(raw_reads, k, 1, 100, 200)
    a, b = from_keys(k, ka), from_keys(k, kb)
    counted = br_amd.Pcon.from_count(raw_reads[100:200], k, 1)
    u, n = _sort_launches(lambda: a | b)
    assert n == 0 and np.array_equal(keys_of_set(u), setops.combine(ka, kb, 0))
    d, n = _sort_launches(lambda: (u - a) ^ b)  # results of combines, chained
    assert n == 0 and np.array_equal(keys_of_set(d), setops.combine(setops.combine(setops.combine(ka, kb, 0), ka, 2), kb, 3))
    m, n = _sort_launches(lambda: u & counted)  # a counted set's list is in no order: it is sorted, the other one is not
    assert n > 0 and np.array_equal(keys_of_set(m), setops.combine(setops.combine(ka, kb, 0), kc, 1))
    cmp, n = _sort_launches(lambda: u.compare(d))
    assert n == 0 and (cmp["a"], cmp["b"], cmp["both"]) == setops.sizes(keys_of_set(u), keys_of_set(d))
    # the marked set is written again: a finish into it leaves the counter's list, in the counter's order
    cnt = br_amd.Counter(k)
    cnt.add_reads(raw_reads[100:200])
    cnt.finish_into(1, u)
    torch.cuda.synchronize()
    again, n = _sort_launches(lambda: u | a)
    assert n > 0 and np.array_equal(keys_of_set(again), setops.combine(kc, ka, 0))
    if k <= 19:  # a bit-vector set takes more reads: its list is dropped, the bits are the set
        b.insert_reads(raw_reads[:10])
        grown, n = _sort_launches(lambda: b | a)
        want = setops.combine(setops.combine(kb, _table(raw_reads, k, 0, 10)[0], 0), ka, 0)
        assert n > 0 and np.array_equal(keys_of_set(grown), want)


# ---- correction through a combined set -----------------------------------------------------------------------------------
def test_k11_union_corrects_like_the_oracle(raw_reads, solid_fixture_bytes):
    k = 11
    bits = np.unpackbits(np.frombuffer(solid_fixture_bytes, dtype=np.uint8)[1:], bitorder="little")
    want = setops.combine(np.flatnonzero(bits).astype(np.uint64), _table(raw_reads, k, 0, 10)[0], "union")
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes) | br_amd.Pcon.from_fasta(raw_reads[:10], k)
    assert gs.to_solid_bytes() == solid_bytes_of(k, want)
    ref = O.Solid.wrap(k, np.frombuffer(solid_bytes_of(k, want), dtype=np.uint8)[1:].copy())
    om = O.build_methods(ref, METHODS, 5, 7)
    sub = raw_reads[10:30]
    got = br_amd.Chain(gs, [(m, 5, 7) for m in METHODS], two_side=False).correct_reads(sub)
    assert got == [O.correct_record(om, r, False) for r in sub]
    assert sum(g != r for g, r in zip(got, sub)) >= 1  # (see the k = 21 test)


def test_k21_difference_corrects_like_the_oracle(raw_reads):
    k = 21
    want = setops.combine(_solid_keys(raw_reads, k, 1, 0, 150), _solid_keys(raw_reads, k, 1, 150, None), "difference")
    gs = br_amd.Pcon.from_count(raw_reads[:150], k, 1) - br_amd.Pcon.from_count(raw_reads[150:], k, 1)
    assert gs.fingerprint() == fingerprint_of(want) and want.size > 1000
    ref = O.Solid(k, _h=O.lib().bro_solid_new_sparse(k, want.ctypes.data, want.size))
    sub = raw_reads[:30]
    changed = 0
    for method in ("one", "graph"):
        om = O.build_methods(ref, [method], 5, 7)
        got = br_amd.Chain(gs, [(method, 5, 7)], two_side=False).correct_reads(sub)
        assert got == [O.correct_record(om, r, False) for r in sub], method
        changed += sum(g != r for g, r in zip(got, sub))
    assert changed >= 1  # (a set that nobody asks, or an empty one, changes no read: the comparison above would prove nothing)


# ---- stream order of the raw entry ---------------------------------------------------------------------------------------
def test_raw_entry_reads_its_inputs_in_stream_order(lane, reads):
    """the two sorted arrays hold a decoy of identical sizes until the lane's delay has run: the answer is the real one's"""
    k = 13
    real = {"a": np.unique(np.concatenate([O.hashes(k, r) for r in reads[:24]])),
            "b": np.unique(np.concatenate([O.hashes(k, r) for r in reads[12:36]]))}
    rng = np.random.default_rng(9)
    fake = {name: _sample(rng, keys.size, 1 << (2 * k - 1)) for name, keys in real.items()}

    def op_combine(op):
        @operation(lambda arrays: {"out": (arrays["a"].size + arrays["b"].size, "int64")})
        def run(ctx, inp, out):
            n, s3 = combine_keys_device(ptr(inp["a"]), inp["a"].numel(), ptr(inp["b"]), inp["b"].numel(), op, ptr(out["out"]),
                                        out["out"].numel(), ctx.stream)
            return n, s3, ctx.fetch(out["out"])[:n].tobytes()
        return run

    for op in ("symmetric_difference", "intersection"):
        n, s3, data = probe(lane, op_combine(op), fake, real)
        want = setops.combine(real["a"], real["b"], op)
        assert n == want.size and s3 == setops.sizes(real["a"], real["b"]) and data == want.tobytes()


# ---- command line --------------------------------------------------------------------------------------------------------
def _write(path, data, zipped=False):
    with (gzip.open(path, "wb") if zipped else open(path, "wb")) as f:
        f.write(data)
    return path


def test_cli_k11_mixed_operands(tmp_path, golden_dir, raw_reads, solid_fixture_bytes):
    from br_amd import cli
    k = 11
    raw = os.path.join(golden_dir, "raw.fasta")
    p = lambda name: str(tmp_path / name)
    base = np.flatnonzero(np.unpackbits(np.frombuffer(solid_fixture_bytes, dtype=np.uint8)[1:], bitorder="little")).astype(np.uint64)
    k_or, k_minus, k_and = _table(raw_reads, k, 0, 10)[0], _solid_keys(raw_reads, k, 3, 0, 100), _table(raw_reads, k, 5, 200)[0]
    _write(p("or.keys.gz"), keyfile.encode(k, k_or), zipped=True)
    _write(p("minus.solid.gz"), solid_bytes_of(k, k_minus), zipped=True)
    counts = np.full(k_and.size, 7, dtype=np.uint8)
    _write(p("and.counts"), keyfile.encode(k, k_and, counts, floor=1))  # a count file: the counts are ignored
    _write(p("plain.solid"), solid_bytes_of(k, k_or))
    common = ["-i", raw, "-c", "one", "-s"]
    tail = ["solid", "-i", os.path.join(golden_dir, "raw.k11.a2.solid"), "-f", "solid"]
    for tag, flags, want in (
            ("1", ["--set-or", p("or.keys.gz"), "--set-minus", p("minus.solid.gz"), "--set-and", p("and.counts")],
             setops.combine(setops.combine(setops.combine(base, k_or, 0), k_minus, 2), k_and, 1)),
            ("2", ["--set-minus", p("minus.solid.gz"), "--set-and", p("and.counts"), "--set-or", p("plain.solid")],
             setops.combine(setops.combine(setops.combine(base, k_minus, 2), k_and, 1), k_or, 0))):
        assert cli.main(common + ["-o", p(tag + ".fa")] + flags + ["--save-set", p(tag + ".keys")] + tail) == 0
        assert open(p(tag + ".keys"), "rb").read() == keyfile.encode(k, want), tag
        assert cli.main(common + ["-o", p(tag + "_again.fa"), "solid", "-i", p(tag + ".keys"), "-f", "keys"]) == 0
        assert open(p(tag + ".fa"), "rb").read() == open(p(tag + "_again.fa"), "rb").read() and os.path.getsize(p(tag + ".fa")) > 1000
    assert open(p("1.keys"), "rb").read() != open(p("2.keys"), "rb").read()  # the order of the flags is the order applied
    # without the flags: what the sub-command's own set gives (an earlier build is not at hand in a test: the yardstick is
    # a `solid -f keys` run on that set, which tests/test_gpu_keyfile.py ties to the other sub-commands' output)
    assert cli.main(common + ["-o", p("none.fa"), "--save-set", p("none.keys")] + tail) == 0
    assert open(p("none.keys"), "rb").read() == keyfile.encode(k, base)
    assert cli.main(common + ["-o", p("none_again.fa"), "solid", "-i", p("none.keys"), "-f", "keys"]) == 0
    assert open(p("none.fa"), "rb").read() == open(p("none_again.fa"), "rb").read()
    assert open(p("none.fa"), "rb").read() != open(p("1.fa"), "rb").read()


def test_cli_k21_and_refusals(tmp_path, golden_dir, raw_reads):
    from br_amd import cli
    k = 21
    raw = os.path.join(golden_dir, "raw.fasta")
    p = lambda name: str(tmp_path / name)
    base = _solid_keys(raw_reads, k, 2, 0, None)
    k_minus, k_or = _solid_keys(raw_reads, k, 1, 100, 200), _table(raw_reads, k, 0, 10)[0]
    _write(p("minus.keys"), keyfile.encode(k, k_minus))
    _write(p("or.keys.gz"), keyfile.encode(k, k_or), zipped=True)
    common = ["-i", raw, "-c", "one", "-s"]
    tail = ["fasta", "-i", raw, "-k", "21", "-a", "2"]
    assert cli.main(common + ["-o", p("a.fa"), "--set-minus", p("minus.keys"), "--set-or", p("or.keys.gz"), "--save-set", p("a.keys")] + tail) == 0
    want = setops.combine(setops.combine(base, k_minus, 2), k_or, 0)
    assert open(p("a.keys"), "rb").read() == keyfile.encode(k, want)
    assert cli.main(common + ["-o", p("b.fa"), "solid", "-i", p("a.keys"), "-f", "keys"]) == 0
    assert open(p("a.fa"), "rb").read() == open(p("b.fa"), "rb").read() and os.path.getsize(p("a.fa")) > 1000
    # another k
    _write(p("k19.keys"), keyfile.encode(19, _table(raw_reads, 19, 0, 3)[0]))
    with pytest.raises(SystemExit) as ei:
        cli.main(common + ["-o", p("x.fa"), "--set-or", p("or.keys.gz"), "--set-minus", p("k19.keys"), "--save-set", p("x.keys")] + tail)
    assert str(ei.value) == "Error: --set-minus %s: k = 19, the set in use has k = 21" % p("k19.keys")
    assert not os.path.exists(p("x.keys"))
    # a library error carries the flag and the path
    _write(p("cut.keys"), keyfile.encode(k, k_minus)[:-3])
    with pytest.raises(SystemExit) as ei:
        cli.main(common + ["-o", p("y.fa"), "--set-and", p("cut.keys")] + tail)
    assert str(ei.value).startswith("Error: --set-and %s: " % p("cut.keys")) and "truncated" in str(ei.value)
