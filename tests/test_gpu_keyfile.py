"""Key files on the GPU path (include/brx.h "key files", br_amd/csrc/brx_keyfile.hip): the radix sort against numpy, saved
files byte for byte against br_amd/keyfile.py, sets and counters that come back from their files, merging, the floor, the
refusals of the device path, streams and the command line."""
import gzip
import io
import os
import struct
import threading

import numpy as np
import pytest
import torch

import br_amd
from br_amd import _lib, abundance, keyfile
from br_amd.set import sort_keys_device
from oracle import oracle as O

pytestmark = pytest.mark.gpu

TABLE = _lib.COUNT_TABLE
METHODS = ["one", "two", "graph", "greedy", "gap_size"]
_cache = {}


def _table(raw_reads, k, lo=0, hi=None):
    """(keys, counts clipped at 255) of raw_reads[lo:hi], in numpy; computed once and never modified"""
    key = ("table", k, lo, hi)
    if key not in _cache:
        _cache[key] = abundance.count_table([abundance.canonical_hashes(r, k) for r in raw_reads[lo:hi]])
    return _cache[key]


def _count_file(raw_reads, k, min_count=1, lo=0, hi=None):
    keys, counts = _table(raw_reads, k, lo, hi)
    keep = counts >= min_count
    return keyfile.encode(k, keys[keep], counts[keep], floor=min_count)


def _counter(reads, k, batch=None):
    cnt = br_amd.Counter(k, 0, TABLE)
    step = batch or max(len(reads), 1)
    for i in range(0, len(reads), step):
        cnt.add_reads(reads[i:i + step])
    return cnt


def _saved(obj, *args):
    f = io.BytesIO()
    (obj.save if isinstance(obj, br_amd.Counter) else obj.save_keys)(f, *args)
    return f.getvalue()


def _queries(k, reads, rng):
    """the query mix of test_gpu_count_table.py: k-mers of the reads, near misses and random ones"""
    fw = []
    for r in reads[:6]:
        for i in range(0, len(r) - k + 1, 3):
            w = r[i:i + k]
            if set(w) <= set(b"ACGT"):
                fw.append(O.seq2bit(w))
    fw = np.array(fw, dtype=np.uint64)
    mask = np.uint64((1 << (2 * k)) - 1)
    return np.concatenate([fw, fw ^ np.uint64(1), fw ^ (np.uint64(2) << np.uint64(2 * (k - 1))),
                           rng.integers(0, 1 << (2 * k), 5000, dtype=np.uint64)]) & mask


# ---- sort ---------------------------------------------------------------------------------------------------------------
def _sort_on_gpu(keys, pay, key_bits):
    dk = torch.from_numpy(keys.view(np.int64).copy()).cuda()
    dp = torch.from_numpy(pay.copy()).cuda() if pay is not None else None
    torch.cuda.synchronize()
    sort_keys_device(dk.data_ptr() if keys.size else None, dp.data_ptr() if dp is not None and keys.size else None, keys.size, key_bits)
    torch.cuda.synchronize()
    return dk.cpu().numpy().view(np.uint64), (dp.cpu().numpy() if dp is not None else None)


def _sort_inputs(n, key_bits, rng):
    passes = (key_bits + 7) // 8
    top_shift = 8 * (passes - 1)
    uni = rng.integers(0, 1 << key_bits, n, dtype=np.uint64)
    const = np.uint64(((1 << key_bits) - 1) & 0x155555555555AA00)
    yield "uniform", uni
    yield "sorted", np.sort(uni)
    yield "reversed", np.sort(uni)[::-1].copy()
    yield "lowest digit", (const & ~np.uint64(0xff)) | rng.integers(0, 256, n, dtype=np.uint64)
    yield "highest digit", ((const & np.uint64((1 << top_shift) - 1))
                            | (rng.integers(0, 1 << (key_bits - top_shift), n, dtype=np.uint64) << np.uint64(top_shift)))
    yield "equal", np.full(n, int(const) | 1, dtype=np.uint64)


def _check_sort(n, key_bits, rng, without_payload=True):
    for name, keys in _sort_inputs(n, key_bits, rng):
        pay = (np.arange(n) % 256).astype(np.uint8)  # arrival index mod 256: equal keys must keep their order
        order = np.argsort(keys, kind="stable")
        got_k, got_p = _sort_on_gpu(keys, pay, key_bits)
        assert np.array_equal(got_k, keys[order]), (n, key_bits, name)
        assert np.array_equal(got_p, pay[order]), (n, key_bits, name, "payload")
        if without_payload or name == "uniform":
            got_k, _ = _sort_on_gpu(keys, None, key_bits)
            assert np.array_equal(got_k, np.sort(keys)), (n, key_bits, name, "no payload")


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 65537])
def test_sort(n):
    """(4096 keys are a tile of a digit pass)"""
    rng = np.random.default_rng(n)
    for key_bits in (9, 41, 49, 61):
        _check_sort(n, key_bits, rng)


@pytest.mark.parametrize("key_bits", [9, 41, 49, 61])
def test_sort_large(key_bits):
    _check_sort(1000003, key_bits, np.random.default_rng(key_bits), without_payload=False)


def test_sort_one_block_loops_over_everything(monkeypatch):
    monkeypatch.setenv("BRX_READ_GRID", "1")
    rng = np.random.default_rng(1)
    for n in (4097, 20000):
        _check_sort(n, 49, rng)


def test_sort_refuses_bad_arguments():
    dk = torch.zeros(4, dtype=torch.int64, device="cuda")
    for bits in (0, 65):
        with pytest.raises(_lib.BrxError) as ei:
            sort_keys_device(dk.data_ptr(), None, 4, bits)
        assert ei.value.status == _lib.BRX_ERR_ARG


# ---- save = the numpy statement, byte for byte --------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [None, 7])
@pytest.mark.parametrize("k", [11, 19, 25, 31])
def test_counter_save_equals_numpy(raw_reads, k, batch):
    """batch = 7: 30 batches, the table regrows several times on the way"""
    cnt = _counter(raw_reads, k, batch)
    spec = cnt.spectrum()
    fp = cnt.finish(2).fingerprint()
    for min_count in (1, 2, 3):
        f = io.BytesIO()
        st = cnt.save(f, min_count)
        assert f.getvalue() == _count_file(raw_reads, k, min_count), (k, min_count)
        assert st["bytes"] == len(f.getvalue()) and st["blocks"] == (st["keys"] + 255) // 256
    assert _saved(cnt, 0) == _count_file(raw_reads, k, 1)  # 0 means 1
    # saving changes nothing the counter answers
    assert np.array_equal(cnt.spectrum(), spec)
    assert cnt.finish(2).fingerprint() == fp
    assert cnt.floor == 1


@pytest.mark.parametrize("k", [7, 25])
def test_counter_save_saturation(k):
    """the poly-A read of test_gpu_count_table.py: 900 occurrences give a count byte of 255"""
    reads = [b"A" * (k + 299)] * 3 + [b"ACGTACGTAC"]
    cnt = _counter(reads, k)
    kk, keys, counts, floor = keyfile.decode(_saved(cnt))
    assert (kk, floor) == (k, 1)
    assert int(keys[0]) == 0 and int(counts[0]) == 255  # poly-A: forward k-mer 0, even popcount, key 0
    exp_k, exp_c = abundance.count_table([abundance.canonical_hashes(r, k) for r in reads])
    assert np.array_equal(keys, exp_k) and np.array_equal(counts, exp_c)


def test_empty_counter_saves_the_header():
    cnt = br_amd.Counter(7, 0, TABLE)
    data = _saved(cnt)
    assert len(data) == 32
    assert data == keyfile.encode(7, np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint8), floor=1)
    back = br_amd.Counter.from_keyfile(io.BytesIO(data))
    assert back.k == 7 and int(back.spectrum()[1:].sum()) == 0
    empty_set = br_amd.Pcon.new(25)
    assert _saved(empty_set) == keyfile.encode(25, np.zeros(0, dtype=np.uint64))
    assert br_amd.Pcon.from_keyfile(io.BytesIO(_saved(empty_set))).popcount() == 0


# ---- set save from every holding, and load ------------------------------------------------------------------------------
def _solid_keys(raw_reads, k, a, lo=0, hi=None):
    keys, counts = _table(raw_reads, k, lo, hi)
    return keys[counts > a]


def _holdings(raw_reads, solid_fixture_bytes, which):
    """(set, k, its sorted keys from numpy / the reference's fixture)"""
    if which == "k11 bits":
        return br_amd.Pcon.from_count(raw_reads, 11, 2, strategy=_lib.COUNT_DENSE), 11, _solid_keys(raw_reads, 11, 2)
    if which == "k11 fixture":
        bits = np.unpackbits(np.frombuffer(solid_fixture_bytes, dtype=np.uint8)[1:], bitorder="little")
        return br_amd.Pcon.from_pcon_solid(solid_fixture_bytes), 11, np.flatnonzero(bits).astype(np.uint64)
    if which == "k19 lazy":
        return br_amd.Pcon.from_count(raw_reads[:150], 19, 2), 19, _solid_keys(raw_reads, 19, 2, 0, 150)
    if which == "k21 counted":
        return br_amd.Pcon.from_count(raw_reads[:150], 21, 1), 21, _solid_keys(raw_reads, 21, 1, 0, 150)
    if which == "k25 counted":
        return br_amd.Pcon.from_count(raw_reads[:150], 25, 1), 25, _solid_keys(raw_reads, 25, 1, 0, 150)
    assert which == "k25 inserted"
    return br_amd.Pcon.from_fasta(raw_reads[:60], 25), 25, _table(raw_reads, 25, 0, 60)[0]


@pytest.mark.parametrize("which", ["k11 bits", "k11 fixture", "k19 lazy", "k21 counted", "k25 counted", "k25 inserted"])
def test_set_save_and_load(raw_reads, solid_fixture_bytes, which):
    gs, k, keys = _holdings(raw_reads, solid_fixture_bytes, which)
    state = gs.bits_state()
    assert state == {"k11 bits": 0, "k11 fixture": 0, "k19 lazy": 1}.get(which, 2)
    data = _saved(gs)
    assert data == keyfile.encode(k, keys), which
    assert gs.bits_state() == state  # a lazy bit vector stays lazy
    if which == "k11 fixture":  # the file of the reference's set = the file of the set counted here with a = 2
        assert data == _saved(br_amd.Pcon.from_count(raw_reads, 11, 2))
    back = br_amd.Pcon.from_keyfile(io.BytesIO(data))
    assert back.k() == k and back.is_sparse() == (k >= 21)
    assert back.fingerprint() == gs.fingerprint()
    assert back.popcount() == gs.popcount() == keys.size > 1000
    q = _queries(k, raw_reads, np.random.default_rng(k))
    want = gs.get_many(q)
    assert want.any() and not want.all()
    assert np.array_equal(back.get_many(q), want)
    assert np.array_equal(want, np.isin(abundance_keys(q, k), keys))
    if k == 11:
        assert back.to_solid_bytes() == solid_fixture_bytes
    assert _saved(back) == data  # and the loaded set saves the same file


def abundance_keys(forward_kmers, k):
    """canonical(kmer) >> 1 of forward k-mers, through the oracle's scalar definition"""
    return np.array([O.khash(int(x), k) for x in forward_kmers], dtype=np.uint64)


def test_set_load_takes_a_count_file(raw_reads):
    """the counts are ignored: every key listed is a member"""
    k = 25
    keys, _ = _table(raw_reads, k, 0, 60)
    back = br_amd.Pcon.from_keyfile(io.BytesIO(_count_file(raw_reads, k, 1, 0, 60)))
    assert back.popcount() == keys.size
    assert _saved(back) == keyfile.encode(k, keys)


def test_loaded_set_corrects_like_the_oracle(raw_reads):
    k, a = 25, 1
    reads = raw_reads[:150]
    data = _saved(br_amd.Pcon.from_count(reads, k, a))
    gs = br_amd.Pcon.from_keyfile(io.BytesIO(data))
    ref = O.Solid.sparse_from_count(k, reads, a)
    assert gs.popcount() == ref.popcount()
    changed = None
    for method in METHODS:
        om = O.build_methods(ref, [method], 5, 7)
        sub = reads[:25] if method == "greedy" else reads[:40]
        got = br_amd.Chain(gs, [(method, 5, 7)], two_side=False).correct_reads(sub)
        for r, g in zip(sub, got):
            assert g == O.correct_record(om, r, False), method
        if method == "one":
            changed = sum(g != r for r, g in zip(sub, got))
    assert changed >= 25  # an empty set would correct nothing


def test_loaded_k15_set_covers_and_corrects(raw_reads):
    """k <= 19: the loaded set has its bits written and its key list attached, like a counted one"""
    k, a = 15, 2
    reads = raw_reads[:100]
    orig = br_amd.Pcon.from_count(reads, k, a)
    gs = br_amd.Pcon.from_keyfile(io.BytesIO(_saved(orig)))
    assert gs.to_solid_bytes() == orig.to_solid_bytes()
    sub = reads[:30]
    fl0, st0 = orig.cover_reads(sub)
    fl1, st1 = gs.cover_reads(sub)
    assert all(np.array_equal(x, y) for x, y in zip(fl0, fl1)) and np.array_equal(st0, st1)
    for method in METHODS:
        want = br_amd.Chain(orig, [(method, 5, 7)], two_side=False).correct_reads(sub[:20])
        assert br_amd.Chain(gs, [(method, 5, 7)], two_side=False).correct_reads(sub[:20]) == want, method


@pytest.mark.parametrize("k", [11, 25])
def test_counter_from_keyfile(raw_reads, k):
    cnt = _counter(raw_reads, k)
    data = _saved(cnt)
    back = br_amd.Counter.from_keyfile(io.BytesIO(data))
    assert back.k == k and back.floor == 1
    assert np.array_equal(back.spectrum(), cnt.spectrum())
    q = _queries(k, raw_reads, np.random.default_rng(3 * k))
    got = back.get_counts(q)
    assert np.array_equal(got, cnt.get_counts(q)) and got.any()
    p0, s0 = cnt.abundance_reads(raw_reads[:12], 2)
    p1, s1 = back.abundance_reads(raw_reads[:12], 2)
    assert all(np.array_equal(x, y) for x, y in zip(p0, p1)) and np.array_equal(s0, s1)
    for a in (1, 2, 3):
        assert back.finish(a).fingerprint() == cnt.finish(a).fingerprint()
    assert _saved(back) == data


# ---- merge --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [25, 11])
def test_merge_of_shards(raw_reads, k):
    a = _saved(_counter(raw_reads[:100], k))
    b = _saved(_counter(raw_reads[100:], k))
    assert a == _count_file(raw_reads, k, 1, 0, 100) and b == _count_file(raw_reads, k, 1, 100, None)
    both = br_amd.Counter(k, 0, TABLE)
    both.load(io.BytesIO(a))
    both.load(io.BytesIO(b))
    assert _saved(both) == _count_file(raw_reads, k)
    # reads counted here and a file loaded on top: the same
    mixed = _counter(raw_reads[:100], k)
    mixed.load(io.BytesIO(b))
    assert _saved(mixed) == _count_file(raw_reads, k)


def test_same_file_three_times_saturates(raw_reads):
    k = 25
    keys, counts = _table(raw_reads, k)
    data = _count_file(raw_reads, k)
    cnt = br_amd.Counter(k, 0, TABLE)
    for _ in range(3):
        cnt.load(io.BytesIO(data))
    exp = np.minimum(3 * counts.astype(np.int64), 255).astype(np.uint8)
    assert int(exp.max()) == 255 or int(counts.max()) < 85
    assert _saved(cnt) == keyfile.encode(k, keys, exp, floor=1)


# ---- floor --------------------------------------------------------------------------------------------------------------
def test_floor(raw_reads):
    k = 25
    full = _counter(raw_reads, k)
    data = _saved(full, 3)
    cnt = br_amd.Counter.from_keyfile(io.BytesIO(data))
    assert cnt.floor == 3
    assert cnt.finish(2).fingerprint() == full.finish(2).fingerprint()
    assert cnt.finish(5).fingerprint() == full.finish(5).fingerprint()
    spec, want = cnt.spectrum(), full.spectrum()
    assert spec[1] == spec[2] == 0 and np.array_equal(spec[3:], want[3:])
    refused = [lambda: cnt.finish(1), lambda: cnt.finish(0), lambda: cnt.add_reads(raw_reads[:2]), lambda: cnt.load(io.BytesIO(data)),
               lambda: cnt.load(io.BytesIO(_count_file(raw_reads, k, 1, 0, 20)))]
    for call in refused:
        with pytest.raises(_lib.BrxError) as ei:
            call()
        assert ei.value.status == _lib.BRX_ERR_ARG
    assert _saved(cnt, 1) == data  # a save writes floor max(f, min_count)
    assert _saved(cnt, 4) == _count_file(raw_reads, k, 4)
    # a floored file does not load into a counter that holds something
    busy = _counter(raw_reads[:5], k)
    with pytest.raises(_lib.BrxError) as ei:
        busy.load(io.BytesIO(data))
    assert ei.value.status == _lib.BRX_ERR_ARG
    assert _saved(busy) == _count_file(raw_reads, k, 1, 0, 5)  # (left as it was)
    # reset reopens the counter
    cnt.reset()
    assert cnt.floor == 1
    cnt.add_reads(raw_reads[:5])
    assert _saved(cnt) == _count_file(raw_reads, k, 1, 0, 5)
    assert cnt.finish(0).popcount() == _table(raw_reads, k, 0, 5)[0].size


# ---- refusals on the device path ----------------------------------------------------------------------------------------
def _valid_k9():
    rng = np.random.default_rng(5)
    keys = np.sort(rng.choice(1 << 17, size=600, replace=False).astype(np.uint64))
    counts = rng.integers(1, 256, size=600).astype(np.uint8)
    return keys, counts, keyfile.encode(9, keys, counts, floor=1)


def _block_start(data, b):
    """offset of block b of a count file"""
    n = struct.unpack_from("<Q", data, 16)[0]
    pos = 32
    for i in range(b):
        m = min(256, n - 256 * i)
        pos += 9 + ((m - 1) * data[pos + 8] + 7) // 8 + m
    return pos


def _bad_files():
    keys, counts, good = _valid_k9()
    total = int(keys.sum(dtype=np.uint64))
    yield "truncated", good[:-1], "truncated"
    yield "truncated in a header", good[:_block_start(good, 1) + 4], "truncated"
    yield "trailing", good + b"\x00", "trailing"
    d = bytearray(good)  # the last block moved up until its last key leaves the range; the key sum made to match
    shift = (1 << 17) - int(keys[-1])
    struct.pack_into("<Q", d, _block_start(good, 2), int(keys[512]) + shift)
    struct.pack_into("<Q", d, 24, (total + shift * (600 - 512)) % (1 << 64))
    yield "key out of range", bytes(d), "not below"
    d = bytearray(good)  # a first key of 2^64 - 1: the prefix sums must not wrap back into the range
    struct.pack_into("<Q", d, _block_start(good, 2), (1 << 64) - 1)
    yield "key far out of range", bytes(d), "not below"
    d = bytearray(good)  # the second block starts at the first block's last key
    struct.pack_into("<Q", d, _block_start(good, 1), int(keys[255]))
    struct.pack_into("<Q", d, 24, (total - (int(keys[256]) - int(keys[255])) * 256) % (1 << 64))
    yield "blocks out of order", bytes(d), "does not start above"
    d = bytearray(good)
    d[24] ^= 1
    yield "key sum", bytes(d), "key sum"
    d = bytearray(good)
    d[-1] = 0
    yield "zero count", bytes(d), "count of 0"
    d = bytearray(good)
    d[0] ^= 1
    yield "magic", bytes(d), "magic"
    d = bytearray(good)
    d[_block_start(good, 1) + 8] = 62
    yield "width", bytes(d), "width"
    yield "set file into a counter", keyfile.encode(9, keys), "set file"


def test_numpy_refuses_the_same_files():
    for name, data, _ in _bad_files():
        if name != "set file into a counter":
            with pytest.raises(ValueError):
                keyfile.decode(data)


def test_device_path_refusals(raw_reads):
    keys, counts, good = _valid_k9()
    cnt = br_amd.Counter(9, 0, TABLE)
    for name, data, word in _bad_files():
        cnt.add_reads(raw_reads[:2])  # something to lose: a failed load leaves the counter reset, never half loaded
        with pytest.raises(_lib.BrxError) as ei:
            cnt.load(io.BytesIO(data))
        assert ei.value.status == _lib.BRX_ERR_FORMAT, name
        assert word in str(ei.value) and "reset" in str(ei.value), (name, str(ei.value))
        assert int(cnt.spectrum()[1:].sum()) == 0 and cnt.floor == 1 and cnt.table_info()["keys"] == 0, name
        cnt.load(io.BytesIO(good))  # and usable
        assert _saved(cnt) == good, name
        cnt.reset()
        if name not in ("set file into a counter",):
            with pytest.raises(_lib.BrxError) as ei:
                br_amd.Pcon.from_keyfile(io.BytesIO(data))
            assert ei.value.status == _lib.BRX_ERR_FORMAT and word in str(ei.value), name


def test_argument_refusals(raw_reads):
    _, _, good = _valid_k9()
    c11 = _counter(raw_reads[:3], 11)
    with pytest.raises(_lib.BrxError) as ei:
        c11.load(io.BytesIO(good))
    assert ei.value.status == _lib.BRX_ERR_ARG and "9-mers" in str(ei.value)
    assert _saved(c11) == _count_file(raw_reads, 11, 1, 0, 3)  # (an argument fault leaves the counter as it was)
    for strategy, word in ((_lib.COUNT_DENSE, "dense"), (_lib.COUNT_SORTED, "partitioned")):
        c = br_amd.Counter(9, 0, strategy)
        for call in (lambda: c.save(io.BytesIO()), lambda: c.load(io.BytesIO(good))):
            with pytest.raises(_lib.BrxError) as ei:
                call()
            assert ei.value.status == _lib.BRX_ERR_UNSUPPORTED
            assert word in str(ei.value) and "BRX_COUNT_TABLE" in str(ei.value)
        assert c.floor == 1


# ---- streams ------------------------------------------------------------------------------------------------------------
def test_small_slices_cut_blocks(raw_reads, monkeypatch):
    """4 KiB pieces: 1600 of them for the 6.6 MB file, nearly every one ending inside a block"""
    monkeypatch.setenv("BRX_KEYFILE_SLICE_KB", "4")
    k = 25
    want = _count_file(raw_reads, k)
    cnt = _counter(raw_reads, k)
    assert _saved(cnt) == want
    back = br_amd.Counter.from_keyfile(io.BytesIO(want))
    monkeypatch.delenv("BRX_KEYFILE_SLICE_KB")
    assert _saved(back) == want
    monkeypatch.setenv("BRX_KEYFILE_SLICE_KB", "4")
    gs = br_amd.Pcon.from_keyfile(io.BytesIO(want))
    assert gs.popcount() == _table(raw_reads, k)[0].size
    with pytest.raises(_lib.BrxError) as ei:
        br_amd.Counter.from_keyfile(io.BytesIO(want[:-700]))
    assert ei.value.status == _lib.BRX_ERR_FORMAT and "truncated" in str(ei.value)


def test_gzip_file_and_pipe(raw_reads, tmp_path):
    k = 25
    want = _count_file(raw_reads, k, 1, 0, 100)
    cnt = _counter(raw_reads[:100], k)
    path = str(tmp_path / "counts.keys.gz")
    with gzip.open(path, "wb") as f:
        cnt.save(f)
    assert gzip.open(path, "rb").read() == want
    with gzip.open(path, "rb") as f:
        assert _saved(br_amd.Counter.from_keyfile(f)) == want
    with gzip.open(path, "rb") as f:
        assert br_amd.Pcon.from_keyfile(f).popcount() == _table(raw_reads, k, 0, 100)[0].size
    # a plain file handed over as its descriptor
    plain = str(tmp_path / "counts.keys")
    with open(plain, "wb") as f:
        cnt.save(f)
    assert open(plain, "rb").read() == want
    with open(plain, "rb") as f:
        assert _saved(br_amd.Counter.from_keyfile(f)) == want
    # a pipe: the library writes to / reads from the descriptor itself
    r, w = os.pipe()
    got = []
    t = threading.Thread(target=lambda: got.append(os.fdopen(r, "rb").read()))
    t.start()
    with os.fdopen(w, "wb") as wf:
        cnt.save(wf)
    t.join()
    assert got[0] == want
    r, w = os.pipe()

    def feed():
        with os.fdopen(w, "wb") as wf:
            wf.write(want)

    t = threading.Thread(target=feed)
    t.start()
    back = br_amd.Counter(k, 0, TABLE)
    st = (_lib.C.c_uint64 * 8)()
    _lib.check(_lib.lib().brx_counter_load_fd(back._h, r, st))
    os.close(r)
    t.join()
    assert int(st[0]) == _table(raw_reads, k, 0, 100)[0].size and int(st[1]) == len(want)
    assert _saved(back) == want


# ---- command line -------------------------------------------------------------------------------------------------------
def test_cli(tmp_path, golden_dir, raw_reads):
    from br_amd import cli
    raw = os.path.join(golden_dir, "raw.fasta")
    p = lambda name: str(tmp_path / name)
    common = ["-i", raw, "-c", "one", "-s"]
    assert cli.main(common + ["-o", p("first.fa"), "--save-set", p("S"), "--save-counts", p("C"), "fasta", "-i", raw, "-k", "25",
                              "-a", "2"]) == 0
    first = open(p("first.fa"), "rb").read()
    assert len(first) > 1000
    assert open(p("C"), "rb").read() == _count_file(raw_reads, 25)
    assert open(p("S"), "rb").read() == keyfile.encode(25, _solid_keys(raw_reads, 25, 2))
    # (--save-counts makes `fasta` count into the hash table: the set is the same)
    assert cli.main(common + ["-o", p("plain.fa"), "fasta", "-i", raw, "-k", "25", "-a", "2"]) == 0
    assert open(p("plain.fa"), "rb").read() == first
    assert cli.main(common + ["-o", p("from_set.fa"), "solid", "-i", p("S"), "-f", "keys"]) == 0
    assert open(p("from_set.fa"), "rb").read() == first
    assert cli.main(common + ["-o", p("from_counts.fa"), "count", "-i", p("C"), "-a", "2"]) == 0
    assert open(p("from_counts.fa"), "rb").read() == first
    # a threshold selector on the loaded counter picks what it picks on the counted one; gzip is sniffed first
    with gzip.open(p("C.gz"), "wb") as f:
        f.write(open(p("C"), "rb").read())
    assert cli.main(common + ["-o", p("min_a.fa"), "fasta", "-i", raw, "-k", "25", "first-minimum"]) == 0
    assert cli.main(common + ["-o", p("min_b.fa"), "--abundance-report", p("ab.tsv"), "count", "-i", p("C.gz"), "first-minimum"]) == 0
    assert open(p("min_b.fa"), "rb").read() == open(p("min_a.fa"), "rb").read()
    assert open(p("ab.tsv"), "rb").read().count(b"\n") == len(raw_reads) + 1
    # refusals
    with pytest.raises(SystemExit) as ei:
        cli.main(common + ["-o", p("x.fa"), "--save-counts", p("C2"), "solid", "-i", p("S"), "-f", "keys"])
    assert "--save-counts" in str(ei.value) and not os.path.exists(p("C2"))
    assert cli.main(common + ["-o", p("x.fa"), "--save-counts", p("C3"), "--save-min-count", "3", "fasta", "-i", raw, "-k", "25",
                              "-a", "2"]) == 0
    assert open(p("C3"), "rb").read() == _count_file(raw_reads, 25, 3)
    assert open(p("x.fa"), "rb").read() == first
    assert cli.main(common + ["-o", p("y.fa"), "count", "-i", p("C3"), "-a", "2"]) == 0
    assert open(p("y.fa"), "rb").read() == first
    with pytest.raises(SystemExit) as ei:
        cli.main(common + ["-o", p("z.fa"), "count", "-i", p("C3"), "-a", "1"])
    assert "--save-min-count 3" in str(ei.value)


def test_cli_count_still_reads_a_pcon_table(tmp_path, golden_dir, raw_reads):
    from br_amd import cli
    raw = os.path.join(golden_dir, "raw.fasta")
    k = 7
    keys, counts = _table(raw_reads, k)
    table = np.zeros(1 << (2 * k - 1), dtype=np.uint8)
    table[keys.astype(np.int64)] = counts
    path = str(tmp_path / "table.pcon")
    with open(path, "wb") as f:
        f.write(bytes([k]) + table.tobytes())
    common = ["-i", raw, "-c", "one", "-s"]
    assert cli.main(common + ["-o", str(tmp_path / "a.fa"), "count", "-i", path, "-a", "200"]) == 0
    assert cli.main(common + ["-o", str(tmp_path / "b.fa"), "--save-set", str(tmp_path / "S7"), "fasta", "-i", raw, "-k", str(k),
                              "-a", "200"]) == 0
    assert open(str(tmp_path / "a.fa"), "rb").read() == open(str(tmp_path / "b.fa"), "rb").read()
    assert open(str(tmp_path / "S7"), "rb").read() == keyfile.encode(k, keys[counts > 200])
    with pytest.raises(SystemExit):  # a dense counter has no key file
        cli.main(common + ["-o", str(tmp_path / "c.fa"), "--save-counts", str(tmp_path / "C7"), "count", "-i", path, "-a", "200"])
