"""Two count lists side by side on the GPU path (include/brx.h "count lists": brx_counts_joint_device, brx_counts_compare;
br_amd/csrc/brx_setops.hip count_joint_kernel): the joint spectrum against countops.joint at the key shapes where a merge can
go wrong and the count shapes where the binning can -- a few hot bins, the edge of the corner kept in LDS, nothing in it --
through 1, 3 and 7 blocks, the refusals, stream order of the raw entry, the objects and the command line.  Every comparison
is exact."""
import io
import os

import numpy as np
import pytest
import torch

import br_amd
from br_amd import _lib, abundance, countops, keyfile
from br_amd.set import CountList, joint_counts_device
from tests.test_gpu_countops import (N_READS, TABLE, _broken_keys, _counter, _list_of, _sample, _saved, _shape_cases, _table, _write, dev,
                                     pair_counts, small_counts, u8, u64)
from tests.test_gpu_setops import forward_kmers
from tests.test_gpu_streams import Lane, decoy, lane, operation, probe, ptr, reads  # noqa: F401

pytestmark = pytest.mark.gpu

TILE, PT, CORNER = countops.TILE, countops.PER_THREAD, countops.JOINT_CORNER
SENTINEL = -0x1111111111111112  # 0xEEEE... as int64
_cache = {}


def run_joint(a, b, stream=None):
    """(J, sizes3) of the raw entry; d_joint is filled with the sentinel first and what it holds afterwards is kept in
    run_joint.left, success or not"""
    (ka, ca), (kb, cb) = (u64(a[0]), u8(a[1])), (u64(b[0]), u8(b[1]))
    dka, dca, dkb, dcb = dev(ka), dev(ca), dev(kb), dev(cb)
    dj = torch.full((65536,), SENTINEL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    try:
        s3 = joint_counts_device(dka.data_ptr() if ka.size else None, dca.data_ptr() if ka.size else None, ka.size,
                                 dkb.data_ptr() if kb.size else None, dcb.data_ptr() if kb.size else None, kb.size, dj.data_ptr(), stream)
    finally:
        torch.cuda.synchronize()
        run_joint.left = dj.cpu().numpy()
    return run_joint.left.view(np.uint64).reshape(256, 256), s3


def check_joint(name, a, b):
    a, b = (u64(a[0]), u8(a[1])), (u64(b[0]), u8(b[1]))
    want = countops.joint(*a, *b)
    got, s3 = run_joint(a, b)
    assert np.array_equal(got, want), (name, np.argwhere(got != want)[:8].tolist())
    assert s3 == countops.sizes(a[0], b[0]), name
    return want


# ---- raw entry: key shapes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("total", [0, 1, 2, PT - 1, PT + 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
def test_raw_sizes_around_thread_and_tile(total):
    rng = np.random.default_rng(total)
    for na in sorted({0, total // 3, total // 2, total}):
        nb = total - na
        hi = max(2 * total, 4)  # about half of the smaller list is in the other one
        ka, kb = _sample(rng, na, hi), _sample(rng, nb, hi)
        want = check_joint((total, na), (ka, small_counts(ka, 1)), (kb, small_counts(kb, 2)))
        assert int(want.sum()) == np.union1d(ka, kb).size


@pytest.mark.parametrize("name,a,b", list(_shape_cases()), ids=[c[0] for c in _shape_cases()])
def test_raw_shapes(name, a, b):
    a, b = u64(a), u64(b)
    ca, cb = pair_counts(a, b)
    want = check_joint(name, (a, ca), (b, cb))
    if np.isin(a, b).any():
        assert want[CORNER:, CORNER:].any() and (name == "a == b" or want[1:CORNER, 0].any() or want[0, 1:CORNER].any())
    # the same keys with every count small: a handful of bins takes them all
    check_joint(name + ", small counts", (a, 1 + (a % np.uint64(3)).astype(np.uint8)), (b, 1 + (b % np.uint64(2)).astype(np.uint8)))


# ---- raw entry: count shapes ---------------------------------------------------------------------------------------------
def _half_shared():
    """about 2 TILE keys in all, about half of them in both lists"""
    if "half" not in _cache:
        rng = np.random.default_rng(77)
        pool = _sample(rng, 3 * TILE // 2 + 5, 1 << 40)
        shared = rng.random(pool.size) < 1 / 3
        side = rng.random(pool.size) < 0.5
        _cache["half"] = (pool[shared | side], pool[shared | ~side])
        ka, kb = _cache["half"]
        assert abs(np.intersect1d(ka, kb).size - (ka.size + kb.size) // 4) < 200 and abs(ka.size + kb.size - 2 * TILE) < 300
    return _cache["half"]


def test_counts_all_in_a_few_corner_bins():
    ka, kb = _half_shared()
    rng = np.random.default_rng(1)
    want = check_joint("1..4", (ka, rng.integers(1, 5, ka.size)), (kb, rng.integers(1, 5, kb.size)))
    assert not want[5:].any() and not want[:, 5:].any() and np.count_nonzero(want) == 24 and int(want.max()) > 50
    # hotter still: every count 1, three bins
    want = check_joint("ones", (ka, np.ones(ka.size, np.uint8)), (kb, np.ones(kb.size, np.uint8)))
    assert np.count_nonzero(want) == 3 and int(want[1, 1]) == np.intersect1d(ka, kb).size


def test_counts_of_pair_counts():
    ka, kb = _half_shared()
    check_joint("pair_counts", (ka, pair_counts(ka, kb)[0]), (kb, pair_counts(ka, kb)[1]))


def test_counts_at_the_corners_edge():
    ka, kb = _half_shared()
    rng = np.random.default_rng(2)
    values = np.array([CORNER - 1, CORNER, 255], dtype=np.uint8)
    want = check_joint("edge", (ka, values[rng.integers(0, 3, ka.size)]), (kb, values[rng.integers(0, 3, kb.size)]))
    for ca, cb in ((CORNER - 1, 0), (0, CORNER), (255, 255), (CORNER - 1, CORNER - 1), (CORNER - 1, CORNER), (CORNER, CORNER - 1)):
        assert int(want[ca, cb]) > 0, (ca, cb)
    assert np.count_nonzero(want) == 15


def test_counts_all_outside_the_corner():
    ka, kb = _half_shared()
    rng = np.random.default_rng(3)
    want = check_joint("large", (ka, rng.integers(CORNER, 256, ka.size)), (kb, rng.integers(CORNER, 256, kb.size)))
    assert not want[1:CORNER].any() and not want[:, 1:CORNER].any() and want[CORNER:, CORNER:].any() and want[CORNER:, 0].any()


def test_one_array_for_both_inputs():
    a = u64(np.arange(0, 3 * TILE, 2))
    ca = small_counts(a)
    da, dc = dev(a), dev(ca)
    dj = torch.full((65536,), SENTINEL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert joint_counts_device(da.data_ptr(), dc.data_ptr(), a.size, da.data_ptr(), dc.data_ptr(), a.size, dj.data_ptr()) == (a.size,) * 3
    torch.cuda.synchronize()
    J = dj.cpu().numpy().view(np.uint64).reshape(256, 256)
    assert np.array_equal(J, np.diag(np.bincount(ca, minlength=256).astype(np.uint64))) and int(J.sum()) == a.size


# ---- raw entry: the grid -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [1, 3, 7])
def test_raw_blocks_loop_over_tiles(monkeypatch, grid):
    """41 tiles through 1, 3 and 7 blocks: a block's corner takes many tiles before its one flush, and the table is summed
    across blocks"""
    monkeypatch.setenv("BRX_READ_GRID", str(grid))
    if "trips" not in _cache:
        rng = np.random.default_rng(40)
        n = 40 * TILE + 77
        ka, kb = _sample(rng, n // 2, 2 * n), _sample(rng, n - n // 2, 2 * n)
        a, b = (ka, small_counts(ka, 3)), (kb, small_counts(kb, 4))
        _cache["trips"] = (a, b, countops.joint(*a, *b))
    a, b, want = _cache["trips"]
    got, s3 = run_joint(a, b)
    assert np.array_equal(got, want) and s3 == countops.sizes(a[0], b[0]) and int(want[1, 0]) > 2000 and int(want[1, 1]) > 100


# ---- raw entry: refusals -------------------------------------------------------------------------------------------------
def _untouched_after(a, b):
    with pytest.raises(_lib.BrxError) as ei:
        run_joint(a, b)
    assert ei.value.status == _lib.BRX_ERR_ARG
    assert (run_joint.left == SENTINEL).all()
    return str(ei.value)


@pytest.mark.parametrize("name,bad,other", list(_broken_keys()), ids=[c[0] for c in _broken_keys()])
def test_raw_refuses_unordered_and_repeated_keys(name, bad, other):
    for a, b in ((bad, other), (other, bad)):
        assert "ascend" in _untouched_after((a, np.ones(a.size, np.uint8)), (b, np.ones(b.size, np.uint8))), name


def test_raw_refuses_a_zero_count():
    good = np.arange(0, 6 * TILE, 2, dtype=np.uint64)
    other = np.arange(1, 2 * TILE, 3, dtype=np.uint64)
    none = (np.zeros(0, np.uint64), np.zeros(0, np.uint8))
    c = np.full(good.size, 3, np.uint8)
    c[1234] = 0
    assert "count of 0" in _untouched_after((good, c), (other, np.ones(other.size, np.uint8)))
    assert "count of 0" in _untouched_after((other, np.ones(other.size, np.uint8)), (good, c))
    c = np.full(good.size, 3, np.uint8)
    c[TILE] = 0  # A empty: tile 0 is B[0 .. TILE), and B[TILE] is the halo behind its piece
    assert "count of 0" in _untouched_after(none, (good, c))


def test_raw_refuses_a_joint_that_overlaps_an_input():
    n = 65536 + 2 * TILE
    dk = dev(np.arange(n, dtype=np.uint64))
    dc = torch.ones(8 * 65536 + n, dtype=torch.uint8, device="cuda")
    spare = torch.full((65536,), SENTINEL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    lists = (dk.data_ptr(), dc.data_ptr(), TILE, dk.data_ptr() + 8 * (n - TILE), dc.data_ptr() + 8 * 65536, TILE)
    for dj in (dk.data_ptr() + 8 * (TILE - 1),           # over the last key of A
               dk.data_ptr() + 8 * (n - TILE - 65535),   # over the first key of B
               dc.data_ptr() + TILE - 8,                 # over the last counts of A
               dc.data_ptr() + 8):                       # the counts of A inside it; its end over the first count of B
        with pytest.raises(_lib.BrxError) as ei:
            joint_counts_device(*lists, dj)
        assert ei.value.status == _lib.BRX_ERR_ARG and "overlap" in str(ei.value)
    torch.cuda.synchronize()
    assert (dk.cpu().numpy() == np.arange(n)).all() and (dc.cpu().numpy() == 1).all()
    with pytest.raises(_lib.BrxError) as ei:
        joint_counts_device(*lists, None)
    assert ei.value.status == _lib.BRX_ERR_ARG
    # disjoint arrays pass: the two lists share no key
    assert joint_counts_device(*lists, spare.data_ptr()) == (TILE, TILE, 0)
    torch.cuda.synchronize()
    J = spare.cpu().numpy().view(np.uint64).reshape(256, 256)
    assert (int(J[1, 0]), int(J[0, 1]), int(J.sum())) == (TILE, TILE, 2 * TILE)


# ---- stream order of the raw entry ---------------------------------------------------------------------------------------
def test_raw_entry_reads_its_inputs_in_stream_order(lane, reads):
    """the four arrays hold a decoy of identical sizes until the lane's delay has run: the joint is the real lists'"""
    k = 13
    ka, ca = abundance.count_table([abundance.canonical_hashes(r, k) for r in reads[:24]])
    kb, cb = abundance.count_table([abundance.canonical_hashes(r, k) for r in reads[12:36]])
    real = {"ka": ka, "ca": ca.astype(np.uint8), "kb": kb, "cb": cb.astype(np.uint8)}
    rng = np.random.default_rng(9)
    fake = {"ka": _sample(rng, ka.size, 1 << (2 * k - 1)), "ca": rng.integers(1, 200, ka.size).astype(np.uint8),
            "kb": _sample(rng, kb.size, 1 << (2 * k - 1)), "cb": rng.integers(1, 200, kb.size).astype(np.uint8)}

    @operation(lambda arrays: {"j": (65536, "int64")})
    def run(ctx, inp, out):
        s3 = joint_counts_device(ptr(inp["ka"]), ptr(inp["ca"]), inp["ka"].numel(), ptr(inp["kb"]), ptr(inp["cb"]), inp["kb"].numel(),
                                 ptr(out["j"]), ctx.stream)
        return s3, ctx.fetch(out["j"]).tobytes()

    s3, joint = probe(lane, run, fake, real)
    want = countops.joint(real["ka"], real["ca"], real["kb"], real["cb"])
    assert s3 == countops.sizes(ka, kb) and s3[2] > 100 and joint == want.tobytes()


# ---- objects -------------------------------------------------------------------------------------------------------------
def _halves(raw_reads, k):
    half = N_READS // 2
    a = CountList.from_counter(_counter(raw_reads[:half], k, TABLE))
    b = CountList.from_counter(_counter(raw_reads[half:N_READS], k, TABLE))
    return a, b


@pytest.mark.parametrize("k", [11, 25])
def test_compare_of_two_halves(raw_reads, k):
    a, b = _halves(raw_reads, k)
    a_np, b_np = a.to_numpy(), b.to_numpy()
    assert np.array_equal(a_np[0], _table(raw_reads, k, 0, N_READS // 2)[0]) and b.n > 1000
    a.prepare_lookup()  # a directory is neither needed nor disturbed: A has one, B has none
    info = a.lookup_info()
    want = countops.joint(*a_np, *b_np)
    either = int(want.sum())
    want[0, 0] = (1 << (2 * k - 1)) - either
    res = a.compare(b)
    J = res["joint"]
    assert J.dtype == np.uint64 and J.shape == (256, 256) and np.array_equal(J, want) and np.array_equal(a.joint(b), want)
    assert np.array_equal(J.sum(axis=1), a.spectrum()) and np.array_equal(J.sum(axis=0), b.spectrum())
    summary = countops.compare_summary(want, k)
    assert {name: res[name] for name in summary} == summary and (res["floor_a"], res["floor_b"]) == (1, 1)
    sizes = countops.sizes(a_np[0], b_np[0])
    assert (res["a"], res["b"], res["both"], res["either"]) == sizes + (either,) and 0 < res["both"] < min(a.n, b.n)
    assert a.compare_stats["both"] == sizes[2] and a.compare_stats["either"] == either and a.compare_stats["ns_wall"] > 0
    assert 0 < res["jaccard"] < 1 and 0 < res["completeness"] < 1 and 0 < res["qv"] < 60
    res2 = a.compare(b, min_a=2, min_b=3)
    assert {name: res2[name] for name in summary} == countops.compare_summary(want, k, 2, 3) and res2["a_solid"] < res["a_solid"]
    # the other way round is the transpose
    assert np.array_equal(b.joint(a), want.T)
    # a list with itself
    same = a.compare(a)
    assert np.array_equal(same["joint"], np.diag(a.spectrum())) and same["jaccard"] == 1.0 and same["qv"] == float("inf")
    assert same["completeness"] == 1.0 and same["both"] == a.n
    # only read, the directory as it was and still answering
    assert all(np.array_equal(x, y) for x, y in zip(a.to_numpy() + b.to_numpy(), a_np + b_np))
    assert a.lookup_info() == info and a.lookup_ready and not b.lookup_ready
    assert np.array_equal(a.get_counts(forward_kmers(a_np[0][::97])), a_np[1][::97])


def test_compare_with_a_floored_list_and_an_empty_one(raw_reads):
    k = 25
    full, b = _halves(raw_reads, k)
    a3 = CountList.from_keyfile(io.BytesIO(_saved(full, 3)))
    assert a3.floor == 3 and 10 < a3.n < full.n
    res = a3.compare(b)
    want = countops.joint(*a3.to_numpy(), *b.to_numpy())
    want[0, 0] = (1 << (2 * k - 1)) - int(want.sum())
    assert (res["floor_a"], res["floor_b"]) == (3, 1) and np.array_equal(res["joint"], want)
    assert not res["joint"][1:3].any() and res["joint"][3:].any()
    assert np.array_equal(res["joint"].sum(axis=1), a3.spectrum()) and np.array_equal(res["joint"].sum(axis=0), b.spectrum())
    # from 3 up it is the unfloored list's joint; what the floor dropped has moved to row 0
    whole = full.joint(b)
    assert np.array_equal(res["joint"][3:], whole[3:]) and np.array_equal(res["joint"][0, 1:], whole[:3, 1:].sum(axis=0))
    back = b.compare(a3)
    assert (back["floor_a"], back["floor_b"]) == (1, 3) and np.array_equal(back["joint"], want.T) and not back["joint"][:, 1:3].any()
    none = _list_of(np.zeros(0, np.uint64), np.zeros(0, np.uint8), k)
    res = none.compare(b)
    assert int(res["joint"][0, 0]) == (1 << 49) - b.n and np.array_equal(res["joint"][0], b.spectrum()) and not res["joint"][1:].any()
    assert (res["a"], res["b"], res["jaccard"]) == (0, b.n, 0.0) and np.isnan(res["qv"])
    res = none.compare(none)
    assert int(res["joint"][0, 0]) == 1 << 49 and int(res["joint"].sum()) == 1 << 49


def test_compare_refuses_other_operands(raw_reads):
    a11, a15 = _list_of(*_table(raw_reads, 11, 0, 10), 11), _list_of(*_table(raw_reads, 15, 0, 10), 15)
    with pytest.raises(_lib.BrxError) as ei:
        a11.compare(a15)
    assert ei.value.status == _lib.BRX_ERR_ARG and "k = 11" in str(ei.value) and "k = 15" in str(ei.value)
    if _lib.device_count() > 1:
        keys, counts = _table(raw_reads, 11, 0, 10)
        far = CountList.from_keyfile(io.BytesIO(keyfile.encode(11, keys, counts, floor=1)), device=1)
        with pytest.raises(_lib.BrxError) as ei:
            a11.joint(far)
        assert ei.value.status == _lib.BRX_ERR_ARG and "device 0" in str(ei.value) and "device 1" in str(ei.value)
    with pytest.raises(TypeError):
        a11.compare(br_amd.Pcon.new(11))
    with pytest.raises(ValueError):
        a11.compare(a11, min_a=0)
    J = np.zeros(65536, dtype=np.uint64)
    assert _lib.lib().brx_counts_compare(a11._h, None, J.ctypes.data_as(_lib.C.POINTER(_lib.C.c_uint64)), None) == _lib.BRX_ERR_ARG
    assert _lib.lib().brx_counts_compare(a11._h, a11._h, None, None) == _lib.BRX_ERR_ARG and not J.any()


# ---- command line --------------------------------------------------------------------------------------------------------
def test_cli_compare_report(tmp_path, golden_dir, raw_reads):
    from br_amd import cli
    k = 15
    raw = os.path.join(golden_dir, "raw.fasta")
    p = lambda name: str(tmp_path / name)
    a_np, b_np, c_np = _table(raw_reads, k, 0, 24), _table(raw_reads, k, 24, N_READS), _table(raw_reads, k, 8, 60)
    keep = c_np[1] >= 2
    _write(p("a.keys"), keyfile.encode(k, *a_np, floor=1))
    _write(p("b.keys"), keyfile.encode(k, *b_np, floor=1))
    _write(p("c.keys.gz"), keyfile.encode(k, c_np[0][keep], c_np[1][keep], floor=2), zipped=True)
    common = ["-i", raw, "-c", "one", "-s"]
    lists = ["count", "-i", p("a.keys"), "--counts-add", p("b.keys")]
    assert cli.main(common + ["-o", p("1.fa")] + lists + ["--counts-compare", p("c.keys.gz"), "--compare-report", p("r.tsv"), "-a", "1",
                                                          "--save-counts", p("1.keys")]) == 0
    assert cli.main(common + ["-o", p("2.fa")] + lists + ["-a", "1", "--save-counts", p("2.keys")]) == 0
    ab = countops.combine(*a_np, *b_np, "add")
    want = countops.joint(*ab, c_np[0][keep], c_np[1][keep])
    report = countops.compare_report(k, 1, 2, want, min_a=2, min_b=1)
    assert open(p("r.tsv"), "rb").read() == report and report.count(b"\n") > 40 and b"#floor_b\t2\n#min_a\t2\n#min_b\t1\n" in report
    assert open(p("1.fa"), "rb").read() == open(p("2.fa"), "rb").read() and os.path.getsize(p("1.fa")) > 1000
    assert open(p("1.keys"), "rb").read() == open(p("2.keys"), "rb").read() == keyfile.encode(k, *ab, floor=1)
    # the flags alone send `count` down the list route; a threshold selector sets min_a
    assert cli.main(common + ["-o", p("3.fa"), "count", "-i", p("a.keys"), "--counts-compare", p("b.keys"), "--compare-report", p("r3.tsv"),
                              "first-minimum"]) == 0
    from br_amd import spectrum
    thr = spectrum.get_threshold(countops.spectrum(k, a_np[1]), "first-minimum", 0.0)
    assert open(p("r3.tsv"), "rb").read() == countops.compare_report(k, 1, 1, countops.joint(*a_np, *b_np), min_a=thr + 1, min_b=1)
    # refusals
    for given, missing in (("--counts-compare", "--compare-report"), ("--compare-report", "--counts-compare")):
        with pytest.raises(SystemExit) as ei:
            cli.main(common + ["-o", p("x.fa")] + lists + [given, p("x"), "-a", "1"])
        assert f"{given} was given without {missing}" in str(ei.value) and not os.path.exists(p("x.fa")) and not os.path.exists(p("x"))
    _write(p("k11.keys"), keyfile.encode(11, *_table(raw_reads, 11, 0, 5), floor=1))
    with pytest.raises(SystemExit) as ei:
        cli.main(common + ["-o", p("y.fa")] + lists + ["--counts-compare", p("k11.keys"), "--compare-report", p("y.tsv"), "-a", "1"])
    assert str(ei.value) == "Error: --counts-compare %s: k = 11, the counts in use have k = 15" % p("k11.keys")
    assert not os.path.exists(p("y.tsv"))
