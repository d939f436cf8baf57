"""Solid coverage of reads on the GPU (include/brx.h "coverage", br_amd/csrc/brx_cover.hip): per-base flags, per-read
statistics, the masked and the split form.  Everything is compared exactly, read by read, against arrays derived from
the oracle's `Solid.mask` through the numpy statement of the definitions (br_amd/cover.py, itself checked against a
brute-force loop in test_cover_cpu.py).  No tolerances, no sampling."""
import threading

import numpy as np
import pytest

import br_amd
from br_amd import _lib, cover, synth
from br_amd.set import pack_reads
from oracle import oracle as O

pytestmark = pytest.mark.gpu

METHODS = ["one", "two", "graph", "greedy", "gap_size"]


def oracle_flags(ref, read):
    k = ref.k
    n = max(len(read) - k + 1, 0)
    solid = np.unpackbits(ref.mask(read), bitorder="little")[:n].astype(bool)
    return cover.flags_from_solid(solid, len(read), k)


def oracle_cover(ref, reads):
    """(flags per read, stats array) from the oracle"""
    fl = [oracle_flags(ref, r) for r in reads]
    st = np.zeros(len(reads), dtype=cover.STATS_DTYPE)
    for i, f in enumerate(fl):
        st[i] = cover.stats_from_flags(f, ref.k)
    return fl, st


def expected_split(reads, flags, min_len):
    out = []
    for i, (r, f) in enumerate(zip(reads, flags)):
        out += [(i, s, b) for s, b in cover.split_read(r, (f & cover.COVERED) != 0, min_len)]
    return out


def check_all(gs, reads, want_fl, want_st, min_lens=(0,)):
    """flags, stats, masked form and split form of `reads` through the host entry"""
    got_fl, got_st = gs.cover_reads(reads)
    assert len(got_fl) == len(reads)
    for i, (g, w) in enumerate(zip(got_fl, want_fl)):
        assert np.array_equal(g, w), f"flags of read {i} (n={len(reads[i])})"
    for nm in cover.STATS_DTYPE.names:
        assert np.array_equal(got_st[nm], want_st[nm]), nm
    masked = gs.mask_reads(reads)
    for i, (r, f) in enumerate(zip(reads, want_fl)):
        assert masked[i] == cover.mask_read(r, (f & cover.COVERED) != 0), f"masked read {i}"
    for ml in min_lens:
        assert gs.split_reads(reads, ml) == expected_split(reads, want_fl, ml), f"split min_len={ml}"


def covered_fraction(st, reads):
    return float(st["covered"].astype(np.int64).sum()) / sum(len(r) for r in reads)


# ---- the fixture set: k = 11, bit vector ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fixture_case(raw_reads, solid_fixture_bytes):
    ref = O.Solid.from_bytes(solid_fixture_bytes)
    fl, st = oracle_cover(ref, raw_reads)
    return ref, fl, st


def test_fixture_host_entry(raw_reads, solid_fixture_bytes, fixture_case):
    _, fl, st = fixture_case
    assert len(raw_reads) == 206
    assert int(st["kmers"].sum()) == 2_517_532 and int(st["solid"].sum()) == 1_883_972
    assert int(st["covered"].sum()) == 2_424_946 and int(st["runs"].sum()) == 17_836
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    check_all(gs, raw_reads, fl, st, min_lens=(0, 100, 500))


def test_fixture_device_entry(raw_reads, solid_fixture_bytes, fixture_case):
    import torch
    _, fl, st = fixture_case
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    hb, ho = pack_reads(raw_reads)
    n, total = len(raw_reads), int(ho[-1])
    stream = torch.cuda.current_stream().cuda_stream
    db, do = torch.from_numpy(hb).cuda(), torch.from_numpy(ho.astype(np.int64)).cuda()
    d_fl = torch.full((total,), 0xee, dtype=torch.uint8, device="cuda")
    d_mk = torch.zeros(total, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n, 4), -1, dtype=torch.int32, device="cuda")
    gs.cover_batch_device(db.data_ptr(), do.data_ptr(), n, total, d_fl.data_ptr(), d_mk.data_ptr(), d_st.data_ptr(), stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_fl.cpu().numpy(), np.concatenate(fl))
    got_st = d_st.cpu().numpy().view(np.uint32)
    for j, nm in enumerate(cover.STATS_DTYPE.names):
        assert np.array_equal(got_st[:, j], st[nm]), nm
    want_mk = b"".join(cover.mask_read(r, (f & cover.COVERED) != 0) for r, f in zip(raw_reads, fl))
    assert d_mk.cpu().numpy().tobytes() == want_mk
    # masked in place, stats alone, flags alone
    d_b2 = db.clone()
    gs.cover_batch_device(d_b2.data_ptr(), do.data_ptr(), n, total, None, d_b2.data_ptr(), None, stream)
    torch.cuda.synchronize()
    assert d_b2.cpu().numpy().tobytes() == want_mk
    d_st.fill_(-1)
    gs.cover_batch_device(db.data_ptr(), do.data_ptr(), n, total, None, None, d_st.data_ptr(), stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_st.cpu().numpy().view(np.uint32)[:, 3], st["runs"])
    # a masked batch has the same k-mers: covering it again gives the same flags
    d_fl.fill_(0xee)
    gs.cover_batch_device(d_b2.data_ptr(), do.data_ptr(), n, total, d_fl.data_ptr(), None, None, stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_fl.cpu().numpy(), np.concatenate(fl))


def split_device(gs, db, do, n, total, min_len, out_cap, piece_cap, stream):
    """one call of the device split entry: (status, n_pieces, out_total, tensors)"""
    import ctypes as C
    import torch
    d_out = torch.zeros(max(out_cap, 1), dtype=torch.uint8, device="cuda")
    d_oo = torch.zeros(piece_cap + 1, dtype=torch.int64, device="cuda")
    d_pr = torch.zeros(max(piece_cap, 1), dtype=torch.int32, device="cuda")
    d_ps = torch.zeros(max(piece_cap, 1), dtype=torch.int64, device="cuda")
    np_, tot = C.c_uint32(0), C.c_uint64(0)
    st = _lib.lib().brx_set_cover_split_batch_device(gs._h, db.data_ptr(), do.data_ptr(), n, total, min_len, d_out.data_ptr(), out_cap,
                                                     d_oo.data_ptr(), d_pr.data_ptr(), d_ps.data_ptr(), piece_cap, C.byref(np_),
                                                     C.byref(tot), stream)
    torch.cuda.synchronize()
    return st, np_.value, tot.value, (d_out, d_oo, d_pr, d_ps)


@pytest.mark.parametrize("min_len", [0, 100, 500])
def test_fixture_split_device_entry_and_overflow_contract(raw_reads, solid_fixture_bytes, fixture_case, min_len):
    import torch
    _, fl, _ = fixture_case
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    want = expected_split(raw_reads, fl, min_len)
    want_bytes = sum(len(b) for _, _, b in want)
    hb, ho = pack_reads(raw_reads)
    n, total = len(raw_reads), int(ho[-1])
    stream = torch.cuda.current_stream().cuda_stream
    db, do = torch.from_numpy(hb).cuda(), torch.from_numpy(ho.astype(np.int64)).cuda()
    # too small: the needed sizes come back with BRX_ERR_OVERFLOW ...
    for out_cap, piece_cap in ((0, 0), (want_bytes - 1, len(want)), (want_bytes, len(want) - 1)):
        st, p, tot, _ = split_device(gs, db, do, n, total, min_len, out_cap, piece_cap, stream)
        assert st == _lib.BRX_ERR_OVERFLOW
        assert (p, tot) == (len(want), want_bytes)
    # ... and the retry with them succeeds
    st, p, tot, (d_out, d_oo, d_pr, d_ps) = split_device(gs, db, do, n, total, min_len, tot, p, stream)
    assert st == _lib.BRX_OK and (p, tot) == (len(want), want_bytes)
    out, oo = d_out.cpu().numpy(), d_oo.cpu().numpy()
    pr, ps = d_pr.cpu().numpy(), d_ps.cpu().numpy()
    got = [(int(pr[i]), int(ps[i]), out[int(oo[i]):int(oo[i + 1])].tobytes()) for i in range(p)]
    assert got == want
    # the bounds of the header hold
    assert tot <= total and p <= n + total // (max(11, min_len, 1) + 1)


# ---- sets built on the GPU: key list + index with a lazy bit vector, sparse table -----------------------------------

def _built_case(raw_reads, k, env, monkeypatch):
    for name, val in env.items():
        monkeypatch.setenv(name, val)
    reads = raw_reads[:150]
    gs = br_amd.Pcon.from_count(reads, k, 1)
    ref = O.Solid.sparse_from_count(k, reads, 1)
    assert gs.popcount() == ref.popcount()
    return gs, ref, reads


@pytest.mark.parametrize("k,env", [(15, {}), (19, {}), (21, {}), (15, {"BRX_INDEX": "0"}),
                                   (15, {"BRX_FORCE_SPARSE": "1", "BRX_INDEX_LOG_LINES": "4"})])
def test_built_sets(raw_reads, k, env, monkeypatch):
    gs, ref, reads = _built_case(raw_reads, k, env, monkeypatch)
    if k == 19:
        assert gs.bits_state() == 1
    if k == 21 or "BRX_FORCE_SPARSE" in env:
        assert gs.is_sparse()
    fl, st = oracle_cover(ref, reads)
    assert 0.5 < covered_fraction(st, reads) < 0.99  # neither all-true nor all-false would pass
    check_all(gs, reads, fl, st, min_lens=(0, 100))
    if k == 19:
        assert gs.bits_state() == 1  # the lazy bit vector stayed lazy
        assert gs.index_info()["valid"]
    if "BRX_FORCE_SPARSE" in env:
        info = gs.index_info()
        assert info["overflow_keys"] > info["keys"] // 10  # chained, overflowing lines


@pytest.mark.parametrize("k", [25, 31])
def test_presence_only_sparse_sets(raw_reads, k):
    gs = br_amd.Pcon.from_fasta(raw_reads[:75], k)
    assert gs.is_sparse()
    ref = O.Solid.sparse_from_count(k, raw_reads[:75], 0)
    reads = raw_reads[:150]
    assert sum(len(r) for r in reads) == 1_758_473
    fl, st = oracle_cover(ref, reads)
    assert 0.5 < covered_fraction(st, reads) < 0.99
    check_all(gs, reads, fl, st, min_lens=(0, 100))


# ---- the shape of a batch does not matter --------------------------------------------------------------------------------

def test_batch_shape_does_not_matter(raw_reads, solid_fixture_bytes, fixture_case):
    ref, fl, st = fixture_case
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    for step in (1, 7, 64):
        for lo in range(0, len(raw_reads), step):
            sub = raw_reads[lo:lo + step]
            got_fl, got_st = gs.cover_reads(sub)
            for j, g in enumerate(got_fl):
                assert np.array_equal(g, fl[lo + j]), (step, lo + j)
            assert np.array_equal(got_st, st[lo:lo + step]), (step, lo)
    # empty reads and reads shorter than k in between
    mixed, origin = [], []
    shorts = [b"", b"A", b"ACGTACGTAC", b"ACGTACGTACG", b"NNNNNNNNNNNN", b""]
    for i, r in enumerate(raw_reads[:60]):
        mixed.append(shorts[i % len(shorts)])
        origin.append(None)
        mixed.append(r)
        origin.append(i)
    mixed.append(b"")
    origin.append(None)
    want_fl = [fl[o] if o is not None else oracle_flags(ref, m) for m, o in zip(mixed, origin)]
    want_st = np.zeros(len(mixed), dtype=cover.STATS_DTYPE)
    for i, f in enumerate(want_fl):
        want_st[i] = cover.stats_from_flags(f, 11)
    check_all(gs, mixed, want_fl, want_st, min_lens=(0, 100))
    # nothing but empty reads; no reads at all
    got_fl, got_st = gs.cover_reads([b"", b""])
    assert [f.size for f in got_fl] == [0, 0] and not got_st["kmers"].any()
    assert gs.split_reads([b"", b""], 0) == [] and gs.split_reads([], 0) == []
    got_fl, got_st = gs.cover_reads([])
    assert got_fl == [] and got_st.size == 0


def test_many_short_reads(raw_reads, solid_fixture_bytes):
    ref = O.Solid.from_bytes(solid_fixture_bytes)
    rng = np.random.default_rng(5)
    pool = b"".join(raw_reads[:40])
    reads = []
    for _ in range(5000):
        n = int(rng.integers(30, 71))
        at = int(rng.integers(0, len(pool) - n))
        reads.append(pool[at:at + n])
    fl, st = oracle_cover(ref, reads)
    assert st["covered"].any()
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    check_all(gs, reads, fl, st, min_lens=(0, 40))
    # one by one, a sample: the same per-read results
    for i in range(0, 5000, 250):
        g_fl, g_st = gs.cover_reads([reads[i]])
        assert np.array_equal(g_fl[0], fl[i]) and np.array_equal(g_st, st[i:i + 1])


# ---- after a correction ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method", METHODS)
def test_after_a_correction(raw_reads, solid_fixture_bytes, method):
    ref = O.Solid.from_bytes(solid_fixture_bytes)
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    sub = raw_reads[:40] if method == "greedy" else raw_reads
    om = O.build_methods(ref, [method], 5, 7)
    want_reads = [O.correct_record(om, r, False) for r in sub]
    got_reads = br_amd.Chain(gs, [(method, 5, 7)], two_side=False).correct_reads(sub)
    fl, st = oracle_cover(ref, want_reads)
    got_fl, got_st = gs.cover_reads(got_reads)
    assert np.array_equal(got_st, st)
    if method in ("one", "greedy"):
        for i, (g, w) in enumerate(zip(got_fl, fl)):
            assert np.array_equal(g, w), (method, i)
    if method == "one" and len(sub) == 206:  # what the oracle gave on the CPU (test_cover_cpu.py pins the same)
        assert sum(len(r) for r in want_reads) == 2_520_330
        assert (int(st["solid"].sum()), int(st["covered"].sum()), int(st["runs"].sum())) == (2_061_179, 2_440_124, 13_612)


# ---- two threads, two streams, one set -------------------------------------------------------------------------------------

def test_two_threads_on_two_streams(raw_reads):
    import torch
    k = 19
    reads = raw_reads[:150]
    gs = br_amd.Pcon.from_count(reads, k, 1)
    assert gs.bits_state() == 1
    hb, ho = pack_reads(reads)
    n, total = len(reads), int(ho[-1])
    db, do = torch.from_numpy(hb).cuda(), torch.from_numpy(ho.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    results, errors = {}, []

    def work(tag, rounds):
        try:
            s = torch.cuda.Stream()
            for _ in range(rounds):
                d_fl = torch.zeros(total, dtype=torch.uint8, device="cuda")
                d_st = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                gs.cover_batch_device(db.data_ptr(), do.data_ptr(), n, total, d_fl.data_ptr(), None, d_st.data_ptr(), s.cuda_stream)
                s.synchronize()
                results.setdefault(tag, []).append((d_fl.cpu().numpy(), d_st.cpu().numpy()))
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    # the very first cover calls of the set race for the index build
    th = [threading.Thread(target=work, args=(t, 3)) for t in ("a", "b")]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    work("one", 1)
    ref = O.Solid.sparse_from_count(k, reads, 1)
    fl, st = oracle_cover(ref, reads)
    want_fl = np.concatenate(fl)
    for tag in ("a", "b", "one"):
        for g_fl, g_st in results[tag]:
            assert np.array_equal(g_fl, want_fl), tag
            assert np.array_equal(g_st.view(np.uint32)[:, 2], st["covered"]), tag
    assert gs.bits_state() == 1


# ---- scale -----------------------------------------------------------------------------------------------------------------------

def test_scale_synthetic_10kb(monkeypatch):
    k, a, n_reads, read_len = 19, 3, 2000, 10_000
    cfg = synth.config(genome_len=n_reads * read_len // 50, read_len=read_len)
    g = synth.genome_host(cfg)
    hb, ho = synth.reads_host(cfg, g, 0, n_reads)
    reads = [hb[int(ho[i]):int(ho[i + 1])].tobytes() for i in range(n_reads)]
    gs = br_amd.Pcon.from_count(reads, k, a)
    ref = O.Solid.sparse_from_count(k, reads, a)
    assert gs.popcount() == ref.popcount()
    _, st_in = oracle_cover(ref, reads)
    _, got_in = gs.cover_reads(reads)
    assert np.array_equal(got_in, st_in)
    om = O.build_methods(ref, ["one"], 5, 7)
    want_reads = [O.correct_record(om, r, False) for r in reads]
    got_reads = br_amd.Chain(gs, [("one", 5, 7)], two_side=False).correct_reads(reads)
    assert got_reads == want_reads
    _, st_out = oracle_cover(ref, want_reads)
    _, got_out = gs.cover_reads(got_reads)
    assert np.array_equal(got_out, st_out)
    assert int(got_out["solid"].astype(np.int64).sum()) > int(got_in["solid"].astype(np.int64).sum())


# ---- arguments ---------------------------------------------------------------------------------------------------------------------

def test_bad_arguments(solid_fixture_bytes):
    import ctypes as C
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    L = _lib.lib()
    offs = np.array([0, 5, 3], dtype=np.uint64)  # decreasing
    bases = np.frombuffer(b"ACGTA", dtype=np.uint8)
    fl = np.zeros(5, dtype=np.uint8)
    assert L.brx_set_cover_batch(gs._h, bases.ctypes.data, offs.ctypes.data, 2, fl.ctypes.data, None, None) == _lib.BRX_ERR_ARG
    assert L.brx_last_error()
    assert L.brx_set_cover_batch(None, bases.ctypes.data, offs.ctypes.data, 2, fl.ctypes.data, None, None) == _lib.BRX_ERR_ARG
    assert L.brx_set_cover_batch_device(gs._h, None, None, 2, 5, None, None, None, None) == _lib.BRX_ERR_ARG
    np_, tot = C.c_uint32(0), C.c_uint64(0)
    assert L.brx_set_cover_split_batch_device(gs._h, None, None, 0, 0, 0, None, 0, None, None, None, 0, None, C.byref(tot),
                                              None) == _lib.BRX_ERR_ARG


# ---- the pipeline: run_correction with an output form ----------------------------------------------------------------

EDGE = (b">r1 first read \t with   description  \r\n"
        b"ACGTACGTTTGACCAGTACGATCGATCGGGATCAGCTAGCATCGACTAGCTAGCATCGATCAGCATCGACTAGCATCGACTAGCTACGACTAGCATCAGCATCAGCT\r\n"
        b"acgtnnACGTTGCA\n"
        b"\n"
        b"GGGTTTAAACCC\r\r\n"
        b">r2\n"
        b">r3\tdesc\n"
        b"ACGT\n"
        b">r4 last one without newline at the end\n"
        b"TTGACCAGTACGATCGATCGGGATCAGCTAGCATCGACTAGCTAGCATCGATCAGCATCGACTAGCATCGACTAGCTACGACTAGCATCAGCATCAGCTAAAAAAAAAAAAAAAAAAAAAAAAAAAACCCCCCCCCCCGGGGGGGT")


def oracle_pipeline(text, ref, om, two_side, mode, min_len):
    """(FASTA text, report text, totals) of a run, from the oracle and the definitions alone"""
    from br_amd import fasta
    from br_amd.driver import COVER_KEYS, REPORT_HEADER
    import io
    out, rep = io.BytesIO(), io.BytesIO()
    rep.write(REPORT_HEADER)
    totals = dict.fromkeys(COVER_KEYS, 0)
    for name, desc, seq in fasta.read_records(io.BytesIO(text)):
        corr = O.correct_record(om, seq, two_side)
        f_in, f_out = oracle_flags(ref, seq), oracle_flags(ref, corr)
        covered = (f_out & cover.COVERED) != 0
        if mode == "mask":
            fasta.write_record(out, name, desc, cover.mask_read(corr, covered))
        elif mode == "split":
            for i, (_, piece) in enumerate(cover.split_read(corr, covered, min_len)):
                fasta.write_record(out, name + b"_%d" % (i + 1), desc, piece)
        else:
            fasta.write_record(out, name, desc, corr)
        a, z = cover.stats_from_flags(f_in, ref.k), cover.stats_from_flags(f_out, ref.k)
        for key, v in zip(COVER_KEYS, a + z):
            totals[key] += v
        rep.write(name + b"\t" + b"\t".join(b"%d" % v for v in (len(seq),) + a + (len(corr),) + z) + b"\n")
    return out.getvalue(), rep.getvalue(), totals


def _inputs(golden_dir):
    import os
    raw = open(os.path.join(golden_dir, "raw.fasta"), "rb").read()
    head = raw[:raw.index(b">", raw.index(b">", 1) + 1)]  # the first two records
    return {"fixture": raw, "empty_record": EDGE, "malformed_tail": EDGE + b"\n>\nACGT\n>r6\nACGT\n",
            "malformed_last": head + b"> no name\nACGT\n"}


@pytest.mark.parametrize("mode,min_len", [("mask", 0), ("split", 0), ("split", 200)])
@pytest.mark.parametrize("which", ["fixture", "gzip", "empty_record", "malformed_tail", "malformed_last"])
def test_pipeline_output_forms(tmp_path, golden_dir, solid_fixture_bytes, which, mode, min_len):
    import gzip
    import io
    from br_amd.driver import COVER_KEYS, run_correction
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    ref = O.Solid.from_bytes(solid_fixture_bytes)
    om = O.build_methods(ref, ["one"], 5, 7)
    methods = br_amd.build_methods(["one"], gs, 5, 7)
    text = _inputs(golden_dir)["fixture" if which == "gzip" else which]
    want_text, want_rep, want_tot = oracle_pipeline(text, ref, om, False, mode, min_len)
    if min_len == 0 or which in ("fixture", "gzip", "malformed_last"):  # (the short records have no run of 200 bases)
        assert want_text.count(b">") > 0
    if mode == "mask" and which in ("fixture", "gzip"):
        assert any(c in want_text for c in b"acgt") and any(c in want_text for c in b"ACGT")

    def source():
        if which == "gzip":
            p = tmp_path / "in.fa.gz"
            with gzip.open(p, "wb") as f:
                f.write(text)
            return gzip.open(p, "rb")
        return io.BytesIO(text)

    results = {}
    for native, batch_records in ((True, 0), (True, 7), (False, 0)):
        out, rep = io.BytesIO(), io.BytesIO()
        with source() as fi:
            st = run_correction([fi], [out], methods, False, native=native, batch_records=batch_records, output_mode=mode,
                                min_len=min_len, reports=[rep])
        results[(native, batch_records)] = (out.getvalue(), rep.getvalue())
        assert out.getvalue() == want_text, (native, batch_records)
        assert rep.getvalue() == want_rep, (native, batch_records)
        assert {k: st[k] for k in COVER_KEYS} == want_tot
        assert st["records"] == want_rep.count(b"\n") - 1
    assert results[(True, 0)] == results[(False, 0)] == results[(True, 7)]
    # totals without a report; a form without totals leaves the dict as a plain run's
    with source() as fi:
        st = run_correction([fi], [io.BytesIO()], methods, False, native=True, output_mode=mode, min_len=min_len, cover_stats=True)
    assert {k: st[k] for k in COVER_KEYS} == want_tot
    for native in (True, False):
        out = io.BytesIO()
        with source() as fi:
            st = run_correction([fi], [out], methods, False, native=native, output_mode=mode, min_len=min_len)
        assert out.getvalue() == want_text and not set(COVER_KEYS) & set(st)


def test_pipeline_report_matches_per_read_stats(golden_dir, raw_reads, solid_fixture_bytes, fixture_case):
    import io
    import os
    from br_amd.driver import COVER_KEYS, run_correction
    _, _, st_in = fixture_case
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    methods = br_amd.build_methods(["one"], gs, 5, 7)
    out, rep = io.BytesIO(), io.BytesIO()
    with open(os.path.join(golden_dir, "raw.fasta"), "rb") as fi:
        st = run_correction([fi], [out], methods, False, native=True, reports=[rep])
    lines = rep.getvalue().split(b"\n")
    assert lines[0].startswith(b"#name\tlen_in") and lines[-1] == b"" and len(lines) == 206 + 2
    rows = np.array([[int(v) for v in ln.split(b"\t")[1:]] for ln in lines[1:-1]])
    assert np.array_equal(rows[:, 0], [len(r) for r in raw_reads])
    for j, nm in enumerate(cover.STATS_DTYPE.names):
        assert np.array_equal(rows[:, 1 + j], st_in[nm]), nm
    corrected = br_amd.Chain(gs, [("one", 5, 7)], two_side=False).correct_reads(raw_reads)
    _, st_out = gs.cover_reads(corrected)
    assert np.array_equal(rows[:, 5], [len(r) for r in corrected])
    for j, nm in enumerate(cover.STATS_DTYPE.names):
        assert np.array_equal(rows[:, 6 + j], st_out[nm]), nm
    assert [st[k] for k in COVER_KEYS] == rows[:, [1, 2, 3, 4, 6, 7, 8, 9]].sum(axis=0).tolist()
    # the report changed nothing in the text: a plain run's bytes
    plain = io.BytesIO()
    with open(os.path.join(golden_dir, "raw.fasta"), "rb") as fi:
        run_correction([fi], [plain], methods, False, native=True)
    assert out.getvalue() == plain.getvalue()


def test_plain_run_through_opts_is_the_plain_run(tmp_path, golden_dir, solid_fixture_bytes):
    import ctypes as C
    import os
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    L = _lib.lib()
    specs = (_lib.Method * 2)(_lib.Method(0, 5, 7), _lib.Method(2, 5, 7))
    src = os.path.join(golden_dir, "raw.fasta")
    _lib.profile_enable(True)
    _lib.profile_reset()
    outs = []
    try:
        for i, opts in enumerate((None, _lib.OutputOpts(0, 0, -1, 0), "old")):
            dst = tmp_path / f"o{i}.fa"
            st = (C.c_uint64 * 8)()
            ifd, ofd = os.open(src, os.O_RDONLY), os.open(dst, os.O_WRONLY | os.O_CREAT, 0o644)
            try:
                if opts == "old":
                    _lib.check(L.brx_run_correction_fd(gs._h, specs, 2, False, ifd, ofd, 16, st))
                else:
                    ct = (C.c_uint64 * 8)(*([7] * 8))
                    _lib.check(L.brx_run_correction_fd_opts(gs._h, specs, 2, False, ifd, ofd, 16, C.byref(opts) if opts else None, st, ct))
                    assert list(ct) == [0] * 8
            finally:
                os.close(ifd)
                os.close(ofd)
            assert st[0] == 206
            outs.append(dst.read_bytes())
        assert outs[0] == outs[1] == outs[2] and len(outs[0]) > 2_000_000
        assert _lib.profile_get("cover")[1] == 0  # a plain run launches no cover kernel
        # ... and the timer does count when a form is asked for
        dst = tmp_path / "m.fa"
        ifd, ofd = os.open(src, os.O_RDONLY), os.open(dst, os.O_WRONLY | os.O_CREAT, 0o644)
        try:
            opts = _lib.OutputOpts(1, 0, -1, 0)
            _lib.check(L.brx_run_correction_fd_opts(gs._h, specs, 2, False, ifd, ofd, 16, C.byref(opts), None, None))
        finally:
            os.close(ifd)
            os.close(ofd)
        assert _lib.profile_get("cover")[1] > 0
        assert dst.read_bytes().upper() == outs[0].upper() and dst.read_bytes() != outs[0]
        bad = _lib.OutputOpts(3, 0, -1, 0)
        assert L.brx_run_correction_fd_opts(gs._h, specs, 2, False, 0, 1, 0, C.byref(bad), None, None) == _lib.BRX_ERR_ARG
    finally:
        _lib.profile_enable(False)


@pytest.mark.parametrize("flags,mode,min_len", [(["--mask-weak"], "mask", 0), (["--trim-split", "200"], "split", 200),
                                                 (["--trim-split=0"], "split", 0)])
def test_command_line(tmp_path, golden_dir, solid_fixture_bytes, flags, mode, min_len):
    import os
    from br_amd import cli
    ref = O.Solid.from_bytes(solid_fixture_bytes)
    om = O.build_methods(ref, ["one"], 5, 7)
    src = os.path.join(golden_dir, "raw.fasta")
    want_text, want_rep, _ = oracle_pipeline(open(src, "rb").read(), ref, om, False, mode, min_len)
    out, rep = tmp_path / "out.fa", tmp_path / "cover.tsv"
    assert cli.main(["-i", src, "-o", str(out), "-c", "one", "--cover-report", str(rep)] + flags +
                    ["solid", "-i", os.path.join(golden_dir, "raw.k11.a2.solid"), "-f", "solid"]) == 0
    assert out.read_bytes() == want_text
    assert rep.read_bytes() == want_rep
