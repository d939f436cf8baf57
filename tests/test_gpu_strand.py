"""The second scan on the reverse complement (BRX_PASS_REVCOMP), on a real MI355X, byte for byte against the composition

    rc(correct_record(M, rc(correct_record(M, s, two_side=True)), two_side=True))

of the existing CPU oracle's single scan with the byte map of br_amd/strand.py; and the reverse-complement entries
brx_revcomp_batch[_device] against strand.revcomp.
"""
import ctypes as C
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import br_amd
from br_amd import _lib, cover, fasta, strand
from br_amd.driver import COVER_KEYS, REPORT_HEADER, run_correction
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_FIVE = ["one", "two", "graph", "greedy", "gap_size"]


def rc_record(om, seq):
    first = O.correct_record(om, seq, True)
    return strand.revcomp(O.correct_record(om, strand.revcomp(first), True))


def rc_chain(gs, names, confirm=5, max_search=7):
    return br_amd.Chain(gs, [(m, confirm, max_search) for m in names], second_pass="revcomp")


def check_chain(gs, ref, names, reads, confirm=5, max_search=7, chain=None):
    om = O.build_methods(ref, list(names), confirm, max_search)
    chain = chain or rc_chain(gs, names, confirm, max_search)
    got = chain.correct_reads(list(reads))
    exp = [rc_record(om, r) for r in reads]
    bad = [i for i, (g, e) in enumerate(zip(got, exp)) if g != e]
    assert not bad, (names, bad[:10])
    st = chain.last_stats()
    assert st["lane_unwritten_units"] == 0
    return chain, got, om


# ---------------------------------------------------------------- the byte map -----------------------------------------
def _torch():
    import torch
    return torch


def _device_revcomp(reads, a=0, b=0):
    """brx_revcomp_batch_device with the bases at byte a and the output at byte b of their 16-byte aligned allocations"""
    torch = _torch()
    bases, offs = br_amd.pack_reads(reads)
    total = int(offs[-1])
    d_in = torch.zeros(total + 32, dtype=torch.uint8, device="cuda")
    d_out = torch.full((total + 48,), 0xEE, dtype=torch.uint8, device="cuda")
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    d_in[a:a + total] = torch.from_numpy(bases.copy()).cuda()
    d_off = torch.from_numpy(offs.astype(np.int64)).cuda()
    _lib.check(_lib.lib().brx_revcomp_batch_device(d_in.data_ptr() + a, d_off.data_ptr(), len(reads), total, d_out.data_ptr() + b,
                                                   torch.cuda.current_stream().cuda_stream))
    out = d_out.cpu().numpy()
    assert (out[:b] == 0xEE).all() and (out[b + total:] == 0xEE).all()  # nothing written outside the batch
    return [out[b + int(offs[i]):b + int(offs[i + 1])].tobytes() for i in range(len(reads))]


def _mixed_reads(rng, lengths):
    alphabet = np.frombuffer(b"ACGTacgtNn", dtype=np.uint8)
    reads = []
    for i, n in enumerate(lengths):
        if i % 3 == 2:
            reads.append(rng.integers(0, 256, size=int(n), dtype=np.uint8).tobytes())   # any byte at all
        else:
            reads.append(rng.choice(alphabet, size=int(n)).tobytes())
    return reads


def test_revcomp_device_every_length_and_alignment():
    rng = np.random.default_rng(5)
    lengths = [0, 1, 15, 16, 17, 31, 33, 0, 2, 47, 48, 49, 64, 100, 255, 256, 257, 1000, 4097]
    reads = _mixed_reads(rng, lengths)
    want = [strand.revcomp(r) for r in reads]
    for a in range(16):
        for b in range(16):
            assert _device_revcomp(reads, a, b) == want, (a, b)
    # every read alone, so that each length also starts at every alignment of both sides
    for r in reads[:7]:
        for a in range(16):
            assert _device_revcomp([r], a, (a * 7 + 3) % 16) == [strand.revcomp(r)]
    assert _device_revcomp([bytes(range(256))]) == [bytes(range(256)).translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))[::-1]]


def test_revcomp_host_entry_many_reads_and_one_long_read():
    rng = np.random.default_rng(6)
    reads = _mixed_reads(rng, rng.integers(0, 41, size=70_000))    # more than 2^16 reads
    assert len(reads) > 1 << 16
    got = br_amd.revcomp_reads(reads)
    assert got == [strand.revcomp(r) for r in reads]
    long_read = rng.integers(0, 256, size=5_000_011, dtype=np.uint8).tobytes()   # several MB in one read
    got = br_amd.revcomp_reads([b"ACGTN", long_read, b"", b"acgt"])
    assert got == [b"NACGT", strand.revcomp(long_read), b"", b"acgt"]
    assert br_amd.revcomp_reads([]) == [] and br_amd.revcomp_reads([b""]) == [b""]
    # involution through the GPU
    assert br_amd.revcomp_reads(br_amd.revcomp_reads(reads[:500])) == reads[:500]


def test_revcomp_bad_arguments():
    torch = _torch()
    L = _lib.lib()
    d = torch.zeros(64, dtype=torch.uint8, device="cuda")
    off = torch.tensor([0, 10], dtype=torch.int64, device="cuda")
    assert L.brx_revcomp_batch_device(d.data_ptr(), off.data_ptr(), 1, 10, d.data_ptr(), None) == _lib.BRX_ERR_ARG  # aliasing
    assert L.brx_revcomp_batch_device(d.data_ptr(), None, 1, 10, d.data_ptr() + 32, None) == _lib.BRX_ERR_ARG
    bad = np.array([0, 5, 3], dtype=np.uint64)
    buf = np.zeros(8, dtype=np.uint8)
    assert L.brx_revcomp_batch(buf.ctypes.data, bad.ctypes.data, 2, buf.ctypes.data, 0) == _lib.BRX_ERR_ARG


# ---------------------------------------------------------------- the chain --------------------------------------------
def test_chain_modes_and_arguments(solid_fixture_bytes):
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    spec = [("one", 5, 7)]
    assert br_amd.Chain(gs, spec).second_pass == "reverse"
    assert br_amd.Chain(gs, spec, two_side=True).second_pass == "none"
    for mode in ("none", "reverse", "revcomp"):
        assert br_amd.Chain(gs, spec, second_pass=mode).second_pass == mode
    h = C.c_void_p()
    arr = (_lib.Method * 1)(_lib.Method(0, 5, 7))
    assert _lib.lib().brx_chain_new_pass(gs._h, arr, 1, 3, C.byref(h)) == _lib.BRX_ERR_ARG
    assert _lib.lib().brx_chain_second_pass(None) == _lib.BRX_ERR_ARG


def test_none_and_reverse_modes_are_the_two_side_chains(raw_reads, solid_fixture_bytes):
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    reads = raw_reads[:40]
    spec = [("one", 5, 7), ("graph", 5, 7)]
    assert br_amd.Chain(gs, spec, second_pass="none").correct_reads(reads) == br_amd.Chain(gs, spec, two_side=True).correct_reads(reads)
    assert br_amd.Chain(gs, spec, second_pass="reverse").correct_reads(reads) == br_amd.Chain(gs, spec, two_side=False).correct_reads(reads)


def _oracle_set(v):
    s = O.Solid(v["k"])
    for q in v["set_seqs"]:
        s.set_seq(q.encode())
    for q in v["set_kmers"]:
        s.set(O.seq2bit(q.encode()))
    return s


def test_unit_vectors_in_revcomp_mode(unit_vectors):
    """the reference's own corrector inputs, each against the composed oracle"""
    ran = 0
    for v in unit_vectors["vectors"]:
        if v["ignored"]:
            continue
        ref = _oracle_set(v)
        gs = br_amd.Pcon.from_pcon_solid(ref.to_bytes())
        om = [O.Corrector(ref, v["method"], v["confirm"], v["max_search"])]
        chain = br_amd.Chain(gs, [(v["method"], v["confirm"], v["max_search"])], second_pass="revcomp")
        inputs = [a.encode() for a, _ in v["cases"]]
        inputs += [strand.revcomp(s) for s in inputs]
        got = chain.correct_reads(inputs)
        for s, g in zip(inputs, got):
            assert g == rc_record(om, s), v["name"]
            ran += 1
    assert ran >= 160


@pytest.mark.parametrize("names", [[m] for m in ALL_FIVE] + [ALL_FIVE], ids=ALL_FIVE + ["default_order"])
def test_raw_fasta_fixture_set(raw_reads, solid_fixture_bytes, names):
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    ref = O.Solid.from_bytes(solid_fixture_bytes)
    reads = raw_reads[:80] if len(names) > 1 or names == ["greedy"] else raw_reads
    chain, got, om = check_chain(gs, ref, names, reads)
    # the mode does something the other modes do not
    assert got != [O.correct_record(om, r, False) for r in reads]
    assert got != [O.correct_record(om, r, True) for r in reads]
    if names[0] in ("one", "graph", "gap_size") and len(names) == 1:
        assert chain.last_stats()["lane_units"] > 0   # the last pass of the second scan took the lane form


def test_fixes_count_both_scans_and_second_scan_takes_the_lane_form(raw_reads, solid_fixture_bytes):
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    ref = O.Solid.from_bytes(solid_fixture_bytes)
    for names in (["one"], ["one", "graph"]):
        om = O.build_methods(ref, names, 5, 7)   # (fresh correctors: their counters start at zero)
        chain = rc_chain(gs, names)
        got = chain.correct_reads(raw_reads)
        assert got == [rc_record(om, r) for r in raw_reads]
        both = sum(m.stats()["fixes"] for m in om)
        st = chain.last_stats()
        assert st["fixes"] == both > 0
        assert st["overflow_retries"] == 0 and st["lane_units"] > 0 and st["lane_unwritten_units"] == 0
        # one scan alone makes fewer
        one_scan = br_amd.Chain(gs, [(m, 5, 7) for m in names], second_pass="none")
        one_scan.correct_reads(raw_reads)
        assert 0 < one_scan.last_stats()["fixes"] < both


def test_second_scan_of_one_runs_the_lane_kernels_not_the_wide_groups(raw_reads, solid_fixture_bytes):
    """profile timers of one One chain: the lane pass ran for both scans, the new kernels ran once each (stage, compaction)
    and compact_kernel did not run"""
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    rc_chain(gs, ["one"]).correct_reads(raw_reads[:20])   # (set-up work outside the window: index, workspaces)
    rev = br_amd.Chain(gs, [("one", 5, 7)], second_pass="reverse")
    rev.correct_reads(raw_reads[:20])
    _lib.profile_enable(True)
    try:
        _lib.profile_reset()
        rev.correct_reads(raw_reads)
        plain = _lib.profile_all()
        assert plain.get("strand", {"launches": 0})["launches"] == 0 and plain.get("strand_compact", {"launches": 0})["launches"] == 0
        assert plain["compact"]["launches"] == 1
        _lib.profile_reset()
        rc_chain(gs, ["one"]).correct_reads(raw_reads)
        prof = _lib.profile_all()
    finally:
        _lib.profile_enable(False)
    assert prof["strand"]["launches"] == 1 and prof["strand_compact"]["launches"] == 1
    assert prof.get("compact", {"launches": 0})["launches"] == 0
    lane = {nm: v["launches"] for nm, v in prof.items() if nm.startswith("lane") and v["launches"]}
    lane_plain = {nm: v["launches"] for nm, v in plain.items() if nm.startswith("lane") and v["launches"]}
    assert lane and lane_plain
    for nm, n in lane_plain.items():       # the reverse mode runs them for its forward scan only
        assert lane.get(nm, 0) == 2 * n, (nm, lane, lane_plain)


@pytest.mark.parametrize("k,env", [(15, {}), (19, {}), (15, {"BRX_INDEX": "0"}), (19, {"BRX_INDEX": "0"})],
                         ids=["k15_lazy", "k19_lazy", "k15_noindex", "k19_noindex"])
def test_built_sets_lazy_bits_and_index_off(raw_reads, k, env, monkeypatch):
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    a = 1
    reads = raw_reads[:100]
    cnt = br_amd.Counter(k, 0)
    cnt.add_reads(reads)
    gs = cnt.finish(a)
    ref = O.Solid.from_count(k, O.count_reads(k, reads), a) if k <= 15 else O.Solid.sparse_from_count(k, reads, a)
    assert gs.popcount() == ref.popcount() > 1000
    check_chain(gs, ref, ["one"], reads)
    check_chain(gs, ref, ["graph", "gap_size"], reads[:50])


@pytest.mark.parametrize("k", [21, 25])
def test_sparse_sets(raw_reads, k):
    reads = raw_reads[:100]
    if k == 21:
        gs = br_amd.Pcon.from_count(reads, k, 1)
        ref = O.Solid.sparse_from_count(k, reads, 1)
    else:   # (the counter stops at k = 21: a presence-only set of every k-mer seen in the other half of the reads)
        gs = br_amd.Pcon.from_fasta(raw_reads[100:206], k)
        ref = O.Solid.sparse_from_count(k, raw_reads[100:206], 0)
    assert gs.is_sparse() and gs.popcount() == ref.popcount() > 1000
    check_chain(gs, ref, ["one"], reads)
    check_chain(gs, ref, ["graph", "gap_size"], reads[:50])


def test_batch_split_invariance(raw_reads, solid_fixture_bytes):
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    names = ["one", "gap_size"]
    chain = rc_chain(gs, names)
    whole = chain.correct_reads(raw_reads)
    cuts = [0, 1, 4, 5, 60, 61, 150, len(raw_reads)]     # seven uneven batches
    parts = []
    for lo, hi in zip(cuts, cuts[1:]):
        parts += chain.correct_reads(raw_reads[lo:hi])
    assert len(cuts) - 1 == 7 and parts == whole
    # ... and through the device entry with the batch behind an odd first offset
    bases, offs = br_amd.pack_reads(raw_reads[3:50])
    out, oo = chain.correct_batch(bases, offs)
    assert [out[int(oo[i]):int(oo[i + 1])].tobytes() for i in range(47)] == whole[3:50]


def test_edge_reads(raw_reads, solid_fixture_bytes):
    """reads shorter than k, empty reads, lower case and N beside fixes"""
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    ref = O.Solid.from_bytes(solid_fixture_bytes)
    assert rc_chain(gs, ["one"]).correct_reads([]) == []
    marked = []
    for r in raw_reads[:30]:
        b = bytearray(r)
        for p in range(40, len(b) - 40, 97):
            b[p] = ord(chr(b[p]).lower())
            if b[p + 5] == ord("G"):
                b[p + 5] = ord("N")
        marked.append(bytes(b))
    reads = [b"", b"A", b"ACGTACGTAC", b"ACGTACGTACG", b"ACGTACGTACGT", b"acgtnACGTNNxyzACGTACGTTTGACCA", b"N" * 300,
             b"ACGT" * 100, b"", raw_reads[0][:10], raw_reads[1][:11], raw_reads[2][:12]] + marked + [b""]
    for names in (["one"], ["two"], ["graph", "gap_size"], ALL_FIVE):
        _, got, om = check_chain(gs, ref, names, reads)
        assert sum(g != r for g, r in zip(got, reads)) >= 20
        assert any(c in b"".join(got) for c in b"acgt") and b"N" in b"".join(got)
        assert got[0] == b"" and got[1] == b"A"


# ---------------------------------------------------------------- the retry paths --------------------------------------
def _gap_world():
    rng = np.random.default_rng(7)
    k = 15   # large enough that the 3 kb random genome has no branching (k-1)-mers
    genome = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=3000).tolist())
    ref = O.Solid(k)
    ref.set_seq(genome)

    def sub(s, positions):
        b = bytearray(s)
        for p in positions:
            b[p] = b"ACGT"[(b"ACGT".index(b[p]) + 1) % 4]
        return bytes(b)
    # reads with 140- to 340-base deletions that Graph / GapSize put back: they outgrow a slot of len + len / 4 + 64, on
    # either strand, beside neighbours that must not be disturbed
    reads = [genome[2000:2300], genome[100:160] + genome[310:370], genome[1500:1530], strand.revcomp(genome[500:560] + genome[900:960]),
             genome[1000:1400], b"", genome[2500:2600], sub(genome[1200:1260], [50]) + genome[1400:1460],
             sub(genome[1200:1260], range(3, 60, 9)) + genome[1400:1460] + genome[1600:1660],
             strand.revcomp(sub(genome[1700:1760], range(3, 60, 9)) + genome[1900:1960] + genome[2100:2160]), sub(genome[2600:2900], [150])]
    return genome, ref, reads


@pytest.mark.parametrize("redo_max", [None, "0"], ids=["redo_default", "redo_0"])
def test_output_slot_overflow_retry(monkeypatch, redo_max):
    """reads that outgrow the first slack.  With BRX_REDO_MAX at its default they are redone outside the batch by a second
    chain of the same mode (one that fits its slot goes back into the stage as the second scan left it, one that does not
    is copied over its place after the compaction); at 0 the whole batch -- both scans -- runs again with 4x the slack."""
    if redo_max is None:
        monkeypatch.delenv("BRX_REDO_MAX", raising=False)
    else:
        monkeypatch.setenv("BRX_REDO_MAX", redo_max)
    genome, ref, reads = _gap_world()
    gs = br_amd.Pcon.from_pcon_solid(ref.to_bytes())
    for names in (["graph"], ["gap_size"], ["one", "graph"]):
        chain, got, om = check_chain(gs, ref, names, reads)
        st = chain.last_stats()
        assert st["slot_overflow_reads"] >= 4
        assert got[1] == genome[100:370] and got[3] == strand.revcomp(genome[500:960]) and got[10] == genome[2600:2900]
        if redo_max == "0":
            assert st["overflow_retries"] >= 1
            # the chain remembers the workspace it needed: the same batch again runs once
            check_chain(gs, ref, names, reads, chain=chain)
            assert chain.last_stats()["overflow_retries"] == 0
        else:
            assert st["overflow_retries"] == 0
            check_chain(gs, ref, names, reads, chain=chain)


@pytest.mark.parametrize("redo_max", [None, "0"], ids=["redo_default", "redo_0"])
def test_walk_list_overflow_retry(raw_reads, solid_fixture_bytes, monkeypatch, redo_max):
    """walks that outgrow a two-entry visited list, in either scan: redone outside the batch, or the batch run again with a
    longer list"""
    monkeypatch.setenv("BRX_MAXPATH", "2")
    if redo_max is None:
        monkeypatch.delenv("BRX_REDO_MAX", raising=False)
    else:
        monkeypatch.setenv("BRX_REDO_MAX", redo_max)
    monkeypatch.setenv("BRX_LANE_WALK", "0")   # (the visited lists are the group kernel's; the lane form keeps none)
    ref = O.Solid.from_bytes(solid_fixture_bytes)
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    reads = raw_reads[:24] + [b"", b"ACGT"]
    for names in (["graph"], ["one", "gap_size", "graph"]):
        chain, got, om = check_chain(gs, ref, names, reads)
        st = chain.last_stats()
        assert st["walk_list_overflows"] > 0
        if redo_max == "0":
            assert st["overflow_retries"] >= 1
        else:
            assert st["overflow_retries"] == 0
        check_chain(gs, ref, names, reads, chain=chain)


# ---------------------------------------------------------------- pipeline and command line ----------------------------
def oracle_flags(ref, read):
    k = ref.k
    n = max(len(read) - k + 1, 0)
    solid = np.unpackbits(ref.mask(read), bitorder="little")[:n].astype(bool)
    return cover.flags_from_solid(solid, len(read), k)


def oracle_pipeline(text, ref, om, mode, min_len=0):
    """(FASTA text, report text, totals) of a revcomp run, record by record from the definitions"""
    out, rep = io.BytesIO(), io.BytesIO()
    rep.write(REPORT_HEADER)
    totals = dict.fromkeys(COVER_KEYS, 0)
    for name, desc, seq in fasta.read_records(io.BytesIO(text)):
        corr = rc_record(om, seq)
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


@pytest.fixture(scope="module")
def fixture_text(golden_dir):
    return open(os.path.join(golden_dir, "raw.fasta"), "rb").read()


@pytest.mark.parametrize("mode,min_len", [("plain", 0), ("mask", 0), ("split", 200)])
def test_run_correction_native_and_record_by_record(fixture_text, solid_fixture_bytes, mode, min_len):
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    ref = O.Solid.from_bytes(solid_fixture_bytes)
    names = ["one", "graph"]
    om = O.build_methods(ref, names, 5, 7)
    methods = br_amd.build_methods(names, gs, 5, 7)
    want_text, want_rep, want_tot = oracle_pipeline(fixture_text, ref, om, mode, min_len)
    assert want_text.count(b">") >= 206
    for native, batch_records in ((True, 0), (True, 7), (False, 0)):
        out, rep = io.BytesIO(), io.BytesIO()
        st = run_correction([io.BytesIO(fixture_text)], [out], methods, False, native=native, batch_records=batch_records,
                            output_mode=mode, min_len=min_len, reports=[rep], second_pass="revcomp")
        assert out.getvalue() == want_text, (native, batch_records)
        assert rep.getvalue() == want_rep, (native, batch_records)
        assert {k: st[k] for k in COVER_KEYS} == want_tot and st["records"] == 206
        # without a report
        out = io.BytesIO()
        st = run_correction([io.BytesIO(fixture_text)], [out], methods, False, native=native, batch_records=batch_records,
                            output_mode=mode, min_len=min_len, second_pass="revcomp")
        assert out.getvalue() == want_text and not set(COVER_KEYS) & set(st)
    # the cover statistics show the gain the mode is for
    rev_tot = run_correction([io.BytesIO(fixture_text)], [io.BytesIO()], methods, False, native=True, cover_stats=True)
    assert want_tot["solid_out"] / want_tot["kmers_out"] > rev_tot["solid_out"] / rev_tot["kmers_out"]


def test_run_correction_other_modes_and_contradictions(fixture_text, solid_fixture_bytes):
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    methods = br_amd.build_methods(["one"], gs, 5, 7)

    def run(**kw):
        out = io.BytesIO()
        run_correction([io.BytesIO(fixture_text)], [out], methods, kw.pop("two_side", False), **kw)
        return out.getvalue()
    default = run(native=True)
    assert run(native=True, second_pass="reverse") == default == run(native=False, second_pass="reverse")
    one_scan = run(native=True, two_side=True)
    assert run(native=True, second_pass="none") == one_scan == run(native=False, two_side=True, second_pass="none")
    assert one_scan != default
    with pytest.raises(ValueError):
        run(native=True, two_side=True, second_pass="revcomp")
    with pytest.raises(ValueError):
        run(native=True, second_pass="other")
    st = (C.c_uint64 * 8)()
    specs = (_lib.Method * 1)(_lib.Method(0, 5, 7))
    assert _lib.lib().brx_run_correction_fd_pass(gs._h, specs, 1, 5, 0, 1, 0, None, st, None) == _lib.BRX_ERR_ARG


def test_command_line(tmp_path, golden_dir, fixture_text, solid_fixture_bytes):
    ref = O.Solid.from_bytes(solid_fixture_bytes)
    om = O.build_methods(ref, ["one"], 5, 7)
    src = os.path.join(golden_dir, "raw.fasta")
    tail = ["solid", "-i", os.path.join(golden_dir, "raw.k11.a2.solid"), "-f", "solid"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def br(out, *flags):
        subprocess.run([sys.executable, "-m", "br_amd", "-i", src, "-o", str(out), "-c", "one"] + list(flags) + tail, check=True,
                       env=env, cwd=ROOT, timeout=600)
        return out.read_bytes()
    want, _, _ = oracle_pipeline(fixture_text, ref, om, "plain")
    assert br(tmp_path / "rc.fa", "--second-pass", "revcomp") == want
    want_mask, want_rep, _ = oracle_pipeline(fixture_text, ref, om, "mask")
    assert br(tmp_path / "rcm.fa", "--second-pass", "revcomp", "--mask-weak", "--cover-report", str(tmp_path / "r.tsv")) == want_mask
    assert (tmp_path / "r.tsv").read_bytes() == want_rep
    want_split, _, _ = oracle_pipeline(fixture_text, ref, om, "split", 200)
    assert br(tmp_path / "rcs.fa", "--second-pass", "revcomp", "--trim-split", "200") == want_split
    # --second-pass reverse, no flag and brx_run_correction_fd write identical files
    plain = br(tmp_path / "p.fa")
    assert br(tmp_path / "r.fa", "--second-pass", "reverse") == plain
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    specs = (_lib.Method * 1)(_lib.Method(0, 5, 7))
    st = (C.c_uint64 * 8)()
    ifd, ofd = os.open(src, os.O_RDONLY), os.open(tmp_path / "fd.fa", os.O_WRONLY | os.O_CREAT, 0o644)
    try:
        _lib.check(_lib.lib().brx_run_correction_fd(gs._h, specs, 1, False, ifd, ofd, 0, st))
    finally:
        os.close(ifd)
        os.close(ofd)
    assert (tmp_path / "fd.fa").read_bytes() == plain and st[0] == 206
    assert br(tmp_path / "n.fa", "--second-pass", "none") == br(tmp_path / "s.fa", "-s") != plain
    bad = subprocess.run([sys.executable, "-m", "br_amd", "-i", src, "-o", str(tmp_path / "x.fa"), "-s", "--second-pass", "revcomp"] + tail,
                         env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and "--second-pass" in bad.stderr


def test_a_plain_run_launches_none_of_the_new_kernels(tmp_path, golden_dir, solid_fixture_bytes):
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    specs = (_lib.Method * 2)(_lib.Method(0, 5, 7), _lib.Method(2, 5, 7))
    src = os.path.join(golden_dir, "raw.fasta")
    L = _lib.lib()

    _lib.profile_enable(True)
    try:
        _lib.profile_reset()
        outs = []
        for second in (False, True):
            dst = tmp_path / f"o{int(second)}.fa"
            st = (C.c_uint64 * 8)()
            ifd, ofd = os.open(src, os.O_RDONLY), os.open(dst, os.O_WRONLY | os.O_CREAT, 0o644)
            try:
                _lib.check(L.brx_run_correction_fd(gs._h, specs, 2, second, ifd, ofd, 16, st))
            finally:
                os.close(ifd)
                os.close(ofd)
            outs.append(dst.read_bytes())
        for mode in (0, 1):   # BRX_PASS_NONE / REVERSE through the new entry: the same files
            dst = tmp_path / f"p{mode}.fa"
            ifd, ofd = os.open(src, os.O_RDONLY), os.open(dst, os.O_WRONLY | os.O_CREAT, 0o644)
            try:
                _lib.check(L.brx_run_correction_fd_pass(gs._h, specs, 2, mode, ifd, ofd, 16, None, None, None))
            finally:
                os.close(ifd)
                os.close(ofd)
            assert dst.read_bytes() == outs[1 - mode]
        br_amd.Chain(gs, [("one", 5, 7), ("gap_size", 5, 7)]).correct_reads([b"ACGT" * 50] * 3)
        assert _lib.profile_get("strand")[1] == 0 and _lib.profile_get("strand_compact")[1] == 0
        assert _lib.profile_get("compact")[1] > 0
        dst = tmp_path / "rc.fa"
        ifd, ofd = os.open(src, os.O_RDONLY), os.open(dst, os.O_WRONLY | os.O_CREAT, 0o644)
        try:
            _lib.check(L.brx_run_correction_fd_pass(gs._h, specs, 2, 2, ifd, ofd, 16, None, None, None))
        finally:
            os.close(ifd)
            os.close(ofd)
        assert _lib.profile_get("strand")[1] > 0 and _lib.profile_get("strand_compact")[1] > 0   # ... and the timers do count in the mode
        assert dst.read_bytes() not in outs
    finally:
        _lib.profile_enable(False)
