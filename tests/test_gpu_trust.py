"""Trusted stretches on the GPU (include/brx.h "trusted stretches", br_amd/csrc/brx_trust.hip) against br_amd/trust.py:
the split form and the statistics bit for bit, counting through the stretches, the native FASTQ batcher against
fasta.read_fastq_sequences, stream order, the `fastq` sub-command, refused arguments.  All comparisons are exact."""
import ctypes as C
import functools
import io
import os

import numpy as np
import pytest

import br_amd
from br_amd import _lib, cli, cover, fasta, trust
from br_amd.set import pack_reads, trust_split_batch, trust_split_batch_device
from oracle import oracle as O

gpu = pytest.mark.gpu
K = 11
DENSE, SORTED, TABLE = _lib.COUNT_DENSE, _lib.COUNT_SORTED, _lib.COUNT_TABLE
STRATEGY = {11: DENSE, 19: SORTED, 25: TABLE}
LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


# ---- the batch of test 1: every length class, every start residue mod 16, the planted cases -----------------------------

def shape_batch(k=K, seed=3):
    rng = np.random.default_rng(seed)
    lens = [0, 1, k - 1, k, k + 1, 63, 64, 65, 1023, 1024, 1025, 2065, 3072]
    order = [3072, 1, 63, 0, 1023, k - 1, 1025, 64, k, 2065, 65, 1024, k + 1]
    assert sorted(order) == sorted(lens)
    # pad reads until the read starts have taken every residue mod 16
    cur = sum(order)
    seen = set(np.concatenate([[0], np.cumsum(order)])[:-1] % 16)
    for r in range(16):
        if r not in seen:
            pad = (r - cur) % 16 or 16
            order.append(pad)
            cur += pad
            seen.add(r)
    order.append(5)
    offs = np.concatenate([[0], np.cumsum(order)]).astype(np.uint64)
    assert set((offs[:-1] % 16).tolist()) == set(range(16)) and int(offs[-1]) < 20000
    total = int(offs[-1])
    bases = LETTERS[rng.integers(0, 4, total)].copy()
    lower = rng.random(total) < 0.1
    bases[lower] |= 0x20
    odd = rng.random(total) < 0.01
    bases[odd] = rng.choice(np.frombuffer(b"Nn-RU", dtype=np.uint8), int(odd.sum()))
    quals = (33 + rng.integers(0, 46, total)).astype(np.uint8)
    quals[rng.random(total) < 0.005] = rng.choice(np.array([0, 32, 200], dtype=np.uint8))  # below Phred+33, above ASCII

    def read_at(length):
        i = order.index(length)
        return int(offs[i])

    def clean(a, b):          # trusted under every configuration
        bases[a:b] = LETTERS[rng.integers(0, 4, b - a)]
        quals[a:b] = 33 + 45

    def spoil(at):            # untrusted under every configuration that can bite
        bases[at] = ord("N")
        quals[at] = 33
    o = read_at(3072)         # tiles [0, 1024), [1024, 2048), [2048, 3072)
    clean(o + 1000, o + 1101)
    spoil(o + 999)
    spoil(o + 1101)           # a stretch 1000 .. 1100 that crosses a tile border
    clean(o + 2000, o + 2048)
    spoil(o + 2048)           # one that ends on a tile's last position
    o = read_at(2065)
    spoil(o + 1023)
    clean(o + 1024, o + 1100)  # one that starts on a tile's first position
    o = read_at(1024)
    clean(o, o + 1024)         # an all-trusted read
    o = read_at(1025)
    bases[o:o + 1025] = ord("N")
    quals[o:o + 1025] = 33     # an all-untrusted read
    o = read_at(1023)
    clean(o, o + 1023)
    for at in range(k - 1, 1023, k):
        spoil(o + at)          # single untrusted bases k apart: stretches of k - 1, gone at min_len = k
    return bases, quals, offs


@functools.lru_cache(maxsize=None)
def shape_case():
    return shape_batch()


@functools.lru_cache(maxsize=None)
def want_split(with_quals, floor, acgt_only, min_len):
    bases, quals, offs = shape_case()
    return trust.split_batch(bases, quals if with_quals else None, offs, floor, acgt_only, min_len)


def same_split(got, want, what):
    for g, w, name in zip(got, want, ("out", "out_offsets", "piece_read", "piece_start", "stats")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name)


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy((a.view(view) if view else a).copy()).cuda()


def dev_quals(quals, shift=5):
    """the qualities on the device at another residue mod 16 than the bases"""
    import torch
    buf = torch.zeros(quals.size + 64, dtype=torch.uint8, device="cuda")
    buf[shift:shift + quals.size] = torch.from_numpy(quals.copy()).cuda()
    return buf, buf.data_ptr() + shift


def device_split(bases, quals, offs, floor, acgt_only, min_len, stream=None, inputs=None):
    """the device entry with buffers cut by the bounds of include/brx.h; inputs: (d_bases, d_quals pointer, d_offs) staged
    elsewhere"""
    import torch
    n, total = offs.size - 1, bases.size
    if inputs is None:
        d_b, d_o = dev(bases), dev(offs)
        keep, d_q = dev_quals(quals) if quals is not None else (None, None)
        inputs = (d_b.data_ptr(), d_q, d_o.data_ptr())
        hold = (d_b, d_o, keep)
    cap = trust.piece_bound(n, total, min_len)
    out = torch.full((max(total, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    oo = torch.full((cap + 1,), -1, dtype=torch.int64, device="cuda")
    pr = torch.full((max(cap, 1),), -1, dtype=torch.int32, device="cuda")
    ps = torch.full((max(cap, 1),), -1, dtype=torch.int64, device="cuda")
    st = torch.full((max(n, 1) * 5,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    np_, bytes_ = trust_split_batch_device(inputs[0], inputs[1], inputs[2], n, total, floor, acgt_only, min_len, out.data_ptr(), total,
                                           oo.data_ptr(), pr.data_ptr(), ps.data_ptr(), cap, st.data_ptr(), 0, stream)
    # (the entry returns after its kernels have completed: the results may be read at once)
    return (out[:bytes_].cpu().numpy(), oo[:np_ + 1].cpu().numpy().view(np.uint64), pr[:np_].cpu().numpy().view(np.uint32),
            ps[:np_].cpu().numpy().view(np.uint64), st[:n * 5].cpu().numpy().view(trust.STATS_DTYPE))


# ---- 1. split against numpy ------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("floor", [0, 2, 20, 41])
def test_split_against_numpy(floor):
    bases, quals, offs = shape_case()
    for with_quals in (True, False):
        for acgt_only in (True, False):
            for min_len in (1, K, 100):
                want = want_split(with_quals, floor, acgt_only, min_len)
                what = (floor, with_quals, acgt_only, min_len)
                got = trust_split_batch(bases, quals if with_quals else None, offs, floor, acgt_only, min_len)
                same_split(got, want, ("host",) + what)
                got = device_split(bases, quals if with_quals else None, offs, floor, acgt_only, min_len)
                same_split(got, want, ("device",) + what)
    # the planted cases are what they are meant to be
    out, oo, pr, ps, st = want_split(True, 20, True, 1)
    lens = np.diff(oo.astype(np.int64))
    starts = np.concatenate([[0], np.cumsum(np.diff(offs.astype(np.int64)))])
    by_len = {int(n): i for i, n in enumerate(np.diff(offs.astype(np.int64)))}
    r = by_len[3072]
    mine = {(int(s), int(n)) for s, n in zip(ps[pr == r], lens[pr == r])}
    assert (1000, 101) in mine and any(s + n == 2048 for s, n in mine)
    assert any(int(s) == 1024 for s in ps[pr == by_len[2065]])
    assert st["pieces"][by_len[1024]] == 1 and st["kept_bases"][by_len[1024]] == 1024
    assert st["pieces"][by_len[1025]] == 0 and st["non_acgt"][by_len[1025]] == 1025
    assert set(lens[pr == by_len[1023]].tolist()) == {K - 1}
    assert want_split(True, 20, True, K)[4]["pieces"][by_len[1023]] == 0
    # with nothing asked the split form is the batch itself, empty reads dropped
    out, oo, pr, ps, st = want_split(True, 0, False, 1)
    assert out.tobytes() == bases.tobytes() and pr.tolist() == [i for i, n in enumerate(np.diff(starts)) if n]


@gpu
def test_sizes_only_and_overflow():
    import torch
    bases, quals, offs = shape_case()
    n, total = offs.size - 1, bases.size
    want = want_split(True, 20, True, K)
    d_b, d_o = dev(bases), dev(offs)
    keep, d_q = dev_quals(quals)
    # zero capacities, no outputs: the sizes, as BRX_ERR_OVERFLOW
    with pytest.raises(_lib.BrxError) as e:
        trust_split_batch_device(d_b.data_ptr(), d_q, d_o.data_ptr(), n, total, 20, True, K)
    assert e.value.status == _lib.BRX_ERR_OVERFLOW and e.value.needed == (want[2].size, want[0].size)
    # a capacity one too small on either side: the sizes again, and not a byte written -- statistics included
    for piece_cap, out_cap in ((want[2].size - 1, total), (want[2].size, want[0].size - 1)):
        bufs = [torch.full((m,), 0x5A, dtype=torch.uint8, device="cuda") for m in (total, 8 * (n + total), 4 * (n + total), 8 * (n + total), 20 * n)]
        torch.cuda.synchronize()
        with pytest.raises(_lib.BrxError) as e:
            trust_split_batch_device(d_b.data_ptr(), d_q, d_o.data_ptr(), n, total, 20, True, K, bufs[0].data_ptr(), out_cap,
                                     bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(), piece_cap, bufs[4].data_ptr())
        assert e.value.status == _lib.BRX_ERR_OVERFLOW and e.value.needed == (want[2].size, want[0].size)
        torch.cuda.synchronize()
        assert all(bool((b == 0x5A).all()) for b in bufs)
    # exactly enough is enough
    got = trust_split_batch_device(d_b.data_ptr(), d_q, d_o.data_ptr(), n, total, 20, True, K, bufs[0].data_ptr(), want[0].size,
                                   bufs[1].data_ptr(), None, None, want[2].size, None)
    assert got == (want[2].size, want[0].size)
    assert bufs[0][:want[0].size].cpu().numpy().tobytes() == want[0].tobytes()
    # an empty batch, and a batch of empty reads
    z = np.zeros(0, dtype=np.uint8)
    out, oo, pr, ps, st = trust_split_batch(z, None, np.zeros(1, dtype=np.uint64), 20, True, K)
    assert out.size == 0 and oo.tolist() == [0] and pr.size == 0 and st.size == 0
    out, oo, pr, ps, st = trust_split_batch(z, z, np.zeros(4, dtype=np.uint64), 20, True, K)
    assert out.size == 0 and oo.tolist() == [0] and st.size == 3 and not st["bases"].any()


# ---- 2. batch shape does not matter ------------------------------------------------------------------------------------------

@gpu
def test_batch_shape_does_not_matter():
    bases, quals, offs = shape_case()
    n = offs.size - 1
    reads = [(bases[int(offs[i]):int(offs[i + 1])], quals[int(offs[i]):int(offs[i + 1])]) for i in range(n)]

    def pieces_per_read(order, as_one):
        got = {}
        groups = [order] if as_one else [[i] for i in order]
        for grp in groups:
            b, o = pack_reads([reads[i][0].tobytes() for i in grp])
            q, _ = pack_reads([reads[i][1].tobytes() for i in grp])
            out, oo, pr, ps, st = trust_split_batch(b, q, o, 20, True, K)
            for j, i in enumerate(grp):
                got[i] = ([(int(ps[p]), out[int(oo[p]):int(oo[p + 1])].tobytes()) for p in np.flatnonzero(pr == j)], list(st[j].tolist()))
        return got
    one = pieces_per_read(list(range(n)), True)
    want = {i: (trust.split_read(reads[i][0].tobytes(), reads[i][1].tobytes(), 20, True, K),
                list(trust.stats_of(reads[i][0].tobytes(), reads[i][1].tobytes(), 20, True, K))) for i in range(n)}
    assert one == want
    assert pieces_per_read(list(range(n)), False) == want
    assert pieces_per_read(list(range(n))[::-1], True) == want


# ---- 3. counting ---------------------------------------------------------------------------------------------------------------

def fastq_text(reads, quals):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, q) for i, (s, q) in enumerate(zip(reads, quals)))


def fasta_text(reads):
    return b"".join(b">r%d\n%s\n" % (i, s) for i, s in enumerate(reads))


@functools.lru_cache(maxsize=None)
def count_case():
    """reads drawn from a small genome (so that k-mers repeat), some N, seeded qualities; one read of 40 N between two
    genome stretches"""
    rng = np.random.default_rng(11)
    genome = LETTERS[rng.integers(0, 4, 3000)].tobytes()
    for k in (11, 19, 25):
        assert b"G" * k not in genome and b"C" * k not in genome
    reads, quals = [], []
    for _ in range(60):
        a = int(rng.integers(0, 3000 - 400))
        s = np.frombuffer(genome[a:a + int(rng.integers(30, 400))], dtype=np.uint8).copy()
        s[rng.random(s.size) < 0.01] = ord("N")
        reads.append(s.tobytes())
        quals.append((33 + np.clip(rng.normal(30, 9, s.size), 0, 45).astype(np.uint8)).tobytes())
    reads.append(genome[100:260] + b"N" * 40 + genome[500:660])
    quals.append(bytes([33 + 40]) * 360)
    return reads, quals


def fingerprint_and_spectrum(cnt, a=1):
    return cnt.finish(a).fingerprint(), cnt.spectrum().tolist()


@gpu
@pytest.mark.parametrize("k", [11, 19, 25])
def test_counting_through_the_stretches(k):
    reads, quals = count_case()
    bases, offs = pack_reads(reads)
    qb, _ = pack_reads(quals)
    out, oo, pr, ps, st = trust.split_batch(bases, qb, offs, 20, True, k)
    pieces = [out[int(oo[i]):int(oo[i + 1])].tobytes() for i in range(pr.size)]
    assert 0 < len(pieces) and int(st["low_quality"].sum()) > 0 and int(st["non_acgt"].sum()) >= 40
    got = br_amd.Counter(k, strategy=STRATEGY[k])
    res = got.count_reads(io.BytesIO(fastq_text(reads, quals)), "fastq", 20, True)
    want = br_amd.Counter(k, strategy=STRATEGY[k])
    want.add_reads(pieces)
    assert res["records"] == len(reads) and res["bases_in"] == bases.size
    assert res["trust"] == dict(trust.totals(st), kmers=trust.kmers_of_pieces(st, k))
    assert fingerprint_and_spectrum(got) == fingerprint_and_spectrum(want)
    if k == 11:  # the oracle's table of the same pieces, bin by bin, and k-mer by k-mer along the pieces
        table = O.count_reads(k, pieces)
        assert got.spectrum().tolist() == np.bincount(table, minlength=256).tolist()
        for p in pieces[:20]:
            assert np.array_equal(got.get_counts(cover.kmers_of(p, k)), table[O.hashes(k, p).astype(np.int64)])
    # nothing asked: the FASTQ count is count_fasta's of the same sequences
    every = br_amd.Counter(k, strategy=STRATEGY[k])
    res = every.count_reads(io.BytesIO(fastq_text(reads, quals)), "fastq", 0, False)
    plain = br_amd.Counter(k, strategy=STRATEGY[k])
    plain.count_fasta(io.BytesIO(fasta_text(reads)))
    assert fingerprint_and_spectrum(every) == fingerprint_and_spectrum(plain)
    assert res["trust"]["kmers"] == sum(max(len(r) - k + 1, 0) for r in reads) and res["trust"]["non_acgt"] == 0
    # the 40 N: a homopolymer k-mer (N codes like G) for count_fasta, nothing through the stretches
    poly = [(1 << (2 * k)) - 1]
    for c in (got, plain):
        if STRATEGY[k] == SORTED:
            c.prepare_lookup()
    assert got.get_counts(poly).tolist() == [0]
    assert plain.get_counts(poly).tolist() == [40 - k + 1]
    # FASTA with acgt_only: the same cut without a floor
    fa = br_amd.Counter(k, strategy=STRATEGY[k])
    fa.count_reads(io.BytesIO(fasta_text(reads)), "fasta", 0, True)
    o2, oo2, pr2, _, _ = trust.split_batch(bases, None, offs, 0, True, k)
    want2 = br_amd.Counter(k, strategy=STRATEGY[k])
    want2.add_reads([o2[int(oo2[i]):int(oo2[i + 1])].tobytes() for i in range(pr2.size)])
    assert fingerprint_and_spectrum(fa) == fingerprint_and_spectrum(want2)


# ---- 4. the native FASTQ batcher against fasta.read_fastq_sequences --------------------------------------------------------------

def parse_fastq(data):
    """fasta.read_fastq_sequences' rules, keeping the qualities"""
    f = io.BytesIO(data)
    while True:
        head = f.readline()
        if not head:
            return
        seq, plus, qual = f.readline(), f.readline(), f.readline()
        head, seq, plus, qual = (x.rstrip(b"\r\n") for x in (head, seq, plus, qual))
        if not head.startswith(b"@") or len(head) < 2 or head[1:2].isspace() or not plus.startswith(b"+") or len(qual) != len(seq):
            return
        yield seq, qual


BOUNDARY_FQ = b"@r1 d\nACGTA\n+\nIIIII\n@r2\r\nGG\r\n+r2\r\nII\r\n@bad\nAC\n+\nI\n@r3\nAAAA\n+\nIIII\n"  # test_boundary's
LONG = b"ACGTTGCATGCCGATAGCTAGGATCCATGCAAGT"
FQ_STREAMS = {
    "boundary": BOUNDARY_FQ,
    "crlf": b"@a x\r\n" + LONG + b"\r\n+\r\n" + b"I" * len(LONG) + b"\r\n@b\r\n" + LONG[::-1] + b"\r\n+b\r\n" + b"5" * len(LONG) + b"\r\n",
    "no_final_newline": b"@a\n" + LONG + b"\n+\n" + b"I" * len(LONG) + b"\n@b\n" + LONG[5:] + b"\n+\n" + b"#" * (len(LONG) - 5),
    "empty_sequence": b"@a\n" + LONG + b"\n+\n" + b"I" * len(LONG) + b"\n@e\n\n+\n\n@b\n" + LONG + b"\n+\n" + b"I" * len(LONG) + b"\n",
    "quality_starts_with_at": b"@a\n" + LONG + b"\n+\n@" + b"I" * (len(LONG) - 1) + b"\n@b\n" + LONG + b"\n+\n" + b"@" * len(LONG) + b"\n",
    "truncated_last": b"@a\n" + LONG + b"\n+\n" + b"I" * len(LONG) + b"\n@b\n" + LONG + b"\n+\n" + b"I" * len(LONG) + b"\n@t\nACGTACGTACGTA\n",
    "mismatch_in_3_of_5": b"".join(b"@r%d\n%s\n+\n%s\n" % (i, LONG, b"I" * (len(LONG) - (1 if i == 2 else 0))) for i in range(5)),
    "nothing": b"",
    "fasta": b">r1\nACGT\n",
}


def test_fastq_streams_are_what_they_claim():
    """no GPU: the streams hold the cases they are named after, under the rules test_boundary pins"""
    want = {"boundary": 2, "crlf": 2, "no_final_newline": 2, "empty_sequence": 3, "quality_starts_with_at": 2, "truncated_last": 2,
            "mismatch_in_3_of_5": 2, "nothing": 0, "fasta": 0}
    for name, data in FQ_STREAMS.items():
        recs = list(parse_fastq(data))
        assert [s for s, _ in recs] == list(fasta.read_fastq_sequences(io.BytesIO(data))), name
        assert len(recs) == want[name], name
    assert b"" in [s for s, _ in parse_fastq(FQ_STREAMS["empty_sequence"])]
    assert b"\r" not in b"".join(s + q for s, q in parse_fastq(FQ_STREAMS["crlf"]))


@gpu
@pytest.mark.parametrize("name", sorted(FQ_STREAMS))
def test_native_fastq_batcher(name):
    data = FQ_STREAMS[name]
    recs = list(parse_fastq(data))
    seqs, quals = [s for s, _ in recs], [q for _, q in recs]
    bases, offs = pack_reads(seqs)
    qb, _ = pack_reads(quals)
    ref = br_amd.Counter(K, strategy=DENSE)
    if seqs:
        ref.add_reads(seqs)
    st = trust.split_batch(bases, qb, offs, 20, True, K)[4]
    out, oo, pr, _, _ = trust.split_batch(bases, qb, offs, 20, True, K)
    cut = br_amd.Counter(K, strategy=DENSE)
    if pr.size:
        cut.add_reads([out[int(oo[i]):int(oo[i + 1])].tobytes() for i in range(pr.size)])
    for max_batch_records in (1, 2, 3, 0):
        c = br_amd.Counter(K, strategy=DENSE)
        res = c.count_reads(io.BytesIO(data), "fastq", 0, False, max_batch_records)
        assert (res["records"], res["bases_in"]) == (len(seqs), bases.size), (name, max_batch_records)
        assert c.spectrum().tolist() == ref.spectrum().tolist(), (name, max_batch_records)
        assert res["trust"]["kmers"] == sum(max(len(s) - K + 1, 0) for s in seqs)
        c = br_amd.Counter(K, strategy=DENSE)
        res = c.count_reads(io.BytesIO(data), "fastq", 20, True, max_batch_records)
        assert (res["records"], res["bases_in"]) == (len(seqs), bases.size), (name, max_batch_records)
        assert res["trust"] == dict(trust.totals(st), kmers=trust.kmers_of_pieces(st, K)), (name, max_batch_records)
        assert c.spectrum().tolist() == cut.spectrum().tolist(), (name, max_batch_records)
        if max_batch_records:
            assert res["batches"] >= -(-len(seqs) // max_batch_records)


# ---- 5. stream order -------------------------------------------------------------------------------------------------------------

@gpu
def test_device_entry_keeps_stream_order():
    """in the manner of tests/test_gpu_streams.py: the inputs are decoys until copies queued behind a long kernel on a busy
    non-blocking stream have run; the entry must answer for the real batch.  Lane.pending() proves that the delay had not
    run out when the call was issued"""
    import torch
    from tests.test_gpu_streams import Lane
    bases, quals, offs = shape_case()
    rng = np.random.default_rng(9)
    lens = rng.permutation(np.diff(offs.astype(np.int64)))
    decoy = {"bases": LETTERS[rng.integers(0, 4, bases.size)].copy(), "quals": np.full(quals.size, 33 + 45, dtype=np.uint8),
             "offs": np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)}
    real = {"bases": bases, "quals": quals, "offs": offs}
    want = want_split(True, 20, True, K)
    dec = trust.split_batch(decoy["bases"], decoy["quals"], decoy["offs"], 20, True, K)
    assert not np.array_equal(dec[1], want[1])
    lane = Lane(32)
    held = lane.stage(decoy, real)
    inputs = (held["bases"].data_ptr(), held["quals"].data_ptr(), held["offs"].data_ptr())
    n, total = offs.size - 1, bases.size
    cap = trust.piece_bound(n, total, K)
    with torch.cuda.stream(lane.s):
        out = torch.empty(total, dtype=torch.uint8, device="cuda")
        oo = torch.empty(cap + 1, dtype=torch.int64, device="cuda")
        pr = torch.empty(cap, dtype=torch.int32, device="cuda")
        ps = torch.empty(cap, dtype=torch.int64, device="cuda")
        st = torch.empty(n * 5, dtype=torch.int32, device="cuda")
    assert lane.pending(), "the delay ran out before the call under test was issued: the probe has no teeth"
    np_, bytes_ = trust_split_batch_device(inputs[0], inputs[1], inputs[2], n, total, 20, True, K, out.data_ptr(), total, oo.data_ptr(),
                                           pr.data_ptr(), ps.data_ptr(), cap, st.data_ptr(), 0, lane.stream)
    got = (lane.fetch(out)[:bytes_], lane.fetch(oo)[:np_ + 1].view(np.uint64), lane.fetch(pr)[:np_].view(np.uint32),
           lane.fetch(ps)[:np_].view(np.uint64), lane.fetch(st).view(trust.STATS_DTYPE))
    lane.wait()
    same_split(got, want, "lane")


# ---- 6. command line ---------------------------------------------------------------------------------------------------------------

@gpu
def test_command_line(tmp_path, raw_reads):
    reads = [r[:4000] for r in raw_reads[:40]]
    reads[3] = reads[3][:1500] + b"N" * 40 + reads[3][1540:]
    rng = np.random.default_rng(5)
    quals = [(33 + np.clip(rng.normal(28, 8, len(r)), 0, 45).astype(np.uint8)).tobytes() for r in reads]
    bases, offs = pack_reads(reads)
    qb, _ = pack_reads(quals)
    out, oo, pr, _, st = trust.split_batch(bases, qb, offs, 20, True, K)
    pieces = [out[int(oo[i]):int(oo[i + 1])].tobytes() for i in range(pr.size)]
    p = {name: str(tmp_path / name) for name in ("x.fq", "pieces.fa", "in.fa", "a.out", "b.out", "a.keys", "c.keys", "c.out")}
    open(p["x.fq"], "wb").write(fastq_text(reads, quals))
    open(p["pieces.fa"], "wb").write(fasta_text(pieces))
    open(p["in.fa"], "wb").write(fasta_text(reads))
    assert cli.main(["-i", p["in.fa"], "-o", p["a.out"], "--save-set", p["a.keys"], "-c", "one", "fastq", "-i", p["x.fq"], "-k", str(K), "-a", "2",
                     "-q", "20"]) == 0
    assert cli.main(["-i", p["in.fa"], "-o", p["b.out"], "-c", "one", "fasta", "-i", p["pieces.fa"], "-k", str(K), "-a", "2"]) == 0
    a, b = open(p["a.out"], "rb").read(), open(p["b.out"], "rb").read()
    assert a == b and a.count(b">") == len(reads)
    want = br_amd.Counter(K)
    want.add_reads(pieces)
    want_fp = want.finish(2).fingerprint()
    with open(p["a.keys"], "rb") as f:
        assert br_amd.Pcon.from_keyfile(f).fingerprint() == want_fp
    # `fasta` without --skip-non-acgt: the set of the old entry, byte for byte as a key file
    assert cli.main(["-i", p["in.fa"], "-o", p["c.out"], "--save-set", p["c.keys"], "-c", "one", "fasta", "-i", p["in.fa"], "-k", str(K), "-a", "2"]) == 0
    old = br_amd.Counter(K)
    st8 = (C.c_uint64 * 8)()
    with open(p["in.fa"], "rb") as f:
        _lib.check(_lib.lib().brx_count_fasta_fd(old._h, f.fileno(), 0, st8))
    buf = io.BytesIO()
    old.finish(2).save_keys(buf)
    assert open(p["c.keys"], "rb").read() == buf.getvalue() and st8[0] == len(reads)
    # ... and with it: the 40 N no longer make a solid homopolymer k-mer
    args = cli.parser().parse_args(["fasta", "-i", p["in.fa"], "-k", str(K), "-a", "2", "--skip-non-acgt"])
    poly = (1 << (2 * K)) - 1
    assert not cli.build_set(args).get(poly) and br_amd.Pcon.from_keyfile(io.BytesIO(buf.getvalue())).get(poly)
    # solid -f fastq: the set the Python parser path gave
    with open(p["x.fq"], "rb") as f:
        parsed = br_amd.Pcon.from_fasta(fasta.read_fastq_sequences(f), K)
    assert cli.presence_set(p["x.fq"], "fastq", K, 0).fingerprint() == parsed.fingerprint()
    cut = br_amd.Pcon.from_fasta(pieces, K)
    assert cli.presence_set(p["x.fq"], "fastq", K, 0, 20, True).fingerprint() == cut.fingerprint() != parsed.fingerprint()


# ---- 7. bad arguments ----------------------------------------------------------------------------------------------------------------

@gpu
def test_bad_arguments_are_refused():
    """each refusal names its cause and leaves the counter as it was.  `a counter of another device` on a machine with one
    GPU is a device index past the last one: the device entry refuses it the way every entry refuses such a handle"""
    reads, quals = count_case()
    data = fastq_text(reads, quals)
    c = br_amd.Counter(K, strategy=DENSE)
    c.count_reads(io.BytesIO(data), "fastq", 20, True)
    before = c.spectrum().tolist()
    st8, tot8 = (C.c_uint64 * 8)(), (C.c_uint64 * 8)()
    L = _lib.lib()
    r, w = os.pipe()
    os.write(w, data[:1000])
    os.close(w)
    try:
        opts = _lib.TrustOpts(94, 1, 0, 0)
        assert L.brx_count_reads_fd(c._h, r, 1, 0, C.byref(opts), st8, tot8) == _lib.BRX_ERR_ARG
        assert b"min_quality=94" in L.brx_last_error()
        assert L.brx_count_reads_fd(c._h, r, 2, 0, None, st8, tot8) == _lib.BRX_ERR_ARG
        assert b"format 2" in L.brx_last_error()
        assert os.read(r, 10) == data[:10]  # refused before anything was read
    finally:
        os.close(r)
    with pytest.raises(_lib.BrxError, match="min_quality=94"):
        c.count_reads(io.BytesIO(data), "fastq", 94, True)
    with pytest.raises(_lib.BrxError, match="format 2"):
        c.count_reads(io.BytesIO(data), 2, 20, True)
    assert c.spectrum().tolist() == before
    bases, _, offs = shape_case()
    d_b, d_o = dev(bases), dev(offs)
    n, total = offs.size - 1, bases.size
    with pytest.raises(_lib.BrxError, match="null bases / offsets") as e:
        trust_split_batch_device(d_b.data_ptr(), None, None, n, total, 20, True, K)
    assert e.value.status == _lib.BRX_ERR_ARG
    with pytest.raises(_lib.BrxError, match="min_quality=94") as e:
        trust_split_batch_device(d_b.data_ptr(), None, d_o.data_ptr(), n, total, 94, True, K)
    assert e.value.status == _lib.BRX_ERR_ARG
    with pytest.raises(_lib.BrxError, match="out of range") as e:
        trust_split_batch_device(d_b.data_ptr(), None, d_o.data_ptr(), n, total, 20, True, K, device=_lib.device_count())
    assert e.value.status == _lib.BRX_ERR_ARG
    with pytest.raises(_lib.BrxError, match="null offsets"):
        outs = (C.POINTER(C.c_uint8)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint64)(), C.c_uint32(0))
        _lib.check(L.brx_trust_split_batch(bases.ctypes.data, None, None, n, C.byref(_lib.TrustOpts(20, 1, 0, K)), C.byref(outs[0]),
                                           C.byref(outs[1]), C.byref(outs[2]), C.byref(outs[3]), None, C.byref(outs[4]), 0))
    with pytest.raises(_lib.BrxError, match="null opts"):
        n_out, t_out = C.c_uint32(0), C.c_uint64(0)
        _lib.check(L.brx_trust_split_batch_device(d_b.data_ptr(), None, d_o.data_ptr(), n, total, None, None, 0, None, None, None, 0, None,
                                                  C.byref(n_out), C.byref(t_out), 0, None))
    assert c.spectrum().tolist() == before
