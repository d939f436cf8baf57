"""Every route to KmerSet::get answers the same for every k-mer.

The device has one definition of the get logic (set_get, br_amd/csrc/brx_index.hpp; the cover kernel keeps a written-out
copy, cover_get) and the host ONE construction of the view a kernel probes with (set_view, brx_index.hip).  The routes
that reach them -- `Pcon.get`, `get_batch_indexed`,
the BRX_COVER_SOLID_START bit of `cover_reads`, the solid mask under a lane-form Graph pass -- are compared here with
the oracle's `Solid.get` on every k-mer start position of the first 20 reads of the reference fixture, over the three
ways a set is held (bit vector + overflowing index, chained table, key list + index with a lazy bit vector), with the
occupancy bits consulted and not (BRX_LINE_BITS).  Exact, no sampling except for the one-k-mer-per-call `Pcon.get`."""
import numpy as np
import pytest

import br_amd
from br_amd import cover
from oracle import oracle as O

pytestmark = pytest.mark.gpu

N_READS = 20
LINE_BITS = [None, "0"]


def _mixed(raw_reads, k):
    """the 20 reads with an empty read, a short one and one of exactly k bases in between"""
    odd = [b"", raw_reads[0][:k - 1], raw_reads[1][:k]]
    out = []
    for i, r in enumerate(raw_reads[:N_READS]):
        out.append(odd[i % len(odd)])
        out.append(r)
    out.append(b"")
    return out


def _oracle_solid(ref, reads):
    """Solid.get of every k-mer start position, read by read (Solid.mask is get over the k-mers of a read)"""
    k = ref.k
    return [np.unpackbits(ref.mask(r), bitorder="little")[:max(len(r) - k + 1, 0)].astype(bool) for r in reads]


@pytest.fixture(scope="module")
def refs(raw_reads, solid_fixture_bytes):
    """per k: (oracle set, the mixed reads, Solid.get per position, all k-mers, all answers); computed once, never changed"""
    sets = {11: O.Solid.from_bytes(solid_fixture_bytes),
            15: O.Solid.sparse_from_count(15, raw_reads[:150], 1),
            19: O.Solid.sparse_from_count(19, raw_reads[:150], 1)}
    out = {}
    for k, ref in sets.items():
        reads = _mixed(raw_reads, k)
        want = _oracle_solid(ref, reads)
        kmers = np.concatenate([cover.kmers_of(r, k) for r in reads])
        flat = np.concatenate(want)
        assert kmers.size == flat.size == sum(max(len(r) - k + 1, 0) for r in reads)
        assert flat.any() and not flat.all()  # neither all-true nor all-false would pass
        for i in range(0, kmers.size, 9973):   # mask IS get, k-mer by k-mer
            assert ref.get(int(kmers[i])) == bool(flat[i])
        out[k] = (ref, reads, want, kmers, flat)
    return out


def _set_line_bits(monkeypatch, line_bits):
    if line_bits is None:
        monkeypatch.delenv("BRX_LINE_BITS", raising=False)
    else:
        monkeypatch.setenv("BRX_LINE_BITS", line_bits)


def _check_routes(gs, case):
    _, reads, want, kmers, flat = case
    # the cover kernel: one probe per position, 64 neighbours a step (also builds the index where the set has none yet)
    got_fl, _ = gs.cover_reads(reads)
    for i, (f, w) in enumerate(zip(got_fl, want)):
        assert f.size == len(reads[i])
        assert np.array_equal((f[:w.size] & cover.SOLID_START) != 0, w), f"cover, read {i} (n={len(reads[i])})"
        assert not (f[w.size:] & cover.SOLID_START).any(), f"cover, tail of read {i}"
    assert gs.index_info()["valid"]
    # the index kernel: one probe per k-mer, no neighbours
    got, n_fallback = gs.get_batch_indexed(kmers)
    assert np.array_equal(got, flat), "get_batch_indexed"
    # one k-mer per call
    for i in range(0, kmers.size, 4001):
        assert gs.get(int(kmers[i])) == bool(flat[i]), f"Pcon.get, k-mer {i}"
    return n_fallback


@pytest.mark.parametrize("line_bits", LINE_BITS)
def test_dense_set_with_an_overflowing_index(raw_reads, solid_fixture_bytes, refs, line_bits, monkeypatch):
    """bit vector + 64 index lines for 25k solid 11-mers: nearly every probe takes the fallback to the bits"""
    monkeypatch.setenv("BRX_INDEX_MIN_K", "5")
    monkeypatch.setenv("BRX_INDEX_LOG_LINES", "6")
    _set_line_bits(monkeypatch, line_bits)
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    assert gs.bits_state() == 0
    n_fallback = _check_routes(gs, refs[11])
    info = gs.index_info()
    assert info["log2_lines"] == 6 and info["overflow_keys"] > 0 and n_fallback > 0
    # the mask a Graph forward pass in lane form scans from (lane_mask_kernel) is not exposed: the pass itself must
    # equal the oracle
    reads = refs[11][1]
    om = O.build_methods(refs[11][0], ["graph"], 5, 7)
    got = br_amd.Chain(gs, [("graph", 5, 7)], two_side=False).correct_reads(reads)
    for i, (r, g) in enumerate(zip(reads, got)):
        assert g == O.correct_record(om, r, False), f"graph, read {i}"


@pytest.mark.parametrize("line_bits", LINE_BITS)
def test_sparse_chained_set(raw_reads, refs, line_bits, monkeypatch):
    """no bit vector, 16 lines: the keys chain from line to line and a get walks the chain"""
    monkeypatch.setenv("BRX_FORCE_SPARSE", "1")
    monkeypatch.setenv("BRX_INDEX_LOG_LINES", "4")
    _set_line_bits(monkeypatch, line_bits)
    gs = br_amd.Pcon.from_count(raw_reads[:150], 15, 1)
    assert gs.is_sparse() and gs.popcount() == refs[15][0].popcount()
    n_fallback = _check_routes(gs, refs[15])
    info = gs.index_info()
    assert info["overflow_keys"] > info["keys"] // 10  # chained, overflowing lines
    assert n_fallback > 0


@pytest.mark.parametrize("line_bits", LINE_BITS)
def test_lazy_bit_vector_stays_lazy(raw_reads, refs, line_bits, monkeypatch):
    """k = 19 counted: key list + index, the bit vector never materialised by a get"""
    _set_line_bits(monkeypatch, line_bits)
    gs = br_amd.Pcon.from_count(raw_reads[:150], 19, 1)
    assert gs.bits_state() == 1 and gs.popcount() == refs[19][0].popcount()
    _check_routes(gs, refs[19])
    assert gs.bits_state() == 1
