"""Whatever holds a solid set -- a current bit vector, a complete key list, an exact chained table, closed or open -- every
entry that enumerates or counts its keys gives the same members (br_amd/csrc/brx_setstate.hpp states who holds them; set_keys
in brx_index.hip resolves it once).  The members come from the oracle's hashes and numpy, never from the library, and every
case first asserts the state it claims to be in: bits_state(), keylist_device(), index_info()."""
import io

import numpy as np
import pytest

import br_amd
from br_amd import _lib, keyfile, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

K = 15


def _members(k, reads, abundance):
    """sorted hashes (canonical >> 1) of the k-mers seen more than `abundance` times, and the number of k-mers counted"""
    allh = np.concatenate([O.hashes(k, r) for r in reads])
    uniq, cnt = np.unique(allh, return_counts=True)
    return np.ascontiguousarray(uniq[np.minimum(cnt, 255) > abundance], dtype=np.uint64), int(allh.size)


def _kmers_of(hashes):
    """the canonical k-mer of every hash: the hash with the bit below it that makes the popcount even"""
    h = np.asarray(hashes, dtype=np.uint64)
    p = h.copy()
    for s in (32, 16, 8, 4, 2, 1):
        p ^= p >> np.uint64(s)
    return (h << np.uint64(1)) | (p & np.uint64(1))


def _fingerprint(members):
    with np.errstate(over="ignore"):
        return int(members.size), int(members.sum(dtype=np.uint64)), int((members * members).sum(dtype=np.uint64))


def _exported_members(bits):
    """bit indices set in a packed Lsb0 array (only the non-zero bytes are unpacked)"""
    nz = np.flatnonzero(bits)
    on = np.unpackbits(bits[nz], bitorder="little").reshape(-1, 8)
    return (nz.astype(np.uint64)[:, None] * np.uint64(8) + np.arange(8, dtype=np.uint64))[on.astype(bool)]


def _state(gs):
    info = gs.index_info()
    return {"bits": gs.bits_state(), "list": gs.keylist_device() is not None, "attached": info["keylist"], "index": info["valid"]}


def _check_entries(gs, k, members, bits=False):
    """popcount, fingerprint, key file, union with itself, probes through the index; `bits`: the exported vector too (last:
    it materialises a lazy one)"""
    want = _fingerprint(members)
    state = gs.bits_state()
    assert gs.popcount() == want[0]
    assert gs.fingerprint() == want
    f = io.BytesIO()
    gs.save_keys(f)
    fk, keys, counts, _ = keyfile.decode(f.getvalue())
    assert fk == k and counts is None and np.array_equal(keys, members)
    u = gs.union(gs)
    assert u.popcount() == want[0] and u.fingerprint() == want
    del u
    assert gs.bits_state() == state  # none of these wrote a lazy vector
    if not gs.index_info()["valid"]:
        if state == 0:
            gs.index_build()
        else:
            gs.get_many(_kmers_of(members[:1]))  # index_ensure: from the list, the vector stays as it is
    assert gs.index_info()["valid"] and gs.bits_state() == state
    inside = members[::97]
    rng = np.random.default_rng(97)
    outside = rng.integers(0, 1 << (2 * k - 1), size=2 * inside.size + 64, dtype=np.uint64)
    outside = outside[~np.isin(outside, members)][:inside.size]
    assert outside.size == inside.size
    got, _ = gs.get_batch_indexed(np.concatenate([_kmers_of(inside), _kmers_of(outside)]))
    assert got[:inside.size].all() and not got[inside.size:].any()
    assert gs.popcount() == want[0] and gs.fingerprint() == want  # ... and with the index beside it
    if bits:
        assert np.array_equal(_exported_members(gs.export_bits()), members)
        assert gs.bits_state() == 0


@pytest.fixture(scope="module")
def genome_reads():
    """400 reads of 2 kb from a 40 kb genome, and the 15-mers seen more than twice"""
    cfg = synth.config(genome_len=40_000, read_len=2_000)
    g = synth.genome_host(cfg)
    bases, offs = synth.reads_host(cfg, g, 0, 400)
    reads = [bases[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(400)]
    members, _ = _members(K, reads, 2)
    assert members.size > 10_000
    return reads, members


def _counted(reads, abundance, monkeypatch, **env):
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    try:
        c = br_amd.Counter(K, 0, _lib.COUNT_SORTED)
        if reads:
            c.add_reads(reads)
        return c.finish(abundance)
    finally:
        for name in env:
            monkeypatch.delenv(name, raising=False)


def _own_list_copy(gs):
    import torch
    from br_amd import dist as bd
    ptr, n = gs.keylist_device()
    return bd.device_view(ptr, n * 8).view(torch.int64).clone()


def test_a_bits_only(solid_fixture_bytes, monkeypatch):
    monkeypatch.setenv("BRX_INDEX_MIN_K", "5")
    members = _exported_members(np.frombuffer(solid_fixture_bytes[1:], dtype=np.uint8))
    assert members.size > 1000
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    assert _state(gs) == {"bits": 0, "list": False, "attached": False, "index": False}
    _check_entries(gs, 11, members, bits=True)


def test_b_lazy_bits_complete_list(genome_reads, monkeypatch):
    reads, members = genome_reads
    gs = _counted(reads, 2, monkeypatch)
    assert _state(gs) == {"bits": 1, "list": True, "attached": True, "index": False}
    assert gs.keylist_device()[1] == members.size
    _check_entries(gs, K, members, bits=True)


def test_c_sparse_list(genome_reads, monkeypatch):
    reads, members = genome_reads
    gs = _counted(reads, 2, monkeypatch, BRX_FORCE_SPARSE="1")
    assert _state(gs) == {"bits": 2, "list": True, "attached": True, "index": False}
    _check_entries(gs, K, members)


def test_d_sparse_closed_table_list_void(genome_reads, monkeypatch):
    reads, members = genome_reads
    gs = _counted(reads, 2, monkeypatch, BRX_FORCE_SPARSE="1")
    keys = _own_list_copy(gs)
    gs.index_build_from_keys_device(keys.data_ptr(), keys.numel())
    assert _state(gs) == {"bits": 2, "list": False, "attached": False, "index": True}
    _check_entries(gs, K, members)
    with pytest.raises(_lib.BrxError):  # closed: built by counting
        gs.insert_reads([b"ACGTTGCATGCCGATAGCTAGGATC"])


def test_e_sparse_open_table(genome_reads, monkeypatch):
    reads, _ = genome_reads
    members, _ = _members(K, reads[:40], 0)  # every k-mer of the reads
    gs = _counted([], 0, monkeypatch, BRX_FORCE_SPARSE="1")  # the empty sparse set
    assert gs.is_sparse() and gs.popcount() == 0
    gs.insert_reads(reads[:25])
    gs.insert_reads(reads[25:40])  # open: more can be added
    assert _state(gs) == {"bits": 2, "list": False, "attached": False, "index": True}
    _check_entries(gs, K, members)


def test_f_lazy_bits_exact_table_list_void(genome_reads, monkeypatch):
    reads, members = genome_reads
    gs = _counted(reads, 2, monkeypatch)
    keys = _own_list_copy(gs)
    gs.index_build_from_keys_device(keys.data_ptr(), keys.numel())
    assert _state(gs) == {"bits": 1, "list": False, "attached": False, "index": True}
    _check_entries(gs, K, members)
    assert gs.bits_state() == 1
    assert np.array_equal(_exported_members(gs.export_bits()), members)  # materialised from the table
    assert _state(gs) == {"bits": 0, "list": False, "attached": False, "index": True}
    _check_entries(gs, K, members, bits=True)


def test_g_current_bits_truncated_list(monkeypatch):
    """One random 2 000 000-base read given twice, abundance 1: every distinct 15-mer is solid, about 2 M of them, and the
    list a finish that also writes the bits sizes at (k-mers counted) / 8 + 2^20 cannot hold them.  The list is attached
    and truncated: it is no list, and the bits answer.  (Before the holder rule was stated in one place the fingerprint of
    this set was that of the list's first 1 548 572 entries -- its capacity -- against 1 996 140 members.)"""
    rng = np.random.default_rng(7)
    read = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=2_000_000)].tobytes()
    members, total = _members(K, [read, read], 1)
    capacity = total // 8 + (1 << 20)
    print(f"members {members.size} capacity {capacity}")
    assert members.size > capacity
    gs = _counted([read, read], 1, monkeypatch, BRX_LAZY_BITS="0")
    assert _state(gs) == {"bits": 0, "list": False, "attached": True, "index": False}
    print(f"fingerprint()[0] {gs.fingerprint()[0]}")
    _check_entries(gs, K, members, bits=True)
    assert gs.keylist_device() is None
