"""br::set mirror: KmerSet trait and the Pcon bitset set, backed by libbrx (HIP).

Reference: src/set.rs:17-23 (trait KmerSet {get, k}, BoxKmerSet), src/set/pcon.rs:13-196
(Pcon::{new, from_pcon_solid, from_fasta}, get/k), src/main.rs:72-115 (build by counting).
"""
from __future__ import annotations

import ctypes as C
import gzip
import io
from typing import Iterable, Optional, Sequence, Tuple

import numpy as np

from . import _lib


def _check_u8(v: int, what: str) -> None:
    if not 0 <= int(v) <= 255:  # u8 in the reference (src/cli.rs:196); ctypes would wrap it silently
        raise ValueError(f"{what}={v} does not fit the reference's u8")


def pack_reads(reads: Sequence[bytes]) -> Tuple[np.ndarray, np.ndarray]:
    """records -> (bases uint8[total], offsets uint64[n+1]): the batch layout of include/brx.h."""
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    if reads:
        offs[1:] = np.cumsum([len(r) for r in reads], dtype=np.uint64)
    bases = np.frombuffer(b"".join(reads), dtype=np.uint8) if reads else np.zeros(0, dtype=np.uint8)
    return np.ascontiguousarray(bases), offs


def seq2bit(seq: bytes) -> int:
    """cocktail::kmer::seq2bit: (ascii >> 1) & 3 per base, first base most significant."""
    k = 0
    for c in seq:
        k = (k << 2) | ((c >> 1) & 3)
    return k


def _keyfile_stats(st) -> dict:
    """stats8 of the key-file entries (include/brx.h "key files")"""
    return {"keys": int(st[0]), "bytes": int(st[1]), "blocks": int(st[2]), "max_width": int(st[3]), "ns_list_sort": int(st[4]),
            "ns_pack": int(st[5]), "ns_fd": int(st[6]), "ns_wall": int(st[7])}


def sort_keys_device(d_keys: int, d_payload: Optional[int], n: int, key_bits: int, stream: Optional[int] = None) -> None:
    """stable radix sort of n u64 keys on the device by their low key_bits bits, a payload byte per key moving along
    (brx_sort_keys_device)"""
    _lib.check(_lib.lib().brx_sort_keys_device(d_keys, d_payload, n, key_bits, stream))


def combine_keys_device(d_a: Optional[int], na: int, d_b: Optional[int], nb: int, op, d_out: Optional[int], cap: int,
                        stream: Optional[int] = None) -> Tuple[int, Tuple[int, int, int]]:
    """(size of the result, (|A|, |B|, |A n B|)) of two strictly ascending u64 key arrays on the device combined by `op`
    (a name of setops.OPS or a BRX_SETOP_* number) into d_out, which holds `cap` keys; d_out None with cap 0 asks for the
    sizes only (brx_keys_combine_device).  A BrxError carries `needed` where the library said how many keys there are"""
    from . import setops
    n, s3 = C.c_uint64(0), (C.c_uint64 * 3)()
    st = _lib.lib().brx_keys_combine_device(d_a, na, d_b, nb, setops.op_id(op) if isinstance(op, str) else int(op), d_out, cap,
                                            C.byref(n), s3, stream)
    try:
        _lib.check(st)
    except _lib.BrxError as e:
        e.needed = int(n.value)
        raise
    return int(n.value), (int(s3[0]), int(s3[1]), int(s3[2]))


def combine_counts_device(d_ka: Optional[int], d_ca: Optional[int], na: int, d_kb: Optional[int], d_cb: Optional[int], nb: int, op,
                          d_kout: Optional[int], d_cout: Optional[int], cap: int, min_count: int = 1,
                          stream: Optional[int] = None) -> Tuple[int, Tuple[int, int, int]]:
    """(size of the result, (|A|, |B|, |A n B|)) of two count lists on the device -- strictly ascending u64 keys, a u8 count
    >= 1 each -- combined by `op` (a name of countops.OPS or a BRX_COUNTOP_* number), results below min_count dropped, into
    d_kout / d_cout, which hold `cap` entries; d_cout None writes the keys only, d_kout None with cap 0 asks for the sizes
    only (brx_counts_combine_device).  A BrxError carries `needed` where the library said how many entries there are"""
    from . import countops
    _check_u8(min_count, "min_count")
    n, s3 = C.c_uint64(0), (C.c_uint64 * 3)()
    st = _lib.lib().brx_counts_combine_device(d_ka, d_ca, na, d_kb, d_cb, nb, countops.op_id(op) if isinstance(op, str) else int(op),
                                              min_count, d_kout, d_cout, cap, C.byref(n), s3, stream)
    try:
        _lib.check(st)
    except _lib.BrxError as e:
        e.needed = int(n.value)
        raise
    return int(n.value), (int(s3[0]), int(s3[1]), int(s3[2]))


def joint_counts_device(d_ka: Optional[int], d_ca: Optional[int], na: int, d_kb: Optional[int], d_cb: Optional[int], nb: int,
                        d_joint: int, stream: Optional[int] = None) -> Tuple[int, int, int]:
    """(|A|, |B|, |A n B|) of two count lists on the device, their joint spectrum -- countops.joint, J[0][0] = 0 -- written
    to d_joint, 65536 u64 on the device, row ca and column cb (brx_counts_joint_device).  A refusal leaves d_joint untouched"""
    s3 = (C.c_uint64 * 3)()
    _lib.check(_lib.lib().brx_counts_joint_device(d_ka, d_ca, na, d_kb, d_cb, nb, d_joint, s3, stream))
    return int(s3[0]), int(s3[1]), int(s3[2])


def format_kmertext_device(k: int, d_keys: Optional[int], d_counts: Optional[int], n: int, d_text: Optional[int], cap: int,
                           strand="lex", stream: Optional[int] = None) -> int:
    """bytes of the k-mer text (kmertext.format_lines) of n entries on the device -- u64 keys, u8 counts, in the order given
    -- written to d_text, which holds `cap` bytes (brx_kmertext_format_device).  A BrxError carries `needed` where the
    library said how many bytes the text takes; d_text is untouched then"""
    from . import kmertext
    n_bytes = C.c_uint64(0)
    st = _lib.lib().brx_kmertext_format_device(k, d_keys, d_counts, n, kmertext.strand_id(strand) if isinstance(strand, str) else int(strand),
                                               d_text, cap, C.byref(n_bytes), stream)
    try:
        _lib.check(st)
    except _lib.BrxError as e:
        e.needed = int(n_bytes.value)
        raise
    return int(n_bytes.value)


def parse_kmertext_device(d_text: Optional[int], n_bytes: int, k: int, d_keys: Optional[int], d_counts: Optional[int], cap: int,
                          stream: Optional[int] = None) -> int:
    """the number of non-empty lines of a k-mer text on the device, their (canonical key, min(255, value)) pairs written to
    d_keys / d_counts in line order, neither sorted nor summed: kmertext.parse_lines (brx_kmertext_parse_device).  A
    BrxError carries `needed` (a cap too small) and `err3` = (cause, line from 0, column) of the first malformed line"""
    n, err3 = C.c_uint64(0), (C.c_uint64 * 3)()
    st = _lib.lib().brx_kmertext_parse_device(d_text, n_bytes, k, d_keys, d_counts, cap, C.byref(n), err3, stream)
    try:
        _lib.check(st)
    except _lib.BrxError as e:
        e.needed = int(n.value)
        e.err3 = (int(err3[0]), int(err3[1]), int(err3[2]))
        raise
    return int(n.value)


def _trust_opts(min_quality: int, acgt_only: bool, min_len: int = 0) -> "_lib.TrustOpts":
    """brx_trust_opts_t; min_quality is handed over as it is (0..255) so that the library's own refusal of 94 and more is seen"""
    _check_u8(min_quality, "min_quality")
    if not 0 <= int(min_len) < 1 << 32:
        raise ValueError(f"min_len={min_len} does not fit 32 bits")
    return _lib.TrustOpts(int(min_quality), 1 if acgt_only else 0, 0, int(min_len))


def _read_opts(min_quality, acgt_only):
    """the opts pointer of the _reads_fd entries: None (every k-mer, every byte a base) when nothing is asked for"""
    if not min_quality and not acgt_only:
        return None
    return C.byref(_trust_opts(min_quality or 0, acgt_only))


def _read_format(fmt) -> int:
    if isinstance(fmt, str):
        if fmt not in _lib.READ_FORMATS:
            raise ValueError(f"read format {fmt!r}: one of {sorted(_lib.READ_FORMATS)}")
        return _lib.READ_FORMATS[fmt]
    return int(fmt)


def _stream_stats(st, tot=None) -> dict:
    d = {"records": int(st[0]), "bases_in": int(st[1]), "batches": int(st[3]), "ns_parse": int(st[4]), "ns_gpu": int(st[5]),
         "ns_wall": int(st[7])}
    if tot is not None:
        from . import trust
        d["trust"] = {name: int(tot[i]) for i, name in enumerate(trust.TOTALS)}
    return d


def trust_split_batch(bases: np.ndarray, quals: Optional[np.ndarray], offsets: np.ndarray, min_quality: int = 0,
                      acgt_only: bool = True, min_len: int = 1, device: int = 0):
    """(out uint8[], out_offsets uint64[p+1], piece_read uint32[p], piece_start uint64[p], stats trust.STATS_DTYPE[n]): the
    trusted stretches of at least max(min_len, 1) bases of a bases / offsets batch, cut on the GPU (brx_trust_split_batch;
    br_amd/trust.py states the definitions).  `quals` (or None) is laid out like `bases`"""
    from . import trust
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    if quals is not None:
        quals = np.ascontiguousarray(quals, dtype=np.uint8)
        if quals.size != bases.size:
            raise ValueError(f"{quals.size} qualities for {bases.size} bases")
    n_reads = offsets.size - 1
    opts = _trust_opts(min_quality, acgt_only, min_len)
    st = np.zeros(n_reads, dtype=trust.STATS_DTYPE)
    L = _lib.lib()
    ob, oo = C.POINTER(C.c_uint8)(), C.POINTER(C.c_uint64)()
    pr, ps, n = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint64)(), C.c_uint32(0)
    _lib.check(L.brx_trust_split_batch(bases.ctypes.data, quals.ctypes.data if quals is not None else None, offsets.ctypes.data,
                                       n_reads, C.byref(opts), C.byref(ob), C.byref(oo), C.byref(pr), C.byref(ps), st.ctypes.data,
                                       C.byref(n), device))
    try:
        p = n.value
        out_off = np.ctypeslib.as_array(oo, shape=(p + 1,)).copy()
        total = int(out_off[-1])
        out = np.ctypeslib.as_array(ob, shape=(max(total, 1),))[:total].copy()
        piece_read = np.ctypeslib.as_array(pr, shape=(max(p, 1),))[:p].copy()
        piece_start = np.ctypeslib.as_array(ps, shape=(max(p, 1),))[:p].copy()
    finally:
        for q in (ob, oo, pr, ps):
            L.brx_buf_free(C.cast(q, C.c_void_p))
    return out, out_off, piece_read, piece_start, st


def trust_split_batch_device(d_bases: Optional[int], d_quals: Optional[int], d_offsets: Optional[int], n_reads: int, total_bases: int,
                             min_quality: int = 0, acgt_only: bool = True, min_len: int = 1, d_out: Optional[int] = None,
                             out_cap: int = 0, d_out_offsets: Optional[int] = None, d_piece_read: Optional[int] = None,
                             d_piece_start: Optional[int] = None, piece_cap: int = 0, d_stats: Optional[int] = None, device: int = 0,
                             stream: Optional[int] = None) -> Tuple[int, int]:
    """(pieces, bytes) of the split form written to the caller's device buffers (brx_trust_split_batch_device); capacities
    of 0 with no outputs ask for the sizes.  A BrxError of status BRX_ERR_OVERFLOW carries them as `needed`"""
    opts = _trust_opts(min_quality, acgt_only, min_len)
    n, total = C.c_uint32(0), C.c_uint64(0)
    st = _lib.lib().brx_trust_split_batch_device(d_bases, d_quals, d_offsets, n_reads, total_bases, C.byref(opts), d_out, out_cap,
                                                 d_out_offsets, d_piece_read, d_piece_start, piece_cap, d_stats, C.byref(n),
                                                 C.byref(total), device, stream)
    try:
        _lib.check(st)
    except _lib.BrxError as e:
        e.needed = (int(n.value), int(total.value))
        raise
    return int(n.value), int(total.value)


class KmerSet:
    """trait KmerSet (src/set.rs:17-21)."""

    def get(self, kmer: int) -> bool:  # pragma: no cover - interface
        raise NotImplementedError

    def k(self) -> int:  # pragma: no cover - interface
        raise NotImplementedError


class Pcon(KmerSet):
    """set::Pcon: canonical-k-mer bitset resident in HBM (src/set/pcon.rs:13-15)."""

    def __init__(self, handle: int, device: int):
        self._h = C.c_void_p(handle)
        self.device = device

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                _lib.lib().brx_set_free(self._h)
                self._h = C.c_void_p(None)
        except Exception:
            pass

    # ---- constructors -----------------------------------------------------------------
    @classmethod
    def new(cls, k: int, device: int = 0) -> "Pcon":
        """Pcon::new(pcon::solid::Solid::new(k)) (src/set/pcon.rs:183-185)."""
        h = C.c_void_p()
        _lib.check(_lib.lib().brx_set_new(k, device, C.byref(h)))
        return cls(h.value, device)

    @classmethod
    def from_pcon_solid(cls, data: bytes, device: int = 0) -> "Pcon":
        """Pcon::from_pcon_solid (src/set/pcon.rs:18-25).  `data` may be gzip (niffler sniffs
        compression at src/cli.rs:415) or the raw [k][bits] stream."""
        if data[:2] == b"\x1f\x8b":
            data = gzip.decompress(data)
        buf = np.frombuffer(data, dtype=np.uint8)
        h = C.c_void_p()
        _lib.check(_lib.lib().brx_set_new_from_solid_bytes(buf.ctypes.data, buf.size, device, C.byref(h)))
        return cls(h.value, device)

    @classmethod
    def from_fasta(cls, reads: Iterable[bytes], k: int, device: int = 0, batch: int = 8192) -> "Pcon":
        """Pcon::from_fasta (src/set/pcon.rs:47-112): presence-only set of every canonical k-mer."""
        s = cls.new(k, device)
        chunk = []
        for r in reads:
            chunk.append(r)
            if len(chunk) == batch:  # populate_buffer(.., 8192), src/set/pcon.rs:82
                s.insert_reads(chunk)
                chunk = []
        if chunk:
            s.insert_reads(chunk)
        return s

    @classmethod
    def from_fasta_file(cls, f, k: int, device: int = 0) -> "Pcon":
        """from_fasta over a FASTA stream (binary file object) through the native host pipeline"""
        from . import hostio
        s = cls.new(k, device)
        st = (C.c_uint64 * 8)()
        with hostio.input_fd(f) as fd:
            _lib.check(_lib.lib().brx_set_insert_fasta_fd(s._h, fd, 0, st))
        return s

    @classmethod
    def from_reads_file(cls, f, fmt, k: int, device: int = 0, min_quality: int = 0, acgt_only: bool = False) -> "Pcon":
        """presence-only set of a FASTA or FASTQ stream (binary file object; fmt "fasta" / "fastq") through the native host
        pipeline (brx_set_insert_reads_fd).  As the reference's from_fasta / from_fastq by default: every k-mer, every byte
        a base; with min_quality > 0 or acgt_only only the k-mers of the trusted stretches (br_amd/trust.py) are inserted.
        The stream's statistics and trust totals are left in `read_stats`"""
        from . import hostio
        s = cls.new(k, device)
        st, tot = (C.c_uint64 * 8)(), (C.c_uint64 * 8)()
        opts = _read_opts(min_quality, acgt_only)
        with hostio.input_fd(f) as fd:
            _lib.check(_lib.lib().brx_set_insert_reads_fd(s._h, fd, _read_format(fmt), 0, opts, st, tot))
        s.read_stats = _stream_stats(st, tot)
        return s

    @classmethod
    def from_count(cls, reads: Iterable[bytes], k: int, abundance: int, device: int = 0, batch: int = 8192,
                   strategy: int = _lib.COUNT_AUTO) -> "Pcon":
        """`br fasta -k K -a A` (src/main.rs:72-115): count canonical k-mers (u8, saturating),
        solid iff count > abundance."""
        c = Counter(k, device, strategy)
        chunk = []
        for r in reads:
            chunk.append(r)
            if len(chunk) == batch:  # count_fasta(reader, 8192), src/main.rs:74
                c.add_reads(chunk)
                chunk = []
        if chunk:
            c.add_reads(chunk)
        return c.finish(abundance)

    @classmethod
    def from_keyfile(cls, f, device: int = 0) -> "Pcon":
        """the set of a key file (br_amd/keyfile.py; binary file object, any compression already undone): k from the header,
        every key listed a member -- the counts of a count file are ignored (brx_set_load_fd)"""
        from . import hostio
        h = C.c_void_p()
        st = (C.c_uint64 * 8)()
        with hostio.input_fd(f) as fd:
            _lib.check(_lib.lib().brx_set_load_fd(fd, device, C.byref(h), st))
        s = cls(h.value, device)
        s.keyfile_stats = _keyfile_stats(st)
        return s

    def save_keys(self, f) -> dict:
        """write the set as a key file to the binary file object `f`: sorted keys, whatever holds the set (brx_set_save_fd);
        the set is left as it was, a lazy bit vector stays lazy"""
        from . import hostio
        st = (C.c_uint64 * 8)()
        with hostio.output_fd(f) as fd:
            _lib.check(_lib.lib().brx_set_save_fd(self._h, fd, st))
        return _keyfile_stats(st)

    # ---- set algebra (include/brx.h "set algebra", br_amd/setops.py) --------------------------------------------------
    def combine(self, other: "Pcon", op) -> "Pcon":
        """a new closed set, `self op other` (op: a name of setops.OPS or a BRX_SETOP_* number): same k and device, sets
        held in any form; both operands are only read (brx_set_combine)"""
        from . import setops
        if not isinstance(other, Pcon):
            raise TypeError("set algebra needs two Pcon sets")
        h = C.c_void_p()
        st = (C.c_uint64 * 8)()
        _lib.check(_lib.lib().brx_set_combine(self._h, other._h, setops.op_id(op), C.byref(h), st))
        s = Pcon(h.value, self.device)
        s.combine_stats = {"a": int(st[0]), "b": int(st[1]), "both": int(st[2]), "keys": int(st[3]), "ns_list_sort": int(st[4]),
                           "ns_merge": int(st[5]), "ns_build": int(st[6]), "ns_wall": int(st[7])}
        return s

    def union(self, other: "Pcon") -> "Pcon":
        return self.combine(other, "union")

    def intersection(self, other: "Pcon") -> "Pcon":
        return self.combine(other, "intersection")

    def difference(self, other: "Pcon") -> "Pcon":
        return self.combine(other, "difference")

    def symmetric_difference(self, other: "Pcon") -> "Pcon":
        return self.combine(other, "symmetric_difference")

    def _operator(name):
        def op(self, other):
            return self.combine(other, name) if isinstance(other, Pcon) else NotImplemented
        return op

    __or__, __and__ = _operator("union"), _operator("intersection")
    __sub__, __xor__ = _operator("difference"), _operator("symmetric_difference")
    del _operator

    def compare(self, other: "Pcon") -> dict:
        """{"a": |self|, "b": |other|, "both": |self n other|, "jaccard": both / |self u other|, 1.0 for two empty sets}:
        the keys of both listed, sorted and walked once, nothing built (brx_set_compare)"""
        from . import setops
        if not isinstance(other, Pcon):
            raise TypeError("set algebra needs two Pcon sets")
        s3 = (C.c_uint64 * 3)()
        _lib.check(_lib.lib().brx_set_compare(self._h, other._h, s3))
        na, nb, both = int(s3[0]), int(s3[1]), int(s3[2])
        return {"a": na, "b": nb, "both": both, "jaccard": setops.jaccard(na, nb, both)}

    # ---- KmerSet ----------------------------------------------------------------------
    def get(self, kmer: int) -> bool:
        return bool(_lib.lib().brx_set_get(self._h, kmer))

    def k(self) -> int:
        return int(_lib.lib().brx_set_k(self._h))

    def get_many(self, kmers: Sequence[int]) -> np.ndarray:
        km = np.ascontiguousarray(np.asarray(kmers, dtype=np.uint64))
        out = np.zeros(km.size, dtype=np.uint8)
        _lib.check(_lib.lib().brx_set_get_batch(self._h, km.ctypes.data, km.size, out.ctypes.data))
        return out.astype(bool)

    # ---- coverage (include/brx.h "coverage", br_amd/cover.py: no counterpart in the reference) ----
    def cover_batch(self, bases: np.ndarray, offsets: np.ndarray, flags: bool = True, masked: bool = False,
                    stats: bool = True):
        """(flags uint8[total] | None, masked uint8[total] | None, stats cover.STATS_DTYPE[n] | None) of a
        bases / offsets batch: one probe per k-mer, on the GPU (brx_set_cover_batch)."""
        from . import cover
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        fl = np.zeros(bases.size, dtype=np.uint8) if flags else None
        mk = np.zeros(bases.size, dtype=np.uint8) if masked else None
        st = np.zeros(n, dtype=cover.STATS_DTYPE) if stats else None
        ptr = lambda a: a.ctypes.data if a is not None else None
        _lib.check(_lib.lib().brx_set_cover_batch(self._h, bases.ctypes.data, offsets.ctypes.data, n, ptr(fl), ptr(mk),
                                                  ptr(st)))
        return fl, mk, st

    def cover_batch_device(self, d_bases: int, d_offsets: int, n_reads: int, total_bases: int, d_flags: Optional[int] = None,
                           d_masked: Optional[int] = None, d_stats: Optional[int] = None,
                           stream: Optional[int] = None) -> None:
        _lib.check(_lib.lib().brx_set_cover_batch_device(self._h, d_bases, d_offsets, n_reads, total_bases, d_flags,
                                                         d_masked, d_stats, stream))

    def cover_reads(self, reads: Sequence[bytes]):
        """(list of per-read flag arrays, stats array) of `reads`"""
        from . import cover
        bases, offs = pack_reads(reads)
        fl, _, st = self.cover_batch(bases, offs)
        return cover.unpack_flags(fl, offs), st

    def mask_reads(self, reads: Sequence[bytes]) -> list:
        """the masked form of every read: upper case where a solid k-mer covers the base, lower case where none does"""
        bases, offs = pack_reads(reads)
        _, mk, _ = self.cover_batch(bases, offs, flags=False, masked=True, stats=False)
        return [mk[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(len(reads))]

    def split_batch(self, bases: np.ndarray, offsets: np.ndarray, min_len: int = 0):
        """(out uint8[], out_offsets uint64[p+1], piece_read uint32[p], piece_start uint64[p]): the split form"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if not 0 <= int(min_len) < 1 << 32:
            raise ValueError(f"min_len={min_len} does not fit 32 bits")
        L = _lib.lib()
        ob, oo = C.POINTER(C.c_uint8)(), C.POINTER(C.c_uint64)()
        pr, ps, n = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint64)(), C.c_uint32(0)
        _lib.check(L.brx_set_cover_split_batch(self._h, bases.ctypes.data, offsets.ctypes.data, offsets.size - 1, int(min_len),
                                               C.byref(ob), C.byref(oo), C.byref(pr), C.byref(ps), C.byref(n)))
        try:
            p = n.value
            out_off = np.ctypeslib.as_array(oo, shape=(p + 1,)).copy()
            total = int(out_off[-1])
            out = np.ctypeslib.as_array(ob, shape=(max(total, 1),))[:total].copy()
            piece_read = np.ctypeslib.as_array(pr, shape=(max(p, 1),))[:p].copy()
            piece_start = np.ctypeslib.as_array(ps, shape=(max(p, 1),))[:p].copy()
        finally:
            for q in (ob, oo, pr, ps):
                L.brx_buf_free(C.cast(q, C.c_void_p))
        return out, out_off, piece_read, piece_start

    def split_reads(self, reads: Sequence[bytes], min_len: int = 0) -> list:
        """[(read index, start, bytes)] of the runs of at least min_len covered bases, in order"""
        bases, offs = pack_reads(reads)
        out, oo, pr, ps = self.split_batch(bases, offs, min_len)
        return [(int(pr[i]), int(ps[i]), out[int(oo[i]):int(oo[i + 1])].tobytes()) for i in range(pr.size)]

    # ---- Solid-level helpers ----------------------------------------------------------
    def set(self, kmer: int, value: bool = True) -> None:
        _lib.check(_lib.lib().brx_set_set(self._h, kmer, value))

    def insert_reads(self, reads: Sequence[bytes]) -> None:
        bases, offs = pack_reads(reads)
        _lib.check(_lib.lib().brx_set_insert_batch(self._h, bases.ctypes.data, offs.ctypes.data, len(reads)))

    def insert_batch_device(self, d_bases: int, d_offsets: int, n_reads: int, total_bases: int,
                            stream: Optional[int] = None) -> None:
        """insert_reads on device buffers, enqueued on `stream` (brx_set_insert_batch_device)"""
        _lib.check(_lib.lib().brx_set_insert_batch_device(self._h, d_bases, d_offsets, n_reads, total_bases, stream))

    def to_solid_bytes(self) -> bytes:
        n = C.c_size_t(0)
        L = _lib.lib()
        L.brx_set_export_solid_bytes(self._h, None, 0, C.byref(n))
        buf = np.zeros(n.value, dtype=np.uint8)
        _lib.check(L.brx_set_export_solid_bytes(self._h, buf.ctypes.data, buf.size, C.byref(n)))
        return buf.tobytes()

    def export_bits(self) -> np.ndarray:
        """the packed Lsb0 bit array (without the k byte) as uint8[]."""
        n = C.c_size_t(0)
        L = _lib.lib()
        L.brx_set_export_solid_bytes(self._h, None, 0, C.byref(n))
        buf = np.zeros(n.value, dtype=np.uint8)
        _lib.check(L.brx_set_export_solid_bytes(self._h, buf.ctypes.data, buf.size, C.byref(n)))
        return buf[1:]

    def is_sparse(self) -> bool:
        """k >= 21: no bit vector, the solid k-mers live in the key list / probe index only (include/brx.h)"""
        return bool(_lib.lib().brx_set_sparse(self._h))

    def bits_state(self) -> int:
        """0 bit vector current, 1 lazy (materialised on demand), 2 sparse (include/brx.h brx_set_bits_state)"""
        return int(_lib.lib().brx_set_bits_state(self._h))

    def popcount(self) -> int:
        n = C.c_uint64(0)
        _lib.check(_lib.lib().brx_set_popcount(self._h, C.byref(n)))
        return n.value

    def device_bits(self) -> Tuple[int, int]:
        p, n = C.c_void_p(), C.c_uint64(0)
        _lib.check(_lib.lib().brx_set_device_bits(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def n_hashes(self) -> int:
        return max(1 << (2 * self.k() - 1), 32)

    def extract_keys_device(self, first_hash: int, n_hashes: int, d_out: int, cap: int, stream: Optional[int] = None) -> int:
        n = C.c_uint64(0)
        _lib.check(_lib.lib().brx_set_extract_keys_device(self._h, first_hash, n_hashes, d_out, cap, C.byref(n), stream))
        return n.value

    def or_keys_device(self, d_keys: int, n: int, stream: Optional[int] = None) -> None:
        _lib.check(_lib.lib().brx_set_or_keys_device(self._h, d_keys, n, stream))

    # ---- probe index (include/brx.h: an HBM-locality copy of the set, no reference counterpart) ----
    def index_build(self, m: int = 0, log2_lines: int = 0, stream: Optional[int] = None) -> dict:
        _lib.check(_lib.lib().brx_set_index_build(self._h, m, log2_lines, stream))
        return self.index_info()

    def index_build_from_keys_device(self, d_keys: int, n: int, m: int = 0, log2_lines: int = 0,
                                     stream: Optional[int] = None) -> dict:
        _lib.check(_lib.lib().brx_set_index_build_from_keys_device(self._h, d_keys, n, m, log2_lines, stream))
        return self.index_info()

    def keylist_device(self, stream: Optional[int] = None):
        """(device pointer, n) of the solid-hash list a partitioned finish left with the set, or None"""
        ptr, n = C.c_void_p(), C.c_uint64(0)
        _lib.check(_lib.lib().brx_set_keylist_device(self._h, C.byref(ptr), C.byref(n), stream))
        return (ptr.value, n.value) if ptr.value else None

    def fingerprint(self, stream: Optional[int] = None) -> Tuple[int, int, int]:
        """(members, sum of their hashes mod 2^64, sum of the squares mod 2^64): the same for the same set whatever holds
        it -- what the ranks of a multi-GPU job compare after the exchange"""
        out = (C.c_uint64 * 3)()
        _lib.check(_lib.lib().brx_set_fingerprint(self._h, out, stream))
        return int(out[0]), int(out[1]), int(out[2])

    def index_drop(self) -> None:
        _lib.check(_lib.lib().brx_set_index_drop(self._h))

    def index_info(self) -> dict:
        v = (C.c_uint64 * 8)()
        _lib.check(_lib.lib().brx_set_index_info(self._h, v))
        return {"valid": bool(v[0]), "m": int(v[1]), "log2_lines": int(v[2]), "keys": int(v[3]),
                "overflow_keys": int(v[4]), "bytes": int(v[5]), "wanted": bool(v[6]), "keylist": bool(v[7])}

    def get_batch_indexed(self, kmers):
        """(answers, n_fallback): `get_batch` through the probe index."""
        ks = np.ascontiguousarray(kmers, dtype=np.uint64)
        out = np.empty(len(ks), dtype=np.uint8)
        fb = C.c_uint64(0)
        _lib.check(_lib.lib().brx_set_get_batch_indexed(self._h, ks.ctypes.data, len(ks), out.ctypes.data, C.byref(fb)))
        return out.astype(bool), fb.value


class CountList:
    """An immutable sorted list of (key, count) on one device: the content of a count file without a counting table
    (include/brx.h "count lists", br_amd/countops.py).  Lists add, subtract, take the minimum and the maximum by a merge;
    `spectrum()` and `finish(abundance)` give what a table counter that loaded the same file gives.  A list answers
    lookups -- get_counts and the abundance calls, with Counter's signatures -- once `prepare_lookup()` has built its
    bucket directory, about n/2 bytes beside the list's 9n; a k-mer that is not listed answers 0, which for a list of floor
    f > 1 means "counted fewer than f times, or never"."""

    def __init__(self, handle: int, device: int):
        self._h = C.c_void_p(handle)
        self.device = device

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                _lib.lib().brx_counts_free(self._h)
                self._h = C.c_void_p(None)
        except Exception:
            pass

    @classmethod
    def from_keyfile(cls, f, device: int = 0) -> "CountList":
        """the list of a count file (binary file object, any compression already undone; read sequentially, so pipes and
        gzip objects work): k and floor from the header (brx_counts_load_fd).  A set file is refused"""
        from . import hostio
        h = C.c_void_p()
        st = (C.c_uint64 * 8)()
        with hostio.input_fd(f) as fd:
            _lib.check(_lib.lib().brx_counts_load_fd(fd, device, C.byref(h), st))
        l = cls(h.value, device)
        l.keyfile_stats = _keyfile_stats(st)
        return l

    @classmethod
    def from_counter(cls, counter: "Counter", min_count: int = 1) -> "CountList":
        """the list `counter.save(f, min_count)` would write: a table counter, or a partitioned one after prepare_lookup();
        the counter is only read (brx_counts_from_counter)"""
        _check_u8(min_count, "min_count")
        h = C.c_void_p()
        _lib.check(_lib.lib().brx_counts_from_counter(counter._h, min_count, C.byref(h), None))
        return cls(h.value, counter.device)

    @classmethod
    def from_arrays(cls, k: int, keys, counts, floor: int = 1, device: int = 0) -> "CountList":
        """the list of plain arrays: keys (canonical k-mer >> 1) strictly ascending and below 2^(2k-1), one count >= floor
        each; checked on the device, a refusal names the first offending index (brx_counts_from_arrays)"""
        _check_u8(floor, "floor")
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        counts = np.ascontiguousarray(counts, dtype=np.uint8)
        if keys.ndim != 1 or counts.shape != keys.shape:
            raise ValueError("one count per key, both one-dimensional")
        h = C.c_void_p()
        _lib.check(_lib.lib().brx_counts_from_arrays(k, keys.ctypes.data if keys.size else None, counts.ctypes.data if keys.size else None,
                                                     keys.size, floor, device, C.byref(h)))
        return cls(h.value, device)

    @classmethod
    def from_text(cls, f, k: Optional[int] = None, floor: int = 1, device: int = 0) -> "CountList":
        """the list a k-mer text states -- KMER<TAB>COUNT lines as jellyfish dump -c -t and kmc_tools dump write them, in any
        order, either strand, equal k-mers added up to 255: kmertext.parse -- read from the binary file object `f`
        sequentially (pipes and gzip objects work); k None: from the first line; `floor`: the smallest count the text kept,
        the list's floor (brx_counts_import_text_fd).  A malformed line is a BrxError that names its line"""
        from . import hostio
        _check_u8(floor, "floor")
        h = C.c_void_p()
        st = (C.c_uint64 * 8)()
        with hostio.input_fd(f) as fd:
            _lib.check(_lib.lib().brx_counts_import_text_fd(fd, int(k or 0), floor, device, C.byref(h), st))
        l = cls(h.value, device)
        l.text_stats = {"entries": int(st[0]), "bytes": int(st[1]), "lines": int(st[2]), "sorted": bool(st[3]), "ns_sort_sum": int(st[4]),
                        "ns_parse": int(st[5]), "ns_fd": int(st[6]), "ns_wall": int(st[7])}
        return l

    def dump_text(self, f, min_count: int = 1, strand="lex") -> dict:
        """write the list as k-mer text (kmertext.format_lines: ascending key order, not alphabetical) to the binary file
        object `f`, the entries below min_count dropped; strand "lex" prints the alphabetically smaller strand, as Jellyfish
        -C and KMC do, "canonical" the list's own (brx_counts_dump_text_fd)"""
        from . import hostio, kmertext
        _check_u8(min_count, "min_count")
        st = (C.c_uint64 * 8)()
        with hostio.output_fd(f) as fd:
            _lib.check(_lib.lib().brx_counts_dump_text_fd(self._h, min_count, kmertext.strand_id(strand), fd, st))
        return {"entries": int(st[0]), "bytes": int(st[1]), "slices": int(st[2]), "ns_compact": int(st[4]), "ns_format": int(st[5]),
                "ns_fd": int(st[6]), "ns_wall": int(st[7])}

    def save(self, f, min_count: int = 1) -> dict:
        """write the list as a count file to the binary file object `f`, the entries below min_count dropped and the floor
        raised to it (brx_counts_save_fd); a loaded file is saved byte for byte"""
        from . import hostio
        _check_u8(min_count, "min_count")
        st = (C.c_uint64 * 8)()
        with hostio.output_fd(f) as fd:
            _lib.check(_lib.lib().brx_counts_save_fd(self._h, min_count, fd, st))
        return _keyfile_stats(st)

    def _info(self):
        v = (C.c_uint64 * 4)()
        _lib.check(_lib.lib().brx_counts_info(self._h, v))
        return int(v[0]), int(v[1]), int(v[2])

    @property
    def k(self) -> int:
        return self._info()[0]

    @property
    def n(self) -> int:
        """entries"""
        return self._info()[1]

    @property
    def floor(self) -> int:
        """the smallest count the list kept (>= 1): k-mers seen fewer times are unknown to it"""
        return self._info()[2]

    def __len__(self) -> int:
        return self.n

    def device_arrays(self) -> Tuple[int, int, int]:
        """(d_keys, d_counts, n): the list's u64 keys and u8 counts on the device (0, 0, 0 for an empty list), to be read
        only, valid while the list lives"""
        pk, pc, n = C.c_void_p(), C.c_void_p(), C.c_uint64(0)
        _lib.check(_lib.lib().brx_counts_device(self._h, C.byref(pk), C.byref(pc), C.byref(n)))
        return pk.value or 0, pc.value or 0, int(n.value)

    def combine(self, other: "CountList", op, min_count: int = 1) -> "CountList":
        """a new list, `self op other` (op: a name of countops.OPS or a BRX_COUNTOP_* number) with the results below
        min_count dropped: same k and device; the floors follow countops.result_floor; both operands are only read
        (brx_counts_combine)"""
        from . import countops
        if not isinstance(other, CountList):
            raise TypeError("count lists combine with count lists")
        _check_u8(min_count, "min_count")
        h = C.c_void_p()
        st = (C.c_uint64 * 8)()
        _lib.check(_lib.lib().brx_counts_combine(self._h, other._h, countops.op_id(op), min_count, C.byref(h), st))
        l = CountList(h.value, self.device)
        l.combine_stats = {"a": int(st[0]), "b": int(st[1]), "both": int(st[2]), "entries": int(st[3]), "ns_merge": int(st[5]),
                           "ns_wall": int(st[7])}
        return l

    def add(self, other: "CountList", min_count: int = 1) -> "CountList":
        return self.combine(other, "add", min_count)

    def maximum(self, other: "CountList", min_count: int = 1) -> "CountList":
        return self.combine(other, "max", min_count)

    def minimum(self, other: "CountList", min_count: int = 1) -> "CountList":
        return self.combine(other, "min", min_count)

    def subtract(self, other: "CountList", min_count: int = 1) -> "CountList":
        return self.combine(other, "sub", min_count)

    def __add__(self, other):
        return self.combine(other, "add") if isinstance(other, CountList) else NotImplemented

    def __sub__(self, other):
        return self.combine(other, "sub") if isinstance(other, CountList) else NotImplemented

    def joint(self, other: "CountList") -> np.ndarray:
        """uint64[256][256], the joint spectrum of the two lists: J[ca][cb] = k-mers counted ca times here and cb times in
        `other` (0: not listed; countops.joint), J[0][0] = 2^(2k-1) - |self u other|, so that the row sums are
        self.spectrum() and the column sums other.spectrum().  Same k and device; floors refuse nothing; both lists are only
        read (brx_counts_compare)"""
        if not isinstance(other, CountList):
            raise TypeError("count lists compare with count lists")
        J = np.zeros((256, 256), dtype=np.uint64)
        st = (C.c_uint64 * 8)()
        _lib.check(_lib.lib().brx_counts_compare(self._h, other._h, J.ctypes.data_as(C.POINTER(C.c_uint64)), st))
        self.compare_stats = {"a": int(st[0]), "b": int(st[1]), "both": int(st[2]), "either": int(st[3]), "ns_merge": int(st[5]),
                              "ns_wall": int(st[7])}
        return J

    def compare(self, other: "CountList", min_a: int = 1, min_b: int = 1) -> dict:
        """countops.compare_summary of the joint spectrum -- a, b, both, either, jaccard as Pcon.compare names them, the same
        from min_a / min_b up, completeness, occurrences, error_rate and qv -- plus "joint" (the array of joint()) and
        "floor_a", "floor_b": a k-mer a floored list does not hold counts as 0 there: fewer than floor times, or never"""
        from . import countops
        J = self.joint(other)
        res = countops.compare_summary(J, self.k, min_a, min_b)
        res.update(joint=J, floor_a=self.floor, floor_b=other.floor)
        return res

    def spectrum(self) -> np.ndarray:
        """uint64[256], Counter.spectrum() of a table counter that loaded the same file: bin 0 the k-mers not listed, the
        bins below the floor 0 (brx_counts_spectrum)"""
        h = np.zeros(256, dtype=np.uint64)
        _lib.check(_lib.lib().brx_counts_spectrum(self._h, h.ctypes.data_as(C.POINTER(C.c_uint64))))
        return h

    def finish(self, abundance: int) -> "Pcon":
        """the solid set, count > abundance: the set Pcon.from_keyfile makes of those keys (brx_counts_finish).  A threshold
        below floor - 1 is refused, as by a floored counter"""
        _check_u8(abundance, "abundance")
        h = C.c_void_p()
        st = (C.c_uint64 * 8)()
        _lib.check(_lib.lib().brx_counts_finish(self._h, abundance, C.byref(h), st))
        s = Pcon(h.value, self.device)
        s.finish_stats = {"entries": int(st[0]), "kept": int(st[1]), "ns_select": int(st[4]), "ns_build": int(st[6]),
                          "ns_wall": int(st[7])}
        return s

    def to_numpy(self) -> Tuple[np.ndarray, np.ndarray]:
        """(keys uint64[n], counts uint8[n]) on the host: a copy by way of the list's file, for tests and small lists"""
        from . import keyfile
        f = io.BytesIO()
        self.save(f)
        _, keys, counts, _ = keyfile.decode(f.getvalue())
        return keys, counts

    # ---- lookups (include/brx.h "lookups in a count list", countops.directory / lookup) ----
    def prepare_lookup(self, log2_buckets: Optional[int] = None) -> None:
        """build the lookup directory: 2^d + 1 offsets into the sorted keys, d = log2_buckets or countops.auto_log2_buckets(n,
        k) (brx_counts_lookup_prepare).  The d already in place: nothing is done; another d: rebuilt"""
        d = -1 if log2_buckets is None else int(log2_buckets)
        if d < -1:
            raise ValueError(f"log2_buckets={log2_buckets}")
        _lib.check(_lib.lib().brx_counts_lookup_prepare(self._h, d))

    def lookup_info(self) -> dict:
        v = (C.c_uint64 * 4)()
        _lib.check(_lib.lib().brx_counts_lookup_info(self._h, v))
        return {"ready": bool(v[0]), "log2_buckets": int(v[1]), "directory_bytes": int(v[2]), "fullest_bucket": int(v[3])}

    @property
    def lookup_ready(self) -> bool:
        """whether the abundance calls and get_counts would answer"""
        return self.lookup_info()["ready"]

    def lookup_directory(self) -> np.ndarray:
        """the directory as uint64[2^d + 1] on the host (a copy, for checks): countops.directory(keys, k, d)"""
        p, n = C.c_void_p(), C.c_uint64(0)
        _lib.check(_lib.lib().brx_counts_lookup_directory(self._h, C.byref(p), C.byref(n)))
        out = np.zeros(int(n.value), dtype=np.uint64)
        _lib.copy_to_host(p.value, out)
        return out

    def drop_lookup(self) -> None:
        """free the directory; the lookups refuse again"""
        _lib.check(_lib.lib().brx_counts_lookup_drop(self._h))

    def abundance_batch(self, bases: np.ndarray, offsets: np.ndarray, abundance: int = 0, profile: bool = True,
                        hist: bool = False):
        """Counter.abundance_batch from the list (brx_counts_abundance_batch): after prepare_lookup()"""
        from . import abundance as ab
        _check_u8(abundance, "abundance")
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        pr = np.zeros(bases.size, dtype=np.uint8) if profile else None
        hi = np.zeros((n, 256), dtype=np.uint32) if hist else None
        st = np.zeros(n, dtype=ab.STATS_DTYPE)
        ptr = lambda a: a.ctypes.data if a is not None else None
        _lib.check(_lib.lib().brx_counts_abundance_batch(self._h, bases.ctypes.data, offsets.ctypes.data, n, abundance,
                                                         ptr(pr), ptr(hi), ptr(st)))
        return pr, hi, st

    def abundance_batch_device(self, d_bases: int, d_offsets: int, n_reads: int, total_bases: int, abundance: int = 0,
                               d_profile: Optional[int] = None, d_hist: Optional[int] = None, d_stats: Optional[int] = None,
                               stream: Optional[int] = None) -> None:
        _check_u8(abundance, "abundance")
        _lib.check(_lib.lib().brx_counts_abundance_batch_device(self._h, d_bases, d_offsets, n_reads, total_bases, abundance,
                                                                d_profile, d_hist, d_stats, stream))

    def abundance_reads(self, reads: Sequence[bytes], abundance: int = 0):
        """(list of per-read uint8 arrays of length kmers, stats array) of `reads`"""
        from . import abundance as ab
        bases, offs = pack_reads(reads)
        pr, _, st = self.abundance_batch(bases, offs, abundance)
        return ab.unpack_profile(pr, offs, self.k), st

    def get_counts(self, kmers: Sequence[int]) -> np.ndarray:
        """uint8 count of every forward k-mer (of its canonical form), 0 where it is not listed: Counter.get_counts' twin"""
        km = np.ascontiguousarray(np.asarray(kmers, dtype=np.uint64))
        out = np.zeros(km.size, dtype=np.uint8)
        _lib.check(_lib.lib().brx_counts_get_counts(self._h, km.ctypes.data, km.size, out.ctypes.data))
        return out


class Counter:
    """pcon::counter::Counter<u8> as used by `br fasta` (src/main.rs:73-78).  Odd k up to 31: COUNT_AUTO takes the dense
    u8 table below 15, the partitioned counter for 15..21 and the counting hash table (COUNT_TABLE) for 23..31."""

    def __init__(self, k: int, device: int = 0, strategy: int = _lib.COUNT_AUTO):
        self._h = C.c_void_p()
        self.k = k
        self.device = device
        _lib.check(_lib.lib().brx_set_count_begin(k, device, strategy, C.byref(self._h)))

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                _lib.lib().brx_counter_free(self._h)
                self._h = C.c_void_p(None)
        except Exception:
            pass

    def add_reads(self, reads: Sequence[bytes]) -> None:
        bases, offs = pack_reads(reads)
        self.add_batch(bases, offs)

    def add_batch(self, bases: np.ndarray, offsets: np.ndarray) -> None:
        _lib.check(_lib.lib().brx_set_count_add_batch(self._h, bases.ctypes.data, offsets.ctypes.data,
                                                      offsets.size - 1))

    def count_fasta(self, f) -> dict:
        """Counter::count_fasta(reader, record_buffer) (src/main.rs:73-78) through the native host pipeline
        (brx_count_fasta_fd): every record of the FASTA stream `f` (a binary file object)."""
        from . import hostio
        st = (C.c_uint64 * 8)()
        with hostio.input_fd(f) as fd:
            _lib.check(_lib.lib().brx_count_fasta_fd(self._h, fd, 0, st))
        return {"records": int(st[0]), "bases_in": int(st[1]), "batches": int(st[3]), "ns_parse": int(st[4]),
                "ns_gpu": int(st[5]), "ns_wall": int(st[7])}

    def count_reads(self, f, fmt="fastq", min_quality: int = 0, acgt_only: bool = True, max_batch_records: int = 0) -> dict:
        """count the records of a FASTQ or FASTA stream (binary file object) through the native host pipeline
        (brx_count_reads_fd).  Only the k-mers none of whose bases is untrusted are counted: a base is untrusted when it is
        not ACGTacgt (acgt_only) or its quality lies below min_quality (Phred+33; FASTQ only) -- br_amd/trust.py.  With
        min_quality 0 and acgt_only off this is count_fasta's rule: every k-mer, every byte a base.  Returns count_fasta's
        dict plus "trust": bases, non_acgt, low_quality, pieces, kept_bases, kmers summed over the stream"""
        from . import hostio
        st, tot = (C.c_uint64 * 8)(), (C.c_uint64 * 8)()
        opts = _read_opts(min_quality, acgt_only)
        fmt_id = _read_format(fmt)
        with hostio.input_fd(f) as fd:
            _lib.check(_lib.lib().brx_count_reads_fd(self._h, fd, fmt_id, max_batch_records, opts, st, tot))
        return _stream_stats(st, tot)

    def add_batch_device(self, d_bases: int, d_offsets: int, n_reads: int, total_bases: int,
                         stream: Optional[int] = None) -> None:
        _lib.check(_lib.lib().brx_set_count_add_batch_device(self._h, d_bases, d_offsets, n_reads, total_bases,
                                                             stream))

    def clamp(self, cap: int, stream: Optional[int] = None) -> None:
        _lib.check(_lib.lib().brx_counter_clamp(self._h, cap, stream))

    def device_counts(self) -> Tuple[int, int]:
        p, n = C.c_void_p(), C.c_uint64(0)
        _lib.check(_lib.lib().brx_counter_device_counts(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def load_counts(self, first: int, counts: bytes) -> None:
        """overwrite counters [first, first + len(counts)) of a dense counter (`br count`: a table counted elsewhere)"""
        _lib.check(_lib.lib().brx_counter_load_counts(self._h, first, bytes(counts), len(counts)))

    # ---- key files (include/brx.h "key files", br_amd/keyfile.py) -----------------------------------------------------
    def save(self, f, min_count: int = 1) -> dict:
        """write the k-mers counted at least min_count times, with min(255, count), as a key file to the binary file object
        `f` (brx_counter_save_fd).  A table counter saves at any time; a partitioned one saves its count view, so call
        prepare_lookup() first (and again after anything that drops the view) -- nothing prepares it implicitly.  Dense
        counters are refused.  The counter, and a partitioned counter's view, are left as they were"""
        from . import hostio
        _check_u8(min_count, "min_count")
        st = (C.c_uint64 * 8)()
        with hostio.output_fd(f) as fd:
            _lib.check(_lib.lib().brx_counter_save_fd(self._h, min_count, fd, st))
        return _keyfile_stats(st)

    def load(self, f) -> dict:
        """ADD the counts of a count file (binary file object) to this counter: counts of one k-mer sum and saturate at 255
        (brx_counter_load_fd).  A file saved with min_count > 1 loads into an empty counter only and floors it"""
        from . import hostio
        st = (C.c_uint64 * 8)()
        with hostio.input_fd(f) as fd:
            _lib.check(_lib.lib().brx_counter_load_fd(self._h, fd, st))
        return _keyfile_stats(st)

    @classmethod
    def from_keyfile(cls, f, device: int = 0) -> "Counter":
        """a table counter holding the counts of a count file; k from the header.  `f` must be able to hand the 32 header
        bytes back (seekable or with peek(), like everything cli.open_input returns)"""
        from . import keyfile
        if hasattr(f, "peek") and len(f.peek(keyfile.HEADER_BYTES)) >= keyfile.HEADER_BYTES:
            head = f.peek(keyfile.HEADER_BYTES)[:keyfile.HEADER_BYTES]
        else:
            at = f.tell()
            head = f.read(keyfile.HEADER_BYTES)
            f.seek(at)
        try:
            k = keyfile.peek(io.BytesIO(head))["k"]
        except ValueError as e:
            raise _lib.BrxError(_lib.BRX_ERR_FORMAT, str(e))
        cnt = cls(k, device, _lib.COUNT_TABLE)
        cnt.load(f)
        return cnt

    @property
    def floor(self) -> int:
        """f > 1 after a count file saved with min_count f was loaded: k-mers seen fewer times are unknown, finish() needs
        a threshold of at least f - 1 and nothing more can be added until reset(); 1 otherwise"""
        v = C.c_uint8(0)
        _lib.check(_lib.lib().brx_counter_floor(self._h, C.byref(v)))
        return int(v.value)

    @classmethod
    def from_count_stream(cls, f, device: int = 0, chunk: int = 64 << 20) -> "Counter":
        """pcon::counter::Counter::<u8>::from_stream (src/main.rs:59-61): a count table written by `pcon count`.
        Layout as restated from pcon's published serializer -- one byte k, then the 2^(2k-1) u8 counters of the
        canonical hashes in order (the reference builds pcon with `count_u8`, Cargo.toml:23); the reference holds no
        count-file fixture, so the layout is UNPINNED.  A short stream is an error, like read_exact's."""
        head = f.read(1)
        if len(head) != 1:
            raise _lib.BrxError(-5, "count stream: empty")
        k = head[0]
        if not 1 <= k <= 19:
            raise _lib.BrxError(-1, f"count stream: k={k} (a dense u8 table fits one GPU for k <= 19)")
        cnt = cls(k, device, _lib.COUNT_DENSE)
        total, pos = 1 << (2 * k - 1), 0
        while pos < total:
            buf = f.read(min(chunk, total - pos))
            if not buf:
                raise _lib.BrxError(-5, f"count stream: ends after {pos} of {total} counters")
            cnt.load_counts(pos, buf)
            pos += len(buf)
        return cnt

    def spectrum(self, stream: Optional[int] = None) -> np.ndarray:
        """pcon::spectrum::Spectrum::from_count: uint64[256] histogram of the counts (255 = 255 or more).
        Any strategy; the counter is left as it was, so `finish(threshold)` can follow."""
        h = np.zeros(256, dtype=np.uint64)
        _lib.check(_lib.lib().brx_counter_spectrum(self._h, h.ctypes.data_as(C.POINTER(C.c_uint64)), stream))
        return h

    def l1_view(self) -> Tuple[int, int, int, int]:
        """(d_keys, d_l1off, n_buckets, n_keys) of the single counted batch (partitioned strategy)."""
        pk, po, nb, nk = C.c_void_p(), C.c_void_p(), C.c_uint32(0), C.c_uint64(0)
        _lib.check(_lib.lib().brx_counter_l1_view(self._h, C.byref(pk), C.byref(po), C.byref(nb), C.byref(nk)))
        return pk.value or 0, po.value or 0, nb.value, nk.value

    def add_partitioned_device(self, d_keys: int, d_l1off: int, n_keys: int) -> None:
        _lib.check(_lib.lib().brx_counter_add_partitioned_device(self._h, d_keys, d_l1off, n_keys))

    def table_info(self, stream: Optional[int] = None) -> dict:
        """the hash table of a COUNT_TABLE counter: log2 of its lines, minimizer length, distinct k-mers, peak bytes held"""
        v = (C.c_uint64 * 4)()
        _lib.check(_lib.lib().brx_counter_table_info(self._h, v, stream))
        return {"log2_lines": int(v[0]), "m": int(v[1]), "keys": int(v[2]), "peak_bytes": int(v[3])}

    def merge_state(self) -> Tuple[int, int]:
        """(world, rank) a table counter was merged over by AbiExchange.merge_table; world 0: not merged.  A merged counter
        holds the k-mers its rank owns with the counts of the whole job, and takes no more reads until `reset()`"""
        w, r = C.c_int(0), C.c_int(0)
        _lib.check(_lib.lib().brx_counter_merge_state(self._h, C.byref(w), C.byref(r)))
        return w.value, r.value

    def reset(self, stream: Optional[int] = None) -> None:
        _lib.check(_lib.lib().brx_counter_reset(self._h, stream))

    # ---- sliced counting (include/brx.h "sliced counting", br_amd/parts.py) -------------------------------------------
    def set_slice(self, part: int, parts: int) -> None:
        """count only the k-mers `part` of `parts` owns (dist.table_owner of the k-mer's hash) from here on: a table counter
        that holds nothing, new or reset since (brx_counter_set_slice).  parts 1 .. 4096; parts == 1 makes it an ordinary
        counter again.  reset() keeps the slice; everything that reads the counter describes the slice"""
        if not (0 <= int(part) < 2 ** 32 and 0 <= int(parts) < 2 ** 32):
            raise _lib.BrxError(_lib.BRX_ERR_ARG, f"set_slice: part {part} of {parts}")
        _lib.check(_lib.lib().brx_counter_set_slice(self._h, int(part), int(parts)))

    @property
    def slice(self) -> Tuple[int, int]:
        """(part, parts); (0, 1) for a counter that is not sliced"""
        p, n = C.c_uint32(0), C.c_uint32(1)
        _lib.check(_lib.lib().brx_counter_slice(self._h, C.byref(p), C.byref(n)))
        return int(p.value), int(n.value)

    def slice_stats(self, stream: Optional[int] = None) -> dict:
        """what the sliced count kernel did since the last reset (all 0 for an unsliced counter): valid k-mers seen, k-mers
        of the part (walked into the table), wave trips into the walk, waves launched.  The part's k-mers are compacted
        before the walk, so trips <= walked // 64 + waves"""
        v = (C.c_uint64 * 4)()
        _lib.check(_lib.lib().brx_counter_slice_stats(self._h, v, stream))
        return {"seen": int(v[0]), "walked": int(v[1]), "trips": int(v[2]), "waves": int(v[3])}

    # ---- abundance (include/brx.h "abundance", br_amd/abundance.py: no counterpart in the reference) ----
    def abundance_batch(self, bases: np.ndarray, offsets: np.ndarray, abundance: int = 0, profile: bool = True,
                        hist: bool = False):
        """(profile uint8[total] | None, hist uint32[n, 256] | None, stats abundance.STATS_DTYPE[n]) of a bases / offsets
        batch: the count of the k-mer that starts at every base, on the GPU (brx_counter_abundance_batch).  Dense and
        table counters, and a partitioned one after prepare_lookup(); the counter is left as it was."""
        from . import abundance as ab
        _check_u8(abundance, "abundance")
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        pr = np.zeros(bases.size, dtype=np.uint8) if profile else None
        hi = np.zeros((n, 256), dtype=np.uint32) if hist else None
        st = np.zeros(n, dtype=ab.STATS_DTYPE)
        ptr = lambda a: a.ctypes.data if a is not None else None
        _lib.check(_lib.lib().brx_counter_abundance_batch(self._h, bases.ctypes.data, offsets.ctypes.data, n, abundance,
                                                          ptr(pr), ptr(hi), ptr(st)))
        return pr, hi, st

    def abundance_batch_device(self, d_bases: int, d_offsets: int, n_reads: int, total_bases: int, abundance: int = 0,
                               d_profile: Optional[int] = None, d_hist: Optional[int] = None, d_stats: Optional[int] = None,
                               stream: Optional[int] = None) -> None:
        _check_u8(abundance, "abundance")
        _lib.check(_lib.lib().brx_counter_abundance_batch_device(self._h, d_bases, d_offsets, n_reads, total_bases, abundance,
                                                                 d_profile, d_hist, d_stats, stream))

    def abundance_reads(self, reads: Sequence[bytes], abundance: int = 0):
        """(list of per-read uint8 arrays of length kmers, stats array) of `reads`"""
        from . import abundance as ab
        bases, offs = pack_reads(reads)
        pr, _, st = self.abundance_batch(bases, offs, abundance)
        return ab.unpack_profile(pr, offs, self.k), st

    def get_counts(self, kmers: Sequence[int]) -> np.ndarray:
        """uint8 count of every forward k-mer (of its canonical form): Pcon.get_many's twin on a counter"""
        km = np.ascontiguousarray(np.asarray(kmers, dtype=np.uint64))
        out = np.zeros(km.size, dtype=np.uint8)
        _lib.check(_lib.lib().brx_counter_get_counts(self._h, km.ctypes.data, km.size, out.ctypes.data))
        return out

    def prepare_lookup(self, stream: Optional[int] = None) -> None:
        """build the count view of a partitioned counter (brx_counter_lookup_prepare), so that the abundance calls and
        get_counts answer from it; nothing to do for a dense or a table counter.  The view holds until the counter is
        next added to, finished, reset or asked for its spectrum: prepare after those"""
        _lib.check(_lib.lib().brx_counter_lookup_prepare(self._h, stream))

    @property
    def lookup_ready(self) -> bool:
        """whether the abundance calls and get_counts would answer (always for dense and table counters)"""
        st = C.c_int(0)
        _lib.check(_lib.lib().brx_counter_lookup_state(self._h, C.byref(st)))
        return bool(st.value)

    def drop_lookup(self) -> None:
        """free the count view of a partitioned counter (harmless for the others)"""
        _lib.check(_lib.lib().brx_counter_lookup_drop(self._h))

    def finish_into(self, abundance: int, dst: "Pcon", stream: Optional[int] = None) -> None:
        _check_u8(abundance, "abundance")
        _lib.check(_lib.lib().brx_set_count_finish_into(self._h, abundance, stream, dst._h))

    def finish(self, abundance: int, stream: Optional[int] = None) -> Pcon:
        """Solid::from_count(k, counts, abundance): solid iff count > abundance."""
        _check_u8(abundance, "abundance")
        h = C.c_void_p()
        _lib.check(_lib.lib().brx_set_count_finish(self._h, abundance, stream, C.byref(h)))
        return Pcon(h.value, self.device)
