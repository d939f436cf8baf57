"""The strand of a read, stated in numpy / bytes: the definitions of include/brx.h (BRX_PASS_*) in their readable form.

The reference scans every record twice and, between the scans, reverses the bytes without complementing them
(src/lib.rs:48-55,111).  A read stored back to front is a sequence of neither strand, so that second scan meets almost
no solid k-mer.  The `revcomp` mode runs it on the reverse complement instead -- the same molecule read along the other
strand, whose k-mers the canonical set knows as well as the first strand's:

  rc(s)     the bytes of s in reverse order with A<->T, C<->G, a<->t, c<->g exchanged; every other byte stays
  none      fwd(s)                      one scan (-s)
  reverse   rev(fwd(rev(fwd(s))))       the reference's default
  revcomp   rc(fwd(rc(fwd(s))))         fwd = every method of the chain in order, each one Corrector::correct
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np

SECOND_PASS = {"none", "reverse", "revcomp"}
PASS_IDS = {"none": 0, "reverse": 1, "revcomp": 2}  # BRX_PASS_NONE / REVERSE / REVCOMP

_COMPLEMENT = np.arange(256, dtype=np.uint8)
_COMPLEMENT[np.frombuffer(b"ACGTacgt", dtype=np.uint8)] = np.frombuffer(b"TGCAtgca", dtype=np.uint8)
_COMPLEMENT.setflags(write=False)


def revcomp(seq):
    """rc(seq): bytes for bytes-like input, a uint8 array for an array.  rc(rc(s)) == s for every byte string."""
    if isinstance(seq, np.ndarray):
        return _COMPLEMENT[np.ascontiguousarray(seq, dtype=np.uint8)[::-1]]
    return _COMPLEMENT[np.frombuffer(bytes(seq), dtype=np.uint8)[::-1]].tobytes()


def resolve_second_pass(second_pass: Optional[str], two_side: Optional[bool]) -> str:
    """The mode named by the two ways of asking for it.  second_pass None keeps two_side's meaning (True = the -s flag
    = "none", False / None = "reverse"); two_side True beside any other mode is a contradiction."""
    if second_pass is None:
        return "none" if two_side else "reverse"
    if second_pass not in SECOND_PASS:
        raise ValueError(f"second_pass={second_pass!r}: one of {sorted(SECOND_PASS)}")
    if two_side and second_pass != "none":
        raise ValueError(f"two_side=True (one scan) contradicts second_pass={second_pass!r}")
    return second_pass


def revcomp_reads(reads: Sequence[bytes], device: int = 0) -> List[bytes]:
    """rc() of every read, computed by the GPU (brx_revcomp_batch: the kernel the revcomp mode runs between its scans)"""
    from . import _lib
    from .set import pack_reads
    reads = [bytes(r) for r in reads]
    bases, offs = pack_reads(reads)
    out = np.empty(max(bases.size, 1), dtype=np.uint8)
    _lib.check(_lib.lib().brx_revcomp_batch(bases.ctypes.data, offs.ctypes.data, len(reads), out.ctypes.data, device))
    return [out[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(len(reads))]
