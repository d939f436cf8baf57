"""K-mer text: a count list as `KMER<TAB>COUNT` lines, the form `jellyfish dump -c -t` and `kmc_tools transform ... dump`
write -- stated in numpy.

One line per entry: the k-mer as k upper-case letters, one TAB, the count in decimal without leading zeros, "\\n".  The lines
are in ascending KEY order -- the order of the list (key = canonical k-mer >> 1 with A C T G = 0 1 2 3), NOT alphabetical
order: a tool that wants its input sorted by k-mer sorts it itself.  A count byte of 255 prints as 255 and means "255 or
more", as everywhere.

The k-mer printed for key x is one of two strands.  With c = (x << 1) | (popcount(x) & 1), the canonical (even-popcount)
k-mer of br_amd/csrc/brx_kmer.hpp:
    strand="canonical"   c itself
    strand="lex"         the alphabetically smaller of c and its reverse complement, A < C < G < T (the default: the member
                         Jellyfish -C and KMC print).  The 2-bit codes order A C T G, so the two are compared after mapping
                         every code v -> v ^ (v >> 1); k is odd, so they never tie.

Reading (`parse`, `parse_lines`):
    lines end with "\\n"; one "\\r" at the end of a line is dropped; a last line without "\\n" counts; empty lines are skipped
    a line is exactly k bytes of ACGTacgt, one or more of TAB / space, one or more decimal digits, and nothing else
    k=None takes k from the number of bytes before the first TAB / space / end of the first non-empty line (odd, 5..31)
    the value of the digits saturates at 255 (any number of digits, leading zeros allowed); a value of 0 is an error
    either strand may be listed: the key is canonical(k-mer) >> 1
    equal keys -- one k-mer twice, or both strands apart as a non-canonical dump lists them -- ADD, saturating at 255
    after that a count below `floor` is an error; the result is sorted by key
Errors are ValueError("line N: cause"), N from 1 with the empty lines counted; CAUSES lists the causes of a malformed line
in the order a line is checked.

The format follows the public descriptions of the two tools' dumps; neither tool was at hand, so it is pinned by this
statement alone.  This module is the expected value of the GPU path (br_amd/csrc/brx_kmertext.hip) and needs no GPU and no
library, except for its command (python -m br_amd.kmertext dump | import), which runs on the GPU."""
from __future__ import annotations

import sys
from typing import Optional, Tuple

import numpy as np

STRANDS = {"lex": 0, "canonical": 1}
CAUSE_BASE, CAUSE_SHORT, CAUSE_LONG, CAUSE_NOCOUNT, CAUSE_DIGIT, CAUSE_ZERO = 1, 2, 3, 4, 5, 6
_M5 = np.uint64(0x5555555555555555)
_LETTERS = np.frombuffer(b"ACTG", dtype=np.uint8)
_BASES = frozenset(b"ACGTacgt")


def cause_text(cause: int, col: int, k: int) -> str:
    """the words for a malformed line, the same in this module and in the library's message"""
    return {CAUSE_BASE: f"column {col} is no base (ACGT, either case)",
            CAUSE_SHORT: f"a k-mer of {col} bases is shorter than k={k}",
            CAUSE_LONG: f"a k-mer of {col} bases is longer than k={k}",
            CAUSE_NOCOUNT: "no count after the k-mer",
            CAUSE_DIGIT: f"column {col} is no digit",
            CAUSE_ZERO: "a count of 0"}[cause]


def strand_id(strand) -> int:
    if strand not in STRANDS:
        raise ValueError(f"strand={strand!r} (one of {sorted(STRANDS)})")
    return STRANDS[strand]


def _check_k(k: int) -> None:
    if not (5 <= k <= 31 and k & 1):
        raise ValueError(f"k-mer text: k={k} (odd k from 5 to 31)")


def _popcount(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint64).copy()
    n = np.zeros(x.shape, dtype=np.uint64)
    for _ in range(64):
        n += x & np.uint64(1)
        x >>= np.uint64(1)
    return n


def _revcomp(c: np.ndarray, k: int) -> np.ndarray:
    """reverse complement of 2-bit k-mers, first base most significant (brx_kmer.hpp revcomp)"""
    x = c ^ np.uint64(0xAAAAAAAAAAAAAAAA)
    r = np.zeros(c.shape, dtype=np.uint64)
    for _ in range(k):
        r = (r << np.uint64(2)) | (x & np.uint64(3))
        x = x >> np.uint64(2)
    return r


def _ascii_order(c: np.ndarray) -> np.ndarray:
    return c ^ ((c >> np.uint64(1)) & _M5)


def kmers_of_keys(k: int, keys, strand="lex") -> np.ndarray:
    """the 2-bit k-mer (uint64, first base most significant) printed for each key"""
    _check_k(k)
    x = np.ascontiguousarray(keys, dtype=np.uint64)
    c = (x << np.uint64(1)) | (_popcount(x) & np.uint64(1))
    if strand_id(strand) == STRANDS["canonical"]:
        return c
    r = _revcomp(c, k)
    return np.where(_ascii_order(r) < _ascii_order(c), r, c)


def keys_of_kmers(k: int, kmers) -> np.ndarray:
    """canonical(k-mer) >> 1 of 2-bit k-mers of either strand"""
    f = np.ascontiguousarray(kmers, dtype=np.uint64)
    return np.where((_popcount(f) & np.uint64(1)).astype(bool), _revcomp(f, k), f) >> np.uint64(1)


def line_lengths(k: int, counts) -> np.ndarray:
    """bytes of each entry's line: k + 3 + (count >= 10) + (count >= 100)"""
    c = np.ascontiguousarray(counts, dtype=np.uint8).astype(np.int64)
    return k + 3 + (c >= 10) + (c >= 100)


def format_lines(k: int, keys, counts, strand="lex") -> bytes:
    """the text of the entries (keys, counts) in the order given -- a list's order is ascending keys"""
    kmers = kmers_of_keys(k, keys, strand)
    c = np.ascontiguousarray(counts, dtype=np.uint8).astype(np.int64)
    n = kmers.size
    if c.size != n:
        raise ValueError("k-mer text: one count per key")
    m = np.zeros((n, k + 5), dtype=np.uint8)
    shifts = (2 * np.arange(k - 1, -1, -1)).astype(np.uint64)
    m[:, :k] = _LETTERS[((kmers[:, None] >> shifts[None, :]) & np.uint64(3)).astype(np.int64)]
    m[:, k] = 9
    m[:, k + 1] = 48 + c // 100
    m[:, k + 2] = 48 + (c // 10) % 10
    m[:, k + 3] = 48 + c % 10
    m[:, k + 4] = 10
    keep = np.ones((n, k + 5), dtype=bool)
    keep[:, k + 1] = c >= 100
    keep[:, k + 2] = c >= 10
    return m[keep].tobytes()


def _lines(data: bytes):
    """(number from 1, the line without its end) of every non-empty line"""
    parts = bytes(data).split(b"\n")
    if parts and parts[-1] == b"":
        parts.pop()
    for no, line in enumerate(parts, 1):
        if line.endswith(b"\r"):
            line = line[:-1]
        if line:
            yield no, line


def _field(line: bytes) -> int:
    """bytes before the first TAB / space"""
    n = len(line)
    a, b = line.find(b"\t"), line.find(b" ")
    return min(n if a < 0 else a, n if b < 0 else b)


def check_line(line: bytes, k: int) -> Tuple[int, int, bytes, int]:
    """(cause, col, k-mer, value) of one non-empty line without its end: cause 0 and the k-mer's k bytes with min(255,
    value), or a cause of CAUSES with its column / number of bases (brx_kmertext.hpp text_parse_line is the same walk)"""
    f = _field(line)
    for i in range(f):
        if line[i] not in _BASES:
            return CAUSE_BASE, i + 1, b"", 0
    if f != k:
        return (CAUSE_SHORT if f < k else CAUSE_LONG), f, b"", 0
    rest = line[f:].lstrip(b"\t ")
    if not rest:
        return CAUSE_NOCOUNT, 0, b"", 0
    if not rest.isdigit() or not rest.isascii():
        at = len(line) - len(rest)
        for i, ch in enumerate(rest):
            if not 48 <= ch <= 57:
                return CAUSE_DIGIT, at + i + 1, b"", 0
    digits = rest.lstrip(b"0")
    v = 255 if len(digits) > 3 else min(255, int(digits or b"0"))
    if v == 0:
        return CAUSE_ZERO, 0, b"", 0
    return 0, 0, line[:k], v


def parse_lines(data: bytes, k: Optional[int] = None) -> Tuple[int, np.ndarray, np.ndarray, np.ndarray]:
    """(k, keys, counts, line numbers): one (canonical key, min(255, value)) pair per non-empty line, in line order, neither
    sorted nor summed -- what the raw device entry returns; the numbers (from 1) are those of the pairs' lines"""
    if k is not None:
        _check_k(k)
    kmers, values, numbers = [], [], []
    for no, line in _lines(data):
        if k is None:
            k = _field(line)
            if not (5 <= k <= 31 and k & 1):
                raise ValueError(f"line {no}: a k-mer of {k} bases gives no k (odd, 5 to 31)")
        cause, col, kmer, v = check_line(line, k)
        if cause:
            raise ValueError(f"line {no}: {cause_text(cause, col, k)}")
        kmers.append(kmer)
        values.append(v)
        numbers.append(no)
    if k is None:
        raise ValueError("k-mer text: an empty text tells no k")
    n = len(kmers)
    codes = (np.frombuffer(b"".join(kmers), dtype=np.uint8).reshape(n, k) >> 1) & 3
    f = np.zeros(n, dtype=np.uint64)
    for i in range(k):
        f = (f << np.uint64(2)) | codes[:, i].astype(np.uint64)
    return k, keys_of_kmers(k, f), np.asarray(values, dtype=np.uint8), np.asarray(numbers, dtype=np.int64)


def sum_runs(keys: np.ndarray, counts: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(distinct keys ascending, the counts of each added up to 255)"""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    uniq, inverse = np.unique(keys, return_inverse=True)
    total = np.bincount(inverse, weights=np.asarray(counts, dtype=np.float64), minlength=uniq.size) if keys.size else np.zeros(0)
    return uniq, np.minimum(total, 255).astype(np.uint8)


def parse(data: bytes, k: Optional[int] = None, floor: int = 1) -> Tuple[int, np.ndarray, np.ndarray]:
    """(k, keys ascending, counts) of a k-mer text: the arrays of the count list it states"""
    if not 1 <= floor <= 255:
        raise ValueError(f"k-mer text: floor={floor} (1 to 255)")
    k, keys, counts, numbers = parse_lines(data, k)
    uniq, total = sum_runs(keys, counts)
    low = total < floor
    if low.any():  # the first line, in the order of the text, whose k-mer stays below the floor
        at = int(np.flatnonzero(low[np.searchsorted(uniq, keys)])[0])
        raise ValueError(f"line {int(numbers[at])}: a count of {int(total[np.searchsorted(uniq, keys[at])])} below the floor {floor}")
    return k, uniq, total


# ---- python -m br_amd.kmertext -------------------------------------------------------------------------------------------
def main(argv=None) -> int:
    import argparse
    p = argparse.ArgumentParser(prog="python -m br_amd.kmertext", description="count files to and from k-mer text "
                                "(KMER<TAB>COUNT lines, as jellyfish dump -c -t and kmc_tools dump write them), on the GPU")
    sub = p.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("dump", help="a count file as text, in the order of its keys")
    d.add_argument("counts", help="count file (.keys; gz / bz2 / xz are sniffed)")
    d.add_argument("-o", "--output", default="-", help="text out, default or - : stdout")
    d.add_argument("--min-count", type=int, default=1, help="drop the entries counted fewer times")
    d.add_argument("--strand", choices=sorted(STRANDS), default="lex", help="the strand printed: the alphabetically smaller "
                   "one (lex, what Jellyfish -C and KMC print) or the list's own canonical one")
    i = sub.add_parser("import", help="a k-mer text as a count file")
    i.add_argument("text", help="KMER<TAB>COUNT lines (gz / bz2 / xz are sniffed)")
    i.add_argument("-o", "--output", required=True, help="count file out")
    i.add_argument("-k", type=int, default=None, help="k, default: from the first line")
    i.add_argument("--floor", type=int, default=1, help="the smallest count the text kept: becomes the file's floor")
    a = p.parse_args(argv)
    from . import cli
    from .set import CountList
    if a.cmd == "dump":
        with cli.open_input(a.counts) as f:
            lst = CountList.from_keyfile(f)
        out = sys.stdout.buffer if a.output == "-" else open(a.output, "wb")
        try:
            st = lst.dump_text(out, a.min_count, a.strand)
            out.flush()
        finally:
            if out is not sys.stdout.buffer:
                out.close()
        print(f"k-mer text: {st['entries']} entries, {st['bytes']} bytes", file=sys.stderr)
    else:
        with cli.open_input(a.text) as f:
            lst = CountList.from_text(f, a.k, a.floor)
        with open(a.output, "wb") as out:
            lst.save(out)
        print(f"k-mer text: {lst.n} entries at k={lst.k}, floor {lst.floor}", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
