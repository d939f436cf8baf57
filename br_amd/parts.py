"""Counting in parts: a job larger than one counting table, counted slice by slice (include/brx.h "sliced counting").

A table counter sliced as (part, parts) counts only the k-mers with `dist.table_owner(hash, parts) == part` -- the rule of
the multi-GPU merge, here applied to sweeps in time instead of ranks in space.  `parts` sweeps over the same files count
every k-mer exactly once, each sweep in a table sized for its share; a sweep leaves a count list (9 bytes an entry, floored
at `min_count`), the lists have disjoint keys, and their maximum is their union: the list one table would have given.

`slice_of`, `join`, `join_floor` and `table_log2_lines` state the rules in numpy and need no GPU and no library -- they are
the expected values of the GPU path, as countops.py is for count lists.  `count_in_parts` is the driver."""
from __future__ import annotations

import time
from functools import reduce
from typing import Sequence, Tuple

import numpy as np

from . import countops, dist

MAX_PARTS = 4096                              # brx_counter_set_slice
TAB_MIN_LOG_LINES, TAB_MAX_LOG_LINES = 12, 30  # brx_counttable.hip


def check_parts(parts: int) -> int:
    if not 1 <= int(parts) <= MAX_PARTS:
        raise ValueError(f"parts={parts}: 1 .. {MAX_PARTS}")
    return int(parts)


def slice_of(keys, counts, part: int, parts: int) -> Tuple[np.ndarray, np.ndarray]:
    """the entries of the list (keys, counts) that `part` of `parts` owns, in the list's order"""
    parts = check_parts(parts)
    if not 0 <= int(part) < parts:
        raise ValueError(f"part={part} of {parts}")
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    counts = np.ascontiguousarray(counts, dtype=np.uint8)
    mine = dist.table_owner(keys, parts) == np.uint32(part)
    return keys[mine], counts[mine]


def join(lists: Sequence[Tuple[np.ndarray, np.ndarray]]) -> Tuple[np.ndarray, np.ndarray]:
    """the one sorted list of lists with disjoint keys; ValueError when two of them share a key (slices never do)"""
    if not lists:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint8)
    keys = np.concatenate([np.ascontiguousarray(k, dtype=np.uint64) for k, _ in lists])
    counts = np.concatenate([np.ascontiguousarray(c, dtype=np.uint8) for _, c in lists])
    if keys.shape != counts.shape:
        raise ValueError("join: keys and counts are arrays of one length")
    order = np.argsort(keys, kind="stable")
    keys, counts = keys[order], counts[order]
    if keys.size > 1 and not (keys[1:] > keys[:-1]).all():
        raise ValueError("join: the lists share the key %d" % int(keys[1:][keys[1:] == keys[:-1]][0]))
    return keys, counts


def join_floor(floors: Sequence[int]) -> int:
    """the floor of the joined list: the lists are joined with `max`, whose floor rule (countops.result_floor) takes
    floored operands"""
    return reduce(lambda a, b: countops.result_floor("max", a, b), [int(f) for f in floors], 1)


def table_log2_lines(need: int) -> int:
    """log2 of the lines of the counting table made for `need` keys: the smallest with 7 * 2^L >= 3 * need (at most about
    half full, 7 slots a line), at least 12, at most 30"""
    log = TAB_MIN_LOG_LINES
    while log < TAB_MAX_LOG_LINES and (7 << log) < 3 * int(need):
        log += 1
    return log


def count_in_parts(paths: Sequence[str], k: int, parts: int, device: int = 0, min_count: int = 1, fmt: str = "fasta",
                   min_quality: int = 0, acgt_only: bool = False):
    """(CountList, spectrum uint64[256], stats): the k-mers of the files counted in `parts` sweeps with one table counter.
    Sweep p resets the counter, slices it as (p, parts), counts every path (reopened, compression sniffed as the command
    line does), adds the counter's spectrum to the job's and lists the counter from `min_count` up; the lists are joined
    with CountList.maximum in balanced order -- a stack that merges two lists of equal rank, so an entry is merged about
    log2(parts) times.  The spectrum comes from the counters, so it is complete below min_count too; bin 0 is 2^(2k-1)
    minus the rest.  fmt "fasta" counts every k-mer as `br fasta` does (acgt_only: as --skip-non-acgt), "fastq" as `br
    fastq` with the quality floor.  stats: {"parts": [per sweep: keys, listed, log2_lines, peak_bytes, slice_stats,
    ns_count, ns_list, ns_join], "ns_join_tail", "trust": the first sweep's totals or None, "list_bytes"}"""
    from . import _lib, trust
    from .cli import open_input
    from .set import Counter, CountList
    parts = check_parts(parts)
    if fmt not in ("fasta", "fastq"):
        raise ValueError(f"fmt={fmt!r}: fasta or fastq")
    if fmt == "fasta" and min_quality:
        raise ValueError("a quality floor needs qualities: fmt='fastq'")
    if not (k & 1) or not 5 <= k <= 31:
        raise ValueError(f"counting in parts goes through the counting table: odd 5 <= k <= 31 (got {k})")
    cnt = Counter(k, device, _lib.COUNT_TABLE)
    spec = np.zeros(256, dtype=np.uint64)
    per_part, stack, first_trust = [], [], None

    def merge_top() -> int:
        t0 = time.perf_counter_ns()
        (ra, a), (_, b) = stack.pop(), stack.pop()
        stack.append((ra + 1, b.maximum(a, min_count)))
        return time.perf_counter_ns() - t0

    for p in range(parts):
        cnt.reset()
        cnt.set_slice(p, parts)
        tot = dict.fromkeys(trust.TOTALS, 0) if fmt == "fastq" or acgt_only else None
        t0 = time.perf_counter_ns()
        for path in paths:
            with open_input(path) as f:
                if tot is None:
                    cnt.count_fasta(f)
                    continue
                st = cnt.count_reads(f, fmt, min_quality, acgt_only)
                for name in tot:
                    tot[name] += st["trust"][name]
        if p == 0:
            first_trust = tot
        spec[1:] += cnt.spectrum()[1:]
        t1 = time.perf_counter_ns()
        lst = CountList.from_counter(cnt, min_count)
        t2 = time.perf_counter_ns()
        info = cnt.table_info()
        row = {"part": p, "keys": info["keys"], "listed": lst.n, "log2_lines": info["log2_lines"], "peak_bytes": info["peak_bytes"],
               "slice_stats": cnt.slice_stats(), "ns_count": t1 - t0, "ns_list": t2 - t1, "ns_join": 0}
        stack.append((0, lst))
        while len(stack) > 1 and stack[-1][0] == stack[-2][0]:
            row["ns_join"] += merge_top()
        per_part.append(row)
    tail = 0
    while len(stack) > 1:
        tail += merge_top()
    spec[0] = np.uint64((1 << (2 * k - 1)) - int(spec[1:].sum()))
    joined = stack[0][1]
    return joined, spec, {"parts": per_part, "ns_join_tail": tail, "trust": first_trust, "list_bytes": 9 * joined.n}
