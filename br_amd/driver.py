"""br::run_correction mirror (src/lib.rs:22-139).

Batches of 8192 records (populate_buffer's hard-coded size, src/lib.rs:90 -- `record_buffer_len`
only sizes a Vec there, :84), every method in order, the reverse pass unless two_side
(src/lib.rs:48,110), records written in input order (the serial path's order, src/lib.rs:29-66).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import BinaryIO, Dict, Optional, Sequence

import contextlib

from . import _lib, cover, fasta, hostio, strand
from .correct import Chain, Corrector

RECORD_BATCH = 8192
COVER_KEYS = ("kmers_in", "solid_in", "covered_in", "runs_in", "kmers_out", "solid_out", "covered_out", "runs_out")
REPORT_HEADER = b"#name\tlen_in\tkmers_in\tsolid_in\tcovered_in\truns_in\tlen_out\tkmers_out\tsolid_out\tcovered_out\truns_out\n"


def run_correction(inputs: Sequence[BinaryIO], outputs: Sequence[BinaryIO], methods: Sequence[Corrector],
                   two_side: bool, record_buffer_len: int = 8192, native: Optional[bool] = None,
                   batch_records: int = 0, output_mode: str = "plain", min_len: int = 0,
                   reports: Optional[Sequence[Optional[BinaryIO]]] = None, cover_stats: bool = False,
                   second_pass: Optional[str] = None) -> Dict[str, int]:
    """native (default; BRX_HOST_PIPELINE=0 selects the other): the C++ pipeline of libbrx (brx_run_correction_fd:
    parse / GPU / format on their own threads, batches that fill the GPU).  native=False: the same job record by
    record in Python (fasta.py + Chain.correct_reads), kept as the readable statement of the behaviour and
    compared byte for byte with the native path by the tests.  batch_records (native): records per GPU batch,
    0 = the library's default (32768 or 256 MB; the reference's 8192 is too small to fill the GPU).

    Not in the reference (include/brx.h "coverage", br_amd/cover.py): output_mode "mask" writes the corrected records
    with the bases no solid k-mer covers in lower case, "split" writes their covered runs of at least min_len bases as
    records `name_i [description]`; reports (one binary file object per output, or None) receive one TSV line of cover
    statistics per input record, before and after; cover_stats (implied by reports) adds the totals `kmers_in` ..
    `runs_out` to the returned dict.  Both paths write the same bytes; a plain run is untouched.

    second_pass (not in the reference; br_amd/strand.py): "none", "reverse" or "revcomp" -- the second scan on the
    reverse complement of the first scan's output.  None keeps two_side's meaning; two_side=True beside another mode
    raises.  With None the calls into the library are the ones made before the option existed."""
    mode = strand.resolve_second_pass(second_pass, two_side)
    if output_mode not in _lib.OUT_MODES:
        raise ValueError(f"output_mode={output_mode!r}: plain, mask or split")
    if min_len and output_mode != "split":
        raise ValueError("min_len belongs to output_mode='split'")
    if not 0 <= int(min_len) < 1 << 32:
        raise ValueError(f"min_len={min_len} does not fit 32 bits")
    if reports is not None and len(reports) != len(outputs):
        raise ValueError("one report per output")
    reports = list(reports) if reports is not None else [None] * len(outputs)
    want_stats = cover_stats or any(r is not None for r in reports)
    extra = output_mode != "plain" or want_stats
    if native is None:
        native = os.environ.get("BRX_HOST_PIPELINE", "1") != "0"
    totals = {"records": 0, "bases_in": 0, "bases_out": 0, "batches": 0, "ns_parse": 0, "ns_gpu": 0, "ns_write": 0, "ns_wall": 0}
    if not methods:
        raise ValueError("empty method list")
    solid = methods[0].valid_kmer()
    if native:
        specs = (_lib.Method * len(methods))(*[_lib.Method(*_spec_codes(m)) for m in methods])
        for inp, out, rep in zip(inputs, outputs, reports):
            st = (C.c_uint64 * 8)()
            if not extra and second_pass is None:
                with hostio.input_fd(inp) as ifd, hostio.output_fd(out) as ofd:
                    _lib.check(_lib.lib().brx_run_correction_fd(solid._h, specs, len(methods), two_side, ifd, ofd, batch_records, st))
            else:
                ct = (C.c_uint64 * 8)()
                with hostio.input_fd(inp) as ifd, hostio.output_fd(out) as ofd, \
                        (hostio.output_fd(rep) if rep is not None else contextlib.nullcontext(-1)) as rfd:
                    opts = _lib.OutputOpts(_lib.OUT_MODES[output_mode], int(min_len), rfd, 1 if want_stats else 0)
                    if second_pass is None:
                        _lib.check(_lib.lib().brx_run_correction_fd_opts(solid._h, specs, len(methods), two_side, ifd, ofd,
                                                                         batch_records, C.byref(opts), st, ct))
                    else:
                        _lib.check(_lib.lib().brx_run_correction_fd_pass(solid._h, specs, len(methods), strand.PASS_IDS[mode], ifd,
                                                                         ofd, batch_records, C.byref(opts), st, ct))
                if want_stats:
                    for key, v in zip(COVER_KEYS, ct):
                        totals[key] = totals.get(key, 0) + int(v)
            for key, v in zip(totals, st):
                totals[key] += int(v)
        return totals
    chain = Chain(solid, [m.spec() for m in methods], two_side=two_side, second_pass=second_pass)
    if want_stats:
        totals.update({key: 0 for key in COVER_KEYS})
    form = (output_mode, int(min_len), want_stats) if extra else None
    for inp, out, rep in zip(inputs, outputs, reports):
        if rep is not None:
            rep.write(REPORT_HEADER)
        batch = []
        for rec in fasta.read_records(inp):
            batch.append(rec)
            if len(batch) == RECORD_BATCH:
                _flush(chain, batch, out, totals, solid, form, rep)
                batch = []
        if batch:
            _flush(chain, batch, out, totals, solid, form, rep)
    return totals


def _spec_codes(m: Corrector):
    name, confirm, max_search = m.spec()
    return _lib.METHOD_IDS[name], confirm, max_search


def _flush(chain, batch, out, totals, solid=None, form=None, rep=None) -> None:
    seqs = [r[2] for r in batch]
    corrected = chain.correct_reads(seqs)
    if form is None:
        for (name, desc, _), seq in zip(batch, corrected):
            fasta.write_record(out, name, desc, seq)
            totals["bases_out"] += len(seq)
    else:
        # the output forms, record by record from the definitions of cover.py; the probes are the GPU's (one per k-mer)
        mode, min_len, want_stats = form
        k = solid.k()
        flags_out, _ = solid.cover_reads(corrected)
        flags_in = solid.cover_reads(seqs)[0] if want_stats else None
        for i, ((name, desc, _), seq) in enumerate(zip(batch, corrected)):
            covered = (flags_out[i] & cover.COVERED) != 0
            if mode == "split":
                header = name + ((b" " + desc) if desc else b"")
                for pdef, piece in cover.split_record(header, seq, covered, min_len):
                    pname, _, pdesc = pdef.partition(b" ")
                    fasta.write_record(out, pname, pdesc or None, piece)
            else:
                fasta.write_record(out, name, desc, cover.mask_read(seq, covered) if mode == "mask" else seq)
            totals["bases_out"] += len(seq)
            if want_stats:
                a, z = cover.stats_from_flags(flags_in[i], k), cover.stats_from_flags(flags_out[i], k)
                for key, v in zip(COVER_KEYS, a + z):
                    totals[key] += v
                if rep is not None:
                    rep.write(name + b"\t" + b"\t".join(str(v).encode() for v in (len(seqs[i]),) + a + (len(seq),) + z) + b"\n")
    totals["records"] += len(batch)
    totals["bases_in"] += sum(len(s) for s in seqs)
    totals["batches"] += 1
