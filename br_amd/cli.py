"""Command-line surface of `br` (src/cli.rs:19-76, 172-185; dispatch src/main.rs:17-58), over the HIP path.

    python -m br_amd -i reads.fa -o corr.fa [-s] [-c one -c graph ...] [-C 5] [-M 7] \
        fasta -i reads.fa -k 19 -a 3                       # count -> threshold -> correct (src/main.rs:72-85)
        solid -i set.solid -f solid                        # load a pcon .solid set     (src/main.rs:117-120)
        count -i table.pcon -a 3                           # load a pcon count table    (src/main.rs:59-70)
        solid -i reads.fa -f fasta -k 19                   # presence-only set          (src/set/pcon.rs:47-112)
        solid -i reads.fq -f fastq -k 19 | solid -i kmers.csv -f csv -k 19   # the reference's optional features

Same flags, defaults and quirks as the reference: `-s/--two-side` DISABLES the reverse pass
(src/lib.rs:48,110); `fasta -k` is forced odd (src/cli.rs:277-279); without `-a` an abundance method
sub-command is needed (src/main.rs:95-110): `first-minimum`, `rarefaction P`, `percent-most P`, `percent-least P`
pick the threshold from the count spectrum (br_amd/spectrum.py: pcon's published formulas, unpinned by the
reference's tests).  `count -i table` loads a pcon count table ([k][2^(2k-1) u8 counters], layout unpinned: the
reference holds no such fixture) and thresholds it the same way; `large-kmer -f fasta` (N4) builds a sparse set for odd k <= 31.  `-t` (rayon
pool size) is accepted and ignored: the GPU is the pool.

Not in the reference, like `--device` (include/brx.h "coverage"; a base is covered when it lies inside a solid k-mer):
    --mask-weak                write the corrected reads with the bases no solid k-mer covers in lower case
    --trim-split [MINLEN]      write the covered stretches of at least MINLEN (default 0) bases of every corrected read
                               as records `name_i [description]` (what LoRDEC's trim-split does after its correction)
    --cover-report PATH        one per -o: TSV of k-mers / solid k-mers / covered bases / runs per read, before and after
    --abundance-report PATH    one per -o, with `fasta` or `count`: TSV of how often the k-mers of every input read were
                               counted -- k-mers / absent / above the threshold / min / median / max / mean per read
                               (br_amd/abundance.py).  `fasta` then counts into the hash table (BRX_COUNT_TABLE) whatever
                               the k: the same set, a slower build
    --save-set PATH            with any sub-command: write the set in use as a key file (br_amd/keyfile.py: sorted keys in
                               blocks of 256, any odd k from 5 to 31) before the correction starts; `solid -i PATH -f keys`
                               loads it again, no -k needed
    --save-counts PATH         with `fasta` or `count`: write the k-mer counts as a key file with a count byte per key;
                               `count -i PATH` loads it again (the magic is sniffed after decompression; anything else is
                               still read as a pcon count table) and -a or a threshold selector follow as usual.  `fasta`
                               at 15 <= k <= 21 keeps its partitioned counter and saves that one's count view (measured
                               faster than the table's count + list + sort: tools/partition_keyfile_bench.py); at any other
                               k, and with --abundance-report, it counts into the hash table: the same set, the same file
    --save-min-count N         keep only the k-mers counted at least N times (default 1) in --save-counts.  A counter loaded
                               from such a file no longer knows the rarer k-mers: thresholds below N - 1 are refused
    --set-or PATH | --set-and PATH | --set-minus PATH
                               combine the set the sub-command built with the set in PATH -- add its k-mers, keep only the
                               k-mers also in it, remove its k-mers (br_amd/setops.py) -- before --save-set and before the
                               correction.  Each is repeatable; they are applied left to right in command-line order.  PATH is
                               a key file (set or count file, the counts are ignored) or a .solid stream, gz / bz2 / xz
                               sniffed, of the same k as the set in use:
                                 python -m br_amd -i reads.fa -o corr.fa --set-or illumina.keys --set-minus mito.keys \
                                     --save-set final.keys -c one fasta -i reads.fa -k 21 -a 3
    count -i A.keys --counts-add PATH | --counts-minus PATH | --counts-min PATH | --counts-max PATH
                               combine the count file given with `count -i` with the count file in PATH (gz / bz2 / xz sniffed,
                               the same k) -- add the counts up to 255, subtract them (a k-mer stays while its count stays
                               positive), keep the smaller or the larger count (br_amd/countops.py).  Each is repeatable; they
                               are applied left to right in command-line order.  The files are merged as sorted lists on the
                               GPU, no counting table is built; -a or a threshold selector then pick the solid k-mers of the
                               combined list, and --save-counts / --save-min-count (also accepted behind `count`) write it.
                               A list answers no lookups as it is: --abundance-report is refused unless --list-lookup is
                               given (below).  Shards counted apart, summed, with a contaminant's counts taken off:
                                 python -m br_amd -i reads.fa -o corr.fa -c one count -i shard0.keys --counts-add shard1.keys \
                                     --counts-minus mito.keys -a 3 --save-counts job.keys
    count -i A.keys [--counts-* ...] --counts-compare PATH --compare-report PATH
                               put the counts in use -- after every --counts-* flag -- side by side with the count file in PATH
                               (gz / bz2 / xz sniffed, the same k) and write a TSV report: the k-mers of either, both, each one
                               alone and their Jaccard index, how much of PATH's k-mers the solid k-mers cover (completeness),
                               the share of the solid k-mers' occurrences PATH does not vouch for, as a per-base error rate and
                               QV (Merqury's k-mer survival formula), then the joint spectrum itself: one line `ca cb kmers`
                               per pair of counts (br_amd/countops.py compare_report; include/brx.h "count lists").  A k-mer of
                               the counts in use counts as kept where the set being built keeps it (count > threshold), a k-mer
                               of PATH as vouched for wherever it is listed.  Each flag needs the other; either takes the list
                               route: -i must be a key file, no counting table is built.  Set, corrected reads and
                               --save-counts file are those of the same command without the two flags.  How good was a
                               correction, given a trusted count file:
                                 python -m br_amd -i reads.fa -o corr.fa -c one count -i corrected.keys \
                                     --counts-compare illumina.keys --compare-report qv.tsv -a 0
    fastq -i R.fq [-i ...] -k K (-a N | first-minimum | ...) [-q MINQ] [--all-bytes]
                               a sub-command like `fasta` that counts FASTQ reads (gz / bz2 / xz sniffed), and only the k-mers
                               none of whose bases is untrusted: a base is untrusted when it is not ACGTacgt or its quality
                               (Phred+33) lies below MINQ (default 0: no floor).  --all-bytes counts every byte as a base, as
                               `fasta` does.  The reads are cut into their trusted stretches on the GPU (br_amd/trust.py), the
                               counters take the pieces; -a, the threshold selectors, --save-counts, --abundance-report,
                               --save-set and --set-* work as with `fasta`.  One line of totals goes to stderr:
                                 python -m br_amd -i reads.fa -o corr.fa --save-set illumina.keys -c one \
                                     fastq -i illumina.fq.gz -k 21 -q 20 first-minimum
    fasta | fastq ... --count-parts P
                               count in P sweeps over the inputs (1 <= P <= 4096), each in a hash table sized for the P-th of
                               the k-mers it owns (br_amd/parts.py), and join the sweeps' count lists: jobs whose k-mers do not
                               fit one table.  Any odd k from 5 to 31; the same set, --save-counts file and correction as
                               without the flag.  A sweep's list keeps the k-mers counted at least --save-min-count times with
                               --save-counts, otherwise more than A times with -a A -- with -a, only solid k-mers are ever kept
                               between sweeps -- otherwise all of them.  Lists answer no lookups as they are:
                               --abundance-report is refused unless --list-lookup is given (below)
    --list-lookup              in front of the sub-command, with `count` or with `fasta` / `fastq` --count-parts: the count list
                               gets a lookup directory (bucket offsets into its sorted keys, about half a byte per k-mer beside
                               the list's 9) and --abundance-report is written from it (include/brx.h "lookups in a count
                               list").  `fasta|fastq ... --count-parts P --list-lookup --abundance-report R`: the sweeps keep
                               every k-mer whatever -a or --save-min-count say, --save-min-count is applied when --save-counts
                               writes the file; report, set, count file and corrected reads are those of the same command
                               without --count-parts.  `count -i A.keys [--counts-* ...] --list-lookup [--abundance-report R]`
                               takes the list route even with no --counts-*: -i must be a key file, no counting table is built,
                               the report uses the threshold in use.  A slower lookup than the table's (README "Count lists"):
                               it is for the jobs that have no table
    fasta ... --skip-non-acgt  count only the k-mers of ACGTacgt bases (off by default: the reference counts every byte)
    solid | large-kmer -f fastq|fasta ... [-q MINQ] [--skip-non-acgt]
                               the same two switches for the presence-only sets
    --second-pass MODE         reverse (default: the reference's second scan, reads reversed and not complemented),
                               revcomp (the second scan on the reverse complement: br_amd/strand.py) or none (= -s)
"""
from __future__ import annotations

import argparse
import bz2
import gzip
import io
import lzma
import sys
from typing import BinaryIO, List, Optional

from . import _lib, abundance, countops, fasta, keyfile, parts, spectrum, strand, trust
from .correct import build_methods
from .driver import run_correction
from .set import Counter, CountList, Pcon

METHOD_NAMES = ["one", "two", "graph", "greedy", "gap-size"]  # clap ValueEnum kebab-case of CorrectionMethod



def u8(text: str) -> int:
    """clap parses -a / -C / -M into u8 fields (src/cli.rs:46,50,196): out-of-range values are rejected, not wrapped"""
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("invalid digit found in string: %r" % text)
    if not 0 <= v <= 255:
        raise argparse.ArgumentTypeError("%r is not in 0..=255" % text)
    return v


def min_quality(text: str) -> int:
    """-q MINQ: a Phred score, 0..93 (Phred+33 ends at '~')"""
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("invalid digit found in string: %r" % text)
    if not 0 <= v <= trust.MAX_QUALITY:
        raise argparse.ArgumentTypeError("%r is not in 0..=%d" % (text, trust.MAX_QUALITY))
    return v


def min_len(text: str) -> int:
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("invalid digit found in string: %r" % text)
    if not 0 <= v < 1 << 32:
        raise argparse.ArgumentTypeError("%r is not in 0..2^32" % text)
    return v


COUNTING = ("fasta", "fastq", "count")  # the sub-commands that build a counter


def output_form(args):
    """(output_mode, min_len, report paths or None) of the parsed flags; the reports pair with the outputs"""
    mode = "mask" if args.mask_weak else ("split" if args.trim_split is not None else "plain")
    n_out = len(args.outputs) if args.outputs else 1
    if args.cover_report is not None and len(args.cover_report) != n_out:
        raise SystemExit("Error: %d --cover-report for %d output(s): give one per -o" % (len(args.cover_report), n_out))
    return mode, (args.trim_split or 0), args.cover_report


def abundance_reports(args):
    """the --abundance-report paths (or None): one per output, and only where a counter is built"""
    paths = args.abundance_report
    if paths is None:
        return None
    if args.subcommand not in COUNTING:
        raise SystemExit("Error: --abundance-report asks the k-mer counter, and `%s` builds its set without a counter: "
                         "use it with `fasta`, `fastq` or `count`" % args.subcommand)
    n_out = len(args.outputs) if args.outputs else 1
    if len(paths) != n_out:
        raise SystemExit("Error: %d --abundance-report for %d output(s): give one per -o" % (len(paths), n_out))
    if not args.inputs:
        raise SystemExit("Error: --abundance-report reads the records a second time: give them with -i, not on stdin")
    return paths


def save_counts_of(args):
    """the --save-counts path (or None): only where a counter is built"""
    if args.save_counts is None:
        if args.save_min_count is not None:
            raise SystemExit("Error: --save-min-count goes with --save-counts")
        return None
    if args.subcommand not in COUNTING:
        raise SystemExit("Error: --save-counts writes the k-mer counter, and `%s` builds its set without a counter: "
                         "use it with `fasta`, `fastq` or `count` (--save-set writes the set)" % args.subcommand)
    return args.save_counts


def second_pass_of(args) -> str:
    """the second-pass mode of the parsed flags: --second-pass wins where given, -s means none, both must agree"""
    if args.two_side and args.second_pass not in (None, "none"):
        raise SystemExit("Error: -s/--two-side means one scan and contradicts --second-pass %s" % args.second_pass)
    return strand.resolve_second_pass(args.second_pass, args.two_side)


SET_FLAGS = {"--set-or": "union", "--set-and": "intersection", "--set-minus": "difference"}


class SetOpAction(argparse.Action):
    """--set-or / --set-and / --set-minus PATH: (operation, flag, path) appended to ONE list, args.set_ops, so that the
    order of the command line is the order they are applied in"""

    def __call__(self, parser, namespace, values, option_string=None):
        ops = list(getattr(namespace, self.dest, None) or [])
        ops.append((SET_FLAGS[option_string], option_string, values))
        setattr(namespace, self.dest, ops)


COUNT_FLAGS = {"--counts-add": "add", "--counts-minus": "sub", "--counts-min": "min", "--counts-max": "max"}


class CountOpAction(argparse.Action):
    """--counts-add / --counts-minus / --counts-min / --counts-max PATH: SetOpAction's twin, one list args.count_ops"""

    def __call__(self, parser, namespace, values, option_string=None):
        ops = list(getattr(namespace, self.dest, None) or [])
        ops.append((COUNT_FLAGS[option_string], option_string, values))
        setattr(namespace, self.dest, ops)


def load_count_list(flag: str, path: str, dev: int) -> CountList:
    """the count list of `count -i` or of a --counts-* operand: a count file, told by its magic after decompression"""
    try:
        with open_input(path) as f:
            if not keyfile.is_keyfile(f.peek(8)[:8]):
                raise SystemExit("Error: %s %s: not a key file.  --counts-add / --counts-minus / --counts-min / --counts-max combine "
                                 "count files (--save-counts writes one); a pcon count table is not a sorted list" % (flag, path))
            return CountList.from_keyfile(f, dev)
    except (_lib.BrxError, OSError) as e:
        raise SystemExit(f"Error: {flag} {path}: {e}")


def list_lookup_of(args) -> bool:
    """--list-lookup: only where a count list is kept -- `fasta` / `fastq` with --count-parts, and `count`, which it sends down
    the list route"""
    if not args.list_lookup:
        return False
    if args.subcommand not in COUNTING:
        raise SystemExit("Error: --list-lookup looks k-mers up in a count list, and `%s` keeps none: use it with `count`, or with "
                         "`fasta` / `fastq` --count-parts" % args.subcommand)
    if args.subcommand != "count" and getattr(args, "count_parts", None) is None:
        raise SystemExit("Error: --list-lookup looks k-mers up in a count list, and `%s` without --count-parts keeps a counter, "
                         "no list: --abundance-report asks the counter there, as it is" % args.subcommand)
    return True


def compare_of(args) -> bool:
    """--counts-compare PATH --compare-report PATH behind `count`: each needs the other; either sends `count` down the list
    route"""
    given = getattr(args, "counts_compare", None) is not None, getattr(args, "compare_report", None) is not None
    if given[0] != given[1]:
        raise SystemExit("Error: --counts-compare names the count file to compare with and --compare-report the file the "
                         "report goes to: %s was given without %s" % (("--counts-compare", "--compare-report") if given[0] else
                                                                      ("--compare-report", "--counts-compare")))
    return given[0]


def write_list_reports(lst: CountList, threshold: int, args, abund_paths) -> None:
    """--list-lookup: the list gets its lookup directory, and every --abundance-report is written from it"""
    if not abund_paths:
        return
    try:
        lst.prepare_lookup()
        for src, dst in zip(args.inputs, abund_paths):
            with open_input(src) as f, open(dst, "wb") as rep:
                write_abundance_report(lst, threshold, f, rep, args.record_buffer or 8192)
        lst.drop_lookup()  # (the directory's memory goes back before the set is built)
    except _lib.BrxError as e:
        raise SystemExit(f"Error: --list-lookup: {e}")


def build_set_from_lists(args, counts_path: Optional[str], abund_paths=None) -> Pcon:
    """the list route of `count`: the count file of -i combined with every --counts-* operand, left to right; the threshold
    from -a or from the combined list's spectrum; --save-counts writes the combined list; with --list-lookup the
    --abundance-report is written from the combined list; with --counts-compare the --compare-report is written from the
    joint spectrum of the combined list and that file; the solid set is its finish"""
    if args.abundance_report is not None and not args.list_lookup:
        raise SystemExit("Error: --abundance-report asks a k-mer counter about single k-mers, and --counts-* work on count lists, "
                         "which answer no lookups: save the combined counts (--save-counts) and run `count -i` on that file.  "
                         "Or pass --list-lookup: the combined list then gets a lookup directory and the report is written from it")
    lst = load_count_list("count -i", args.sub_inputs, args.device)
    for name, flag, path in args.count_ops or []:
        other = load_count_list(flag, path, args.device)
        if other.k != lst.k:
            raise SystemExit("Error: %s %s: k = %d, the counts in use have k = %d" % (flag, path, other.k, lst.k))
        try:
            lst = lst.combine(other, name)
        except _lib.BrxError as e:
            raise SystemExit(f"Error: {flag} {path}: {e}")
    compare = None
    if compare_of(args):
        compare = load_count_list("--counts-compare", args.counts_compare, args.device)
        if compare.k != lst.k:
            raise SystemExit("Error: --counts-compare %s: k = %d, the counts in use have k = %d" % (args.counts_compare, compare.k, lst.k))
    thr = args.abundance
    if thr is None:
        if args.abundance_selection is None:
            raise SystemExit("Error: You must provide an abundance method or an abundance threshold")      # main.rs:109
        thr = spectrum.get_threshold(lst.spectrum(), args.abundance_selection, getattr(args, "percent", 0.0))
        if thr is None:
            raise SystemExit("Error: Can't compute minimal abundance")                  # error.rs ComputeAbundanceThreshold
    if thr < lst.floor - 1:
        raise SystemExit("Error: the combined counts hold only the k-mers counted at least %d times, so the set of abundance %d would "
                         "miss members; the lowest threshold they support is %d" % (lst.floor, thr, lst.floor - 1))
    if counts_path is not None:
        try:
            with open(counts_path, "wb") as f:
                lst.save(f, 1 if args.save_min_count is None else args.save_min_count)
        except _lib.BrxError as e:
            raise SystemExit(f"Error: --save-counts: {e}")
    if args.list_lookup:
        write_list_reports(lst, thr, args, abund_paths)
    if compare is not None:
        # A: the combined list, a k-mer kept where the set being built keeps it; B: the file, vouching wherever it lists
        try:
            J = lst.joint(compare)
            with open(args.compare_report, "wb") as f:
                f.write(countops.compare_report(lst.k, lst.floor, compare.floor, J, min_a=thr + 1, min_b=1))
        except _lib.BrxError as e:
            raise SystemExit(f"Error: --counts-compare {args.counts_compare}: {e}")
        del compare  # (the file's list goes back before the set is built)
    return lst.finish(thr)


def count_parts(text: str) -> int:
    """argparse type for --count-parts: 1 .. 4096 sweeps"""
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"invalid int value: {text!r}")
    if not 1 <= v <= parts.MAX_PARTS:
        raise argparse.ArgumentTypeError(f"{v} is not in 1..{parts.MAX_PARTS}")
    return v


COUNT_PARTS_HELP = ("count in P sweeps over the inputs (1 <= P <= 4096), each sweep in a hash table (BRX_COUNT_TABLE) sized for "
                    "the P-th of the k-mers it owns, and join the sweeps' count lists: for jobs whose k-mers do not fit one table; "
                    "any odd k from 5 to 31; the same set, counts and correction.  Between sweeps a list keeps the k-mers counted "
                    "at least --save-min-count times with --save-counts, otherwise more than A times with -a A -- with -a, only "
                    "solid k-mers are ever kept between sweeps -- otherwise all of them: a selector's threshold is not known "
                    "until the last sweep (not in the reference)")


def build_set_in_parts(args, counts_path: Optional[str], abund_paths=None) -> Pcon:
    """the --count-parts route of `fasta` and `fastq`: parts.count_in_parts, the threshold from -a or from the summed
    spectrum, --save-counts writes the joined list, the solid set is its finish.  With --list-lookup the sweeps keep every
    k-mer, --save-min-count is applied at the save, and the --abundance-report is written from the joined list"""
    if args.abundance_report is not None and not args.list_lookup:
        raise SystemExit("Error: --abundance-report asks a k-mer counter about single k-mers, and --count-parts keeps count lists, "
                         "which answer no lookups: save the joined counts (--save-counts) and run `count -i` on that file.  "
                         "Or pass --list-lookup: the joined list then gets a lookup directory and the report is written from it")
    k = fasta_kmer_size(args.kmer_size)
    if not 5 <= k <= 31:
        raise SystemExit("Error: --count-parts counts through the hash table, which takes odd k from 5 to 31 (k=%d)" % k)
    if args.abundance is None and args.abundance_selection is None:
        raise SystemExit("Error: You must provide an abundance method or an abundance threshold")  # main.rs:109
    save_floor = max(1, args.save_min_count or 1)
    if args.list_lookup:
        floor = 1  # a report counts every k-mer of a read: nothing may be dropped between the sweeps
    elif counts_path is not None:
        floor = save_floor
    elif args.abundance is not None:
        floor = min(255, args.abundance + 1)
    else:
        floor = 1
    fastq = args.subcommand == "fastq"
    try:
        lst, spec, st = parts.count_in_parts(args.sub_inputs, k, args.count_parts, args.device, floor, "fastq" if fastq else "fasta",
                                             args.min_quality if fastq else 0, (not args.all_bytes) if fastq else args.skip_non_acgt)
    except _lib.BrxError as e:
        raise SystemExit(f"Error: --count-parts: {e}")
    if fastq:  # (every sweep sees the same reads: the first one's totals)
        sys.stderr.write("fastq: %(bases)d bases, %(non_acgt)d not ACGT, %(low_quality)d below the quality floor, "
                         "%(pieces)d trusted stretches of %(kept_bases)d bases, %(kmers)d k-mers counted\n" % st["trust"])
    thr = args.abundance
    if thr is None:
        thr = spectrum.get_threshold(spec, args.abundance_selection, getattr(args, "percent", 0.0))
        if thr is None:
            raise SystemExit("Error: Can't compute minimal abundance")                  # error.rs ComputeAbundanceThreshold
    if thr < lst.floor - 1:
        raise SystemExit("Error: the counts are saved with --save-min-count %d: k-mers seen fewer times are not kept between the "
                         "sweeps, so the set of abundance %d would miss members; the lowest threshold they support is %d"
                         % (lst.floor, thr, lst.floor - 1))
    if counts_path is not None:
        try:
            with open(counts_path, "wb") as f:
                lst.save(f, max(floor, save_floor))
        except _lib.BrxError as e:
            raise SystemExit(f"Error: --save-counts: {e}")
    if args.list_lookup:
        write_list_reports(lst, thr, args, abund_paths)
    return lst.finish(thr)


def load_operand(path: str, dev: int) -> Pcon:
    """the set of a --set-* operand: a key file (told by its magic after decompression; the counts of a count file are
    ignored) or else a .solid stream"""
    with open_input(path) as f:
        if keyfile.is_keyfile(f.peek(8)[:8]):
            return Pcon.from_keyfile(f, dev)
        return Pcon.from_pcon_solid(f.read(), dev)


def apply_set_ops(kmer_set: Pcon, set_ops, dev: int) -> Pcon:
    """the set in use combined with every operand, left to right"""
    for name, flag, path in set_ops or []:
        try:
            other = load_operand(path, dev)
            if other.k() != kmer_set.k():
                raise SystemExit("Error: %s %s: k = %d, the set in use has k = %d" % (flag, path, other.k(), kmer_set.k()))
            kmer_set = kmer_set.combine(other, name)
        except (_lib.BrxError, OSError) as e:
            raise SystemExit(f"Error: {flag} {path}: {e}")
    return kmer_set


def open_input(path: str) -> BinaryIO:
    """niffler::get_reader: sniff gz / bz2 / xz by magic bytes (src/cli.rs:209,269,404,415)."""
    raw = open(path, "rb")
    head = raw.peek(6)[:6] if hasattr(raw, "peek") else b""
    # (peek does not move the logical position: a plain file can still be handed to the native pipeline as a descriptor)
    if head[:2] == b"\x1f\x8b":
        return gzip.open(raw, "rb")
    if head[:3] == b"BZh":
        return bz2.open(raw, "rb")
    if head[:6] == b"\xfd7zXZ\x00":
        return lzma.open(raw, "rb")
    return raw


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="br", description="Br: Brutal rewrite a simple long read corrector based on kmer "
                                                       "spectrum methode (MI355X-native hot path)")
    # clap derive, Option<Vec<T>>: ONE value per occurrence, repeat the flag for more (-i a -i b)
    p.add_argument("-i", "--inputs", action="append", default=None, help="Path to inputs, default read stdin")
    p.add_argument("-o", "--outputs", action="append", default=None, help="Path to output, default stdout")
    p.add_argument("-s", "--two-side", action="store_true", help="Correct in two side (sic: disables the reverse pass)")
    p.add_argument("-c", "--corrections", action="append", choices=METHOD_NAMES, default=None,
                   help="Correction method")
    p.add_argument("-C", "--confirm", type=u8, default=None, help="Number of kmer required to validate correction")
    p.add_argument("-M", "--max-search", type=u8, default=None, help="Number of base we use to try correct error")
    p.add_argument("-b", "--record_buffer", type=int, default=None, help="Number of sequence record load in buffer")
    p.add_argument("-t", "--threads", type=int, default=None, help="accepted for compatibility, ignored")
    p.add_argument("-q", "--quiet", action="store_true")
    p.add_argument("-v", "--verbosity", action="count", default=0)
    p.add_argument("-T", "--timestamp", default=None)
    p.add_argument("--device", type=int, default=0, help="GPU index (not in the reference)")
    form = p.add_mutually_exclusive_group()
    form.add_argument("--mask-weak", action="store_true",
                      help="lower-case the bases of the output that no solid k-mer covers (not in the reference)")
    form.add_argument("--trim-split", type=min_len, nargs="?", const=0, default=None, metavar="MINLEN",
                      help="write the covered stretches of at least MINLEN bases as records name_i (not in the reference)")
    p.add_argument("--cover-report", action="append", default=None, metavar="PATH",
                   help="per-read cover statistics before and after as TSV, one per -o (not in the reference)")
    p.add_argument("--abundance-report", action="append", default=None, metavar="PATH",
                   help="per-read k-mer abundance (k-mers, absent, above the threshold, min, median, max, mean count) of the "
                        "input reads as TSV, one per -o; with `fasta` or `count` only.  `fasta` then counts into the hash "
                        "table (BRX_COUNT_TABLE) whatever the k: the same set, a slower build (not in the reference)")
    p.add_argument("--second-pass", choices=["reverse", "revcomp", "none"], default=None,
                   help="second scan of every read: reverse (default, the reference's), revcomp (on the reverse complement) "
                        "or none (what -s means) (not in the reference)")
    p.add_argument("--save-set", default=None, metavar="PATH",
                   help="write the set in use as a key file before the correction starts; `solid -i PATH -f keys` loads it "
                        "(not in the reference)")
    for flag, what in (("--set-or", "add the k-mers of"), ("--set-and", "keep only the k-mers also in"),
                       ("--set-minus", "remove the k-mers of")):
        p.add_argument(flag, action=SetOpAction, dest="set_ops", default=None, metavar="PATH",
                       help=what + " the set in PATH (a key file or a .solid stream of the same k) before --save-set and the "
                            "correction; repeatable, applied in command-line order (not in the reference)")
    p.add_argument("--save-counts", default=None, metavar="PATH",
                   help="write the k-mer counts as a key file; with `fasta` or `count` only; `count -i PATH` loads it.  `fasta` "
                        "then counts into the hash table (BRX_COUNT_TABLE), except at 15 <= k <= 21 without --abundance-report, "
                        "where its partitioned counter saves its count view (not in the reference)")
    p.add_argument("--save-min-count", type=u8, default=None, metavar="N",
                   help="keep only the k-mers counted at least N times in --save-counts (default 1)")
    p.add_argument("--list-lookup", action="store_true",
                   help="with `count`, or `fasta` / `fastq` --count-parts: keep the counts as a count list that answers lookups "
                        "(a bucket directory of about half a byte per k-mer beside it), so that --abundance-report is written "
                        "from the list; `count -i` must then be a key file (not in the reference)")
    sub = p.add_subparsers(dest="subcommand", required=True)

    def abundance_methods(sp):
        ssub = sp.add_subparsers(dest="abundance_selection")
        ssub.add_parser("first-minimum")
        for name in ("rarefaction", "percent-most", "percent-least"):
            ssub.add_parser(name).add_argument("percent", type=float)

    c = sub.add_parser("count", help="With Count")
    c.add_argument("-i", "--inputs", dest="sub_inputs", required=True)
    c.add_argument("-a", "--abundance", type=u8, default=None)
    for flag, what in (("--counts-add", "add the counts of"), ("--counts-minus", "subtract the counts of"),
                       ("--counts-min", "keep the smaller of each count and that of"), ("--counts-max", "keep the larger of each count and that of")):
        c.add_argument(flag, action=CountOpAction, dest="count_ops", default=None, metavar="PATH",
                       help=what + " the count file in PATH (the same k); -i must be a count file too.  Repeatable, applied in "
                            "command-line order, merged as sorted lists without a counting table (not in the reference)")
    c.add_argument("--counts-compare", default=None, metavar="PATH",
                   help="with --compare-report: compare the counts in use, after every --counts-* flag, with the count file in PATH "
                        "(the same k) by their joint spectrum; -i must be a count file too (not in the reference)")
    c.add_argument("--compare-report", default=None, metavar="PATH",
                   help="with --counts-compare: write shared and private k-mers, completeness, error rate, QV and the joint spectrum "
                        "as TSV (br_amd/countops.py compare_report)")
    # (the two top-level flags are also taken behind `count`, where a command line that combines count files has its paths)
    c.add_argument("--save-counts", default=argparse.SUPPRESS, metavar="PATH", help="as in front of the sub-command")
    c.add_argument("--save-min-count", type=u8, default=argparse.SUPPRESS, metavar="N", help="as in front of the sub-command")
    abundance_methods(c)
    f = sub.add_parser("fasta", help="With Fasta")
    f.add_argument("-i", "--inputs", dest="sub_inputs", action="append", required=True)
    f.add_argument("-k", "--kmer-size", type=int, required=True)
    f.add_argument("-a", "--abundance", type=u8, default=None)
    f.add_argument("--skip-non-acgt", action="store_true",
                   help="count only the k-mers of ACGTacgt bases (not in the reference, which counts every byte)")
    f.add_argument("--count-parts", type=count_parts, default=None, metavar="P", help=COUNT_PARTS_HELP)
    abundance_methods(f)
    fq = sub.add_parser("fastq", help="With Fastq: count the trusted stretches of FASTQ reads (not in the reference)")
    fq.add_argument("-i", "--inputs", dest="sub_inputs", action="append", required=True)
    fq.add_argument("-k", "--kmer-size", type=int, required=True)
    fq.add_argument("-a", "--abundance", type=u8, default=None)
    fq.add_argument("-q", "--min-quality", type=min_quality, default=0, metavar="MINQ",
                    help="skip the k-mers over a base of Phred quality below MINQ (Phred+33; default 0: no floor)")
    fq.add_argument("--all-bytes", action="store_true", help="count every byte as a base, as `fasta` does (default: ACGTacgt only)")
    fq.add_argument("--count-parts", type=count_parts, default=None, metavar="P", help=COUNT_PARTS_HELP)
    abundance_methods(fq)
    s = sub.add_parser("solid", help="With Solid")
    s.add_argument("-i", "--input", dest="sub_input", required=True)
    s.add_argument("-f", "--format", choices=["solid", "fasta", "fastq", "csv", "keys"], required=True)
    s.add_argument("-k", "--kmer-size", type=int, default=None)
    lk = sub.add_parser("large-kmer", help="Large Kmer mode")
    lk.add_argument("-i", "--input", dest="sub_input", required=True)
    lk.add_argument("-f", "--format", choices=["fasta", "fastq", "csv"], required=True)
    lk.add_argument("-k", "--kmer-size", type=int, required=True)
    for sp in (s, lk):
        sp.add_argument("-q", "--min-quality", type=min_quality, default=0, metavar="MINQ",
                        help="-f fastq: skip the k-mers over a base of Phred quality below MINQ (not in the reference)")
        sp.add_argument("--skip-non-acgt", action="store_true",
                        help="-f fasta / fastq: skip the k-mers over a byte that is not ACGTacgt (not in the reference)")
    return p


def fasta_kmer_size(k: int) -> int:
    """Fasta::kmer_size, src/cli.rs:277-279: even k becomes k-1 (asserted 14 -> 13 at src/cli.rs:459)."""
    return k - ((~(k & 1)) & 1)


first_minimum = spectrum.first_minimum


def _records(paths: List[str]):
    for path in paths:
        with open_input(path) as f:
            for _, _, seq in fasta.read_records(f):
                yield seq


def threshold_and_finish(cnt: Counter, args, keep: Optional[dict] = None) -> Pcon:
    """count2solid, src/main.rs:86-115: `-a N` wins; otherwise the counts are histogrammed on the GPU (no u8 table
    for the partitioned counter: its keys are binned bucket by bucket), the threshold is picked on the host and the
    same counter is finished with it.  keep (a dict): receives the counter and the threshold in use"""
    thr = args.abundance
    if thr is None:
        if args.abundance_selection is None:
            raise SystemExit("Error: You must provide an abundance method or an abundance threshold")      # main.rs:109
        thr = spectrum.get_threshold(cnt.spectrum(), args.abundance_selection, getattr(args, "percent", 0.0))
        if thr is None:
            raise SystemExit("Error: Can't compute minimal abundance")                  # error.rs ComputeAbundanceThreshold
    if thr < cnt.floor - 1:
        raise SystemExit("Error: the counts were saved with --save-min-count %d: k-mers seen fewer times are not in the file, so the "
                         "set of abundance %d would miss members; the lowest threshold it supports is %d"
                         % (cnt.floor, thr, cnt.floor - 1))
    if keep is not None:
        keep.update(counter=cnt, threshold=thr)
    return cnt.finish(thr)


def build_set(args, keep: Optional[dict] = None) -> Pcon:
    """keep (a dict, --abundance-report / --save-counts): the counter is left in it, and `fasta` counts into the hash table, whose counts
    can be looked up at every k.  (The partitioned counter of 15 <= k <= 21 answers too once Counter.prepare_lookup has
    built its count view, but count + view + lookup measured slower there than the table's count + lookup: DESIGN.md
    section 10.11, tools/partition_lookup_bench.py.)  --save-counts alone at 15 <= k <= 21 keeps the partitioned counter:
    its count + view + compaction measured faster than the table's count + list + sort at k = 19 and k = 21 (DESIGN.md
    section 4, tools/partition_keyfile_bench.py), and main() builds the view before it saves"""
    dev = args.device
    if args.subcommand in ("fasta", "fastq"):
        k = fasta_kmer_size(args.kmer_size)
        if args.abundance is None and args.abundance_selection is None:
            raise SystemExit("Error: You must provide an abundance method or an abundance threshold")  # main.rs:109
        # (the table takes odd k from 5; below that the dense u8 table is the default anyway and can be looked up too)
        view_save = keep is not None and args.abundance_report is None and 15 <= k <= 21
        cnt = Counter(k, dev) if keep is None or view_save else Counter(k, dev, _lib.COUNT_TABLE if k >= 5 else _lib.COUNT_DENSE)
        tot = dict.fromkeys(trust.TOTALS, 0)
        for path in args.sub_inputs:
            with open_input(path) as f:
                if args.subcommand == "fastq":
                    st = cnt.count_reads(f, "fastq", args.min_quality, not args.all_bytes)
                elif args.skip_non_acgt:
                    st = cnt.count_reads(f, "fasta", 0, True)
                else:
                    cnt.count_fasta(f)  # the reference's rule, and its launches: every k-mer, every byte a base
                    continue
                for name in tot:
                    tot[name] += st["trust"][name]
        if args.subcommand == "fastq":
            sys.stderr.write("fastq: %(bases)d bases, %(non_acgt)d not ACGT, %(low_quality)d below the quality floor, "
                             "%(pieces)d trusted stretches of %(kept_bases)d bases, %(kmers)d k-mers counted\n" % tot)
        return threshold_and_finish(cnt, args, keep)
    if args.subcommand == "solid":
        if args.format == "solid":
            with open_input(args.sub_input) as f:
                return Pcon.from_pcon_solid(f.read(), dev)
        if args.format == "keys":  # a key file carries its k
            with open_input(args.sub_input) as f:
                try:
                    return Pcon.from_keyfile(f, dev)
                except _lib.BrxError as e:
                    raise SystemExit(f"Error: {args.sub_input}: {e}")
        if args.kmer_size is None:
            raise SystemExit("Error: Solid input fasta require kmer size")            # error.rs SolidRequireKmerSize
        return presence_set(args.sub_input, args.format, args.kmer_size, dev, args.min_quality, args.skip_non_acgt)
    if args.subcommand == "count":
        # src/main.rs:59-70: Counter::from_stream, then the same threshold -> Solid::from_count as `fasta`
        # a key file (--save-counts) is told from a pcon table by its magic, after decompression
        with open_input(args.sub_inputs) as f:
            if keyfile.is_keyfile(f.peek(8)[:8]):
                try:
                    cnt = Counter.from_keyfile(f, dev)
                except _lib.BrxError as e:
                    raise SystemExit(f"Error: {args.sub_inputs}: {e}")
            else:
                cnt = Counter.from_count_stream(f, dev)
        return threshold_and_finish(cnt, args, keep)
    # large-kmer -f fasta: set::Hash::from_fasta (src/set/hash.rs:40-60, src/main.rs:147-163) = every canonical k-mer of
    # every record, no counting.  Same membership as a presence-only Pcon; for k >= 21 the set is sparse (a chained
    # hash table in HBM instead of the bit vector).  Odd k only: cocktail's parity-canonical form is not a function
    # of the {k-mer, revcomp} pair for even k.
    if args.kmer_size % 2 == 0 or not 1 <= args.kmer_size <= 31:
        raise SystemExit("Error: large-kmer mode needs an odd k <= 31 on the HIP path (k=%d)" % args.kmer_size)
    return presence_set(args.sub_input, args.format, args.kmer_size, dev, args.min_quality, args.skip_non_acgt)


def presence_set(path: str, fmt: str, k: int, dev: int, min_q: int = 0, skip_non_acgt: bool = False) -> Pcon:
    """Pcon::from_fasta / from_fastq / from_csv and their set::Hash twins: every canonical k-mer of every record
    (FASTA and FASTQ through the native pipeline; CSV -- an optional feature of the reference -- parsed on the host).
    min_q / skip_non_acgt (not in the reference): only the k-mers of the trusted stretches (br_amd/trust.py)"""
    if fmt == "csv" and (min_q or skip_non_acgt):
        raise SystemExit("Error: -q / --skip-non-acgt go with -f fasta or -f fastq")
    if fmt == "fasta" and min_q:
        raise SystemExit("Error: -q needs qualities: use it with -f fastq")
    with open_input(path) as f:
        if fmt == "fasta" and not skip_non_acgt:
            return Pcon.from_fasta_file(f, k, dev)
        if fmt in ("fasta", "fastq"):
            return Pcon.from_reads_file(f, fmt, k, dev, min_q, skip_non_acgt)
        try:
            return Pcon.from_fasta(fasta.read_csv_kmers(f, k), k, dev)
        except ValueError as e:
            raise SystemExit(f"Error: {e}")


def write_abundance_report(cnt, threshold: int, f: BinaryIO, rep: BinaryIO, batch_records: int) -> None:
    """one TSV line (abundance.report_line) per record of the FASTA stream `f`, in input order: the records go through
    the abundance_batch of `cnt` -- a Counter, or a CountList after prepare_lookup -- in batches of batch_records, statistics
    only"""
    from .set import pack_reads
    rep.write(abundance.REPORT_HEADER)

    def flush(batch):
        bases, offs = pack_reads([seq for _, seq in batch])
        _, _, st = cnt.abundance_batch(bases, offs, threshold, profile=False)
        for (name, seq), row in zip(batch, st):
            rep.write(abundance.report_line(name, len(seq), row))

    batch = []
    for name, _, seq in fasta.read_records(f):
        batch.append((name, seq))
        if len(batch) == batch_records:
            flush(batch)
            batch = []
    if batch:
        flush(batch)


def main(argv: Optional[List[str]] = None) -> int:
    args = parser().parse_args(argv)
    mode, split_min, report_paths = output_form(args)
    second_pass = second_pass_of(args)
    abund_paths = abundance_reports(args)
    counts_path = save_counts_of(args)
    list_lookup = list_lookup_of(args)
    if getattr(args, "count_ops", None) or (list_lookup and args.subcommand == "count") or compare_of(args):
        kmer_set = build_set_from_lists(args, counts_path, abund_paths)
    elif getattr(args, "count_parts", None) is not None:
        kmer_set = build_set_in_parts(args, counts_path, abund_paths)
    elif abund_paths is None and counts_path is None:
        kmer_set = build_set(args)
    else:
        # the threshold is known, nothing is corrected yet: the reads to be corrected, asked about their k-mers' counts
        kept: dict = {}
        kmer_set = build_set(args, kept)
        if counts_path is not None:
            try:
                if not kept["counter"].lookup_ready:  # the partitioned counter (build_set): its count file is its count view
                    kept["counter"].prepare_lookup()
                with open(counts_path, "wb") as f:
                    kept["counter"].save(f, 1 if args.save_min_count is None else args.save_min_count)
            except _lib.BrxError as e:
                raise SystemExit(f"Error: --save-counts: {e}")
        for src, dst in zip(args.inputs, abund_paths or []):
            with open_input(src) as f, open(dst, "wb") as rep:
                write_abundance_report(kept["counter"], kept["threshold"], f, rep, args.record_buffer or 8192)
        kept.clear()  # (the counter's memory goes back before the correction starts)
    if args.set_ops:
        kmer_set = apply_set_ops(kmer_set, args.set_ops, args.device)
    if args.save_set is not None:
        with open(args.save_set, "wb") as f:
            kmer_set.save_keys(f)
    names = args.corrections or METHOD_NAMES                          # src/cli.rs:121-131: all five by default
    confirm = 5 if args.confirm is None else args.confirm            # src/cli.rs:135-137
    max_search = 7 if args.max_search is None else args.max_search   # src/cli.rs:140-142
    methods = build_methods(names, kmer_set, confirm, max_search)
    inputs = [open_input(p) for p in args.inputs] if args.inputs else [sys.stdin.buffer]
    outputs = [open(p, "wb") for p in args.outputs] if args.outputs else [io.BufferedWriter(sys.stdout.buffer)]
    reports = [open(p, "wb") for p in report_paths] if report_paths else None
    try:
        run_correction(inputs, outputs, methods, args.two_side, args.record_buffer or 8192, output_mode=mode, min_len=split_min,
                       reports=reports, second_pass=second_pass if args.second_pass is not None else None)
    finally:
        for f in outputs + (reports or []):
            f.flush()
        for f in inputs + outputs + (reports or []):
            if f not in (sys.stdin.buffer,):
                try:
                    f.close()
                except Exception:
                    pass
    return 0


if __name__ == "__main__":
    sys.exit(main())
