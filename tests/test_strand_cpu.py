"""The second scan on the reverse complement, without a GPU: the byte map (br_amd/strand.py), the argument checks of
Chain / run_correction / the CLI parser, and the quality claim that motivates the mode, pinned on the CPU oracle alone.

The expected bytes of the mode are the existing oracle plus the byte map:
    rc(correct_record(M, rc(correct_record(M, s, two_side=True)), two_side=True))
"""
import io

import numpy as np
import pytest

from br_amd import cli, strand
from br_amd.correct import Chain
from br_amd.driver import run_correction
from oracle import oracle as O

TABLE = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def rc_oracle(methods, seq):
    """the revcomp mode of a chain, composed from the oracle's single scan"""
    first = O.correct_record(methods, seq, two_side=True)
    return strand.revcomp(O.correct_record(methods, strand.revcomp(first), two_side=True))


def test_revcomp_is_an_involution_on_any_bytes():
    rng = np.random.default_rng(7)
    cases = [b"", b"A", b"ACGT", b"acgtn", b"ACGTNacgtnRYKM-*", bytes(range(256)), bytes(range(255, -1, -1))]
    cases += [rng.integers(0, 256, size=int(n), dtype=np.uint8).tobytes() for n in rng.integers(0, 400, size=50)]
    cases += [bytes(rng.choice(np.frombuffer(b"ACGTacgtNn", dtype=np.uint8), size=int(n))) for n in rng.integers(0, 400, size=50)]
    for s in cases:
        r = strand.revcomp(s)
        assert isinstance(r, bytes) and len(r) == len(s)
        assert strand.revcomp(r) == s


def test_revcomp_is_translate_and_reverse():
    rng = np.random.default_rng(8)
    assert strand.revcomp(b"AACGTtgcaNx\x00\xff") == b"\xff\x00xNtgcaACGTT"
    for n in rng.integers(0, 300, size=100):
        s = rng.integers(0, 256, size=int(n), dtype=np.uint8).tobytes()
        assert strand.revcomp(s) == s.translate(TABLE)[::-1]
        a = strand.revcomp(np.frombuffer(s, dtype=np.uint8))
        assert isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.tobytes() == s.translate(TABLE)[::-1]
    assert strand.SECOND_PASS == {"none", "reverse", "revcomp"}


def test_mode_resolution():
    assert strand.resolve_second_pass(None, False) == "reverse"
    assert strand.resolve_second_pass(None, True) == "none"
    assert strand.resolve_second_pass("none", True) == "none"
    assert strand.resolve_second_pass("none", False) == "none"
    assert strand.resolve_second_pass("revcomp", False) == "revcomp"
    with pytest.raises(ValueError):
        strand.resolve_second_pass("revcomp", True)
    with pytest.raises(ValueError):
        strand.resolve_second_pass("reverse", True)
    with pytest.raises(ValueError):
        strand.resolve_second_pass("complement", False)


def test_chain_and_run_correction_check_their_arguments_before_touching_the_gpu():
    # (the checks come first: neither call gets as far as the set, so None stands in for it)
    with pytest.raises(ValueError, match="contradicts"):
        Chain(None, [("one", 5, 7)], two_side=True, second_pass="revcomp")
    with pytest.raises(ValueError, match="second_pass"):
        Chain(None, [("one", 5, 7)], second_pass="both")
    with pytest.raises(ValueError, match="contradicts"):
        run_correction([io.BytesIO(b"")], [io.BytesIO()], [], True, second_pass="reverse")
    with pytest.raises(ValueError, match="second_pass"):
        run_correction([io.BytesIO(b"")], [io.BytesIO()], [], False, second_pass="rc")


def test_cli_parser():
    base = ["-i", "a.fa", "-o", "b.fa"]
    tail = ["solid", "-i", "x.solid", "-f", "solid"]
    p = cli.parser()
    a = p.parse_args(base + tail)
    assert a.second_pass is None and cli.second_pass_of(a) == "reverse"
    a = p.parse_args(base + ["-s"] + tail)
    assert cli.second_pass_of(a) == "none"
    for mode in ("reverse", "revcomp", "none"):
        a = p.parse_args(base + ["--second-pass", mode] + tail)
        assert cli.second_pass_of(a) == mode
    a = p.parse_args(base + ["-s", "--second-pass", "none"] + tail)
    assert cli.second_pass_of(a) == "none"
    for mode in ("reverse", "revcomp"):
        a = p.parse_args(base + ["-s", "--second-pass", mode] + tail)
        with pytest.raises(SystemExit) as e:
            cli.second_pass_of(a)
        assert "--second-pass" in str(e.value) and "-s" in str(e.value)
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--second-pass", "both"] + tail)
    # the mode combines with the output forms
    a = p.parse_args(base + ["--second-pass", "revcomp", "--mask-weak", "--cover-report", "r.tsv"] + tail)
    assert cli.output_form(a) == ("mask", 0, ["r.tsv"]) and cli.second_pass_of(a) == "revcomp"
    a = p.parse_args(base + ["--second-pass", "revcomp", "--trim-split", "50"] + tail)
    assert cli.output_form(a) == ("split", 50, None)


# ---- the quality claim -------------------------------------------------------------------------------------------------
# numpy default_rng(0xB12): 100 000 i.i.d. bases; 1 300 reads of 3 000 reference bases, strand +/- with p = 1/2; per-base
# errors: substitution 2 %, insertion 1.5 %, deletion 1.5 %; k = 13, dense count, abundance 3; the first 300 reads corrected.
# Measured with these numbers: One 0.83 (none) / 0.83 (reverse) / 0.87 (revcomp); all five 0.94 / 0.92 / 0.98.
K, ABUNDANCE, N_READS, N_CORRECTED = 13, 3, 1300, 300


def synthetic():
    rng = np.random.default_rng(0xB12)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    genome = acgt[rng.integers(0, 4, size=100_000)]
    reads = []
    for _ in range(N_READS):
        start = int(rng.integers(0, genome.size - 3000 + 1))
        ref = genome[start:start + 3000]
        if rng.random() < 0.5:
            ref = strand.revcomp(ref)
        u = rng.random(ref.size)
        out = []
        for b, x in zip(ref.tolist(), u.tolist()):
            if x < 0.02:                      # substitution: one of the three other bases
                out.append(int(acgt[(int(np.searchsorted(acgt, b)) + 1 + int(rng.integers(0, 3))) % 4]))
            elif x < 0.035:                   # insertion in front of the base
                out.append(int(acgt[int(rng.integers(0, 4))]))
                out.append(b)
            elif x < 0.05:                    # deletion
                continue
            else:
                out.append(b)
        reads.append(bytes(out))
    return genome.tobytes(), reads


@pytest.fixture(scope="module")
def world():
    genome, reads = synthetic()
    solid = O.Solid.from_count(K, O.count_reads(K, reads), ABUNDANCE)
    truth = O.Solid(K)
    truth.set_seq(genome)  # (the bitset is canonical: the k-mers of either strand)
    return solid, truth, reads[:N_CORRECTED]


def genome_fraction(truth, reads):
    good = total = 0
    for r in reads:
        total += max(len(r) - K + 1, 0)
        good += int(np.unpackbits(truth.mask(r)).sum())
    return good / total


@pytest.mark.parametrize("names", [["one"], ["one", "two", "graph", "greedy", "gap_size"]], ids=["one", "all_five"])
def test_second_scan_on_the_other_strand_recovers_more_genome_kmers(world, names):
    solid, truth, reads = world
    methods = O.build_methods(solid, names, 5, 7)
    frac = {"input": genome_fraction(truth, reads),
            "none": genome_fraction(truth, [O.correct_record(methods, r, two_side=True) for r in reads]),
            "reverse": genome_fraction(truth, [O.correct_record(methods, r, two_side=False) for r in reads]),
            "revcomp": genome_fraction(truth, [rc_oracle(methods, r) for r in reads])}
    print("genome k-mer fraction", names, {k: round(v, 4) for k, v in frac.items()})
    assert frac["none"] > frac["input"]
    assert frac["revcomp"] > frac["none"]
    assert frac["revcomp"] > frac["reverse"]
