"""K-mer text as br_amd/kmertext.py states it: hand-written strings, the round trip in both strand modes, summing,
saturation, the spellings a reader accepts and every cause of a refusal with its line.  No GPU, no library."""
import numpy as np
import pytest

from br_amd import kmertext
from br_amd.set import seq2bit

COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s: bytes) -> bytes:
    return s.translate(COMP)[::-1]


def key_of(s: bytes) -> int:
    """canonical(k-mer) >> 1 by the definition: the strand with an even number of set bits"""
    f = seq2bit(s)
    c = f if bin(f).count("1") % 2 == 0 else seq2bit(revcomp(s))
    assert bin(c).count("1") % 2 == 0
    return c >> 1


def u64(v):
    return np.asarray(v, dtype=np.uint64)


def u8(v):
    return np.asarray(v, dtype=np.uint8)


def sample(k, n, seed):
    """n distinct ascending keys at k with both ends of the key space, and counts on both sides of every digit border"""
    rng = np.random.default_rng(seed)
    top = (1 << (2 * k - 1)) - 1
    keys = np.unique(np.concatenate([u64([0, 1, top - 1, top]), rng.integers(0, top, n, dtype=np.uint64, endpoint=True)]))
    counts = rng.choice(u8([1, 9, 10, 99, 100, 255]), keys.size)
    return keys, counts


def test_hand_written_lines():
    assert kmertext.format_lines(5, u64([0]), u8([1])) == b"AAAAA\t1\n"
    assert kmertext.format_lines(5, u64([0]), u8([1]), "canonical") == b"AAAAA\t1\n"
    # ACGTA: A C G T A = 0 1 3 2 0 -> 0b0001111000, four bits set: canonical as it stands, key = that >> 1
    assert seq2bit(b"ACGTA") == 0b0001111000 and key_of(b"ACGTA") == 0b000111100
    assert kmertext.format_lines(5, u64([0b000111100]), u8([12]), "canonical") == b"ACGTA\t12\n"
    assert kmertext.format_lines(5, u64([0, 0b000111100]), u8([255, 100])) == b"AAAAA\t255\nACGTA\t100\n"
    assert kmertext.line_lengths(5, u8([1, 9, 10, 99, 100, 255])).tolist() == [8, 8, 9, 9, 10, 10]


def test_a_canonical_member_that_is_the_larger_strand_prints_differently():
    # TTTTG = 2 2 2 2 3: six bits set, so it is canonical; its reverse complement CAAAA comes first in the alphabet
    s = b"TTTTG"
    assert bin(seq2bit(s)).count("1") % 2 == 0 and revcomp(s) == b"CAAAA"
    key = u64([key_of(s)])
    assert kmertext.format_lines(5, key, u8([3]), "canonical") == b"TTTTG\t3\n"
    assert kmertext.format_lines(5, key, u8([3]), "lex") == b"CAAAA\t3\n"
    assert kmertext.format_lines(5, key, u8([3])) == b"CAAAA\t3\n"  # lex is the default
    for text in (b"TTTTG\t3\n", b"CAAAA\t3\n"):
        k, keys, counts = kmertext.parse(text)
        assert (k, keys.tolist(), counts.tolist()) == (5, key.tolist(), [3])


def test_lex_is_the_smaller_string_and_g_sorts_before_t():
    rng = np.random.default_rng(5)
    for k in (5, 19, 31):
        keys = np.unique(rng.integers(0, 1 << (2 * k - 1), 300, dtype=np.uint64))
        lex = kmertext.format_lines(k, keys, np.ones(keys.size, np.uint8), "lex").split(b"\n")[:-1]
        can = kmertext.format_lines(k, keys, np.ones(keys.size, np.uint8), "canonical").split(b"\n")[:-1]
        differ = 0
        for key, a, b in zip(keys.tolist(), lex, can):
            a, b = a.split(b"\t")[0], b.split(b"\t")[0]
            assert key_of(b) == key and bin(seq2bit(b)).count("1") % 2 == 0
            assert a == min(b, revcomp(b))
            differ += a != b
        assert 0 < differ < keys.size


@pytest.mark.parametrize("k", [5, 19, 31])
@pytest.mark.parametrize("strand", ["lex", "canonical"])
def test_round_trip(k, strand):
    keys, counts = sample(k, 2000, k)
    assert int(keys[-1]) == (1 << (2 * k - 1)) - 1
    text = kmertext.format_lines(k, keys, counts, strand)
    assert len(text) == int(kmertext.line_lengths(k, counts).sum())
    for given in (None, k):
        got_k, got_keys, got_counts = kmertext.parse(text, given)
        assert got_k == k and np.array_equal(got_keys, keys) and np.array_equal(got_counts, counts)
    pk, pkeys, pcounts, numbers = kmertext.parse_lines(text)
    assert np.array_equal(pkeys, keys) and np.array_equal(pcounts, counts) and numbers.tolist() == list(range(1, keys.size + 1))


def test_lines_in_any_order_come_back_sorted():
    keys, counts = sample(19, 500, 1)
    lines = kmertext.format_lines(19, keys, counts).split(b"\n")[:-1]
    order = np.random.default_rng(2).permutation(len(lines))
    text = b"".join(lines[i] + b"\n" for i in order)
    _, got_keys, got_counts = kmertext.parse(text)
    assert np.array_equal(got_keys, keys) and np.array_equal(got_counts, counts)
    _, raw_keys, _, _ = kmertext.parse_lines(text)
    assert np.array_equal(raw_keys, keys[order])


def test_sums_and_saturation():
    key = key_of(b"TTTTG")
    for text, want in ((b"TTTTG\t3\nCAAAA\t4\n", 7), (b"TTTTG\t200\nAAAAA\t1\nTTTTG\t100\n", 255), (b"TTTTG\t1000\n", 255),
                       (b"TTTTG\t007\n", 7), (b"TTTTG\t255\n", 255), (b"TTTTG\t256\n", 255), (b"TTTTG\t" + b"9" * 5000 + b"\n", 255),
                       (b"TTTTG\t000000000000000000000000012\n", 12), (b"CAAAA\t1\n" * 300, 255), (b"CAAAA\t1\n" * 200, 200)):
        k, keys, counts = kmertext.parse(text)
        at = keys.tolist().index(key)
        assert k == 5 and int(counts[at]) == want, text[:40]
        assert np.all(keys[1:] > keys[:-1])


def test_spellings_a_reader_accepts():
    want = kmertext.parse(b"ACGTA\t12\nTTTTG\t3\n")
    for text in (b"acgta\t12\nttttg\t3\n", b"AcGtA \t  12\nTTTTG   3\n", b"ACGTA\t12\r\nTTTTG\t3\r\n", b"ACGTA\t12\nTTTTG\t3",
                 b"ACGTA\t12\nTTTTG\t3\r", b"\n\nACGTA\t12\n\n\r\nTTTTG\t3\n\n", b"ACGTA 12\nTTTTG 3\n"):
        got = kmertext.parse(text)
        assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), text
    k, keys, counts, numbers = kmertext.parse_lines(b"\n\nACGTA\t12\n\n\r\nTTTTG\t3\n\n")
    assert numbers.tolist() == [3, 6]


def test_empty_texts():
    for text in (b"", b"\n", b"\r\n\n"):
        with pytest.raises(ValueError, match="tells no k"):
            kmertext.parse(text)
        k, keys, counts = kmertext.parse(text, 7)
        assert k == 7 and keys.size == 0 and counts.size == 0 and keys.dtype == np.uint64 and counts.dtype == np.uint8
    assert kmertext.format_lines(7, u64([]), u8([])) == b""


@pytest.mark.parametrize("text, k, message", [
    (b"ACGTA\t1\nACXTA\t1\n", None, "line 2: column 3 is no base"),
    (b"\n\nACGTA\t1\n\nACGT\t1\n", None, "line 5: a k-mer of 4 bases is shorter than k=5"),
    (b"ACGTA\t1\nACGTAC\t1\n", None, "line 2: a k-mer of 6 bases is longer than k=5"),
    (b"ACGTA\t1\nACGTACG\t1\n", 5, "line 2: a k-mer of 7 bases is longer than k=5"),
    (b"ACGTA\t1\n\t1\n", None, "line 2: a k-mer of 0 bases is shorter than k=5"),
    (b"ACGTA\t1\nACGTA\n", None, "line 2: no count after the k-mer"),
    (b"ACGTA\t1\nACGTA\t \n", None, "line 2: no count after the k-mer"),
    (b"ACGTA\t1\nACGTA\t1x\n", None, "line 2: column 8 is no digit"),
    (b"ACGTA\t1\nACGTA\t-1\n", None, "line 2: column 7 is no digit"),
    (b"ACGTA\t1\nACGTA\t1 \n", None, "line 2: column 8 is no digit"),
    (b"ACGTA\t1\nACGTA\t1\r\r\n", None, "line 2: column 8 is no digit"),
    (b"ACGTA\t1\r\nACGTA\t0\r\n", None, "line 2: a count of 0"),
    (b"ACGTA\t1\nACGTA\t000\n", None, "line 2: a count of 0"),
    (b"ACGTA\t1\n1\tACGTA\n", None, "line 2: column 1 is no base"),
    (b"ACGT\t1\n", None, "line 1: a k-mer of 4 bases gives no k"),
    (b"\nACGTAC\t1\n", None, "line 2: a k-mer of 6 bases gives no k"),
    (b"A" * 33 + b"\t1\n", None, "line 1: a k-mer of 33 bases gives no k"),
    (b"ACGTA\t1\n", 7, "line 1: a k-mer of 5 bases is shorter than k=7"),
])
def test_every_cause_names_its_line(text, k, message):
    with pytest.raises(ValueError) as e:
        kmertext.parse(text, k)
    assert str(e.value).startswith(message), str(e.value)


def test_floor():
    text = b"ACGTA\t5\nTTTTG\t1\nAAAAA\t3\nCAAAA\t1\n"
    with pytest.raises(ValueError) as e:
        kmertext.parse(text, floor=3)
    assert str(e.value) == "line 2: a count of 2 below the floor 3"
    k, keys, counts = kmertext.parse(b"ACGTA\t5\nTTTTG\t1\nAAAAA\t3\nCAAAA\t2\n", floor=3)
    assert sorted(counts.tolist()) == [3, 3, 5]
    for bad in (0, 256):
        with pytest.raises(ValueError, match="floor"):
            kmertext.parse(text, floor=bad)


def test_arguments():
    for k in (4, 3, 33, 6):
        with pytest.raises(ValueError, match="odd k"):
            kmertext.format_lines(k, u64([0]), u8([1]))
        with pytest.raises(ValueError, match="odd k"):
            kmertext.parse(b"", k)
    with pytest.raises(ValueError, match="strand"):
        kmertext.format_lines(5, u64([0]), u8([1]), "forward")
    with pytest.raises(ValueError, match="one count per key"):
        kmertext.format_lines(5, u64([0, 1]), u8([1]))
