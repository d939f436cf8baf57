"""K-mer text on the GPU path (include/brx.h "k-mer text", br_amd/csrc/brx_kmertext.hip) against br_amd/kmertext.py: the raw
format and parse entries at the shapes where a block scan, a shared 16-byte chunk or a line index can go wrong, their stream
order, the objects through 4 KiB pieces, the run-sum across block borders, floors, from_arrays, a counter's list through
text and back, import errors with the line of the whole stream, and the command.  Every comparison is exact."""
import gzip
import io
import os
import threading

import numpy as np
import pytest
import torch

import br_amd
from br_amd import _lib, keyfile, kmertext
from br_amd.set import CountList, format_kmertext_device, parse_kmertext_device
from tests.test_gpu_streams import Lane, decoy, lane, operation, probe, ptr, reads  # noqa: F401

pytestmark = pytest.mark.gpu

SENT = 0xEE
KEY_SENTINEL = -0x1111111111111112  # 0xEEEE... as int64
SIZES = [0, 1, 255, 256, 257, 2 * 256 + 3, 5000]
KS = [5, 19, 31]
COUNT_PICKS = np.array([1, 9, 10, 99, 100, 255], dtype=np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")
_cache = {}


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy((a.view(np.int64) if a.dtype == np.uint64 else a).copy()).cuda()


def entries(k, n, seed=0):
    """n entries in no order, repeats allowed (the raw entries take what they are given), both ends of the key space among
    them, counts on both sides of every digit border so that neighbouring blocks differ in bytes; computed once"""
    key = (k, n, seed)
    if key not in _cache:
        rng = np.random.default_rng(1000 * k + n + seed)
        top = (1 << (2 * k - 1)) - 1
        keys = rng.integers(0, top, n, dtype=np.uint64, endpoint=True)
        if n >= 2:
            keys[0], keys[-1] = 0, top
        _cache[key] = (keys, rng.choice(COUNT_PICKS, n))
    return _cache[key]


def sorted_list(k, n, seed=0):
    """distinct ascending keys (about n) with counts: the arrays of a count list"""
    keys, counts = entries(k, n, seed)
    keys, first = np.unique(keys, return_index=True)
    return keys, counts[first]


def run_format(k, keys, counts, strand, cap=None, shift=0, stream=None):
    """(bytes_out, the text, what lies behind it) of the raw entry; the buffer is pre-filled with the sentinel and starts
    `shift` bytes behind an aligned address"""
    dk, dc = dev(keys), dev(counts)
    need = int(kmertext.line_lengths(k, counts).sum())
    cap = need + 64 if cap is None else cap
    buf = torch.full((shift + max(cap, 1) + 64,), SENT, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        n = format_kmertext_device(k, dk.data_ptr() if keys.size else None, dc.data_ptr() if keys.size else None, keys.size,
                                   buf.data_ptr() + shift, cap, strand, stream)
    finally:
        torch.cuda.synchronize()
        run_format.left = buf.cpu().numpy()
    whole = run_format.left
    assert (whole[:shift] == SENT).all()
    return n, whole[shift:shift + n].tobytes(), whole[shift + n:]


# ---- format ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strand", ["lex", "canonical"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", SIZES)
def test_format_is_format_lines(n, k, strand):
    keys, counts = entries(k, n)
    want = kmertext.format_lines(k, keys, counts, strand)
    got_n, text, behind = run_format(k, keys, counts, strand)
    assert got_n == len(want) and text == want
    assert (behind == SENT).all()


@pytest.mark.parametrize("shift", [1, 7, 15, 16, 33])
def test_format_into_a_buffer_at_any_alignment(shift):
    keys, counts = entries(19, 2 * 256 + 3)
    want = kmertext.format_lines(19, keys, counts)
    got_n, text, behind = run_format(19, keys, counts, "lex", shift=shift)
    assert got_n == len(want) and text == want and (behind == SENT).all()


def test_format_blocks_loop_over_their_trips(monkeypatch):
    monkeypatch.setenv("BRX_READ_GRID", "3")
    keys, counts = entries(31, 5000)
    got_n, text, behind = run_format(31, keys, counts, "lex")
    assert text == kmertext.format_lines(31, keys, counts) and (behind == SENT).all()


def test_format_cap_one_byte_short_is_refused_untouched():
    for n in (1, 257, 5000):
        keys, counts = entries(19, n)
        need = int(kmertext.line_lengths(19, counts).sum())
        with pytest.raises(_lib.BrxError) as e:
            run_format(19, keys, counts, "lex", cap=need - 1)
        assert e.value.status == _lib.BRX_ERR_ARG and e.value.needed == need
        assert (run_format.left == SENT).all()
        assert run_format(19, keys, counts, "lex", cap=need)[1] == kmertext.format_lines(19, keys, counts)
    dk, dc = dev(entries(19, 257)[0]), dev(entries(19, 257)[1])
    with pytest.raises(_lib.BrxError) as e:  # sizes only
        format_kmertext_device(19, dk.data_ptr(), dc.data_ptr(), 257, None, 0)
    assert e.value.needed == int(kmertext.line_lengths(19, entries(19, 257)[1]).sum())
    for k, strand in ((6, 0), (33, 0), (19, 2)):
        with pytest.raises(_lib.BrxError) as e:
            format_kmertext_device(k, dk.data_ptr(), dc.data_ptr(), 257, None, 0, strand)
        assert e.value.status == _lib.BRX_ERR_ARG


# ---- parse -----------------------------------------------------------------------------------------------------------------
def respell(text, seed):
    """the same entries in the odd but legal spellings: lower case, several separators, CRLF, blank lines, leading zeros,
    counts above 255, the other strand, no final newline"""
    rng = np.random.default_rng(seed)
    out = []
    for i, line in enumerate(text.split(b"\n")[:-1]):
        kmer, count = line.split(b"\t")
        r = rng.integers(0, 16)
        if r & 1:
            kmer = kmer.lower()
        if i % 5 == 2:
            kmer = kmer.translate(COMP)[::-1] if not r & 1 else kmer.upper().translate(COMP)[::-1].lower()
        if r & 2:
            count = b"000" + count
        if count == b"255" and r & 4:
            count = [b"256", b"1000", b"99999999999999999999999999"][i % 3]
        sep = [b"\t", b" ", b"\t\t ", b"   \t"][int(rng.integers(0, 4))]
        out.append(kmer + sep + count + (b"\r" if r & 8 else b""))
        if i % 17 == 3:
            out.append(b"")
        if i % 29 == 5:
            out.append(b"\r")
    return b"\n".join(out) + (b"\n" if seed & 1 else b"")


def run_parse(text, k, cap=None, shift=0, stream=None):
    """(n, keys, counts) of the raw entry over `text`, placed `shift` bytes behind an aligned address"""
    buf = torch.full((shift + max(len(text), 1),), SENT, dtype=torch.uint8, device="cuda")
    if text:
        buf[shift:shift + len(text)] = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    cap = text.count(b"\n") + 1 if cap is None else cap
    kout = torch.full((max(cap, 1),), KEY_SENTINEL, dtype=torch.int64, device="cuda")
    cout = torch.full((max(cap, 1),), SENT, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        n = parse_kmertext_device(buf.data_ptr() + shift if text else None, len(text), k, kout.data_ptr(), cout.data_ptr(), cap, stream)
    finally:
        torch.cuda.synchronize()
        run_parse.left = (kout.cpu().numpy(), cout.cpu().numpy())
    wk, wc = run_parse.left
    assert (wk[n:] == KEY_SENTINEL).all() and (wc[n:] == SENT).all()
    return n, wk[:n].view(np.uint64), wc[:n]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", SIZES)
def test_parse_is_parse_lines(n, k):
    keys, counts = entries(k, n)
    for strand, seed in (("lex", 1), ("canonical", 2)):
        plain = kmertext.format_lines(k, keys, counts, strand)
        for text, shift in ((plain, 0), (respell(plain, seed + n), seed)):  # (shift 1: the text starts off a 16-byte border)
            got_n, gk, gc = run_parse(text, k, shift=shift)
            if n:
                _, wk, wc, _ = kmertext.parse_lines(text, k)
                assert np.array_equal(wk, keys) and np.array_equal(wc, counts)  # (the spellings change no entry)
            assert got_n == n and np.array_equal(gk, keys) and np.array_equal(gc, counts)


def test_parse_blank_texts_and_cap():
    for text in (b"", b"\n", b"\r\n\n\n", b"\n" * 5000):
        assert run_parse(text, 19)[0] == 0
    keys, counts = entries(19, 257)
    text = kmertext.format_lines(19, keys, counts)
    with pytest.raises(_lib.BrxError) as e:
        run_parse(text, 19, cap=256)
    assert e.value.status == _lib.BRX_ERR_ARG and e.value.needed == 257
    assert (run_parse.left[0] == KEY_SENTINEL).all() and (run_parse.left[1] == SENT).all()
    assert run_parse(text, 19, cap=257)[0] == 257


BAD_LINES = [  # (line, cause, column) at k = 19
    (b"ACGTACGTANACGTACGTA\t3", kmertext.CAUSE_BASE, 10),
    (b"ACGTACGTACGTACGTA\t3", kmertext.CAUSE_SHORT, 17),
    (b"\t3", kmertext.CAUSE_SHORT, 0),
    (b"ACGTACGTACGTACGTACGTA\t3", kmertext.CAUSE_LONG, 21),
    (b"ACGTACGTACGTACGTACG", kmertext.CAUSE_NOCOUNT, 0),
    (b"ACGTACGTACGTACGTACG \t", kmertext.CAUSE_NOCOUNT, 0),
    (b"ACGTACGTACGTACGTACG\t3x", kmertext.CAUSE_DIGIT, 22),
    (b"ACGTACGTACGTACGTACG\t3 ", kmertext.CAUSE_DIGIT, 22),
    (b"ACGTACGTACGTACGTACG\t-3", kmertext.CAUSE_DIGIT, 21),
    (b"ACGTACGTACGTACGTACG\t000", kmertext.CAUSE_ZERO, 0),
]


@pytest.mark.parametrize("bad, cause, col", BAD_LINES)
def test_parse_reports_the_first_malformed_line(bad, cause, col):
    k = 19
    keys, counts = entries(k, 2000)
    lines = kmertext.format_lines(k, keys, counts).split(b"\n")[:-1]
    lines[3] = b""  # empty lines are counted
    for first, second in ((700, 1900), (255, 256), (0, 1999), (1999, None)):
        mine = list(lines)
        mine[first] = bad
        if second is not None:
            mine[second] = b"ACGTACGTACGTACGTACG\t0"  # another cause, in a later block
        text = b"\n".join(mine) + b"\n"
        with pytest.raises(_lib.BrxError) as e:
            run_parse(text, k)
        assert e.value.status == _lib.BRX_ERR_FORMAT and e.value.needed == 0
        assert e.value.err3 == (cause, first, col)
        with pytest.raises(ValueError) as want:
            kmertext.parse_lines(text, k)
        assert str(e.value).endswith("k-mer text: " + str(want.value)) and f"line {first + 1}:" in str(e.value)


# ---- stream order of the raw entries -----------------------------------------------------------------------------------------
def test_raw_entries_read_their_inputs_in_stream_order(lane):
    """the arrays hold a decoy of identical sizes until the lane's delay has run: the answers are the real ones'"""
    k = 25
    keys, counts = sorted_list(k, 3000, 1)
    other = sorted_list(k, 3000, 2)[0][:keys.size]
    assert other.size == keys.size
    real = {"keys": keys, "counts": counts}
    fake = {"keys": other, "counts": counts[::-1].copy()}

    @operation(lambda arrays: {"text": (arrays["keys"].size * (k + 5), "uint8")})
    def op_format(ctx, inp, out):
        n = format_kmertext_device(k, ptr(inp["keys"]), ptr(inp["counts"]), inp["keys"].numel(), ptr(out["text"]), out["text"].numel(), "lex",
                                   ctx.stream)
        return n, ctx.fetch(out["text"])[:n].tobytes()

    n, text = probe(lane, op_format, fake, real)
    assert text == kmertext.format_lines(k, keys, counts) and n > 50000

    real_t = np.frombuffer(kmertext.format_lines(k, keys, counts, "canonical"), dtype=np.uint8)
    fake_t = np.frombuffer(kmertext.format_lines(k, other, counts, "canonical"), dtype=np.uint8)

    @operation(lambda arrays: {"k": (keys.size, "int64"), "c": (keys.size, "uint8")})
    def op_parse(ctx, inp, out):
        n = parse_kmertext_device(ptr(inp["text"]), inp["text"].numel(), k, ptr(out["k"]), ptr(out["c"]), out["k"].numel(), ctx.stream)
        return n, ctx.fetch(out["k"])[:n].tobytes(), ctx.fetch(out["c"])[:n].tobytes()

    n, gk, gc = probe(lane, op_parse, {"text": fake_t}, {"text": real_t})
    assert n == keys.size and gk == keys.tobytes() and gc == counts.tobytes()


# ---- objects ---------------------------------------------------------------------------------------------------------------
@pytest.fixture
def small_pieces(monkeypatch):
    """4 KiB pieces: a few thousand entries cross dozens of slice and carry borders"""
    monkeypatch.setenv("BRX_KEYFILE_SLICE_KB", "4")


def dumped(lst, *args):
    f = io.BytesIO()
    lst.stats = lst.dump_text(f, *args)
    return f.getvalue()


def saved(lst, *args):
    f = io.BytesIO()
    lst.save(f, *args)
    return f.getvalue()


def same_arrays(lst, keys, counts):
    gk, gc = lst.to_numpy()
    return lst.n == keys.size and np.array_equal(gk, keys) and np.array_equal(gc, counts)


def other_strand(line):
    kmer, count = line.split(b"\t")
    return kmer.translate(COMP)[::-1] + b"\t" + count


def test_dump_and_import_through_small_pieces(small_pieces):
    k = 25
    keys, counts = sorted_list(k, 5000)
    lst = CountList.from_arrays(k, keys, counts)
    for strand in ("lex", "canonical"):
        text = dumped(lst, 1, strand)
        assert text == kmertext.format_lines(k, keys, counts, strand)
        assert lst.stats["entries"] == keys.size and lst.stats["bytes"] == len(text) and lst.stats["slices"] > 30
        for given in (None, k):
            back = CountList.from_text(io.BytesIO(text), given)
            assert back.k == k and back.floor == 1 and same_arrays(back, keys, counts) and not back.text_stats["sorted"]
            assert back.text_stats["lines"] == keys.size and back.text_stats["bytes"] == len(text)
    keep = counts >= 10
    assert dumped(lst, 10) == kmertext.format_lines(k, keys[keep], counts[keep])
    lines = text.split(b"\n")[:-1]
    rng = np.random.default_rng(3)
    shuffled = b"".join(lines[i] + b"\n" for i in rng.permutation(len(lines)))
    back = CountList.from_text(io.BytesIO(shuffled))
    assert same_arrays(back, keys, counts) and back.text_stats["sorted"]
    flipped = b"\n".join(other_strand(l) if rng.random() < 0.5 else l for l in lines)  # (no final newline)
    assert same_arrays(CountList.from_text(io.BytesIO(flipped)), keys, counts)
    assert same_arrays(CountList.from_text(io.BytesIO(respell(text, 8)), k), keys, counts)
    assert same_arrays(CountList.from_text(gzip.GzipFile(fileobj=io.BytesIO(gzip.compress(shuffled)))), keys, counts)
    r, w = os.pipe()

    def feed():
        with os.fdopen(w, "wb", buffering=0) as f:
            for at in range(0, len(shuffled), 997):
                f.write(shuffled[at:at + 997])

    t = threading.Thread(target=feed)
    t.start()
    with os.fdopen(r, "rb") as f:
        back = CountList.from_text(f)
    t.join()
    assert same_arrays(back, keys, counts)


def test_default_pieces_and_empty_lists():
    k = 19
    keys, counts = sorted_list(k, 5000)
    lst = CountList.from_arrays(k, keys, counts)
    text = dumped(lst)
    assert text == kmertext.format_lines(k, keys, counts) and lst.stats["slices"] == 1
    assert same_arrays(CountList.from_text(io.BytesIO(text)), keys, counts)
    empty = CountList.from_arrays(k, [], [])
    assert empty.n == 0 and dumped(empty) == b"" and saved(empty) == keyfile.encode(k, [], np.zeros(0, np.uint8), floor=1)
    for text in (b"", b"\n\r\n"):
        back = CountList.from_text(io.BytesIO(text), k, 4)
        assert back.n == 0 and back.k == k and back.floor == 4
        with pytest.raises(_lib.BrxError) as e:
            CountList.from_text(io.BytesIO(text))
        assert e.value.status == _lib.BRX_ERR_FORMAT and "tells no k" in str(e.value)


# ---- run-sum ---------------------------------------------------------------------------------------------------------------
def test_runs_longer_than_a_block_saturate_or_add_up(small_pieces):
    k = 25
    keys, counts = sorted_list(k, 700)
    lines = kmertext.format_lines(k, keys, counts).split(b"\n")[:-1]
    for at in (0, 350, keys.size - 1):  # the run at the front, in the middle, at the end of the sorted order
        for times, want in ((3000, 255), (200, 200)):
            rest = [l for i, l in enumerate(lines) if i != at]
            kmer = lines[at].split(b"\t")[0]
            mine = rest[:100] + [kmer + b"\t1"] * times + rest[100:]
            back = CountList.from_text(io.BytesIO(b"\n".join(mine) + b"\n"))
            expect = counts.copy()
            expect[at] = want
            assert same_arrays(back, keys, expect)
            wk, wc = kmertext.parse(b"\n".join(mine) + b"\n")[1:]
            assert np.array_equal(wk, keys) and np.array_equal(wc, expect)


def test_runs_of_two_across_every_block_border(small_pieces):
    k = 25
    uniq, _ = sorted_list(k, 5000)
    seq = []
    for key in uniq.tolist():  # the sorted order of the pairs: entries 256 j - 1 and 256 j are one key, for every j
        if seq and len(seq) % 256 == 0:
            seq.append(seq[-1])
        seq.append(key)
    seq = np.asarray(seq, dtype=np.uint64)
    assert all(seq[j] == seq[j - 1] for j in range(256, seq.size, 256)) and seq.size > 4096 + 256
    rng = np.random.default_rng(4)
    counts = rng.choice(np.array([1, 2, 100, 200], dtype=np.uint8), seq.size)
    counts[255:257] = 200  # one pair saturates whatever the draw
    lines = kmertext.format_lines(k, seq, counts).split(b"\n")[:-1]
    twins = np.flatnonzero(seq[1:] == seq[:-1]) + 1
    for i in twins[::2]:
        lines[i] = other_strand(lines[i])  # both strands listed apart
    wk, wc = kmertext.sum_runs(seq, counts)
    assert wk.size == uniq.size and (wc == 255).any()
    for text in (b"\n".join(lines), b"\n".join(lines[i] for i in rng.permutation(len(lines)))):
        back = CountList.from_text(io.BytesIO(text))
        assert same_arrays(back, wk, wc)


# ---- floor -----------------------------------------------------------------------------------------------------------------
def test_floor_is_checked_after_summing():
    head = b"ACGTACGTACGTACGTACGTACGTA\t7\n"
    one, other = b"T" * 24 + b"G\t", b"C" + b"A" * 24 + b"\t"  # the two strands of one 25-mer
    with pytest.raises(_lib.BrxError) as e:
        CountList.from_text(io.BytesIO(head + one + b"1\n" + other + b"1\n"), floor=3)
    assert e.value.status == _lib.BRX_ERR_FORMAT and "below the floor 3" in str(e.value) and "2 times" in str(e.value)
    lst = CountList.from_text(io.BytesIO(head + one + b"1\n" + other + b"2\n"), floor=3)
    assert lst.floor == 3 and lst.k == 25 and sorted(lst.to_numpy()[1].tolist()) == [3, 7]
    assert keyfile.decode(saved(lst))[3] == 3


# ---- from_arrays -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 19, 31])
def test_from_arrays_is_the_list_of_the_file(k):
    keys, counts = sorted_list(k, 3000 if k > 5 else 400)
    for floor in (1, 9):
        keep = counts >= floor
        data = keyfile.encode(k, keys[keep], counts[keep], floor=floor)
        a, b = CountList.from_arrays(k, keys[keep], counts[keep], floor), CountList.from_keyfile(io.BytesIO(data))
        assert (a.k, a.n, a.floor) == (b.k, b.n, b.floor) == (k, int(keep.sum()), floor)
        assert all(np.array_equal(x, y) for x, y in zip(a.to_numpy(), b.to_numpy()))
        assert np.array_equal(a.spectrum(), b.spectrum()) and saved(a) == data == saved(b)


def test_from_arrays_names_the_first_bad_index():
    k = 19
    keys, counts = sorted_list(k, 3000)

    def refused(keys_, counts_, floor, index, word):
        with pytest.raises(_lib.BrxError) as e:
            CountList.from_arrays(k, keys_, counts_, floor)
        assert e.value.status == _lib.BRX_ERR_ARG and f"index {index}:" in str(e.value) and word in str(e.value), str(e.value)

    for at in (1, 256, 2047):
        bad = keys.copy()
        bad[at], bad[at + 1] = keys[at + 1], keys[at]
        bad[2500] = bad[2499]  # a later fault does not win
        refused(bad, counts, 1, at + 1, "ascend")
        bad = keys.copy()
        bad[at] = bad[at - 1]
        refused(bad, counts, 1, at, "ascend")
        low = counts.copy()
        low[at], low[2900] = 0, 0
        refused(keys, low, 1, at, "floor")
    low = np.full(keys.size, 9, np.uint8)
    low[1234] = 8
    refused(keys, low, 9, 1234, "floor 9")
    bad = keys.copy()
    bad[-1] = 1 << (2 * k - 1)
    refused(bad, counts, 1, keys.size - 1, "not below")
    for bad_k in (4, 6, 33):
        with pytest.raises(_lib.BrxError) as e:
            CountList.from_arrays(bad_k, keys[:4], counts[:4])
        assert e.value.status == _lib.BRX_ERR_ARG


# ---- against a counter ---------------------------------------------------------------------------------------------------------
def test_a_counters_list_through_text_and_back():
    from br_amd import synth
    k, n_reads, read_len = 25, 300, 1000
    cfg = synth.config(genome_len=n_reads * read_len // 20, read_len=read_len)
    bases, offs = synth.reads_host(cfg, synth.genome_host(cfg), 0, n_reads)
    c = br_amd.Counter(k, 0, _lib.COUNT_TABLE)
    c.add_batch(bases, offs)
    want = saved(c)
    lst = CountList.from_counter(c)
    assert lst.n > 10000 and int(lst.to_numpy()[1].max()) > 10
    text = dumped(lst)
    back = CountList.from_text(io.BytesIO(text))
    assert saved(back) == want
    assert back.finish(2).fingerprint() == c.finish(2).fingerprint()


# ---- import errors -----------------------------------------------------------------------------------------------------------
def test_import_errors_leave_no_list_and_name_the_line_of_the_stream(small_pieces):
    k = 19
    keys, counts = sorted_list(k, 2000)
    lines = kmertext.format_lines(k, keys, counts).split(b"\n")[:-1]
    lines[10] = b""
    assert len(b"\n".join(lines[:1000])) > 5 * 4096  # line 1001 lies several pieces in
    for bad, cause, col in BAD_LINES:
        for at in (1000, len(lines) - 1):
            mine = list(lines)
            mine[at] = bad
            text = b"\n".join(mine) + (b"\n" if at == 1000 else b"")
            with pytest.raises(ValueError) as want:
                kmertext.parse(text)
            assert str(want.value).startswith(f"line {at + 1}: ")
            for given in (None, k):
                with pytest.raises(_lib.BrxError) as e:
                    CountList.from_text(io.BytesIO(text), given)
                assert e.value.status == _lib.BRX_ERR_FORMAT and str(e.value).endswith("k-mer text: " + str(want.value)), str(e.value)
    mine = list(lines)
    mine[1000] = b"A" * 5000
    with pytest.raises(_lib.BrxError) as e:
        CountList.from_text(io.BytesIO(b"\n".join(mine) + b"\n"))
    assert e.value.status == _lib.BRX_ERR_FORMAT and "line 1001: longer than a piece" in str(e.value)
    for first in (b"ACGTACGT\t1", b"ACG\t1", b"A" * 33 + b"\t1"):
        with pytest.raises(_lib.BrxError) as e:
            CountList.from_text(io.BytesIO(b"\n\n" + first + b"\n" + b"\n".join(lines) + b"\n"))
        assert e.value.status == _lib.BRX_ERR_FORMAT and f"line 3: a k-mer of {len(first) - 2} bases gives no k" in str(e.value)
    with pytest.raises(_lib.BrxError) as e:
        CountList.from_text(io.BytesIO(b"\n".join(lines)), 21)
    assert "line 1: a k-mer of 19 bases is shorter than k=21" in str(e.value)


# ---- command ---------------------------------------------------------------------------------------------------------------
def test_command_dump_then_import_reproduces_the_file(tmp_path, small_pieces):
    k = 25
    keys, counts = sorted_list(k, 5000)
    lst = CountList.from_arrays(k, keys, counts)
    src, txt, dst = tmp_path / "a.keys", tmp_path / "a.tsv", tmp_path / "b.keys"
    src.write_bytes(saved(lst))
    assert kmertext.main(["dump", str(src), "-o", str(txt)]) == 0
    assert txt.read_bytes() == kmertext.format_lines(k, keys, counts)
    assert kmertext.main(["import", str(txt), "-o", str(dst)]) == 0
    assert dst.read_bytes() == src.read_bytes()
    gz = tmp_path / "a.tsv.gz"
    gz.write_bytes(gzip.compress(txt.read_bytes()))
    assert kmertext.main(["dump", str(src), "-o", str(txt), "--min-count", "4", "--strand", "canonical"]) == 0
    keep = counts >= 4
    assert txt.read_bytes() == kmertext.format_lines(k, keys[keep], counts[keep], "canonical")
    assert kmertext.main(["import", str(txt), "-o", str(dst), "--floor", "4", "-k", "25"]) == 0
    assert dst.read_bytes() == saved(lst, 4)
    assert kmertext.main(["import", str(gz), "-o", str(dst)]) == 0
    assert dst.read_bytes() == src.read_bytes()
