"""The replay kernels of the lane form (lane_apply_kernel, lane_apply_walk_kernel in br_amd/csrc/brx_onelane.hip) put a
16-byte output chunk that holds fixes together in registers: one 16-byte load per stretch of copied bytes, the fixes'
bases between them, one aligned store.  These inputs aim at that path: fixes on every residue of the destination
address for every kind of fix, several fixes in one chunk, fixes in the first and last bytes of a read, short reads,
every alignment of input and slot, batches of more than 256 fixes, more than 128 units, bytes that are copied through
unchanged (lower case, N) beside fixes -- through One, the walking correctors and the reverse passes.

The expected bytes are the oracle's, whatever it does with a planted error.  That the oracle really makes fixes where
they are meant to fall is asserted first, on the CPU (the tests without the gpu mark), from the edit script between
a read and its corrected form."""
import difflib
import functools

import numpy as np
import pytest

import br_amd
from oracle import oracle as O

K, CONFIRM = 9, 2
SPACINGS = (3, 4, 5, 6, 8, 12, 40)
KINDS = ("sub", "del", "ins")     # what is planted: the corrector answers with used = 1, 0 (the read grows), 2 (it shrinks)
ANSWER = {"sub": "sub", "del": "grow", "ins": "shrink"}
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def genome():
    return np.random.default_rng(11).choice(ACGT, 12_000).tobytes()


@functools.lru_cache(maxsize=None)
def ref_set():
    ref = O.Solid(K)
    ref.set_seq(genome())
    return ref


def plant(read, kind, positions, rng):
    r = bytearray(read)
    for pos in sorted(positions, reverse=True):
        if kind == "sub":
            r[pos] = int(rng.choice([c for c in b"ACGT" if c != r[pos]]))
        elif kind == "del":
            del r[pos]
        else:
            r.insert(pos, int(rng.choice(ACGT)))
    return bytes(r)


@functools.lru_cache(maxsize=None)
def planted_reads(kind, spacing, n_reads=8, length=800):
    """stretches of the genome with an error of one kind every `spacing` bases, from base K on to the last bases"""
    rng = np.random.default_rng(1000 * KINDS.index(kind) + spacing)
    g = genome()
    reads = []
    for _ in range(n_reads):
        s = int(rng.integers(0, len(g) - length))
        first = K + int(rng.integers(0, spacing))
        reads.append(plant(g[s:s + length], kind, range(first, length - 3, spacing), rng))
    return tuple(reads)


@functools.lru_cache(maxsize=None)
def edits(inp, out):
    """[(kind, offset in out)] of the edit script inp -> out: sub, grow (a base put in), shrink (a base taken out)"""
    res = []
    for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, inp, out, autojunk=False).get_opcodes():
        if tag == "equal":
            continue
        common = min(i2 - i1, j2 - j1)
        res += [("sub", j1 + t) for t in range(common)]
        res += [("grow", j) for j in range(j1 + common, j2)]
        res += [("shrink", j1 + common)] * ((i2 - i1) - common)
    return res


@functools.lru_cache(maxsize=None)
def oracle_out(reads, names=("one",), two_side=False):
    om = O.build_methods(ref_set(), list(names), CONFIRM, 7)
    return tuple(O.correct_record(om, r, two_side) for r in reads)


def every_planted_read():
    return tuple(r for kind in KINDS for sp in SPACINGS for r in planted_reads(kind, sp))


@functools.lru_cache(maxsize=None)
def short_reads():
    """k - 1 ... 33 bases, every length mod 16 around 200 (odd and even: the offsets of the batch and the slots start at
    every alignment), an empty read; an error in the middle of those that have room for one"""
    rng = np.random.default_rng(77)
    g = genome()
    reads = []
    for n in [K - 1, K, K + 1, 15, 16, 17, 31, 32, 33] + list(range(185, 218)) + [0, 201, 203, 199]:
        s = int(rng.integers(0, len(g) - 300))
        kind, at = KINDS[n % 3], ([n // 2] + ([K + 1, n - 5] if n > 100 else []) if n >= 31 else [])
        grown = len(at) * {"sub": 0, "del": -1, "ins": 1}[kind]           # (the read is n bases long with its errors in)
        reads.append(plant(g[s:s + n - grown], kind, at, rng))
    return tuple(reads)


@functools.lru_cache(maxsize=None)
def long_reads():
    """6 000 bases with a substitution every 12 (more than 256 fixes: one unit's piece at BRX_LANE_CHUNK=8192) and
    11 000 bases with one every 40 (more than 128 units at BRX_LANE_CHUNK=64)"""
    rng = np.random.default_rng(78)
    g = genome()
    return (plant(g[500:6500], "sub", range(K + 4, 5990, 12), rng), plant(g[300:11300], "sub", range(K + 7, 10990, 40), rng),
            plant(g[6000:11000], "del", range(K + 2, 4990, 12), rng))


@functools.lru_cache(maxsize=None)
def marked_reads():
    """bytes that are not ACGT beside the errors: lower case (the same 2-bit code, copied through as it is) on both sides
    of every error, and N (the code of G) in place of a G two bases further on"""
    rng = np.random.default_rng(79)
    g = genome()
    reads = []
    for i, kind in enumerate(KINDS * 4):
        s = int(rng.integers(0, len(g) - 1200))
        r = bytearray(plant(g[s:s + 1200], "sub" if kind == "sub" else kind, range(K + 5 + i, 1190, 14), rng))
        for pos in range(K + 5 + i, len(r) - 4, 14):
            for q in (pos - 1, pos + 1):
                r[q] = ord(chr(r[q]).lower())
            for q in (pos + 2, pos - 2, pos + 3):
                if r[q] == ord("G"):
                    r[q] = ord("N")
                    break
        reads.append(bytes(r))
    return tuple(reads)


# ---------------------------------------------------------------- the layout, on the CPU ----------------------
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_fixes_fall_on_every_residue(kind):
    """for every kind of planted error and every spacing, the answers of the oracle (used = 1 / 0 / 2) fall on all 16
    residues of the offset in the output, so on all 16 residues of the destination address wherever the slot starts"""
    for sp in SPACINGS:
        reads = planted_reads(kind, sp)
        seen = set()
        for r, o in zip(reads, oracle_out(reads)):
            seen |= {off % 16 for kd, off in edits(r, o) if kd == ANSWER[kind]}
        assert seen == set(range(16)), (kind, sp, sorted(seen))


def test_oracle_makes_reads_that_only_grow_and_only_shrink():
    """reads whose length changes in one direction only (substitutions aside): every fix that moves the input position
    moves it the same way"""
    grow = planted_reads("del", 90, 30, 300)
    shrink = planted_reads("ins", 90, 30, 300)
    assert sum(len(o) > len(r) and "shrink" not in {kd for kd, _ in edits(r, o)} for r, o in zip(grow, oracle_out(grow))) >= 3
    assert sum(len(o) < len(r) and "grow" not in {kd for kd, _ in edits(r, o)} for r, o in zip(shrink, oracle_out(shrink))) >= 3


def test_oracle_puts_two_and_three_fixes_into_one_chunk():
    """errors 5 to 12 bases apart: wherever a read's slot starts (a = 0 .. 15), there are 16-byte chunks of the output with
    two and with three fixes; and there are fixes in the first and in the last 16 bytes of a read"""
    reads = tuple(r for kind in KINDS for sp in (5, 6, 8, 12) for r in planted_reads(kind, sp))
    outs = oracle_out(reads)
    per_read = [sorted({off for _, off in edits(r, o)}) for r, o in zip(reads, outs)]
    for a in range(16):
        most = [max(np.bincount((np.array(offs) + a) // 16)) for offs in per_read if offs]
        assert sum(m >= 2 for m in most) >= 20 and sum(m >= 3 for m in most) >= 5, (a, most)
    everything = every_planted_read()
    firsts = [edits(r, o) for r, o in zip(everything, oracle_out(everything))]
    assert any(off < 16 for e in firsts for _, off in e)
    assert any(off >= len(o) - 16 for e, o in zip(firsts, oracle_out(everything)) for _, off in e)


def test_short_reads_start_at_every_alignment():
    reads = short_reads()
    lens = [len(r) for r in reads]
    assert {K - 1, K, K + 1, 15, 16, 17, 31, 32, 33, 0} <= set(lens) and {n % 16 for n in lens if 185 <= n < 218} == set(range(16))
    starts = np.cumsum([0] + lens[:-1])
    assert {int(s) % 16 for s in starts} == set(range(16))
    assert sum(1 for r, o in zip(reads, oracle_out(reads)) if r != o) >= 10


def test_long_reads_hold_more_than_a_batch_of_fixes():
    """(the oracle's own count of the fixes it made: an edit script of reads this long takes minutes)"""
    many, units, grows = long_reads()
    fixes = []
    for r in long_reads():
        one = O.Corrector(ref_set(), "one", CONFIRM, 7)
        one.correct(r)
        fixes.append(one.stats()["fixes"])
    assert fixes[0] > 256 and fixes[2] > 256 and fixes[1] > 100, fixes
    assert len(units) > 128 * 64 and len(oracle_out(long_reads())[2]) > len(grows)


def test_marked_bytes_sit_beside_fixes_and_pass_through():
    reads = marked_reads()
    beside_lower = beside_n = 0
    for r, o in zip(reads, oracle_out(reads)):
        assert sum(c in b"acgt" for c in o) == sum(c in b"acgt" for c in r) or r != o
        for _, off in edits(r, o):
            near = o[max(off - 3, 0):off + 4]
            beside_lower += any(c in b"acgt" for c in near)
            beside_n += b"N" in near
    assert beside_lower >= 100 and beside_n >= 20, (beside_lower, beside_n)


# ---------------------------------------------------------------- the replay, on the GPU ----------------------
@pytest.fixture
def lane_env(monkeypatch):
    def set_(chunk=None, sync=None, rev=None):
        for key, v in (("BRX_LANE_CHUNK", chunk), ("BRX_LANE_SYNC", sync), ("BRX_LANE_REV", rev)):
            if v is None:
                monkeypatch.delenv(key, raising=False)
            else:
                monkeypatch.setenv(key, str(v))
        for key in ("BRX_LANE", "BRX_LANE_MASK", "BRX_LANE_WALK"):
            monkeypatch.delenv(key, raising=False)
    return set_


@functools.lru_cache(maxsize=None)
def gpu_set():
    return br_amd.Pcon.from_fasta([genome()], K)


def check(reads, names=("one",), two_side=False):
    """every read as the oracle leaves it, and the units of the lane form really ran and all left their records"""
    chain = br_amd.Chain(gpu_set(), [(m, CONFIRM, 7) for m in names], two_side=two_side)
    got = chain.correct_reads(list(reads))
    st = chain.last_stats()
    print(f"{names} two_side={two_side} reads={len(reads)} lane_units={st['lane_units']} redone={st['lane_redone_reads']} "
          f"fixes={st['fixes']} overflow_retries={st['overflow_retries']}")
    exp = oracle_out(tuple(reads), tuple(names), two_side)
    bad = [i for i, (x, e) in enumerate(zip(got, exp)) if x != e]
    assert not bad, (names, bad[:10])
    assert st["lane_units"] > 0 and st["lane_unwritten_units"] == 0
    assert st["fixes"] > 0
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("chunk,sync", [(None, None), (64, 1)])
def test_one_replay_every_residue(lane_env, kind, chunk, sync):
    lane_env(chunk, sync)
    for sp in SPACINGS:
        check(planted_reads(kind, sp))
    check(planted_reads(kind, 90, 30, 300))   # (among them the reads that only grow / only shrink)
    # all spacings of the kind in one batch, in another order: other input offsets, other slots
    check(tuple(r for sp in reversed(SPACINGS) for r in planted_reads(kind, sp)[::-1]))


@pytest.mark.gpu
@pytest.mark.parametrize("chunk,sync", [(None, None), (64, 1)])
def test_one_replay_short_reads_and_alignments(lane_env, chunk, sync):
    lane_env(chunk, sync)
    check(short_reads())
    check(short_reads()[::-1] + planted_reads("del", 6)[:5] + short_reads())


@pytest.mark.gpu
def test_one_replay_batches_of_fixes_and_many_units(lane_env):
    lane_env(8192, 1)
    st = check(long_reads())
    assert st["lane_units"] <= 4            # one unit per read: more than 256 fixes in one piece
    lane_env(64, 1)
    st = check(long_reads())
    assert st["lane_units"] > 128


@pytest.mark.gpu
def test_one_replay_marked_bytes(lane_env):
    lane_env(64, 1)
    check(marked_reads())
    lane_env()
    check(marked_reads())


@pytest.mark.gpu
@pytest.mark.parametrize("names", [("one", "graph"), ("gap_size",)])
@pytest.mark.parametrize("rev", [None, 3])
def test_walk_replay(lane_env, names, rev):
    """the same inputs through the walking correctors' replay (a fix writes several bases from its list), forward and --
    BRX_LANE_REV=3, both sides -- over reads stored back to front"""
    lane_env(64, 1, rev=rev)
    two_side = rev is not None
    for kind in KINDS:
        check(tuple(r for sp in (3, 5, 8, 12, 40) for r in planted_reads(kind, sp)[:8]), names, two_side)
    check(short_reads(), names, two_side)
    check(marked_reads(), names, two_side)
    lane_env(None, None, rev=rev)
    check(long_reads() + planted_reads("ins", 6), names, two_side)
