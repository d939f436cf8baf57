"""Stream order: every stream-taking entry of include/brx.h that Python reaches, on a busy non-blocking stream.

The rest of the GPU suite hands the library `None` or torch's current stream -- the legacy null stream, which serialises
with everything else the process does, so that a launch on the wrong stream, an unordered memset or an unsynchronised
hand-over between two streams cannot give a wrong answer there.  Here the caller owns a non-blocking stream `s` (the LANE)
that is kept busy: the inputs of a call hold a DECOY -- a valid batch of identical sizes -- until a delay queued on `s` has
run, and become the real batch only in the order of `s`.  An entry that keeps the contract of include/brx.h ("streams")
answers for the real batch; one that reads its inputs, zeroes its state or publishes a result outside the order of `s`
answers for the decoy, for a mixture, or for nothing -- a wrong ANSWER, never a fault: whichever version a kernel sees has
the same number of reads, the same number of bases and monotone offsets that end there, and every key is below 2^(2k).

Every expected value is the same operation done the ordinary way (null stream, device synchronised before and after);
where the suite has an oracle (oracle.hashes / count_reads / Solid, br_amd/cover.py, br_amd/abundance.py, correct_record)
it is checked against that as well.  All comparisons are exact.  The control (the `lane` fixture, reported by
test_control_keeps_a_stream_with_teeth) proves first that the delay is long enough to be seen: a call on ANOTHER stream
must answer for the decoy; if no stream out of four shows that, the module fails rather than pass without teeth.  Probes
C, D and E also assert, by an event recorded behind the delay (Lane.pending), that the delay had not run out when the call
under test was issued: a host step that outlasts it fails the probe.

Probes: A inputs late; B steady state (reset -> count -> finish_into -> cover / correct, the host waiting nowhere);
C fresh objects used at once while the null stream is busy and the pool hands back a dirty block; D a stream call followed
by a host-path call; E lazy state built on one stream and used on another; F the same with the kernel timers on.

Out of scope: the collectives (brx_exchange_*, brx_comm_*), whose ordering is between ranks; the fd pipelines
(brx_run_correction_fd*, brx_count_fasta_fd, brx_set_insert_fasta_fd), which own their streams; and two host threads
mutating one counter.
"""
import ctypes as C

import numpy as np
import pytest

import br_amd
from br_amd import _lib, abundance as ab, cover, strand, synth
from br_amd.set import pack_reads, sort_keys_device
from oracle import oracle as O

gpu = pytest.mark.gpu

N_READS = 48        # reads 0..47 of raw.fasta: the batch every probe works on (0.6 Mbases, read lengths 3 k .. 62 k)
OTHER_AT = 60       # reads 60..107: the "other" batch of probes B and D
ABUNDANCE = 1       # solid iff counted more than once
SENTINEL = 0xEE
DENSE, SORTED, TABLE = _lib.COUNT_DENSE, _lib.COUNT_SORTED, _lib.COUNT_TABLE
STRATEGY_NAMES = {DENSE: "dense", SORTED: "sorted", TABLE: "table"}


# ---- real and decoy inputs (numpy only: the CPU test below runs them without a GPU) ----------------------------------------

def decoy_reads(reads, seed):
    """a valid batch of the same sizes: the read lengths permuted, every base drawn afresh"""
    rng = np.random.default_rng(seed)
    lens = rng.permutation([len(r) for r in reads])
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    return [letters[rng.integers(0, 4, int(n))].tobytes() for n in lens]


def batch_of(reads):
    bases, offs = pack_reads(reads)
    return {"bases": bases, "offs": offs}


def keys_of(k, reads, abundance=-1):
    """sorted bit indices (canonical >> 1) of the k-mers counted more than `abundance` times (-1: all that occur): what
    oracle.Solid.sparse_from_count keeps"""
    parts = [O.hashes(k, r) for r in reads if len(r) >= k]
    uniq, cnt = np.unique(np.concatenate(parts), return_counts=True)
    return np.ascontiguousarray(uniq[np.minimum(cnt, 255) > abundance], dtype=np.uint64)


def decoy_keys(k, n, seed):
    """n other keys below 2^(2k-1) (so also below 2^(2k)): valid bit indices of a set of this k"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << (2 * k - 1), n, dtype=np.uint64)


def fingerprint_of(keys):
    """brx_set_fingerprint of the set with these members"""
    keys = np.asarray(keys, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return int(keys.size), int(keys.sum(dtype=np.uint64)), int((keys * keys).sum(dtype=np.uint64))


def solid_bytes_of(k, keys):
    """the .solid stream ([k][bits Lsb0]) of the set with these members"""
    bits = np.zeros(max(1 << (2 * k - 1), 8) // 8, dtype=np.uint8)
    keys = np.asarray(keys, dtype=np.uint64)
    np.bitwise_or.at(bits, (keys >> np.uint64(3)).astype(np.int64), (np.uint8(1) << (keys & np.uint64(7)).astype(np.uint8)))
    return bytes([k]) + bits.tobytes()


def cover_of(k, keys, reads):
    """(flags of the batch, cover.STATS_DTYPE array) by br_amd/cover.py from set membership in numpy"""
    fl = [cover.flags_from_solid(np.isin(O.hashes(k, r), keys), len(r), k) for r in reads]
    st = np.zeros(len(reads), dtype=cover.STATS_DTYPE)
    for i, f in enumerate(fl):
        st[i] = cover.stats_from_flags(f, k)
    return np.concatenate(fl), st


def profile_of(k, counted, reads):
    """the abundance profile of `reads` (one byte per base) against the counts of `counted`, by br_amd/abundance.py"""
    table = ab.count_table([O.hashes(k, r) for r in counted])
    return np.concatenate([ab.profile_bytes(ab.lookup(table, O.hashes(k, r)), len(r)) for r in reads])


@pytest.fixture(scope="module")
def reads(raw_reads):
    return raw_reads[:N_READS]


@pytest.fixture(scope="module")
def other(raw_reads):
    return raw_reads[OTHER_AT:OTHER_AT + N_READS]


@pytest.fixture(scope="module")
def decoy(reads):
    return decoy_reads(reads, 1)


def test_fixtures_have_teeth(reads, other, decoy):
    """no GPU: the decoy is a valid batch of the same sizes, and the oracle tells it from the real one at every k used"""
    real_b, dec_b = batch_of(reads), batch_of(decoy)
    assert len(decoy) == len(reads) == N_READS == len(other)
    assert dec_b["bases"].size == real_b["bases"].size and dec_b["offs"].size == real_b["offs"].size
    assert dec_b["offs"][0] == 0 and int(dec_b["offs"][-1]) == real_b["bases"].size
    assert np.all(np.diff(dec_b["offs"].astype(np.int64)) >= 0)
    assert sorted(len(r) for r in decoy) == sorted(len(r) for r in reads)
    assert [len(r) for r in decoy] != [len(r) for r in reads]
    assert set(dec_b["bases"].tolist()) <= set(b"ACGT")
    assert not np.array_equal(dec_b["bases"], real_b["bases"])
    for k in (11, 13, 15, 19, 21, 25):
        real_all, real_solid = keys_of(k, reads), keys_of(k, reads, ABUNDANCE)
        assert np.array_equal(O.hashes(k, reads[0]), ab.canonical_hashes(reads[0], k))  # the two oracles agree
        assert 0 < real_solid.size < real_all.size
        assert fingerprint_of(real_all) != fingerprint_of(keys_of(k, decoy))
        assert fingerprint_of(real_solid) != fingerprint_of(keys_of(k, decoy, ABUNDANCE))
        assert fingerprint_of(real_solid) != fingerprint_of(keys_of(k, other, ABUNDANCE))
        dk = decoy_keys(k, real_all.size, 2)
        assert dk.size == real_all.size and int(dk.max()) < 1 << (2 * k)
        assert fingerprint_of(np.unique(dk)) != fingerprint_of(real_all)
    for k in (15, 19, 25):  # probe B's decoy
        assert fingerprint_of(keys_of(k, decoy_reads(reads, 5), ABUNDANCE)) != fingerprint_of(keys_of(k, reads, ABUNDANCE))
        assert fingerprint_of(keys_of(k, decoy_reads(reads, 5))) != fingerprint_of(keys_of(k, reads))
    few_decoy = decoy_reads(reads[:12], 4)  # the correction probes' decoy
    assert sum(map(len, few_decoy)) == sum(map(len, reads[:12])) and b"".join(few_decoy) != b"".join(reads[:12])
    k = 11
    assert O.Solid.from_count(k, O.count_reads(k, reads), ABUNDANCE).to_bytes() == solid_bytes_of(k, keys_of(k, reads, ABUNDANCE))
    assert O.Solid.sparse_from_count(15, reads, ABUNDANCE).popcount() == keys_of(15, reads, ABUNDANCE).size
    # cover and abundance tell the batches apart against the real counts
    keys = keys_of(15, reads, ABUNDANCE)
    assert not np.array_equal(cover_of(15, keys, reads)[0], cover_of(15, keys, decoy)[0])
    assert not np.array_equal(profile_of(15, reads, reads), profile_of(15, reads, decoy))


# ---- the lane ----------------------------------------------------------------------------------------------------------------

def dev(a):
    """a numpy array on the device (uint64 travels as int64: same bytes)"""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


class Plain:
    """the ordinary way: null stream, the device synchronised around every step"""
    stream = None

    @staticmethod
    def fetch(t):
        import torch
        torch.cuda.synchronize()
        return t.cpu().numpy()

    @staticmethod
    def wait():
        import torch
        torch.cuda.synchronize()


class Lane:
    """one non-blocking stream of the caller's, kept busy"""

    def __init__(self, rounds):
        import torch
        self.torch = torch
        self.s = torch.cuda.Stream()
        self.stream = self.s.cuda_stream
        self.rounds = rounds
        self.ballast = torch.randint(0, 1 << 30, (1 << 24,), dtype=torch.int32, device="cuda")
        self.keep = []
        torch.cuda.synchronize()

    def delay(self, on=None):
        """ordinary torch work queued on the lane's stream (or on `on`; the null stream when on == "null")"""
        torch = self.torch
        ctx = torch.cuda.stream(torch.cuda.default_stream()) if on == "null" else torch.cuda.stream(on or self.s)
        with ctx:
            x = self.ballast
            for _ in range(self.rounds):
                x = torch.sort(x).values.flip(0)
            self.keep.append(x)
            self.gate = torch.cuda.Event()
            self.gate.record()  # (on the stream the delay went to)

    def pending(self):
        """the last delay has not run to its end yet: what a probe asserts at the moment its call under test is issued, so
        that a host step that outlasted the delay fails the probe instead of leaving it without teeth"""
        return not self.gate.query()

    def stage(self, decoy, real):
        """device tensors that hold `decoy` now (copied, the host synchronised) and become `real` only in the order of the
        lane's stream: delay, then copy_ from a device copy of `real`"""
        torch = self.torch
        assert decoy.keys() == real.keys()
        for name in real:
            assert decoy[name].shape == real[name].shape and decoy[name].dtype == real[name].dtype, name
        held = {name: dev(a) for name, a in decoy.items()}
        src = {name: dev(a) for name, a in real.items()}
        torch.cuda.synchronize()
        self.delay()
        with torch.cuda.stream(self.s):
            for name in real:
                held[name].copy_(src[name], non_blocking=True)
        self.keep.append(src)
        return held

    def fetch(self, t):
        with self.torch.cuda.stream(self.s):
            h = t.cpu()  # a copy in the order of the lane's stream; waits for that stream alone
        self.s.synchronize()
        return h.numpy()

    def wait(self):
        self.s.synchronize()
        self.keep.clear()


def control_once(lane, away, real_b, decoy_b):
    """stage a batch on the lane, count it on the stream `away`: 'decoy' / 'real' / 'neither'"""
    k = 11
    want = {}
    for tag, b in (("real", real_b), ("decoy", decoy_b)):
        c = br_amd.Counter(k, strategy=DENSE)
        c.add_batch(b["bases"], b["offs"])
        want[tag] = c.finish(ABUNDANCE).to_solid_bytes()
    assert want["real"] != want["decoy"]
    c = br_amd.Counter(k, strategy=DENSE)
    inp = lane.stage(decoy_b, real_b)
    n, total = inp["offs"].numel() - 1, inp["bases"].numel()
    c.add_batch_device(inp["bases"].data_ptr(), inp["offs"].data_ptr(), n, total, away.cuda_stream)
    away.synchronize()
    lane.wait()
    got = c.finish(ABUNDANCE).to_solid_bytes()
    return "decoy" if got == want["decoy"] else "real" if got == want["real"] else "neither"


@pytest.fixture(scope="module")
def lane(reads, decoy):
    """the lane the probes use: the first stream (of up to four fresh ones) and delay on which the control sees the decoy"""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("the stream tests need a GPU")
    real_b, decoy_b = batch_of(reads), batch_of(decoy)
    away = torch.cuda.Stream()
    seen = []
    for attempt in range(4):
        ln = Lane(0)
        for rounds in (4, 16, 64):  # (the control picks the delay: the first that a call on another stream cannot outwait)
            ln.rounds = rounds
            verdict = control_once(ln, away, real_b, decoy_b)
            seen.append((attempt, rounds, verdict))
            if verdict == "decoy":
                ln.second = away
                ln.report = (f"control: kept stream {attempt + 1} of 4 (handle {ln.stream:#x}); a delay of {rounds} sorts showed the "
                             f"decoy and is what the probes use; tried {seen}")
                print(ln.report)
                return ln
    pytest.fail(f"no teeth: a call on another stream never saw the decoy behind the delay {seen}: two streams on one "
                "hardware queue, or a delay too short -- the probes of this module would prove nothing")


@gpu
def test_control_keeps_a_stream_with_teeth(lane):
    print(lane.report)
    assert lane.stream != 0 and lane.second.cuda_stream not in (0, lane.stream)


# ---- operations: one function per entry, run the ordinary way and on the lane --------------------------------------------------

def ptr(t):
    return t.data_ptr() if t is not None else None


def sizes(inp):
    return inp["offs"].numel() - 1, inp["bases"].numel()


def alloc(spec):
    """output buffers, pre-filled with the sentinel"""
    import torch
    out = {}
    for name, (numel, dtype) in spec.items():
        t = torch.empty(max(int(numel), 1), dtype=getattr(torch, dtype), device="cuda")
        t.view(torch.uint8).fill_(SENTINEL)
        out[name] = t
    return out


def run_plain(op, arrays):
    import torch
    inp = {name: dev(a) for name, a in arrays.items()}
    out = alloc(op.outs(arrays))
    torch.cuda.synchronize()
    res = op(Plain, inp, out)
    torch.cuda.synchronize()
    return res


def run_lane(lane, op, decoy, real):
    out = alloc(op.outs(real))
    inp = lane.stage(decoy, real)  # (synchronises the device, then queues the delay and the copies)
    res = op(lane, inp, out)
    lane.wait()
    return res


def probe(lane, op, decoy, real):
    """the contract for one entry: on the busy lane it answers what it answers the ordinary way for the real inputs, and
    that differs from its answer for the decoy"""
    want = run_plain(op, real)
    assert run_plain(op, decoy) != want, "the decoy's answer must differ from the real one"
    got = run_lane(lane, op, decoy, real)
    assert got == want
    return want


def operation(outs=None):
    def wrap(f):
        f.outs = outs or (lambda arrays: {})
        return f
    return wrap


def insert_device(st, inp, stream):
    n, total = sizes(inp)
    st.insert_batch_device(ptr(inp["bases"]), ptr(inp["offs"]), n, total, stream)


def add_device(cnt, inp, stream):
    n, total = sizes(inp)
    cnt.add_batch_device(ptr(inp["bases"]), ptr(inp["offs"]), n, total, stream)


def set_answer(ctx, st):
    """what a set holds, read in the order of the caller's stream"""
    return st.fingerprint(ctx.stream)


@operation()
def op_insert(ctx, inp, out):
    st = br_amd.Pcon.new(13)
    insert_device(st, inp, ctx.stream)
    fp = st.fingerprint(ctx.stream)
    ctx.wait()  # (to_solid_bytes is a host-path reader: the caller orders it)
    return fp, st.to_solid_bytes()


@operation()
def op_or_keys(ctx, inp, out):
    st = br_amd.Pcon.new(13)
    st.or_keys_device(ptr(inp["keys"]), inp["keys"].numel(), ctx.stream)
    ctx.wait()
    return st.to_solid_bytes()


@operation(lambda arrays: {"list": (arrays["keys"].size, "int64")})
def op_extract_keys(ctx, inp, out):
    st = br_amd.Pcon.new(13)
    st.or_keys_device(ptr(inp["keys"]), inp["keys"].numel(), ctx.stream)
    n = st.extract_keys_device(0, st.n_hashes(), ptr(out["list"]), out["list"].numel(), ctx.stream)
    return n, np.sort(ctx.fetch(out["list"])[:n]).tobytes()


def op_index_build(query):
    @operation()
    def run(ctx, inp, out):
        st = br_amd.Pcon.new(15)
        insert_device(st, inp, ctx.stream)
        info = st.index_build(stream=ctx.stream)
        ctx.wait()
        return info["keys"], info["overflow_keys"], st.get_batch_indexed(query)[0].tobytes()
    return run


@operation()
def op_keylist(ctx, inp, out):
    cnt = br_amd.Counter(15, strategy=SORTED)
    add_device(cnt, inp, ctx.stream)
    st = cnt.finish(ABUNDANCE, ctx.stream)
    d_keys, n = st.keylist_device(ctx.stream)
    twin = br_amd.Pcon.new(15)
    twin.or_keys_device(d_keys, n, ctx.stream)
    return n, twin.fingerprint(ctx.stream)


def op_cover(st):
    @operation(lambda arrays: {"flags": (arrays["bases"].size, "uint8"), "masked": (arrays["bases"].size, "uint8"),
                               "stats": (4 * (arrays["offs"].size - 1), "int32")})
    def run(ctx, inp, out):
        n, total = sizes(inp)
        st.cover_batch_device(ptr(inp["bases"]), ptr(inp["offs"]), n, total, ptr(out["flags"]), ptr(out["masked"]), ptr(out["stats"]),
                              ctx.stream)
        return tuple(ctx.fetch(out[name]).tobytes() for name in ("flags", "masked", "stats"))
    return run


def op_cover_split(st, min_len):
    def outs(arrays):
        n, total = arrays["offs"].size - 1, arrays["bases"].size
        cap = n + total // (max(st.k(), min_len, 1) + 1)  # the bound of include/brx.h: no retry needed
        return {"out": (total, "uint8"), "out_offs": (cap + 1, "int64"), "piece_read": (cap, "int32"), "piece_start": (cap, "int64")}

    @operation(outs)
    def run(ctx, inp, out):
        n, total = sizes(inp)
        cap = out["piece_read"].numel()
        n_pieces, out_total = C.c_uint32(0), C.c_uint64(0)
        _lib.check(_lib.lib().brx_set_cover_split_batch_device(st._h, ptr(inp["bases"]), ptr(inp["offs"]), n, total, min_len,
                                                               ptr(out["out"]), total, ptr(out["out_offs"]), ptr(out["piece_read"]),
                                                               ptr(out["piece_start"]), cap, C.byref(n_pieces), C.byref(out_total),
                                                               ctx.stream))
        p, t = n_pieces.value, out_total.value
        return (p, t, ctx.fetch(out["out"])[:t].tobytes(), ctx.fetch(out["out_offs"])[:p + 1].tobytes(),
                ctx.fetch(out["piece_read"])[:p].tobytes(), ctx.fetch(out["piece_start"])[:p].tobytes())
    return run


def op_counter(strategy, k, tail):
    """a fresh counter, one batch on the caller's stream, then the entry named by `tail` as the first consumer"""
    def outs(arrays):
        if tail != "abundance":
            return {}
        n, total = arrays["offs"].size - 1, arrays["bases"].size
        return {"profile": (total, "uint8"), "hist": (256 * n, "int32"), "stats": (ab.STATS_DTYPE.itemsize * n, "uint8")}

    @operation(outs)
    def run(ctx, inp, out):
        cnt = br_amd.Counter(k, strategy=strategy)
        add_device(cnt, inp, ctx.stream)
        if tail == "finish":
            st = cnt.finish(ABUNDANCE, ctx.stream)
            return set_answer(ctx, st), st.bits_state()
        if tail == "finish_into":
            st = br_amd.Pcon.new(k)
            cnt.finish_into(ABUNDANCE, st, ctx.stream)
            return set_answer(ctx, st), st.bits_state()
        if tail == "spectrum":
            return cnt.spectrum(ctx.stream).tobytes()
        if tail == "clamp":
            cnt.clamp(2, ctx.stream)
            return cnt.spectrum(ctx.stream).tobytes()
        if tail == "table_info":
            info = cnt.table_info(ctx.stream)
            return info["keys"], info["log2_lines"]
        if tail == "prepare_lookup":
            cnt.prepare_lookup(ctx.stream)
            return cnt.lookup_ready, cnt.spectrum(ctx.stream).tobytes()
        assert tail == "abundance"
        n, total = sizes(inp)
        cnt.prepare_lookup(ctx.stream)
        cnt.abundance_batch_device(ptr(inp["bases"]), ptr(inp["offs"]), n, total, ABUNDANCE, ptr(out["profile"]), ptr(out["hist"]),
                                   ptr(out["stats"]), ctx.stream)
        return tuple(ctx.fetch(out[name]).tobytes() for name in ("profile", "hist", "stats"))
    return run


def op_correct(chain):
    @operation(lambda arrays: {"out": (2 * arrays["bases"].size + 4096, "uint8"), "out_offs": (arrays["offs"].size, "int64")})
    def run(ctx, inp, out):
        n, total = sizes(inp)
        t = chain.correct_batch_device(ptr(inp["bases"]), ptr(inp["offs"]), n, total, ptr(out["out"]), out["out"].numel(),
                                       ptr(out["out_offs"]), ctx.stream)
        return t, ctx.fetch(out["out"])[:t].tobytes(), ctx.fetch(out["out_offs"]).tobytes()
    return run


@operation(lambda arrays: {"out": (arrays["bases"].size, "uint8")})
def op_revcomp(ctx, inp, out):
    n, total = sizes(inp)
    _lib.check(_lib.lib().brx_revcomp_batch_device(ptr(inp["bases"]), ptr(inp["offs"]), n, total, ptr(out["out"]), ctx.stream))
    return ctx.fetch(out["out"]).tobytes()


def op_synth(cfg, n_reads):
    cap = n_reads * (2 * cfg.read_len + 8)

    @operation(lambda arrays: {"bases": (cap, "uint8"), "offs": (n_reads + 1, "int64")})
    def run(ctx, inp, out):
        t = synth.reads_device(cfg, 0, ptr(inp["genome"]), 0, n_reads, ptr(out["bases"]), cap, ptr(out["offs"]), ctx.stream)
        return t, ctx.fetch(out["bases"])[:t].tobytes(), ctx.fetch(out["offs"]).tobytes()
    return run


def op_sort(key_bits):
    @operation()
    def run(ctx, inp, out):
        sort_keys_device(ptr(inp["keys"]), ptr(inp["payload"]), inp["keys"].numel(), key_bits, ctx.stream)
        return ctx.fetch(inp["keys"]).tobytes(), ctx.fetch(inp["payload"]).tobytes()
    return run


# ---- A: inputs late ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def key_inputs(reads):
    """(decoy, real) key arrays for k = 13: the real ones are the k-mers of the batch, in read order with repeats"""
    k = 13
    real = np.concatenate([O.hashes(k, r) for r in reads[:8]])
    return {"keys": decoy_keys(k, real.size, 2)}, {"keys": real}


@gpu
def test_a_insert_batch_device(lane, reads, decoy):
    fp, solid = probe(lane, op_insert, batch_of(decoy), batch_of(reads))
    keys = keys_of(13, reads)
    assert fp == fingerprint_of(keys) and solid == solid_bytes_of(13, keys)


@gpu
def test_a_or_keys_device(lane, key_inputs):
    solid = probe(lane, op_or_keys, *key_inputs)
    assert solid == solid_bytes_of(13, np.unique(key_inputs[1]["keys"]))


@gpu
def test_a_extract_keys_device(lane, key_inputs):
    n, listed = probe(lane, op_extract_keys, *key_inputs)
    want = np.unique(key_inputs[1]["keys"])
    assert n == want.size and listed == want.tobytes()


@gpu
def test_a_index_build(lane, reads, decoy):
    k = 15
    query = np.concatenate([cover.kmers_of(reads[0], k)[:3000], cover.kmers_of(decoy[0], k)[:3000]])
    keys_n, _, answers = probe(lane, op_index_build(query), batch_of(decoy), batch_of(reads))
    keys = keys_of(k, reads)
    assert keys_n == keys.size
    want = np.isin(np.concatenate([O.hashes(k, reads[0])[:3000], O.hashes(k, decoy[0])[:3000]]), keys)
    assert answers == want.tobytes()


@gpu
def test_a_keylist_device(lane, reads, decoy):
    n, fp = probe(lane, op_keylist, batch_of(decoy), batch_of(reads))
    keys = keys_of(15, reads, ABUNDANCE)
    assert n == keys.size and fp == fingerprint_of(keys)
    assert O.Solid.sparse_from_count(15, reads, ABUNDANCE).popcount() == n


@pytest.fixture(scope="module")
def solid15(reads):
    """the solid set of the batch at k = 15, built the ordinary way"""
    st = br_amd.Pcon.from_count(reads, 15, ABUNDANCE)
    assert st.fingerprint() == fingerprint_of(keys_of(15, reads, ABUNDANCE))
    return st


@gpu
def test_a_cover_batch_device(lane, reads, decoy, solid15):
    flags, masked, stats = probe(lane, op_cover(solid15), batch_of(decoy), batch_of(reads))
    want_fl, want_st = cover_of(15, keys_of(15, reads, ABUNDANCE), reads)
    assert flags == want_fl.tobytes() and stats == want_st.tobytes()
    at = 0
    for r in reads:
        assert masked[at:at + len(r)] == cover.mask_read(r, want_fl[at:at + len(r)] & cover.COVERED)
        at += len(r)


@gpu
def test_a_cover_split_batch_device(lane, reads, decoy, solid15):
    min_len = 100
    p, t, out, out_offs, piece_read, piece_start = probe(lane, op_cover_split(solid15, min_len), batch_of(decoy), batch_of(reads))
    want_fl, _ = cover_of(15, keys_of(15, reads, ABUNDANCE), reads)
    pieces, at = [], 0
    for i, r in enumerate(reads):
        pieces += [(i, s, piece) for s, piece in cover.split_read(r, want_fl[at:at + len(r)] & cover.COVERED, min_len)]
        at += len(r)
    assert p == len(pieces) > 0 and out == b"".join(x[2] for x in pieces) and t == len(out)
    assert np.frombuffer(piece_read, dtype=np.int32).tolist() == [x[0] for x in pieces]
    assert np.frombuffer(piece_start, dtype=np.int64).tolist() == [x[1] for x in pieces]
    assert np.frombuffer(out_offs, dtype=np.int64).tolist() == np.concatenate(([0], np.cumsum([len(x[2]) for x in pieces]))).tolist()


COUNT_CASES = [(DENSE, 11), (DENSE, 15), (SORTED, 15), (SORTED, 19), (TABLE, 25)]
TAIL_CASES = ([(s, k, "finish") for s, k in COUNT_CASES] +
              [(s, k, tail) for tail in ("finish_into", "spectrum", "abundance") for s, k in ((DENSE, 11), (SORTED, 15), (TABLE, 25))] +
              [(DENSE, 11, "clamp"), (TABLE, 25, "table_info"), (SORTED, 15, "prepare_lookup")])


@gpu
@pytest.mark.parametrize("strategy,k,tail", TAIL_CASES, ids=[f"{STRATEGY_NAMES[s]}-k{k}-{t}" for s, k, t in TAIL_CASES])
def test_a_counter(lane, reads, decoy, strategy, k, tail):
    got = probe(lane, op_counter(strategy, k, tail), batch_of(decoy), batch_of(reads))
    if tail in ("finish", "finish_into"):
        assert got[0] == fingerprint_of(keys_of(k, reads, ABUNDANCE))
    elif tail in ("spectrum", "clamp", "prepare_lookup"):
        hist = np.frombuffer(got if tail != "prepare_lookup" else got[1], dtype=np.uint64)
        _, cnt = ab.count_table([O.hashes(k, r) for r in reads])
        want = np.bincount(np.minimum(cnt, 2) if tail == "clamp" else cnt, minlength=256).astype(np.uint64)
        want[0] = (1 << (2 * k - 1)) - cnt.size
        assert np.array_equal(hist, want)
    elif tail == "table_info":
        assert got[0] == keys_of(k, reads).size
    else:
        assert got[0] == profile_of(k, reads, reads).tobytes()
        profiles = ab.unpack_profile(np.frombuffer(got[0], dtype=np.uint8), batch_of(reads)["offs"], k)
        assert got[2] == ab.stats_array(profiles, ABUNDANCE).tobytes()


@gpu
def test_a_sort_keys_device_with_payload(lane, key_inputs):
    k = 13
    rng = np.random.default_rng(3)
    decoy_in, real_in = ({"keys": a["keys"], "payload": rng.integers(0, 256, a["keys"].size, dtype=np.uint8)} for a in key_inputs)
    keys, payload = probe(lane, op_sort(2 * k - 1), decoy_in, real_in)
    order = np.argsort(real_in["keys"], kind="stable")
    assert keys == real_in["keys"][order].tobytes() and payload == real_in["payload"][order].tobytes()


@gpu
@pytest.mark.parametrize("methods", [("one",), ("graph", "gap_size")], ids=["one", "graph+gap_size"])
def test_a_correct_batch_device(lane, reads, decoy, solid_fixture_bytes, methods):
    few, few_decoy = reads[:12], decoy_reads(reads[:12], 4)
    st = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    chain = br_amd.Chain(st, [(m, 5, 7) for m in methods], two_side=False)
    _, out, out_offs = probe(lane, op_correct(chain), batch_of(few_decoy), batch_of(few))
    om = O.build_methods(O.Solid.from_bytes(solid_fixture_bytes), list(methods), 5, 7)
    want = [O.correct_record(om, r, False) for r in few]
    assert out == b"".join(want)
    assert np.frombuffer(out_offs, dtype=np.int64).tolist() == np.concatenate(([0], np.cumsum([len(w) for w in want]))).tolist()


@gpu
def test_a_revcomp_batch_device(lane, reads, decoy):
    out = probe(lane, op_revcomp, batch_of(decoy), batch_of(reads))
    assert out == b"".join(strand.revcomp(r) for r in reads)


@gpu
def test_a_synth_reads_device(lane):
    n_reads = 40
    cfg = synth.config(genome_len=20_000, read_len=1000)
    other_cfg = synth.config(genome_len=20_000, read_len=1000, seed=synth.DEFAULT_SEED + 1)
    genome, other_genome = synth.genome_host(cfg), synth.genome_host(other_cfg)
    t, bases, offs = probe(lane, op_synth(cfg, n_reads), {"genome": other_genome}, {"genome": genome})
    want_b, want_o = synth.reads_host(cfg, genome, 0, n_reads)
    assert t == want_b.size and bases == want_b.tobytes() and offs == want_o.tobytes()


# ---- B: steady state on a busy stream --------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("strategy,k", [(DENSE, 15), (SORTED, 19), (TABLE, 25)], ids=["dense-k15-bits", "sorted-k19-lazy", "table-k25"])
def test_b_steady_state(lane, reads, other, strategy, k):
    """delay -> reset -> count -> finish_into a set that held another solid set, its probe index built -> cover and correct,
    all on the lane and the host waiting nowhere in between"""
    import torch
    cnt = br_amd.Counter(k, strategy=strategy)
    cnt.add_reads(other)
    dst = cnt.finish(ABUNDANCE)
    chain = br_amd.Chain(dst, [("one", 5, 7)], two_side=False)
    old = dev(batch_of(other)["bases"]), dev(batch_of(other)["offs"])
    old_flags = torch.zeros(old[0].numel(), dtype=torch.uint8, device="cuda")
    dst.cover_batch_device(ptr(old[0]), ptr(old[1]), len(other), old[0].numel(), ptr(old_flags), None, None, None)
    torch.cuda.synchronize()
    assert dst.index_info()["valid"] and dst.fingerprint() == fingerprint_of(keys_of(k, other, ABUNDANCE))
    assert old_flags.cpu().numpy().tobytes() == cover_of(k, keys_of(k, other, ABUNDANCE), other)[0].tobytes()

    real_b = batch_of(reads)
    out = alloc({"flags": (real_b["bases"].size, "uint8"), "out": (2 * real_b["bases"].size + 4096, "uint8"),
                 "out_offs": (real_b["offs"].size, "int64")})
    decoy5 = decoy_reads(reads, 5)
    assert fingerprint_of(keys_of(k, decoy5, ABUNDANCE)) != fingerprint_of(keys_of(k, reads, ABUNDANCE))  # the decoy's answer differs
    inp = lane.stage(batch_of(decoy5), real_b)
    n, total = sizes(inp)
    s = lane.stream
    cnt.reset(s)
    add_device(cnt, inp, s)
    cnt.finish_into(ABUNDANCE, dst, s)
    dst.cover_batch_device(ptr(inp["bases"]), ptr(inp["offs"]), n, total, ptr(out["flags"]), None, None, s)
    t = chain.correct_batch_device(ptr(inp["bases"]), ptr(inp["offs"]), n, total, ptr(out["out"]), out["out"].numel(),
                                   ptr(out["out_offs"]), s)
    fp = dst.fingerprint(s)
    flags, corrected, out_offs = lane.fetch(out["flags"]), lane.fetch(out["out"])[:t].tobytes(), lane.fetch(out["out_offs"])
    lane.wait()
    keys = keys_of(k, reads, ABUNDANCE)
    assert fp == fingerprint_of(keys)
    assert flags.tobytes() == cover_of(k, keys, reads)[0].tobytes()
    om = O.build_methods(O.Solid.sparse_from_count(k, reads, ABUNDANCE), ["one"], 5, 7)
    want = [O.correct_record(om, r, False) for r in reads]
    assert corrected == b"".join(want)
    assert out_offs.tolist() == np.concatenate(([0], np.cumsum([len(w) for w in want]))).tolist()


# ---- C: fresh objects, used at once ----------------------------------------------------------------------------------------------

def dirty_the_pool(reads):
    """fill a k = 15 set and free it: the device pool now hands its 64 MiB block back as it is"""
    import torch
    st = br_amd.Pcon.new(15)
    st.insert_reads(reads)
    assert st.popcount() > 0
    del st
    torch.cuda.synchronize()


@gpu
def test_c_fresh_bit_vector_set(lane, reads, decoy):
    import torch
    k = 15
    inp = {name: dev(a) for name, a in batch_of(reads).items()}
    dirty_the_pool(decoy)
    torch.cuda.synchronize()
    lane.delay(on="null")  # the host's own work keeps the null stream busy
    assert lane.pending()
    st = br_amd.Pcon.new(k)
    insert_device(st, inp, lane.stream)
    lane.wait()
    assert st.to_solid_bytes() == solid_bytes_of(k, keys_of(k, reads))


@gpu
def test_c_fresh_sparse_set(lane, reads):
    import torch
    k = 25
    inp = {name: dev(a) for name, a in batch_of(reads).items()}
    torch.cuda.synchronize()
    lane.delay(on="null")
    assert lane.pending()
    st = br_amd.Pcon.new(k)
    insert_device(st, inp, lane.stream)
    fp = st.fingerprint(lane.stream)
    lane.wait()
    assert st.is_sparse() and fp == fingerprint_of(keys_of(k, reads)) and st.popcount() == fp[0]


@gpu
@pytest.mark.parametrize("strategy,k", [(DENSE, 15), (SORTED, 15), (TABLE, 25)], ids=["dense-k15", "sorted-k15", "table-k25"])
def test_c_fresh_counter(lane, reads, decoy, strategy, k):
    import torch
    inp = {name: dev(a) for name, a in batch_of(reads).items()}
    if strategy == DENSE:  # park a dirty 512 MiB count table for the new counter to take
        c0 = br_amd.Counter(k, strategy=DENSE)
        c0.add_reads(decoy)
        del c0
    torch.cuda.synchronize()
    lane.delay(on="null")
    assert lane.pending()
    cnt = br_amd.Counter(k, strategy=strategy)
    add_device(cnt, inp, lane.stream)
    st = cnt.finish(ABUNDANCE, lane.stream)
    fp = st.fingerprint(lane.stream)
    lane.wait()
    assert fp == fingerprint_of(keys_of(k, reads, ABUNDANCE))


# ---- D: a stream call, then a host-path call -------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("on", ["null", "lane"])
@pytest.mark.parametrize("strategy,k", [(DENSE, 15), (SORTED, 15), (TABLE, 25)], ids=["dense-k15", "sorted-k15", "table-k25"])
def test_d_reset_then_add_reads(lane, reads, other, strategy, k, on):
    """reset on a busy stream X, then the host-path add_reads (which works on the counter's own stream), then finish on X:
    exactly the set of `other` -- nothing from before the reset, nothing lost"""
    import torch
    cnt = br_amd.Counter(k, strategy=strategy)
    cnt.add_reads(reads)
    torch.cuda.synchronize()
    x = None if on == "null" else lane.stream
    lane.delay(on="null" if on == "null" else None)
    cnt.reset(x)
    assert lane.pending()  # the reset is still queued behind the delay when the host-path call is issued
    cnt.add_reads(other)
    st = cnt.finish(ABUNDANCE, x)
    fp = st.fingerprint(x)
    lane.wait()
    assert fp != fingerprint_of(keys_of(k, reads + other, ABUNDANCE))
    assert fp == fingerprint_of(keys_of(k, other, ABUNDANCE))


@gpu
@pytest.mark.parametrize("on", ["null", "lane"])
def test_d_reset_then_load(lane, reads, other, on, tmp_path):
    """the same with Counter.load in place of add_reads (key files: the table strategy)"""
    import torch
    k = 25
    src = br_amd.Counter(k, strategy=TABLE)
    src.add_reads(other)
    with open(tmp_path / "other.keys", "wb") as f:
        src.save(f)
    cnt = br_amd.Counter(k, strategy=TABLE)
    cnt.add_reads(reads)
    torch.cuda.synchronize()
    x = None if on == "null" else lane.stream
    lane.delay(on="null" if on == "null" else None)
    with open(tmp_path / "other.keys", "rb") as f:  # (a plain descriptor: nothing between the reset and the load but the read)
        cnt.reset(x)
        assert lane.pending()
        cnt.load(f)
    st = cnt.finish(ABUNDANCE, x)
    fp = st.fingerprint(x)
    lane.wait()
    assert fp == fingerprint_of(keys_of(k, other, ABUNDANCE))


@gpu
@pytest.mark.parametrize("on", ["null", "lane"])
def test_d_reset_then_load_counts(lane, reads, other, on):
    """the same with Counter.load_counts, the host-path entry of the dense table (a synchronous copy on the null stream)"""
    import torch
    k = 11
    table = O.count_reads(k, other).tobytes()
    cnt = br_amd.Counter(k, strategy=DENSE)
    cnt.add_reads(reads)
    torch.cuda.synchronize()
    x = None if on == "null" else lane.stream
    lane.delay(on="null" if on == "null" else None)
    cnt.reset(x)
    assert lane.pending()
    cnt.load_counts(0, table)
    st = cnt.finish(ABUNDANCE, x)
    fp = st.fingerprint(x)
    lane.wait()
    assert fp == fingerprint_of(keys_of(k, other, ABUNDANCE))


@gpu
@pytest.mark.parametrize("on", ["null", "lane"])
@pytest.mark.parametrize("strategy,k", [(DENSE, 15), (SORTED, 15), (TABLE, 25)], ids=["dense-k15", "sorted-k15", "table-k25"])
def test_d_finish_into_then_reset_then_add_reads(lane, reads, other, strategy, k, on):
    """finish_into queued on a busy stream X, reset on X, then the host-path add_reads at once: the finish still reads the
    counter (the partitioned one: its batches and its partition workspace) when the next batch arrives on the counter's own
    stream.  `dst` is the set of the first batch, the counter's next finish the set of `other`"""
    import torch
    cnt = br_amd.Counter(k, strategy=strategy)
    cnt.add_reads(reads)
    want_first = cnt.finish(ABUNDANCE).fingerprint()  # the ordinary way (and the table's key count is read back here, not below)
    dst = br_amd.Pcon.new(k)
    torch.cuda.synchronize()
    x = None if on == "null" else lane.stream
    lane.delay(on="null" if on == "null" else None)
    cnt.finish_into(ABUNDANCE, dst, x)
    cnt.reset(x)
    assert lane.pending()  # the finish and the reset are still queued behind the delay
    cnt.add_reads(other)
    first = dst.fingerprint(x)
    second = cnt.finish(ABUNDANCE, x).fingerprint(x)
    lane.wait()
    assert want_first == fingerprint_of(keys_of(k, reads, ABUNDANCE)) != fingerprint_of(keys_of(k, other, ABUNDANCE))
    assert first == want_first
    assert second == fingerprint_of(keys_of(k, other, ABUNDANCE))


def emptied_counter(k, strategy, reads):
    """a counter that has counted a batch of this size and was reset, the ordinary way: the counting table exists and is
    large enough, so that the next add_batch_device only enqueues (a first batch allocates the table and waits for its stream)"""
    import torch
    cnt = br_amd.Counter(k, strategy=strategy)
    cnt.add_reads(reads)
    cnt.reset()
    torch.cuda.synchronize()
    return cnt


@gpu
@pytest.mark.parametrize("strategy,k", [(DENSE, 11), (TABLE, 25)], ids=["dense-k11", "table-k25"])
@pytest.mark.parametrize("reader", ["abundance_batch", "get_counts"])
def test_d_add_batch_device_then_host_lookup(lane, reads, decoy, strategy, k, reader):
    """a batch counted on the lane behind the delay, then a host-path lookup (which works on the counter's own stream) at
    once: it answers for the batch, not for the empty counter"""
    real_b = batch_of(reads)
    cnt = emptied_counter(k, strategy, decoy)
    inp = lane.stage(batch_of(decoy), real_b)
    add_device(cnt, inp, lane.stream)
    assert lane.pending()
    if reader == "abundance_batch":
        got = cnt.abundance_batch(real_b["bases"], real_b["offs"], ABUNDANCE)[0]
        want, empty = profile_of(k, reads, reads), profile_of(k, [], reads)
    else:
        got = cnt.get_counts(cover.kmers_of(reads[0], k)[:4000])
        table = ab.count_table([O.hashes(k, r) for r in reads])
        want = ab.lookup(table, O.hashes(k, reads[0])[:4000])
        empty = np.zeros_like(want)
    lane.wait()
    assert not np.array_equal(want, empty) and not np.array_equal(want, profile_of(k, decoy, reads)[:want.size])
    assert np.array_equal(got, want)


@gpu
def test_d_add_batch_device_then_save(lane, reads, decoy, tmp_path):
    """the same with the host-path Counter.save: the key file holds the batch counted on the lane"""
    k = 25
    cnt = emptied_counter(k, TABLE, decoy)
    inp = lane.stage(batch_of(decoy), batch_of(reads))
    with open(tmp_path / "lane.keys", "wb") as f:
        add_device(cnt, inp, lane.stream)
        assert lane.pending()
        cnt.save(f)
    lane.wait()
    back = br_amd.Counter(k, strategy=TABLE)
    with open(tmp_path / "lane.keys", "rb") as f:
        back.load(f)
    assert back.table_info()["keys"] == keys_of(k, reads).size
    assert back.finish(ABUNDANCE).fingerprint() == fingerprint_of(keys_of(k, reads, ABUNDANCE))


@gpu
@pytest.mark.parametrize("on", ["null", "lane"])
def test_d_reset_then_count_fasta(lane, reads, other, on, tmp_path):
    """reset on a busy stream X, then Counter.count_fasta (the host pipeline counts on the counter's own stream)"""
    import torch
    k = 25
    with open(tmp_path / "other.fasta", "wb") as f:
        f.write(b"".join(b">%d\n%s\n" % (i, r) for i, r in enumerate(other)))
    cnt = br_amd.Counter(k, strategy=TABLE)
    cnt.add_reads(reads)
    torch.cuda.synchronize()
    x = None if on == "null" else lane.stream
    lane.delay(on="null" if on == "null" else None)
    with open(tmp_path / "other.fasta", "rb") as f:
        cnt.reset(x)
        assert lane.pending()
        cnt.count_fasta(f)
    st = cnt.finish(ABUNDANCE, x)
    fp = st.fingerprint(x)
    lane.wait()
    assert fp == fingerprint_of(keys_of(k, other, ABUNDANCE))


# ---- E: lazy state across streams ------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("k", [19, 21], ids=["k19-lazy-bits", "k21-sparse"])
def test_e_lazy_set_state_on_two_streams(lane, reads, k):
    """a set whose probe index (and, at k = 19, bit vector) does not exist yet: first use on the lane behind the delay, then
    at once on a second stream from the same thread"""
    import torch
    st = br_amd.Pcon.from_count(reads, k, ABUNDANCE, strategy=SORTED)
    assert st.bits_state() == (1 if k == 19 else 2) and not st.index_info()["valid"]
    inp = {name: dev(a) for name, a in batch_of(reads).items()}
    n, total = sizes(inp)
    out = alloc({"a": (total, "uint8"), "b": (total, "uint8"), "c": (2 * total + 4096, "uint8"), "c_offs": (n + 1, "int64")})
    s2 = lane.second
    torch.cuda.synchronize()
    lane.delay()
    assert lane.pending()  # (the first use builds the lazy state and may wait for the lane: asserted as the call is issued)
    st.cover_batch_device(ptr(inp["bases"]), ptr(inp["offs"]), n, total, ptr(out["a"]), None, None, lane.stream)
    st.cover_batch_device(ptr(inp["bases"]), ptr(inp["offs"]), n, total, ptr(out["b"]), None, None, s2.cuda_stream)
    fp = st.fingerprint(s2.cuda_stream)
    with torch.cuda.stream(s2):
        b = out["b"].cpu().numpy()
    a = lane.fetch(out["a"])
    keys = keys_of(k, reads, ABUNDANCE)
    want = cover_of(k, keys, reads)[0]
    assert a.tobytes() == want.tobytes() and b.tobytes() == want.tobytes() and fp == fingerprint_of(keys)
    if k == 19:  # a walking corrector materialises the lazy bit vector: on the lane, then the vector is read on the second stream
        chain = br_amd.Chain(st, [("graph", 5, 7)], two_side=True)
        few = reads[:6]
        fb = {name: dev(x) for name, x in batch_of(few).items()}
        torch.cuda.synchronize()
        lane.delay()
        assert lane.pending()
        t = chain.correct_batch_device(ptr(fb["bases"]), ptr(fb["offs"]), len(few), fb["bases"].numel(), ptr(out["c"]), out["c"].numel(),
                                       ptr(out["c_offs"]), lane.stream)
        assert st.bits_state() == 0
        listed = alloc({"list": (keys.size, "int64")})["list"]
        got_n = st.extract_keys_device(0, st.n_hashes(), ptr(listed), keys.size, s2.cuda_stream)
        with torch.cuda.stream(s2):
            got_keys = listed.cpu().numpy()
        corrected = lane.fetch(out["c"])[:t].tobytes()
        assert got_n == keys.size and np.array_equal(np.sort(got_keys.view(np.uint64)), keys)
        om = O.build_methods(O.Solid.sparse_from_count(k, reads, ABUNDANCE), ["graph"], 5, 7)
        assert corrected == b"".join(O.correct_record(om, r, True) for r in few)
    lane.wait()


@gpu
def test_e_count_view_on_two_streams(lane, reads):
    """prepare_lookup on the lane behind the delay, abundance at once on a second stream"""
    import torch
    k = 15
    cnt = br_amd.Counter(k, strategy=SORTED)
    cnt.add_reads(reads)
    inp = {name: dev(a) for name, a in batch_of(reads).items()}
    n, total = sizes(inp)
    out = alloc({"profile": (total, "uint8")})
    s2 = lane.second
    torch.cuda.synchronize()
    lane.delay()
    assert lane.pending()
    cnt.prepare_lookup(lane.stream)
    cnt.abundance_batch_device(ptr(inp["bases"]), ptr(inp["offs"]), n, total, ABUNDANCE, ptr(out["profile"]), None, None, s2.cuda_stream)
    with torch.cuda.stream(s2):
        got = out["profile"].cpu().numpy()
    lane.wait()
    assert got.tobytes() == profile_of(k, reads, reads).tobytes()


# ---- F: the kernel timers record on the caller's stream ----------------------------------------------------------------------------

@gpu
def test_f_timers_on_the_lane(lane, reads, decoy):
    _lib.profile_reset()
    _lib.profile_enable(True)
    try:
        got = probe(lane, op_counter(DENSE, 11, "finish"), batch_of(decoy), batch_of(reads))
        launches = {name: _lib.profile_get(name)[1] for name in ("count_dense", "threshold")}
    finally:
        _lib.profile_enable(False)
        _lib.profile_reset()
    assert got[0] == fingerprint_of(keys_of(11, reads, ABUNDANCE))
    assert launches == {"count_dense": 3, "threshold": 3}  # plain real, plain decoy, lane
