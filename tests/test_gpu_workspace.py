"""Workspaces that are grown and then reused (br_amd/csrc/brx_devbuf.hpp): a small batch, a batch large enough to grow
every buffer of the object, then the small batch again in the grown buffers -- on one correction chain, and on a counter of
each strategy that keeps a workspace between batches.  Every expected value comes from the CPU oracle."""
import numpy as np
import pytest

import br_amd
from br_amd import _lib, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

K, ABUNDANCE = 15, 2
METHODS = ["one", "two", "graph", "greedy", "gap_size"]
GENOME_LEN = 20_000

_cache = {}


def _batch(read_len, first, n):
    cfg = synth.config(genome_len=GENOME_LEN, read_len=read_len)
    bases, offs = synth.reads_host(cfg, synth.genome_host(cfg), first, n)
    return bases, offs


def _reads(bases, offs):
    return [bases[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(offs.size - 1)]


def data():
    """the two batches, the oracle's set of small + large + small, and the oracle's corrections: computed once, never modified"""
    if not _cache:
        small, large = _batch(300, 0, 40), _batch(900, 40, 600)
        counted = _reads(*small) + _reads(*large) + _reads(*small)
        ref = O.Solid.from_count(K, O.count_reads(K, counted), ABUNDANCE)
        om = O.build_methods(ref, METHODS, 5, 7)
        _cache.update(small=small, large=large, counted=counted, ref=ref,
                      exp_small=O.correct_batch(om, small[0], small[1], False),
                      exp_large=O.correct_batch(om, large[0], large[1], False))
    return _cache


def _fixed(batch, exp):
    """reads of the batch that the oracle changes"""
    got = _reads(exp[0], exp[1])
    return sum(a != b for a, b in zip(_reads(*batch), got))


def test_chain_small_large_small():
    d = data()
    assert _fixed(d["small"], d["exp_small"]) >= 1 and _fixed(d["large"], d["exp_large"]) >= 1
    gs = br_amd.Pcon.from_count(d["counted"], K, ABUNDANCE)
    assert gs.to_solid_bytes() == d["ref"].to_bytes()
    chain = br_amd.Chain(gs, [(m, 5, 7) for m in METHODS], two_side=False)  # (the reverse second pass)
    outs = []
    for name in ("small", "large", "small"):
        out, oo = chain.correct_batch(*d[name])
        exp, exp_o = d["exp_" + name]
        assert np.array_equal(oo, exp_o) and np.array_equal(out, exp), name
        assert chain.last_stats()["fixes"] > 0, name
        outs.append((out, oo))
    assert np.array_equal(outs[2][0], outs[0][0]) and np.array_equal(outs[2][1], outs[0][1])


def test_counters_small_large_small_reset():
    d = data()
    want = d["ref"].to_bytes()
    sets = {}
    for strategy in (_lib.COUNT_SORTED, _lib.COUNT_TABLE):
        cnt = br_amd.Counter(K, 0, strategy)
        for rnd in range(2):  # count, finish, reset, count again in the grown workspace, finish
            for name in ("small", "large", "small"):
                cnt.add_batch(*d[name])
            sets[strategy, rnd] = cnt.finish(ABUNDANCE).to_solid_bytes()
            cnt.reset()
    for key, got in sets.items():
        assert got == want, key
    assert sets[_lib.COUNT_SORTED, 1] == sets[_lib.COUNT_TABLE, 1]
