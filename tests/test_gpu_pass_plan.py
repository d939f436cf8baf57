"""The chain executes what plan_pass (br_amd/csrc/brx_plan.hpp) decides, from ONE reading of the switches per batch, taken
on the thread that calls the library: the form a pass took shows in Chain.last_stats() and in the profile timers, the
bytes are the oracle's whatever the form.  The rule itself is checked without a GPU by test_pass_plan_cpu.py."""
import functools

import pytest

import br_amd
from br_amd import _lib
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CONFIRM, MAX_SEARCH = 2, 7


@pytest.fixture(scope="module")
def reads(raw_reads):
    return tuple(r[:2000] for r in raw_reads[:25])


@pytest.fixture(scope="module")
def expected(reads, solid_fixture_bytes):
    ref = O.Solid.from_bytes(solid_fixture_bytes)

    @functools.lru_cache(maxsize=None)
    def of(names, two_side):
        om = O.build_methods(ref, list(names), CONFIRM, MAX_SEARCH)
        return [O.correct_record(om, r, two_side) for r in reads]
    return of


def chain_of(gs, names, two_side):
    return br_amd.Chain(gs, [(m, CONFIRM, MAX_SEARCH) for m in names], two_side=two_side)


def test_one_takes_the_lane_form_unless_switched_off(monkeypatch, reads, expected, solid_fixture_bytes):
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    monkeypatch.delenv("BRX_LANE", raising=False)
    chain = chain_of(gs, ("one",), True)
    assert chain.correct_reads(reads) == expected(("one",), True)
    assert chain.last_stats()["lane_units"] > 0
    monkeypatch.setenv("BRX_LANE", "0")
    chain = chain_of(gs, ("one",), True)
    assert chain.correct_reads(reads) == expected(("one",), True)
    assert chain.last_stats()["lane_units"] == 0


def test_graph_reverse_pass_is_lean_unless_switched_off(monkeypatch, reads, expected, solid_fixture_bytes):
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    _lib.profile_enable(True)
    try:
        for lean, launched in ((None, True), ("0", False)):
            if lean is None:
                monkeypatch.delenv("BRX_REV_LEAN", raising=False)
            else:
                monkeypatch.setenv("BRX_REV_LEAN", lean)
            _lib.profile_reset()
            assert chain_of(gs, ("graph",), False).correct_reads(reads) == expected(("graph",), False)
            assert _lib.profile_get("correct_pass_graph")[1] > 0
            assert (_lib.profile_get("rev_verify")[1] > 0) == launched, lean
    finally:
        _lib.profile_enable(False)


def test_switches_are_read_per_batch_not_per_chain(monkeypatch, reads, expected, solid_fixture_bytes):
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    chain = chain_of(gs, ("one",), True)
    monkeypatch.setenv("BRX_LANE", "0")
    assert chain.correct_reads(reads) == expected(("one",), True)
    assert chain.last_stats()["lane_units"] == 0
    monkeypatch.delenv("BRX_LANE")
    assert chain.correct_reads(reads) == expected(("one",), True)
    assert chain.last_stats()["lane_units"] > 0


def test_async_batch_runs_under_the_switches_of_the_call(monkeypatch, reads, expected, solid_fixture_bytes):
    """the record is taken by brx_chain_correct_batch_async itself, on the calling thread: what the host does to its
    environment once the call has returned does not reach the batch"""
    gs = br_amd.Pcon.from_pcon_solid(solid_fixture_bytes)
    chain = chain_of(gs, ("one",), True)
    bases, offs = br_amd.pack_reads(reads)
    monkeypatch.setenv("BRX_LANE", "0")
    chain.correct_batch_async(bases, offs)
    monkeypatch.delenv("BRX_LANE")
    out, oo = chain.correct_batch_wait()
    got = [out[int(oo[i]):int(oo[i + 1])].tobytes() for i in range(len(reads))]
    assert got == expected(("one",), True)
    assert chain.last_stats()["lane_units"] == 0
