"""Who holds the keys of a solid set (br_amd/csrc/brx_setstate.hpp: set_holder), on the host: tests/set_holder_host.cpp
built with the address and undefined-behaviour sanitizers and run as a child process.  The expected column was written by
hand from the rule's three sentences and from what the enumerating entries did before the rule was stated once
(ensure_bits, index_ensure, the key-file listing, popcount, keylist_device, fingerprint), not from the program's output.

A case is bits x list x index, after the table of reachable states in brx_internal.hpp (struct brx_set)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

# bits: sparse, bits_stale
CURRENT, LAZY, SPARSE = "0,0", "0,1", "1,0"
CAP = 1_548_572
# list: keylist_valid, listed_n, list_cap
NO_LIST = "0,0,0"
DROPPED = f"0,{CAP - 5},{CAP}"          # an invalidated list: counter and buffer are still there
COMPLETE = f"1,{CAP - 5},{CAP}"
EMPTY = "1,0,0"                          # the empty list of a fresh sparse set: no buffer at all
FULL = f"1,{CAP},{CAP}"                 # the boundary: every entry used
TRUNCATED = f"1,{CAP + 1},{CAP}"        # ... one key more than the list holds
FAR = f"1,1996140,{CAP}"
# index: idx_valid, idx_exact, have_lines
NO_INDEX = "0,0,0"
STALE_INDEX = "0,1,1"                    # invalidated by a mutation: the flags of the last build and the lines remain
ACCELERATOR = "1,0,1"
EXACT = "1,1,1"                          # closed or open alike: the rule does not ask

TABLE = [
    # ---- a current bit vector -------------------------------------------------------------------------------------------
    (CURRENT, NO_LIST, NO_INDEX, "Bits"),          # brx_set_new, a .solid stream, a dense finish, k below the indexed range
    (CURRENT, NO_LIST, ACCELERATOR, "Bits"),       # ... after brx_set_index_build / index_ensure
    (CURRENT, NO_LIST, STALE_INDEX, "Bits"),       # ... after a mutation
    (CURRENT, DROPPED, NO_INDEX, "Bits"),          # or_keys / insert on a finished set: the list is void
    (CURRENT, NO_LIST, EXACT, "Bits"),             # a lazy set with a handed-over table, materialised since
    (CURRENT, COMPLETE, NO_INDEX, "KeyList"),      # BRX_LAZY_BITS=0 finish; set algebra and key files at indexed k
    (CURRENT, COMPLETE, ACCELERATOR, "KeyList"),   # ... after index_ensure
    (CURRENT, COMPLETE, EXACT, "KeyList"),         # a lazy finish, indexed, materialised since
    (CURRENT, FULL, NO_INDEX, "KeyList"),
    (CURRENT, TRUNCATED, NO_INDEX, "Bits"),        # BRX_LAZY_BITS=0 finish that found more than its list holds
    (CURRENT, FAR, NO_INDEX, "Bits"),
    (CURRENT, TRUNCATED, ACCELERATOR, "Bits"),     # ... after index_ensure (built from the bits)
    # ---- a lazy bit vector ------------------------------------------------------------------------------------------------
    (LAZY, COMPLETE, NO_INDEX, "KeyList"),         # the partitioned finish
    (LAZY, FULL, NO_INDEX, "KeyList"),
    (LAZY, COMPLETE, EXACT, "KeyList"),            # ... after index_ensure
    (LAZY, COMPLETE, STALE_INDEX, "KeyList"),      # a second finish_into the same set: the old lines are still allocated
    (LAZY, NO_LIST, EXACT, "Table"),               # brx_set_index_build_from_keys_device with a foreign list
    (LAZY, DROPPED, EXACT, "Table"),
    (LAZY, DROPPED, NO_INDEX, "None"),             # ... and brx_set_index_drop after that: the keys are gone
    (LAZY, TRUNCATED, NO_INDEX, "None"),           # unreachable (a lazy list gets the exact bound): still no list
    (LAZY, TRUNCATED, EXACT, "Table"),
    (LAZY, NO_LIST, ACCELERATOR, "None"),          # unreachable: an accelerator is not exact
    # ---- a sparse set -------------------------------------------------------------------------------------------------------
    (SPARSE, EMPTY, NO_INDEX, "KeyList"),          # the fresh set: the empty list
    (SPARSE, COMPLETE, NO_INDEX, "KeyList"),       # a finish, a key file, set algebra
    (SPARSE, COMPLETE, EXACT, "KeyList"),          # ... indexed
    (SPARSE, DROPPED, EXACT, "Table"),             # closed: a handed-over list (multi-GPU exchange); open: insert_batch
    (SPARSE, NO_LIST, EXACT, "Table"),
    (SPARSE, DROPPED, STALE_INDEX, "None"),
    (SPARSE, NO_LIST, "1,1,0", "None"),            # (a valid index without lines cannot be: it would still not be read)
    (SPARSE, TRUNCATED, NO_INDEX, "None"),         # what index_ensure refuses with "without a complete key list"
    (SPARSE, FAR, NO_INDEX, "None"),
]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not found")
    exe = tmp_path_factory.mktemp("set_holder") / "set_holder_host"
    build = subprocess.run(
        ["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-Wall", "-Wextra",
         os.path.join(HERE, "set_holder_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    assert not build.stderr.strip(), build.stderr  # no warnings
    return str(exe)


def test_set_holder_table(program):
    cases = [f"{b},{l},{i}" for b, l, i, _ in TABLE]
    run = subprocess.run([program] + cases, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    got = run.stdout.splitlines()
    assert len(got) == len(TABLE), run.stdout
    bad = [(c, g, row[3]) for c, g, row in zip(cases, got, TABLE) if g != row[3]]
    assert not bad, "\n".join(f"{c}: got {g}, want {w}" for c, g, w in bad)


def test_the_rule_is_asked_not_restated():
    """outside the rule, the marker, the resolver and index_info nobody reads keylist_valid; outside the list's writers and
    the resolver nobody reads its device counter"""
    csrc = os.path.join(os.path.dirname(HERE), "br_amd", "csrc")
    for name in sorted(n for n in os.listdir(csrc) if n.endswith((".hip", ".hpp"))):
        with open(os.path.join(csrc, name)) as f:
            text = f.read()
        if name not in ("brx_setstate.hpp", "brx_internal.hpp", "brx_index.hip"):
            assert "keylist_valid" not in text, name
        if name not in ("brx_internal.hpp", "brx_index.hip", "brx_partbuild.hip", "brx_counttable.hip", "brx_set.hip", "brx_keyfile.hip"):
            assert "d_keylist_n" not in text, name
