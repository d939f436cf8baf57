"""The rule that gives a correction pass its form (br_amd/csrc/brx_plan.hpp: read_correct_tuning, plan_pass and the grid
rules), on the host: tests/pass_plan_host.cpp built with the address and undefined-behaviour sanitizers and run as a
child process, once per environment.  The expected lines were worked out from the chain's control flow as it stood
before the rule was gathered in one place (the method loop of brx_correct.hip, launch_pass, lane_pass), not from the
program's output."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")

ONE, TWO, GRAPH, GREEDY, GAP = range(5)
N, TOTAL = 100_000, 100_000_000     # reads and bases of the batch (1 kb reads)
SET = "19,1,25,5,1"                 # k = 19, bit vector, index of 2^25 lines, 5 windows, occupancy bits
SET27 = "19,1,27,5,1"               # ... of 2^27 lines
SPARSE = "21,0,25,7,1"              # k = 21: no bit vector
NOTHING = "21,0,0,0,0"              # neither bits nor index (a stale vector, index switched off)
BITS_ONLY = "15,1,0,0,0"


def case(method, d, s=SET, confirm=2, max_search=7, revcomp=0, flip=None, n=N, total=TOTAL):
    """dir 1 is entered with flip = 1 by the first method of the scan; what follows reads a buffer stored back to front"""
    flip = d if flip is None else flip
    return f"pass:{s},{method},{confirm},{max_search},{d},{revcomp},{flip},{n},{total}"


NO_TAIL = "tail=4294967295/4294967295"
UNITS = TOTAL // 256 + N + 1        # one unit per 256 bases and one more per read
LANE_ONE = f"LANE idx=1 mask=0 succ=0 chunk=256 sync=4 {NO_TAIL} units<={UNITS} ap_grid=1048576"
LANE_WALK = f"LANE idx=1 mask=1 succ=1 chunk=256 sync=4 {NO_TAIL} units<={UNITS} ap_grid=1048576"
REV_LEAN = "REV_LEAN scan=64 verify=8/8 idx=1 rev_batch=1 blocks=2048"
TUNING = ("tuning group=0/0 group_rev=0/0 walk=8 verify=8 one_v1=0 balance=0 tune=0 rev_lean=1 rev_batch=1 rev_lean_one=0 index_fwd=29 "
          "lane_rev=0 line_bits=1 redo_max=4096 maxpath=0 lane=1 lane_walk=1 max_log_lines=26 chunk=0 sync=4 tail=0 mask=1 succ=1 "
          "ap_grid=1048576")


def tuning(**changed):
    fields = [f.split("=") for f in TUNING.split()[1:]]
    assert set(changed) <= {k for k, _ in fields}
    return "tuning " + " ".join(f"{k}={changed.get(k, v)}" for k, v in fields)


def group(kernel, width, idx, rev_batch, blocks, lds="0/0", tune=0):
    return f"GROUP {kernel} width={width} idx={idx} rev_batch={rev_batch} blocks={blocks} lds={lds} tune={tune}"


# (environment, [(case, expected line)])
TABLE = [
    # ---- defaults ----------------------------------------------------------------------------------------------------
    ({}, [
        ("tuning", TUNING),
        ("blocks:100000,64", "blocks reads=100000 width=64 plain=2048 balanced=2048"),
        (case(ONE, 0), "one dir0 " + LANE_ONE),
        (case(TWO, 0), "two dir0 " + group("correct_kernel", 16, 0, 0, 2048)),
        (case(GRAPH, 0), "graph dir0 " + LANE_WALK),
        (case(GAP, 0), "gap_size dir0 " + LANE_WALK),
        (case(GREEDY, 0), "greedy dir0 " + group("correct_kernel", 16, 1, 0, 2048, "1984/31744")),
        (case(ONE, 1), "one dir1 " + group("one_kernel", 64, 1, 1, 2048)),
        (case(TWO, 1), "two dir1 " + group("correct_kernel", 64, 1, 1, 2048)),
        (case(GRAPH, 1), "graph dir1 " + REV_LEAN),
        (case(GAP, 1), "gap_size dir1 " + REV_LEAN),
        (case(GAP, 1, flip=0), "gap_size dir1 " + REV_LEAN),  # a later method of the scan: its input is stored reversed already
        (case(GREEDY, 1), "greedy dir1 " + group("correct_kernel", 64, 1, 1, 2048, "1984/7936")),
        # the second scan over the reverse complement: forward passes in every respect, never in block form
        (case(ONE, 0, revcomp=1), "one dir0 " + LANE_ONE),
        (case(TWO, 0, revcomp=1), "two dir0 " + group("correct_kernel", 16, 0, 0, 2048)),
        (case(GRAPH, 0, revcomp=1), "graph dir0 " + LANE_WALK),
        (case(GAP, 0, revcomp=1), "gap_size dir0 " + LANE_WALK),
        (case(GREEDY, 0, revcomp=1), "greedy dir0 " + group("correct_kernel", 16, 1, 0, 2048, "1984/31744")),
        # an index of 2^27 lines: One stays with the groups (8 lanes with an index), the walkers do not; no block form
        # past 2^26 lines
        (case(ONE, 0, SET27), "one dir0 " + group("one_kernel", 8, 1, 0, 2048)),
        (case(GRAPH, 0, SET27), "graph dir0 " + LANE_WALK),
        (case(ONE, 1, SET27), "one dir1 " + group("one_kernel", 64, 1, 0, 2048)),
        (case(ONE, 1, "19,1,25,9,1"), "one dir1 " + group("one_kernel", 64, 1, 0, 2048)),  # nine windows
        (case(ONE, 1, "19,1,25,5,0"), "one dir1 " + group("one_kernel", 64, 1, 0, 2048)),  # no occupancy bits
        # no bit vector: everything probes the index
        (case(TWO, 0, SPARSE), "two dir0 " + group("correct_kernel", 16, 1, 0, 2048)),
        # no index: 16-lane groups forward, lanes over the bit vector without a successor table
        (case(ONE, 0, BITS_ONLY), f"one dir0 LANE idx=0 mask=0 succ=0 chunk=256 sync=4 {NO_TAIL} units<={UNITS} ap_grid=1048576"),
        (case(GRAPH, 0, BITS_ONLY), f"graph dir0 LANE idx=0 mask=1 succ=0 chunk=256 sync=4 {NO_TAIL} units<={UNITS} ap_grid=1048576"),
        (case(TWO, 1, BITS_ONLY), "two dir1 " + group("correct_kernel", 64, 0, 0, 2048)),
        # where the lane form does not apply: neither bits nor index, k above 31, a forward pass over a buffer stored back
        # to front, confirm outside 1 .. 5 (Graph has no look-aheads), unit numbers past 32 bits
        (case(ONE, 0, NOTHING), "one dir0 " + group("one_kernel", 16, 0, 0, 2048)),
        (case(ONE, 0, "33,1,25,5,1"), "one dir0 " + group("one_kernel", 8, 1, 0, 2048)),
        (case(ONE, 0, flip=1), "one dir0 " + group("one_kernel", 8, 1, 0, 2048)),
        (case(ONE, 0, confirm=6), "one dir0 " + group("one_kernel", 8, 1, 0, 2048)),
        (case(ONE, 0, confirm=0), "one dir0 " + group("one_kernel", 8, 1, 0, 2048)),
        (case(GAP, 0, confirm=6), "gap_size dir0 " + group("correct_kernel", 8, 1, 0, 2048)),
        (case(GRAPH, 0, confirm=6), "graph dir0 " + LANE_WALK),
        (case(ONE, 0, total=0xfffffff0 * 2048), "one dir0 " + group("one_kernel", 8, 1, 0, 2048)),
        # the chunk follows the input: 1 Gbp -> 544 bases, 4 Gbp -> the cap
        (case(ONE, 0, total=10 ** 9), f"one dir0 LANE idx=1 mask=0 succ=0 chunk=544 sync=4 {NO_TAIL} units<={10 ** 9 // 544 + N + 1} ap_grid=1048576"),
        (case(ONE, 0, total=4 * 10 ** 9),
         f"one dir0 LANE idx=1 mask=0 succ=0 chunk=2048 sync=4 {NO_TAIL} units<={4 * 10 ** 9 // 2048 + N + 1} ap_grid=1048576"),
        # Greedy: 16 groups of 11 408 B do not fit 160 KiB, 8 do; a 143 x 143 table fits at no width
        (case(GREEDY, 0, "31,1,25,5,1", max_search=39), "greedy dir0 " + group("correct_kernel", 32, 1, 0, 2048, "11408/91264")),
        (case(GREEDY, 1, "31,1,25,5,1", max_search=110), "greedy dir1 NO_LDS table=143x143"),
        (case(GREEDY, 0, "31,1,25,5,1", max_search=110), "greedy dir0 NO_LDS table=143x143"),
        # the visited lists of 100 000 reads: 2048 blocks of 32 eight-lane groups
        ("lists:100000", "lists reads=100000 lists=65536 verify_grid=2048x32 redo_grid=2048x4 walk_list_grid=128x32"),
        ("lists:20", "lists reads=20 lists=64 verify_grid=2x32 redo_grid=16x4 walk_list_grid=2x32"),
    ]),
    # ---- the group kernels only ----------------------------------------------------------------------------------------
    ({"BRX_LANE": "0"}, [
        ("tuning", tuning(lane=0)),
        (case(ONE, 0), "one dir0 " + group("one_kernel", 8, 1, 0, 2048)),
        (case(GRAPH, 0), "graph dir0 " + group("correct_kernel", 8, 1, 0, 2048)),
        (case(GAP, 0), "gap_size dir0 " + group("correct_kernel", 8, 1, 0, 2048)),
        (case(ONE, 0, BITS_ONLY), "one dir0 " + group("one_kernel", 16, 0, 0, 2048)),
        # 8192 reads: fewer than the resident groups, so the width doubles while 2 * reads * width <= 393 216 lanes
        (case(ONE, 0, n=8192, total=8_192_000), "one dir0 " + group("correct_kernel", 32, 1, 0, 1024)),
        (case(GRAPH, 0, n=8192, total=8_192_000), "graph dir0 " + group("correct_kernel", 32, 1, 0, 1024)),
        (case(TWO, 0, n=8192, total=8_192_000), "two dir0 " + group("correct_kernel", 32, 0, 0, 1024)),
        (case(ONE, 0, n=2000, total=2_000_000), "one dir0 " + group("one_kernel", 64, 1, 0, 500)),
    ]),
    ({"BRX_LANE_WALK": "0"}, [
        (case(ONE, 0), "one dir0 " + LANE_ONE),
        (case(GRAPH, 0), "graph dir0 " + group("correct_kernel", 8, 1, 0, 2048)),
    ]),
    # ---- widths ----------------------------------------------------------------------------------------------------------
    ({"BRX_LANE": "0", "BRX_GROUP": "5"}, [  # invalid: the default, and a set variable switches the widening off
        ("tuning", tuning(lane=0, group="1/5")),
        (case(ONE, 0, n=8192, total=8_192_000), "one dir0 " + group("one_kernel", 8, 1, 0, 256)),
        (case(ONE, 1, n=8192, total=8_192_000), "one dir1 " + group("one_kernel", 64, 1, 1, 2048)),  # (BRX_GROUP_REV falls back to it)
    ]),
    ({"BRX_LANE": "0", "BRX_GROUP": "4"}, [
        (case(ONE, 0), "one dir0 " + group("one_kernel", 4, 1, 0, 1563)),
        (case(GRAPH, 0), "graph dir0 " + group("correct_kernel", 8, 1, 0, 2048)),  # below 16: BRX_GROUP_WALK
        (case(TWO, 0), "two dir0 " + group("correct_kernel", 16, 0, 0, 2048)),
        (case(GRAPH, 1), "graph dir1 " + group("correct_kernel", 8, 1, 1, 2048)),  # the reverse pass follows BRX_GROUP: not lean
    ]),
    ({"BRX_LANE": "0", "BRX_GROUP": "32"}, [
        (case(ONE, 0), "one dir0 " + group("correct_kernel", 32, 1, 0, 2048)),
    ]),
    ({"BRX_LANE": "0", "BRX_ONE_V1": "1", "BRX_TUNE": "3"}, [
        ("tuning", tuning(lane=0, one_v1=1, tune=3)),
        (case(ONE, 0), "one dir0 " + group("correct_kernel", 8, 1, 0, 2048, tune=3)),
    ]),
    ({"BRX_LANE": "0", "BRX_GROUP_WALK": "4"}, [
        (case(GRAPH, 0), "graph dir0 " + group("correct_kernel", 4, 1, 0, 1563)),
        ("lists:100000", "lists reads=100000 lists=100032 verify_grid=2048x32 redo_grid=2048x4 walk_list_grid=128x32"),
    ]),
    ({"BRX_GROUP_WALK": "3"}, [("tuning", TUNING)]),
    ({"BRX_GROUP_REV": "16"}, [
        ("tuning", tuning(group_rev="1/16")),
        (case(GRAPH, 1), "graph dir1 " + group("correct_kernel", 16, 1, 1, 2048)),
        (case(ONE, 0), "one dir0 " + LANE_ONE),
    ]),
    ({"BRX_BALANCE": "1"}, [
        ("blocks:100000,8", "blocks reads=100000 width=8 plain=2048 balanced=1563"),
        ("blocks:50000,8", "blocks reads=50000 width=8 plain=1563 balanced=1563"),
    ]),
    # ---- reverse passes ----------------------------------------------------------------------------------------------------
    ({"BRX_REV_LEAN": "0"}, [
        (case(GRAPH, 1), "graph dir1 " + group("correct_kernel", 64, 1, 1, 2048)),
        (case(GAP, 1), "gap_size dir1 " + group("correct_kernel", 64, 1, 1, 2048)),
    ]),
    ({"BRX_REV_LEAN_ONE": "1"}, [
        (case(ONE, 1), "one dir1 " + REV_LEAN),
        (case(TWO, 1), "two dir1 " + group("correct_kernel", 64, 1, 1, 2048)),
    ]),
    ({"BRX_LANE_REV": "1"}, [
        (case(GRAPH, 1), "graph dir1 " + LANE_WALK),
        (case(GAP, 1), "gap_size dir1 " + REV_LEAN),
    ]),
    ({"BRX_LANE_REV": "2"}, [
        (case(GRAPH, 1), "graph dir1 " + REV_LEAN),
        (case(GAP, 1), "gap_size dir1 " + LANE_WALK),
    ]),
    ({"BRX_REV_BATCH": "0"}, [
        (case(ONE, 1), "one dir1 " + group("one_kernel", 64, 1, 0, 2048)),
        (case(GRAPH, 1), "graph dir1 REV_LEAN scan=64 verify=8/8 idx=1 rev_batch=0 blocks=2048"),
    ]),
    ({"BRX_LINE_BITS": "0"}, [
        ("tuning", tuning(line_bits=0)),
        (case(ONE, 1), "one dir1 " + group("one_kernel", 64, 1, 0, 2048)),
    ]),
    # the grid that indexed 64 lists where the chain had sized 32: 20 reads in 16-lane groups are 2 blocks of 16 lists,
    # raised to the 64 a block of 4-lane verify groups indexes; every grid stays within them
    ({"BRX_REV_VERIFY_G": "4", "BRX_GROUP_WALK": "16", "BRX_REV_LEAN_ONE": "1"}, [
        ("tuning", tuning(verify=4, walk=16, rev_lean_one=1)),
        ("lists:20", "lists reads=20 lists=64 verify_grid=1x64 redo_grid=16x4 walk_list_grid=2x32"),
        (case(GRAPH, 1, n=20, total=20_000), "graph dir1 REV_LEAN scan=64 verify=4/4 idx=1 rev_batch=1 blocks=5"),
        (case(ONE, 1, n=20, total=20_000), "one dir1 REV_LEAN scan=64 verify=8/4 idx=1 rev_batch=1 blocks=5"),  # (One verifies at 8 lanes only)
    ]),
    ({"BRX_REV_VERIFY_G": "5"}, [("tuning", TUNING)]),
    # ---- index or bit vector -------------------------------------------------------------------------------------------------
    ({"BRX_INDEX_FWD": "2"}, [
        (case(TWO, 0), "two dir0 " + group("correct_kernel", 16, 1, 0, 2048)),
        (case(ONE, 0), f"one dir0 LANE idx=0 mask=0 succ=0 chunk=256 sync=4 {NO_TAIL} units<={UNITS} ap_grid=1048576"),
        (case(GRAPH, 0), f"graph dir0 LANE idx=0 mask=1 succ=0 chunk=256 sync=4 {NO_TAIL} units<={UNITS} ap_grid=1048576"),
        (case(GREEDY, 1), "greedy dir1 " + group("correct_kernel", 64, 0, 0, 2048, "1984/7936")),  # Greedy's reverse pass follows the mask too
        (case(ONE, 0, SPARSE), "one dir0 " + LANE_ONE),
    ]),
    # ---- the lane form's own switches ----------------------------------------------------------------------------------------
    ({"BRX_LANE_MAX_LOG_LINES": "27"}, [(case(ONE, 0, SET27), "one dir0 " + LANE_ONE)]),
    ({"BRX_LANE_SYNC": "0"}, [("tuning", tuning(sync=1))]),
    ({"BRX_LANE_SYNC": "99"}, [("tuning", tuning(sync=32))]),
    ({"BRX_LANE_CHUNK": "10", "BRX_LANE_SYNC": "7", "BRX_AP_GRID": "512"}, [
        ("tuning", tuning(chunk=64, sync=7, ap_grid=512)),
        (case(ONE, 0), f"one dir0 LANE idx=1 mask=0 succ=0 chunk=64 sync=7 {NO_TAIL} units<={TOTAL // 64 + N + 1} ap_grid=512"),
    ]),
    ({"BRX_LANE_CHUNK": "1000"}, [
        (case(GRAPH, 0), f"graph dir0 LANE idx=1 mask=1 succ=1 chunk=1000 sync=4 {NO_TAIL} units<={TOTAL // 1000 + N + 1} ap_grid=1048576"),
    ]),
    ({"BRX_LANE_TAIL": "1"}, [  # One only, from 64 reads on: units are bounded at a quarter of the chunk
        (case(ONE, 0), f"one dir0 LANE idx=1 mask=0 succ=0 chunk=256 sync=4 tail=80000/95000 units<={TOTAL // 64 + N + 1} ap_grid=1048576"),
        (case(ONE, 0, n=63, total=63_000), f"one dir0 LANE idx=1 mask=0 succ=0 chunk=256 sync=4 {NO_TAIL} units<={63_000 // 256 + 64} ap_grid=1048576"),
        (case(GRAPH, 0), "graph dir0 " + LANE_WALK),
    ]),
    ({"BRX_LANE_MASK": "2"}, [
        (case(ONE, 0), f"one dir0 LANE idx=1 mask=1 succ=0 chunk=256 sync=4 {NO_TAIL} units<={UNITS} ap_grid=1048576"),
        (case(GRAPH, 0), "graph dir0 " + LANE_WALK),
    ]),
    ({"BRX_LANE_MASK": "0", "BRX_LANE_SUCC": "0"}, [
        (case(GRAPH, 0), f"graph dir0 LANE idx=1 mask=0 succ=0 chunk=256 sync=4 {NO_TAIL} units<={UNITS} ap_grid=1048576"),
    ]),
    # ---- what a chain and the redo of poisoned reads take from the record ------------------------------------------------------
    ({"BRX_MAXPATH": "16", "BRX_REDO_MAX": "0"}, [("tuning", tuning(maxpath=16, redo_max=0))]),
    ({"BRX_MAXPATH": "0"}, [("tuning", TUNING)]),
    ({"BRX_MAXPATH": "2000000"}, [("tuning", TUNING)]),
]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not found")
    exe = tmp_path_factory.mktemp("pass_plan") / "pass_plan_host"
    build = subprocess.run(
        ["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-Wall", "-Wextra",
         "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INCLUDE, os.path.join(HERE, "pass_plan_host.cpp"), "-o", str(exe)],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    assert not build.stderr.strip(), build.stderr  # no warnings
    return str(exe)


@pytest.mark.parametrize("env,rows", TABLE, ids=[",".join(f"{k}={v}" for k, v in e.items()) or "defaults" for e, _ in TABLE])
def test_pass_plan_table(program, env, rows):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("BRX_")}
    run = subprocess.run([program] + [c for c, _ in rows], capture_output=True, text=True, env=dict(clean, **env))
    assert run.returncode == 0, run.stdout + run.stderr
    got = run.stdout.splitlines()
    assert len(got) == len(rows), run.stdout
    bad = [(c, g, w) for (c, w), g in zip(rows, got) if g != w]
    assert not bad, "\n".join(f"{c}\n  got  {g}\n  want {w}" for c, g, w in bad)


def test_every_switch_of_the_issue_is_in_the_record():
    """the header reads each of the chain's switches, and the correction sources read none of them themselves"""
    names = ("BRX_GROUP BRX_GROUP_REV BRX_GROUP_WALK BRX_REV_VERIFY_G BRX_ONE_V1 BRX_BALANCE BRX_TUNE BRX_REV_LEAN BRX_REV_BATCH "
             "BRX_REV_LEAN_ONE BRX_INDEX_FWD BRX_LANE_REV BRX_LINE_BITS BRX_REDO_MAX BRX_MAXPATH BRX_LANE BRX_LANE_WALK "
             "BRX_LANE_MAX_LOG_LINES BRX_LANE_CHUNK BRX_LANE_SYNC BRX_LANE_TAIL BRX_LANE_MASK BRX_LANE_SUCC BRX_AP_GRID").split()
    csrc = os.path.join(os.path.dirname(HERE), "br_amd", "csrc")
    with open(os.path.join(csrc, "brx_plan.hpp")) as f:
        plan = f.read()
    for n in names:
        assert f'("{n}"' in plan, n
    for src in ("brx_correct.hip", "brx_group.hip", "brx_one.hip", "brx_revscan.hip", "brx_onelane.hip", "brx_pipeline.hip"):
        with open(os.path.join(csrc, src)) as f:
            text = f.read()
        for n in names:
            assert f'"{n}"' not in text, (src, n)
