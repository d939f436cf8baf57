"""What the tests of the shipped multi-GPU exchange share (test_gpu_exchange_abi.py, test_gpu_table_exchange.py):

  run_world   starts `world` fresh processes of a worker script on the one card, with tests/libfake_rccl.so behind the
              library's librccl entry points, supervises them, and returns what each rank pickled;
  the CPU statement of every figure an exchange reports about its traffic -- who owns which key, what each shard sends
  to each owner, what each owner ends up counting -- from the oracle's hashes and the numpy statements of br_amd/dist.py
  (owner_bounds, table_owner, shard_range) alone.  No GPU, and nothing here reads a rank's output.

Not a conftest and not collected (no test_ prefix)."""
import functools
import os
import pickle
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FAKE = os.path.join(HERE, "libfake_rccl.so")
MAX_PROCESSES = 9          # this process and 8 ranks hold the GPU at once; never two worlds at a time
WORLD_LIMIT_S = 240.0      # one time limit for a whole world
GRACE_S = 20.0             # what the others get once one rank has exited non-zero

world_times = []           # (worker, world, argv, seconds) of every world this process ran, in order


def _tail(path, n=25):
    try:
        with open(path, "rb") as f:
            return b"\n".join(f.read().splitlines()[-n:]).decode(errors="replace")
    except OSError as e:
        return "(no log: %s)" % e


def run_world(tmp_path, worker, world, argv, extra_env=None, limit=WORLD_LIMIT_S, grace=GRACE_S):
    """`world` processes `python WORKER RANK WORLD K ABUNDANCE N_READS OUT_PREFIX MODE [...]` (the workers' usage lines),
    with argv = [K, ABUNDANCE, N_READS, MODE, ...].  One pickle and one traffic record per rank come back.  The ranks are
    polled, never waited for one after another; no retry: once a rank has exited non-zero the others get `grace`
    seconds, a world gets `limit` seconds in all, then whatever still runs is killed and the test fails with every
    rank's exit code, the path of its stderr log (the workers log their phases there) and the log's tail.  That the
    transport has been built is the caller's to check: the runner itself needs neither it nor a GPU."""
    assert world + 1 <= MAX_PROCESSES                    # processes that hold the GPU at once, this one included
    prefix = str(tmp_path / "x")
    env = dict(os.environ)
    env["BRX_RCCL_PATH"] = FAKE
    env["FAKE_RCCL_DIR"] = str(tmp_path)
    env["FAKE_RCCL_STATS"] = prefix + ".traffic"
    env["BRX_DEVPOOL_GB"] = "1"                          # eight ranks on one card: no 48 GiB of parked device memory each,
    env["BRX_HOSTPOOL_GB"] = "1"                         # nor 4 GiB of page-locked memory
    env.update(extra_env or {})
    k, a, n_reads = argv[:3]
    logs = ["%s.rank%d.log" % (prefix, r) for r in range(world)]
    procs, files = [], []
    t0 = time.monotonic()
    why = None
    try:
        for r in range(world):
            files.append(open(logs[r], "wb"))
            cmd = [sys.executable, worker, str(r), str(world), str(k), str(a), str(n_reads), prefix] + [str(x) for x in argv[3:]]
            procs.append(subprocess.Popen(cmd, env=env, stderr=files[-1]))
        first_bad = None
        while True:
            codes = [p.poll() for p in procs]
            if all(c is not None for c in codes):
                break
            now = time.monotonic()
            if first_bad is None and any(c not in (None, 0) for c in codes):
                first_bad = now
            if first_bad is not None and now - first_bad > grace:
                why = "a rank failed and its peers were still running %.1f s later" % grace
                break
            if now - t0 > limit:
                why = "the world did not end within %.1f s" % limit
                break
            time.sleep(0.02)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()
        for f in files:
            f.close()
    seconds = time.monotonic() - t0
    world_times.append((os.path.basename(worker), world, tuple(argv), seconds))
    print("world_time %s world=%d argv=%s %.2f s" % (os.path.basename(worker), world, list(argv), seconds))
    if why is not None or codes != [0] * world:
        report = ["%s; exit codes %s (None: killed by this runner)" % (why or "a rank failed", codes)]
        report += ["---- rank %d, exit %s, %s ----\n%s" % (r, codes[r], logs[r], _tail(logs[r])) for r in range(world)]
        raise AssertionError("\n".join(report))
    out = []
    for r in range(world):
        with open("%s.rank%d.pkl" % (prefix, r), "rb") as f:
            out.append(pickle.load(f))
        with open("%s.traffic.rank%d" % (prefix, r)) as f:
            out[-1]["msgs"], out[-1]["bytes"] = (int(x) for x in f.read().split())
    return out


# ---- the CPU statement of an exchange's traffic ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def fixture_reads():
    from tests.conftest import GOLDEN, read_fasta
    return tuple(read_fasta(os.path.join(GOLDEN, "raw.fasta"))[1])


def shard_cuts(n_reads, world, cuts=None):
    """world + 1 cut points: rank r holds reads [cuts[r], cuts[r + 1]); br_amd.dist.shard_range unless `cuts` is given"""
    from br_amd import dist as D
    if cuts is None:
        cuts = [D.shard_range(n_reads, world, r)[0] for r in range(world)] + [n_reads]
    cuts = list(cuts)
    assert len(cuts) == world + 1 and cuts[0] == 0 and cuts[-1] == n_reads and all(x <= y for x, y in zip(cuts, cuts[1:]))
    return cuts


def even_cuts(n_reads, world):
    """NOT shard_range: blocks of ceil(n / world) reads, the last ones short -- what the figures must differ from"""
    per = -(-n_reads // world)
    return [min(r * per, n_reads) for r in range(world + 1)]


def first_digit_bits(k):
    """width of the first radix digit of the partitioned counter at this k (make_plan, br_amd/csrc/brx_partbuild.hip: the
    2k - 1 - 12 bits above a fine bucket spread evenly over ceil(. / 9) >= 2 levels, larger digits first, and at least
    what leaves 32 bits for the keys that travel): 2^bits first digits are what owner_bounds divides among the ranks.
    A restatement: the library tells its number of first digits only through a counter on a GPU, so the guard against a
    change of make_plan is the GPU tests' `n_buckets == 1 << first_digit_bits(k)`, for every k in use; without a GPU only
    the widths themselves are pinned (test_first_digit_widths)."""
    nbits = 2 * k - 1
    p = nbits - 12
    nlev = max(2, -(-p // 9))
    return max(-(-p // nlev), nbits - 32)


@functools.lru_cache(maxsize=None)
def read_hashes(k, n_reads):
    """the oracle's canonical hash of every k-mer occurrence, read by read (shared, never modified)"""
    from oracle import oracle as O
    return tuple(O.hashes(k, r) for r in fixture_reads()[:n_reads])


def _shard_hashes(k, n_reads, cuts, s):
    parts = read_hashes(k, n_reads)[cuts[s]:cuts[s + 1]]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)


def part_messages(k, n_reads, world, cuts=None, owners=None):
    """int64[world, owners]: m[s, r] = the k-mer OCCURRENCES of shard s whose first digit lies in
    owner_bounds(...)[r : r + 1] -- the keys rank s sends to rank r in brx_exchange_build_partitioned.  Column sums are
    keys_counted_here, the maximum is largest_message_keys.  `owners` (default: world) divides the digits among another
    number of ranks: what the figures of a job of that world would be."""
    from br_amd import dist as D
    owners = world if owners is None else owners
    cuts = shard_cuts(n_reads, world, cuts)
    bits = first_digit_bits(k)
    bounds = np.array(D.owner_bounds(1 << bits, owners), dtype=np.int64)
    m = np.zeros((world, owners), dtype=np.int64)
    for s in range(world):
        digit = (_shard_hashes(k, n_reads, cuts, s) >> np.uint64(2 * k - 1 - bits)).astype(np.int64)
        per_digit = np.concatenate([[0], np.cumsum(np.bincount(digit, minlength=1 << bits))])
        m[s] = per_digit[bounds[1:]] - per_digit[bounds[:-1]]
    return m


def part_solid_per_owner(k, n_reads, world, a):
    """int64[world]: the k-mers counted more than `a` times (u8 counts: saturating at 255) over ALL the reads whose first
    digit rank r owns: solid_here of brx_exchange_build_partitioned"""
    from br_amd import dist as D
    bits = first_digit_bits(k)
    bounds = np.array(D.owner_bounds(1 << bits, world), dtype=np.int64)
    h, cnt = np.unique(np.concatenate(read_hashes(k, n_reads)), return_counts=True)
    digit = (h[np.minimum(cnt, 255) > a] >> np.uint64(2 * k - 1 - bits)).astype(np.int64)
    per_digit = np.concatenate([[0], np.cumsum(np.bincount(digit, minlength=1 << bits))])
    return per_digit[bounds[1:]] - per_digit[bounds[:-1]]


def part_sent_messages(m, solid_here, chunk=None, builds=2):
    """int64[world]: the messages rank r SENDS in `builds` calls of brx_exchange_build_partitioned (what the test transport
    counts), from the message matrix m, the owners' solid counts and BRX_A2A_CHUNK (None: unset, no message is split).
    Per call and peer: five small collectives (status, offset tables, status, list sizes, status: one message each), the
    keys for that peer in ceil(m[r, p] / chunk) capped rounds (none where it has no key for it), and the rank's own solid
    list in ceil(solid_here[r] / (chunk / 2)) rounds of the list gather.  A rank that stopped after its own rounds would
    still show this count -- that it also RECEIVED every round of its peers shows in its set, which the oracle checks, and
    in the transport, which ends a world whose receive finds a message of another size or none."""
    world = m.shape[0]
    chunk = (1 << 28) if chunk is None else int(chunk)
    out = np.zeros(world, dtype=np.int64)
    for r in range(world):
        keys = sum(-(-int(m[r, p]) // chunk) for p in range(world) if p != r)
        lists = (world - 1) * -(-int(solid_here[r]) // max(chunk // 2, 1))
        out[r] = builds * (5 * (world - 1) + keys + lists)
    return out


def table_messages(k, n_reads, world, cuts=None, owners=None):
    """int64[world, owners]: m[s, r] = the DISTINCT k-mers of shard s with table_owner(hash, owners) == r -- the entries
    rank s sends to rank r in brx_exchange_table_merge.  Column sums are the entries merged at r."""
    from br_amd import dist as D
    owners = world if owners is None else owners
    cuts = shard_cuts(n_reads, world, cuts)
    m = np.zeros((world, owners), dtype=np.int64)
    for s in range(world):
        h = np.unique(_shard_hashes(k, n_reads, cuts, s))
        if h.size:
            m[s] = np.bincount(D.table_owner(h, owners).astype(np.int64), minlength=owners)
    return m


def table_keys_per_owner(k, n_reads, owners, a=0):
    """int64[owners]: the distinct k-mers of ALL the reads with table_owner == r: table_info()["keys"] of a merged counter;
    with `a`, those among them counted more than `a` times: solid_here of brx_exchange_table_finish"""
    from br_amd import dist as D
    h, cnt = np.unique(np.concatenate(read_hashes(k, n_reads)), return_counts=True)
    return np.bincount(D.table_owner(h[np.minimum(cnt, 255) > a], owners).astype(np.int64), minlength=owners)
