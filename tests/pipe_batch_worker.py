"""Child process of tests/test_gpu_grid_trips.py: one native run_correction of a FASTA file with chain [one] against the
raw.k11.a2.solid fixture.  The pipeline reads BRX_PIPE_BATCH_MB, BRX_PIPE_WORKERS and BRX_PIPE_WRITERS once per process,
so every setting of them needs a process of its own.  usage: pipe_batch_worker.py IN OUT; prints the run's statistics
as one JSON line."""
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import br_amd
from br_amd.driver import run_correction


def main(src, dst):
    with open(os.path.join(ROOT, "tests", "golden", "raw.k11.a2.solid"), "rb") as f:
        gs = br_amd.Pcon.from_pcon_solid(gzip.decompress(f.read()))
    methods = br_amd.build_methods(["one"], gs, 5, 7)
    with open(src, "rb") as fi, open(dst, "wb") as fo:
        st = run_correction([fi], [fo], methods, False, native=True, batch_records=0)
    print(json.dumps({k: int(v) for k, v in st.items()}))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
