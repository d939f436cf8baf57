# One round's evidence from one GPU box: bench line, rocprofv3 kernel stats of the same command, fuzz runs.
# usage (repo root, on the GPU box): bash tools/collect_round.sh TAG [OUT_DIR]   (OUT_DIR: collect_out/TAG)
set -e
TAG=${1:-r2}
OUT=${2:-collect_out/$TAG}
mkdir -p "$OUT"
OUT=$(cd "$OUT" && pwd)
timeout -k 10 600 python bench.py --full --steps 10 --warmup 2 > $OUT/bench.log 2>&1
tail -1 $OUT/bench.log > $OUT/bench_n1.json
R=$PWD
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/stats -o s -- python3 $R/bench.py --steps 3 --warmup 1 > $OUT/stats.log 2>&1
cd $R
timeout -k 10 200 python tools/fuzz_parity.py 90 77 > $OUT/fuzz_parity.log 2>&1
BRX_PIPE_BATCH_MB=1 timeout -k 10 200 python tools/fuzz_fasta.py 45 78 > $OUT/fuzz_fasta.log 2>&1
tail -1 $OUT/fuzz_parity.log; tail -1 $OUT/fuzz_fasta.log
find $OUT/stats -name "*kernel_stats.csv" | head
