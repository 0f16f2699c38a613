set -o pipefail
OUT=${OUT:-/tmp/spec_amd_reh}
mkdir -p $OUT; export TMPDIR=/tmp
timeout -k 10 400 python bench.py --full --gpus 2 --backend gloo --steps 10 --warmup 3 --no-cpu > $OUT/bench_gpus2_gloo.json 2> $OUT/err.log || { tail -n 30 $OUT/err.log; exit 1; }
cut -c1-700 $OUT/bench_gpus2_gloo.json
