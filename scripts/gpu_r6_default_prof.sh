set -o pipefail
mkdir -p gpurun_out/r6b
export TMPDIR=/tmp
T0=$(date +%s)
BENCH_LOG=$(mktemp); timeout -k 10 580 python bench.py --full --gpus 1 --steps 20 --warmup 5 > $BENCH_LOG 2>&1 || { tail -5 $BENCH_LOG; exit 1; }
echo "default bench wall $(( $(date +%s) - T0 )) s"
bash scripts/gpu_prof_all.sh r6b c2
