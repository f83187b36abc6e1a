# rocprofv3 kernel statistics of the bench's VQGAN leg (1 attention layer rides along; OUT_DIR: where the results go)
R=$(cd "$(dirname "$0")/.." && pwd); O=${OUT_DIR:-$R/out}
mkdir -p $O; cd /tmp && export TMPDIR=/tmp
rm -rf $O/vqprof
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $O/vqprof -o vq -- python $R/bench.py --full --steps 1 --warmup 0 --layers 1 --no-full-model --no-cpu-baseline > $O/vqprof.log 2>&1
find $O/vqprof -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $O/vq_kernel_stats.csv
find $O/vqprof -name "*kernel_trace.csv" -size +1M -delete
head -25 $O/vq_kernel_stats.csv | cut -c1-150
