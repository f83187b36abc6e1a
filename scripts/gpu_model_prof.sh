# rocprofv3 kernel statistics of the bench's model_full leg (32 layers of LWM-7B, S = 32768, fwd+bwd; OUT_DIR: where the results go)
R=$(cd "$(dirname "$0")/.." && pwd); O=${OUT_DIR:-$R/out}
mkdir -p $O; cd /tmp && export TMPDIR=/tmp
rm -rf $O/mprof
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $O/mprof -o m -- python $R/bench.py --full --steps 1 --warmup 0 --layers 1 --no-cpu-baseline > $O/mprof.log 2>&1
find $O/mprof -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $O/model_kernel_stats.csv
find $O/mprof -name "*kernel_trace.csv" -size +1M -delete
head -30 $O/model_kernel_stats.csv | cut -c1-110
tail -c 600 $O/mprof.log
