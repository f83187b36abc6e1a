# VQGAN verification pass: GPU parity tests of the VQGAN kernels, then the bench's VQGAN leg (OUT_DIR: where the logs go)
R=$(cd "$(dirname "$0")/.." && pwd); O=${OUT_DIR:-$R/out}
cd $R; mkdir -p $O
timeout 900 python -m pytest tests/test_gpu_vqgan.py -x -q > $O/vq_tests.log 2>&1; echo "pytest rc=$?" >> $O/vq_tests.log
timeout 600 python bench.py --full --steps 1 --warmup 0 --layers 1 --no-full-model --no-cpu-baseline > $O/vq_bench.json 2> $O/vq_bench.err
tail -3 $O/vq_tests.log
python - $O/vq_bench.json <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(json.dumps(d["vqgan"], indent=1))
PY
