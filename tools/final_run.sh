# Round-end validation on an MI355X: the GPU suite, smoke(), the full bench line + details, a 2-rank and an 8-rank bench on
# one GPU, the single-read latency.  Usage: tools/final_run.sh <tag> <output dir>
set -x
TAG=${1:-r03}
OUT=${2:?usage: tools/final_run.sh <tag> <output dir>}
mkdir -p "$OUT"
timeout 1500 python -m pytest tests -m gpu -q > $OUT/pytest_gpu_final.txt 2>&1; echo "pytest rc=$?" >> $OUT/pytest_gpu_final.txt
grep -E "passed|failed|rc=" $OUT/pytest_gpu_final.txt | tail -3
python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.txt 2>&1; tail -2 $OUT/smoke.txt
( time timeout 900 python bench.py --full --steps 20 --warmup 5 --details $OUT/bench_${TAG}_details.json > $OUT/bench_${TAG}_final.json 2> $OUT/bench_${TAG}_final.err ) 2> $OUT/bench_${TAG}_final.time
tail -3 $OUT/bench_${TAG}_final.time; grep "^\[bench" $OUT/bench_${TAG}_final.err | tail -12; wc -c $OUT/bench_${TAG}_final.json
timeout 600 python bench.py --full --gpus 2 --force-device 0 --dist-backend gloo --steps 5 --warmup 2 --no-cpu-baseline --no-encode --no-reads --no-others --no-refine --details $OUT/bench_${TAG}_2ranks_details.json > $OUT/bench_${TAG}_2ranks_1gpu.json 2> $OUT/bench_${TAG}_2ranks_1gpu.err; tail -c 400 $OUT/bench_${TAG}_2ranks_1gpu.json
timeout 900 python bench.py --full --gpus 8 --force-device 0 --dist-backend gloo --chunks 125000 --steps 5 --warmup 2 --no-cpu-baseline --no-encode --no-reads --no-others --no-refine --details $OUT/bench_${TAG}_8ranks_details.json > $OUT/bench_${TAG}_8ranks_1gpu.json 2> $OUT/bench_${TAG}_8ranks_1gpu.err; tail -c 300 $OUT/bench_${TAG}_8ranks_1gpu.json; grep "bench rank" $OUT/bench_${TAG}_8ranks_1gpu.err | head -16
python tools/time_single_read.py > $OUT/single_read_${TAG}.log 2>&1; tail -2 $OUT/single_read_${TAG}.log
