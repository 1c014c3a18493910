# End-of-round evidence at the current library: GPU suite, smoke, bench lines (C3 default with companions and
# CPU baselines: --full; C4 and C5 single-GPU lines with their rooflines).  Every GPU step under its own limit;
# stop after a hang/fault.  Usage: tools/final_bench.sh [output directory, default _scratch/final]
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}" || exit 2
OUT=${1:-_scratch/final}
mkdir -p "$OUT"
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > "$OUT/gpu_tests.log" 2>&1
rc=$?; tail -n 2 "$OUT/gpu_tests.log"; [ $rc -le 1 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1
rc=$?; tail -n 3 "$OUT/smoke.log"; [ $rc -le 1 ] || exit $rc
timeout -k 10 400 python bench.py --full > "$OUT/bench_c3_default.jsonl" 2> "$OUT/bench_c3.err" || exit $?
timeout -k 10 300 python bench.py --full --workload c4 --steps 10 --warmup 3 --no-cpu-baseline > "$OUT/bench_c4_1gpu.jsonl" 2> "$OUT/bench_c4.err" || exit $?
timeout -k 10 300 python bench.py --full --workload c5 --steps 5 --warmup 2 --no-cpu-baseline > "$OUT/bench_c5_1gpu.jsonl" 2> "$OUT/bench_c5.err" || exit $?
timeout -k 10 300 python bench.py --full --workload c5big --steps 3 --warmup 1 --no-cpu-baseline > "$OUT/bench_c5big_1gpu.jsonl" 2> "$OUT/bench_c5big.err" || exit $?
for f in c3_default c4_1gpu c5_1gpu c5big_1gpu; do tail -n 1 "$OUT/bench_$f.jsonl" | python -c "import json,sys; d=json.loads(sys.stdin.read()); r=d['roofline']; print('$f', d['value'], d['ms_per_step'], r['bound'], r['frac'], r.get('frac_isolated'), r.get('pmc_stale'))"; done
