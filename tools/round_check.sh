set -o pipefail
OUT=${OUT:-check_out/fin}
mkdir -p $OUT
timeout -k 10 500 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/gputests.log 2>&1 || { echo TESTS_FAILED; tail -30 $OUT/gputests.log; exit 1; }
tail -2 $OUT/gputests.log
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 || { echo SMOKE_FAILED; exit 1; }
tail -1 $OUT/smoke.log
for wl in orswot apply mvreg map; do
  timeout -k 10 240 python bench.py --full --workload $wl > $OUT/bench_$wl.json 2> $OUT/bench_$wl.err || { echo BENCH_FAILED $wl; exit 1; }
  echo "$wl $(cut -c1-160 $OUT/bench_$wl.json)"
done
timeout -k 10 500 python tools/map_bincode_bench.py --out profiles/map_bincode_bench.json > $OUT/map_bincode_bench.log 2>&1 || { echo BENCH_FAILED map_bincode; exit 1; }
echo "map_bincode $(cut -c1-160 profiles/map_bincode_bench.json)"
timeout -k 10 500 python tools/nested_bincode_bench.py --out profiles/nested_bincode_bench.json > $OUT/nested_bincode_bench.log 2>&1 || { echo BENCH_FAILED nested_bincode; exit 1; }
echo "nested_bincode $(cut -c1-160 profiles/nested_bincode_bench.json)"
for wl in apply mvreg map; do bash tools/profile_workload.sh r01e $wl || { echo PROF_FAILED $wl; exit 1; }; done
echo ALL_OK
