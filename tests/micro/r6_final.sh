OUT=${OUT:-bench_out/r6}
mkdir -p $OUT
python -m pytest tests -m gpu -x -q --durations=8 > $OUT/gpu_tests_final.log 2>&1; echo "gpu suite rc=$?"; tail -n 14 $OUT/gpu_tests_final.log | grep -v amdgpu.ids
python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1; echo "smoke rc=$?"; tail -n 2 $OUT/smoke.log
python bench.py --full > $OUT/bench_final.json 2> $OUT/bench_final.err; echo "bench rc=$?"
