# Round-end check: full GPU parity suite, smoke(), rocprof stats of the full bench, the full bench
# line (CPU baseline + live roofline).  usage: scripts/gpu_round_end.sh [out dir, default build/round_end]
set -u
root=$(cd "$(dirname "$0")/.." && pwd)
cd "$root"; out=$(mkdir -p "${1:-build/round_end}" && cd "${1:-build/round_end}" && pwd) || exit 1
timeout -k 10 900 python -u -m pytest tests -m gpu -q -p no:cacheprovider --timeout 120 --timeout-method thread > "$out/pytest_gpu.log" 2>&1; rc=$?
echo "pytest rc=$rc"; tail -3 "$out/pytest_gpu.log"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$out/smoke.log" 2>&1; rc=$?; echo "smoke rc=$rc"; tail -1 "$out/smoke.log"; [ $rc -eq 0 ] || exit $rc
cd "${TMPDIR:-/tmp}" && timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$out/prof" -o run --output-format csv -- python3 "$root/bench.py" --full --steps 5 --warmup 2 --no-cpu-baseline --detail-out none > "$out/prof.log" 2>&1; rc=$?; echo "prof rc=$rc"; [ $rc -eq 0 ] || exit $rc
cd "$root" && timeout -k 10 600 python bench.py --full --detail-out "$out/bench_detail.json" > "$out/bench.log" 2>&1; rc=$?; echo "bench rc=$rc"; tail -1 "$out/bench.log"; exit $rc
