cd "$(dirname "$0")/.." && OUT=${1:-build/run16} && mkdir -p "$OUT"
python -c "import __graft_entry__ as g; g.build()" > "$OUT/build.log" 2>&1
( time timeout -k 10 900 python bench.py --gpus 1 --steps 20 --warmup 5 --full > "$OUT/bench_final.json" 2> "$OUT/bench_final.err" ) 2> "$OUT/bench_final.time"
echo "bench exit $?"; cat "$OUT/bench_final.time"
timeout -k 10 900 python tests/fuzz_parity.py > "$OUT/fuzz_parity.txt" 2>&1; echo "fuzz exit $?"; tail -2 "$OUT/fuzz_parity.txt"
