cd $GRAFT_REPO_ROOT
export ROUND=r06
out=${1:?usage: tools/r06_bench.sh OUTDIR}
mkdir -p "$out"
timeout 1200 python3 bench.py --full > "$out/r06_bench_stdout.txt" 2> "$out/r06_bench_stderr.txt"; echo "bench rc=$?"
cp bench_full.json "$out/r06_bench_full.json" 2>/dev/null
timeout 1500 tools/profile_bench.sh --full --steps 20 --warmup 3 2>&1 | tail -3
cut -c1-600 "$out/r06_bench_stdout.txt"
