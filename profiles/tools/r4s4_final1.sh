cd $GRAFT_REPO_ROOT
OUT=${OUT:-${TMPDIR:-/tmp}/r4s4}; mkdir -p "$OUT"
bash profiles/tools/profile_cxx_amr_gaps.sh r4s4_gaps2 > "$OUT/r4s4_gaps2.txt" 2>&1
bash profiles/tools/profile_cxx_amr_trace.sh r4s4_cxx_amr2 > "$OUT/r4s4_cxx_amr2.txt" 2>&1
python bench.py --full > "$OUT/r4s4_bench_v6.json" 2> "$OUT/r4s4_bench_v6.err"
head -40 "$OUT/r4s4_gaps2.txt"; tail -c 600 "$OUT/r4s4_bench_v6.err"
