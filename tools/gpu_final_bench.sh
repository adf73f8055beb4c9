# round-end default bench line on the committed tree (traffic files stamped with it)
set -o pipefail
OUT=${OUT:-build/bench}
mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -k 10 600 python3 -u bench.py --full > "$OUT/final_bench2.json" 2> "$OUT/final_bench2.err"
