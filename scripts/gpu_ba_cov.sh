#!/bin/bash
# Time per covariance() call at C3, C4, C5 (scripts/ba_cov_time.py): one JSON
# line per shape into OUT_DIR/time.jsonl (default build/ba_cov).  Every GPU step under its
# own time limit; the chain stops at the first step that fails.
#   scripts/gpu_ba_cov.sh [OUT_DIR]
set -o pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
cd "$ROOT"
OUT=${1:-build/ba_cov}
mkdir -p "$OUT"
: > "$OUT/time.jsonl"
timeout -k 10 120 python3 scripts/ba_cov_time.py c3 2>"$OUT/c3.err" | tee -a "$OUT/time.jsonl" &&
timeout -k 10 180 python3 scripts/ba_cov_time.py c4 2>"$OUT/c4.err" | tee -a "$OUT/time.jsonl" &&
timeout -k 10 300 python3 scripts/ba_cov_time.py c5 2>"$OUT/c5.err" | tee -a "$OUT/time.jsonl" &&
timeout -k 10 300 python3 scripts/ba_cov_time.py c5open 2>"$OUT/c5open.err" | tee -a "$OUT/time.jsonl" &&
echo ok
