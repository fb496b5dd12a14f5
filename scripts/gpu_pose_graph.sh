#!/bin/bash
# Time per LM iteration of the SE(3) pose graph at 500 and 5000 poses, with the
# skyline and with the profile forced full (scripts/pose_graph_time.py): one JSON
# line per run into OUT_DIR/time.jsonl (default build/pose_graph).  `cov`: one
# covariance() call per shape instead (the last pose's column, and 8 columns
# spread over the trajectory) into OUT_DIR/cov_time.jsonl.  Every GPU step
# under its own time limit; the chain stops at the first step that fails.
#   scripts/gpu_pose_graph.sh [OUT_DIR] [iter|cov]
set -o pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
cd "$ROOT"
OUT=${1:-build/pose_graph}
MODE=${2:-iter}
mkdir -p "$OUT"
if [ "$MODE" = cov ]; then
  : > "$OUT/cov_time.jsonl"
  timeout -k 10 120 python3 scripts/pose_graph_time.py loop500 cov 2>"$OUT/loop500_cov.err" | tee -a "$OUT/cov_time.jsonl" &&
  timeout -k 10 120 python3 scripts/pose_graph_time.py back500 cov 2>"$OUT/back500_cov.err" | tee -a "$OUT/cov_time.jsonl" &&
  timeout -k 10 240 python3 scripts/pose_graph_time.py big5000 cov 2>"$OUT/big5000_cov.err" | tee -a "$OUT/cov_time.jsonl" &&
  echo ok
  exit $?
fi
: > "$OUT/time.jsonl"
timeout -k 10 120 python3 scripts/pose_graph_time.py loop500 2>"$OUT/loop500.err" | tee -a "$OUT/time.jsonl" &&
timeout -k 10 120 python3 scripts/pose_graph_time.py back500 2>"$OUT/back500.err" | tee -a "$OUT/time.jsonl" &&
timeout -k 10 240 python3 scripts/pose_graph_time.py big5000 2>"$OUT/big5000.err" | tee -a "$OUT/time.jsonl" &&
timeout -k 10 120 python3 scripts/pose_graph_time.py loop500 full 2>"$OUT/loop500_full.err" | tee -a "$OUT/time.jsonl" &&
timeout -k 10 120 python3 scripts/pose_graph_time.py back500 full 2>"$OUT/back500_full.err" | tee -a "$OUT/time.jsonl" &&
echo ok
