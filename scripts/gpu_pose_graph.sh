#!/bin/bash
# Time per LM iteration of the SE(3) pose graph at 500 and 5000 poses, with the
# skyline and with the profile forced full (scripts/pose_graph_time.py): one JSON
# line per run into OUT_DIR/time.jsonl (default build/pose_graph).  Every GPU
# step under its own time limit; the chain stops at the first step that fails.
#   scripts/gpu_pose_graph.sh [OUT_DIR]
set -o pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
cd "$ROOT"
OUT=${1:-build/pose_graph}
mkdir -p "$OUT"
: > "$OUT/time.jsonl"
timeout -k 10 120 python3 scripts/pose_graph_time.py loop500 2>"$OUT/loop500.err" | tee -a "$OUT/time.jsonl" &&
timeout -k 10 120 python3 scripts/pose_graph_time.py back500 2>"$OUT/back500.err" | tee -a "$OUT/time.jsonl" &&
timeout -k 10 240 python3 scripts/pose_graph_time.py big5000 2>"$OUT/big5000.err" | tee -a "$OUT/time.jsonl" &&
timeout -k 10 120 python3 scripts/pose_graph_time.py loop500 full 2>"$OUT/loop500_full.err" | tee -a "$OUT/time.jsonl" &&
timeout -k 10 120 python3 scripts/pose_graph_time.py back500 full 2>"$OUT/back500_full.err" | tee -a "$OUT/time.jsonl" &&
echo ok
