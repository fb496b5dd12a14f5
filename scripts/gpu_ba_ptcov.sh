#!/bin/bash
# Records of profiles/ba_ptcov: time per point_covariance() call at C3 and C4
# (scripts/ba_ptcov_time.py; with a parent tree, its covariance() by its own
# scripts/ba_cov_time.py), then the existing paths -- this tree and the parent
# tree, each with its own build, alternated (odd pairs parent first), 4 runs
# each of the tracking line and of --workload ba, and --dump-outputs of the BA
# line compared array for array.  Every GPU step under its own time limit; the
# chain stops at the first step that fails.
#   scripts/gpu_ba_ptcov.sh OUT_DIR [PARENT_TREE]     (PARENT_TREE: built, relative to the root or absolute)
set -o pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
cd "$ROOT"
OUT=${1:-build/ba_ptcov}
PAR=${2:-}
mkdir -p "$OUT"
OUT="$(cd "$OUT" && pwd)"
: > "$OUT/time.jsonl"
timeout -k 10 120 python3 scripts/ba_ptcov_time.py c3 2>"$OUT/c3.err" | tee -a "$OUT/time.jsonl" &&
timeout -k 10 240 python3 scripts/ba_ptcov_time.py c4 2>"$OUT/c4.err" | tee -a "$OUT/time.jsonl" || exit 1
[ -n "$PAR" ] || { echo ok; exit 0; }
PAR="$(cd "$PAR" && pwd)"
: > "$OUT/time_parent.jsonl"
(cd "$PAR" && timeout -k 10 120 python3 scripts/ba_cov_time.py c3 2>"$OUT/c3_parent.err" | tee -a "$OUT/time_parent.jsonl" &&
 timeout -k 10 240 python3 scripts/ba_cov_time.py c4 2>"$OUT/c4_parent.err" | tee -a "$OUT/time_parent.jsonl") || exit 1
run() {  # $1 = parent|change, $2 = index
  local dir=$ROOT; [ "$1" = parent ] && dir=$PAR
  (cd "$dir" && timeout -k 10 200 python3 bench.py --gpus 1 --steps 20 --warmup 5 2>/dev/null | tail -1 > "$OUT/track_$1_$2.json" &&
   timeout -k 10 120 python3 bench.py --gpus 1 --workload ba --steps 40 --warmup 5 2>/dev/null | tail -1 > "$OUT/ba_$1_$2.json") || return 1
  python3 -c "import json;a=json.load(open('$OUT/track_$1_$2.json'));b=json.load(open('$OUT/ba_$1_$2.json'));print('$1', $2, 'tracking', round(a['value']), '| ba', round(b['value']))"
}
for i in 1 2 3 4; do
  if [ $((i % 2)) = 1 ]; then run parent $i && run change $i || exit 1; else run change $i && run parent $i || exit 1; fi
done
(cd "$PAR" && timeout -k 10 120 python3 bench.py --gpus 1 --workload ba --steps 40 --warmup 5 --dump-outputs "$OUT/dump_parent" >/dev/null 2>&1) &&
timeout -k 10 120 python3 bench.py --gpus 1 --workload ba --steps 40 --warmup 5 --dump-outputs "$OUT/dump_change" >/dev/null 2>&1 &&
python3 - "$OUT" <<'EOF' || exit 1
import glob, os, sys
import numpy as np
out = sys.argv[1]
names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(out, "dump_parent", "*.npy")))
assert names, "no dumped arrays"
for n in names:
    a, b = np.load(os.path.join(out, "dump_parent", n)), np.load(os.path.join(out, "dump_change", n))
    assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), n
print("dump-outputs equal:", " ".join(names))
EOF
echo ok
