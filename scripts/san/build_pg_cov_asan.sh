#!/usr/bin/env bash
# Host-only ASan/UBSan build of the pose graph's C ABI (capi.hip,
# posegraph_se3.hip) + the driver of its covariance request validation (CPU host
# only).  Device code is compiled as usual; -Xarch_host puts the sanitizers on
# the host half only.
#   scripts/san/build_pg_cov_asan.sh && slam-1_amd/build_asan/pg_cov_args
set -euo pipefail
cd "$(dirname "$0")/../.."
OUT=slam-1_amd/build_asan
mkdir -p "$OUT"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer -Xarch_host -fno-sanitize-recover=undefined"
FLAGS="-O1 -g -std=c++17 --offload-arch=gfx950 -fPIC -ffp-contract=off -munsafe-fp-atomics \
       -fhip-fp32-correctly-rounded-divide-sqrt -mllvm -amdgpu-mfma-vgpr-form -Iinclude"
objs=()
for n in capi posegraph_se3; do
  $HIPCC $FLAGS $SAN -c "slam-1_amd/csrc/$n.hip" -o "$OUT/pgcov_$n.o" &
  objs+=("$OUT/pgcov_$n.o")
done
wait
gcc -O1 -g -std=c11 -Iinclude -fsanitize=address,undefined -fno-omit-frame-pointer \
    -c scripts/san/pg_cov_args.c -o "$OUT/pg_cov_args.o"
$HIPCC --offload-arch=gfx950 -fsanitize=address,undefined -o "$OUT/pg_cov_args" \
    "$OUT/pg_cov_args.o" "${objs[@]}"
echo "built $OUT/pg_cov_args"
