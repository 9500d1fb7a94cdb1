#!/usr/bin/env bash
# the product sources with extra -D switches -> armada_amd/csrc/libarmada_sched_<name>.so (A/B runs: ASCHED_LIB_PATH; tools/ab_call.sh)
#   tools/build_variant.sh eng0 -DENG_START_AFTER=0
#   tools/build_variant.sh prof -DASCHED_FASTPROF   (shader-clock reads at the segment borders of the fast iteration, round_fast.h SEG(); ASCHED_PRINT_SEG=1 prints them)
# The translation units and flags are __graft_entry__.HIP_TUS / HIPCC_FLAGS: the variant links every code object the product does.
set -e
NAME=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
read -r -a TUS <<< "$(cd "$ROOT" && python3 -c 'import __graft_entry__ as g; print(" ".join(g.HIP_TUS))')"
read -r -a FLAGS <<< "$(cd "$ROOT" && python3 -c 'import __graft_entry__ as g; print(" ".join(g.HIPCC_FLAGS))')"
cd "$ROOT/armada_amd/csrc"
T=$(mktemp -d); trap 'rm -rf $T' EXIT
OBJS=()
for tu in "${TUS[@]}"; do OBJS+=("$T/${tu%.hip}.o"); hipcc "${FLAGS[@]}" "$@" -c "$tu" -o "${OBJS[-1]}" & done
for job in $(jobs -p); do wait "$job"; done
hipcc --offload-arch=gfx950 -fPIC -shared -pthread -o "libarmada_sched_$NAME.so" "${OBJS[@]}"
ls -la "libarmada_sched_$NAME.so"
