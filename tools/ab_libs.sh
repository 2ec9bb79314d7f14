#!/usr/bin/env bash
# Alternating-process A/B of prebuilt libraries abl/librt_<name>.so (made by
# tools/build_exp.sh from the working tree, or tools/build_rev.sh from a git
# revision), interleaved per repetition so clock drift hits all of them alike.
# Run on the GPU box from the repo root.  The log's first line is the command
# that made it (profiles/r04 convention).
#
# usage: bash tools/ab_libs.sh <log> <configs> <reps> <name>...
#   TOOL=variants (default): tools/variants.py plain frames of <configs>
#   TOOL=share:              tools/share_cost.py (1/8 C3 tile share + full frame)
#   TOOL=bench:              bench.py --steps 200 --warmup 10 of <configs> (the headline's
#                            ms_per_step; BENCH_ARGS: further arguments, e.g. "--shard 0/8")
#   ENV="A=1 B=2":           extra environment for every run
#   HOOKS=1:                 TOOL=variants makes its renderers with RT_FLAG_TEST_HOOKS
#                            (_lib.test_flags), so the library reads its A/B switches
#                            from ENV (e.g. HOOKS=1 ENV="RT_SORT=0")
#   e.g. bash tools/ab_libs.sh gpurun_out/r04/node_ab.log c3,c5,c5d 3 base dword
set -e -o pipefail
LOG=${1:?log}; CFGS=${2:?configs}; REPS=${3:?reps}; shift 3
[ $# -ge 1 ] || { echo "name at least one build" >&2; exit 2; }
TOOL=${TOOL:-variants}
export TMPDIR=/tmp
mkdir -p "$(dirname "$LOG")"
echo "# cmd: TOOL=$TOOL HOOKS=${HOOKS:-} ENV='${ENV:-}'${BENCH_ARGS:+ BENCH_ARGS='$BENCH_ARGS'} bash tools/ab_libs.sh $LOG $CFGS $REPS $*" >> "$LOG"
for i in $(seq "$REPS"); do
  for L in "$@"; do
    case $TOOL in
      variants)
        env ${ENV:-} RT_AMD_LIB=$PWD/abl/librt_$L.so timeout -k 10 200 python tools/variants.py \
            --configs "$CFGS" --variants 0 --rounds 5 ${HOOKS:+--test-hooks} | sed "s/^/$L /" >> "$LOG" ;;
      share)
        env ${ENV:-} RT_AMD_LIB=$PWD/abl/librt_$L.so timeout -k 10 120 python tools/share_cost.py \
            2>/dev/null | sed "s/^/$L /" >> "$LOG" ;;
      bench)
        for C in ${CFGS//,/ }; do
          env ${ENV:-} RT_AMD_LIB=$PWD/abl/librt_$L.so timeout -k 10 200 python bench.py --gpus 1 --steps 200 \
              --warmup 10 --config "$C" --cpu-baseline off --secondary= ${BENCH_ARGS:-} 2>/dev/null |
              python -c 'import json,sys; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(json.dumps({"config": sys.argv[1], "ms_per_step": d["ms_per_step"], "kernel_ms": d["config"].get("kernel_ms")}))' "$C" |
              sed "s/^/$L /" >> "$LOG"
        done ;;
      *) echo "unknown TOOL=$TOOL" >&2; exit 2 ;;
    esac
  done
done
