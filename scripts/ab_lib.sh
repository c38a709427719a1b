#!/bin/bash
# A/B the C2 bench (CFG=c4|c5: that config) over library builds on one box: scripts/ab_lib.sh LIB1 LIB2 ...
# (each LIB a libphj_hip.so built beforehand in-tree, e.g. from another commit or with
#  measurement-only compile flags: `make prof-lib` -> build/libphj_prof.so, the phase-clock
#  forms of S's pass 1 and of the LDS join (-DPHJ_P1_PROF=1 -DPHJ_CL_PROF=1, stderr per join);
#  `make build/libphj_res1.so HIPDEFS=-DPHJ_PIPE_RES=1`-style variants the same way; PHJ_LIB selects it;
#  `make build/libphj_nopreagg.so HIPDEFS=-DPHJ_PREAGG=0`: without the hot-key pre-aggregation, csrc/phj_hot.h;
#  `HIPDEFS=-DPHJ_HOT_FREE_CUS=N`: the CUs per XCD R's pass 1 leaves to the prologue;
#  `make build/libphj_acc0.so HIPDEFS=-DPHJ_IX_ACC_CACHE=0` (or =512 / =1024): k_ix_accumulate with plain global atomics / another cache size (scripts/ordinal_bench.py --acc-libs))
# The JSON lines go to $OUT (default ab_out/).
set -o pipefail
OUT=${OUT:-ab_out}
mkdir -p "$OUT"
i=0
for lib in "$@"; do
  i=$((i+1))
  PHJ_LIB=$lib timeout -k 10 150 python bench.py --full --config ${CFG:-c2} --no-cpu-baseline --no-traffic --verbose > "$OUT/abl_$i.json" 2> "$OUT/abl_$i.err" || { echo "$lib failed"; tail -5 "$OUT/abl_$i.err"; exit 9; }
  python -c "import json,sys; d=json.load(open('$OUT/abl_$i.json')); k=d['kernels_ms']; print('$lib', round(d['ms_per_step'],3), d['correct'], {n: round(v,3) for n,v in k.items()})"
done
