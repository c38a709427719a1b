#!/bin/bash
# A/B the C2 bench (CFG=c4|c5: that config) over library builds on one box: scripts/ab_lib.sh LIB1 LIB2 ...
# (each LIB a libphj_hip.so built beforehand in-tree, e.g. from another commit or with
#  measurement-only compile flags: `make prof-lib` -> build/libphj_prof.so, the phase-clock
#  forms of S's pass 1 and of the LDS join (-DPHJ_P1_PROF=1 -DPHJ_CL_PROF=1, stderr per join);
#  `make build/libphj_res1.so HIPDEFS=-DPHJ_PIPE_RES=1`-style variants the same way; PHJ_LIB selects it;
#  `make build/libphj_nopreagg.so HIPDEFS=-DPHJ_PREAGG=0`: without the hot-key pre-aggregation, csrc/phj_hot.h;
#  `make build/libphj_late.so HIPDEFS=-DPHJ_HOT_EARLY_R=0`: R's chain after S's pass 1, not beside the hot-key prologue;
#  `HIPDEFS=-DPHJ_HOT_FREE_CUS=N`: the CUs per XCD R's pass 1 leaves to the prologue;
#  `make build/libphj_nofuse.so HIPDEFS=-DPHJ_HOT_FUSE=0`: S's pass with the weight add and the rank claim as two LDS atomics;
#  `make build/libphj_nobatch.so HIPDEFS=-DPHJ_P1_BATCH=0`: S's pre-aggregating pass with its sort stage once per input tile, not per 4096 kept codes;
#  `HIPDEFS=-DPHJ_P1F_BUFLOAD=0` / `_SET128=0` / `_WTADDR=1` / `_FULL=0` / `_CMPBALLOT=0` / `_WAVEFAST=0`: the front of S's batched pass 1, one item each (csrc/phj_partition.h);
#  `make build/libphj_acc0.so HIPDEFS=-DPHJ_IX_ACC_CACHE=0` (or =512 / =1024): k_ix_accumulate with plain global atomics / another cache size (scripts/ordinal_bench.py --acc-libs);
#  `make build/libphj_col8.so HIPDEFS=-DPHJ_COL_LOAD16=0`: the column form of the code pass with 8-B loads (scripts/columns_bench.py))
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
