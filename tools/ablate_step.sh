#!/bin/bash
# Where does the step time go?  bench.py with one kernel family NOT launched at a time (wrong results, timing only): the drop in
# ms/step is what that family costs the step INCLUDING its contention with the other streams (the sum of in-step kernel durations
# over-counts: the streams time-slice).   usage: bash tools/ablate_step.sh > gpurun_out/ablate.txt
# Stops at the first run that fails or exceeds LIMIT seconds (three times one such run: 4.7-4.9 s from start to exit on an MI355X).
set -eo pipefail
LIMIT=15
run() { VDM4CDM_EXPERIMENT=$1 timeout -k 10 $LIMIT python bench.py --steps 30 --no-cpu-baseline --no-kernel-events --sample-steps 0 | python -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('%-28s %.3f ms/step' % ('$2', d['ms_per_step']))"; }
run ablate= "full step"
run ablate_reduce "no wgrad slab reduces"
run ablate=wgrad "no weight gradients"
run ablate=wgrad1 "no 1x1 weight gradients"
run ablate=conv1 "no 1x1 convs (fwd+dgrad)"
run ablate=gn_fwd "no gn_silu_fwd"
run ablate=gn_apply "no gn_bwd_apply"
run ablate=pack "no weight re-packing"
run ablate= "full step (again)"
