#!/bin/bash
# Bench configuration <cfg> with the library rebuilt under each extra flag set:  tools/variants_cfg.sh c4 "-DSC_QR_IB=8" "-DSC_QR_IB=16"
# (SC_QR_IB is read by the panel kernels of sy2sb.hip AND by the slab layout of twostage.hip, which must agree: touching the header
# they share, which every object depends on, rebuilds both -- and everything else)
set -u
cd ${GRAFT_REPO_ROOT:-.}
mkdir -p results
. tools/ab_lib.sh
CFG=$1; shift
ab_keep springcraft_amd/csrc/twostage_internal.h   # (the file is not changed; the EXIT trap rebuilds the library without extra flags)
for rep in 1 2; do
  for flags in "$@"; do
    touch springcraft_amd/csrc/twostage_internal.h
    ab_build "$flags" || continue
    timeout -k 10 120 python bench.py --full --config $CFG --no-cpu-baseline --steps 5 --warmup 1 > results/varc.json 2>/dev/null
    echo "[$flags] $(python tools/show_bench.py results/varc.json | sed 's/.*modes\/s //')"
  done
done
