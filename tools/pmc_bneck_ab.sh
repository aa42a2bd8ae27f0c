#!/bin/bash
# fabric reads and writes of the fused bottleneck kernel (nt policy on its residual re-read and output stores; the default-policy arm this
# was compared with went with the compile-time switch: profiles/r06_ab_nt_policy.txt keeps its figures)
R=$GRAFT_REPO_ROOT; cd $R
PMC_SETS="FETCH_SIZE WRITE_SIZE" bash tools/pmc_bneck.sh 1000 2>&1 | tail -8
rm -rf $R/gpurun_out/pmc_bneck
