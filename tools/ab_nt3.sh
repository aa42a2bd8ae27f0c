#!/bin/bash
R=$GRAFT_REPO_ROOT; cd $R; O=$R/gpurun_out/ab_nt; mkdir -p $O
timeout 900 python -m pytest tests/test_gpu_parity.py -q -m gpu -k "conv or embedding or fused or bottleneck or stem" 2>&1 | tail -3 | tee $O/tests3.txt
timeout 900 python tools/ab_inproc.py --reps ${REPS:-6} $VARS > $O/ab3.txt 2>&1; tail -45 $O/ab3.txt
