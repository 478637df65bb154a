#!/bin/bash
# usage (GPU box): bash tools/pmc_gemm.sh <tag>   -- SQ / LDS counters for the SAGE GEMM
tag=$1
R=$GRAFT_REPO_ROOT
OUT=${OUT:-$R/runs}; mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
run() { name=$1; shift; rocprofv3 --pmc "$@" --kernel-trace --output-format csv -d $OUT/pmc_$tag/$name -- python3 $R/bench.py --full --no-cpu-baseline --steps 3 --warmup 1 > $OUT/pmc_$tag.$name.log 2>&1 || echo "$name failed"; }
run sq1 SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU SQ_INSTS_LDS
run sq2 SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAIT_INST_LDS SQ_ACTIVE_INST_LDS SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VALU_MFMA_MOPS_F32 SQ_INSTS_VMEM_RD SQ_ACTIVE_INST_VALU
echo done
